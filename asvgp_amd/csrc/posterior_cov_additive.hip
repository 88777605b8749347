// Posterior cross-covariance of the additive model (asvgp_predict_cov_additive):
//   cov[a, b] = sum_i k_i(x1_ai, x2_bi) + phi(x1_a)^T W phi(x2_b),   W = P^-1 - blockdiag(K_1^-1 .. K_d^-1)   (M_tot x M_tot, dense)
// phi(x) = [phi_1(x_1); ..; phi_d(x_d)] has k + 1 contiguous non-zeros per block, rows off_i + idx_i + k - j, so per row a the product
// g_a = phi(x1_a)^T W is a combination of d (k + 1) rows of W, formed once per workgroup in the LDS from coalesced reads (the plan of
// posterior_cov.hip); the x2 points are swept across the lanes, and for every one of them each dimension's cell and k + 1 B-spline
// weights are contracted with k + 1 LDS reads of g_a per row, that dimension's Matern closed form added in fp64, and the rows of cov
// stored coalesced.  The per-dimension scalars travel in a by-value kernel argument (no copy, no allocation, no per-handle state).
//
// Components and gradient (asvgp_predict_components_additive), per point a and dimensions i, j, derivative order p in {0, 1}:
//   mean[a, i] = phi_i^(p)(x_ai)^T alpha_i,   cov[a, i, j] = [i = j] prior_i + phi_i^(p)(x_ai)^T W_ij phi_j^(p)(x_aj)
// One point per thread: for every pair j <= i the (k + 1) x (k + 1) block of W at the two cells is gathered into registers (k + 1 row
// segments of k + 1 contiguous doubles, 64-bit offsets) and contracted with both weight vectors; W is read in place, so M_tot has no LDS
// limit.  The loops over i and j are rolled and dimension j's cell and weights re-evaluated inside the j loop, so that no register array
// is indexed by a runtime index.
#include "asvgp_common.hpp"

namespace asvgp {

constexpr int CA_THREADS = 256;
constexpr int CA_ROWS = 4;                           // rows a per workgroup when R * M_tot doubles fit CA_LDS_PREF
constexpr size_t CA_LDS_PREF = 64 * 1024;            // two workgroups per CU
constexpr size_t CA_LDS_MAX = 156 * 1024;            // one row alone may take up to this (the 1-D kernel's plan)

struct AddDims {
  int d;
  int mesh_off[ASVGP_ADDITIVE_COV_MAX_D];            // dimension i's mesh: meshes + mesh_off[i], n_mesh[i] knots
  int n_mesh[ASVGP_ADDITIVE_COV_MAX_D];
  int off[ASVGP_ADDITIVE_COV_MAX_D];                 // dimension i's block of W starts at row / column off[i]
  int kind[ASVGP_ADDITIVE_COV_MAX_D];
  double inv_delta[ASVGP_ADDITIVE_COV_MAX_D], v[ASVGP_ADDITIVE_COV_MAX_D], inv_l[ASVGP_ADDITIVE_COV_MAX_D];
};

// the per-dimension checks both entry points share (what: the entry point's name in the error text)
static int check_additive_dims(const char* what, int d, const int64_t* n_mesh, const double* delta, const int64_t* m, int order,
                               const int* kind, const double* variance, const double* lengthscale) {
  if (d > ASVGP_ADDITIVE_COV_MAX_D) {
    set_error("%s: d = %d above the maximum %d", what, d, (int)ASVGP_ADDITIVE_COV_MAX_D);
    return ASVGP_ERR_UNSUPPORTED;
  }
  for (int i = 0; i < d; ++i)
    if (!(delta[i] > 0.0) || !(variance[i] > 0.0) || !(lengthscale[i] > 0.0)) {
      set_error("%s: bad argument (dimension %d: delta %g, variance %g, lengthscale %g)", what, i, delta[i], variance[i], lengthscale[i]);
      return ASVGP_ERR_BAD_ARG;
    }
  if (order < 1 || order > ASVGP_MAX_ORDER) { set_error("%s: order %d unsupported", what, order); return ASVGP_ERR_UNSUPPORTED; }
  for (int i = 0; i < d; ++i)
    if (kind[i] < ASVGP_MATERN12 || kind[i] > ASVGP_MATERN52) {
      set_error("%s: kernel kind %d of dimension %d unsupported", what, kind[i], i);
      return ASVGP_ERR_UNSUPPORTED;
    }
  for (int i = 0; i < d; ++i)
    if (m[i] < order + 1 || n_mesh[i] != m[i] - order + 1) {
      set_error("%s: bad argument (dimension %d: n_mesh = %ld, m = %ld, order %d)", what, i, (long)n_mesh[i], (long)m[i], order);
      return ASVGP_ERR_BAD_ARG;
    }
  return ASVGP_OK;
}

// the kernel argument of both entry points (the checks above passed, and M_tot fits an int)
static AddDims make_dims(int d, const int64_t* n_mesh, const double* delta, const int64_t* m, const int* kind, const double* variance,
                         const double* lengthscale) {
  AddDims P;
  P.d = d;
  int mesh_off = 0, off = 0;
  for (int i = 0; i < ASVGP_ADDITIVE_COV_MAX_D; ++i) {
    const bool on = i < d;
    P.mesh_off[i] = on ? mesh_off : 0;
    P.n_mesh[i] = on ? (int)n_mesh[i] : 0;
    P.off[i] = on ? off : 0;
    P.kind[i] = on ? kind[i] : 0;
    P.inv_delta[i] = on ? 1.0 / delta[i] : 0.0;
    P.v[i] = on ? variance[i] : 0.0;
    P.inv_l[i] = on ? 1.0 / lengthscale[i] : 0.0;
    if (on) { mesh_off += (int)n_mesh[i]; off += (int)m[i]; }
  }
  return P;
}

// k(x, x') of gpflow's Matern kernels, r = |x - x'| / l (the closed form of posterior_cov.hip)
__device__ __forceinline__ double matern_a(int kind, double v, double inv_l, double x, double y) {
  const double r = fabs(x - y) * inv_l;
  if (kind == ASVGP_MATERN12) return v * exp(-r);
  if (kind == ASVGP_MATERN32) {
    const double sr = 1.7320508075688772 * r;
    return v * (1.0 + sr) * exp(-sr);
  }
  const double sr = 2.23606797749979 * r;
  return v * (1.0 + sr + (5.0 / 3.0) * r * r) * exp(-sr);
}

template <int K, int R>
__global__ __launch_bounds__(CA_THREADS) void predict_cov_additive_kernel(const double* __restrict__ x1, long n1,
                                                                          const double* __restrict__ x2, long n2,
                                                                          const double* __restrict__ meshes, AddDims P, int M,
                                                                          const double* __restrict__ W, long chunk,
                                                                          double* __restrict__ cov, long ldc) {
  extern __shared__ double g[];                      // g[r * M + m] = (phi(x1_{a0 + r})^T W)[m]
  __shared__ double xs[R * ASVGP_ADDITIVE_COV_MAX_D];  // x1 rows of the workgroup, [r][i]
  const int d = P.d;
  const long a0 = (long)blockIdx.x * R;
  const int nr = (n1 - a0 < R) ? (int)(n1 - a0) : R;
  for (int e = threadIdx.x; e < R * d; e += CA_THREADS) {
    const int r = e / d, i = e - r * d;
    xs[r * ASVGP_ADDITIVE_COV_MAX_D + i] = r < nr ? x1[(a0 + r) * d + i] : 0.0;
  }
  for (int r = 0; r < nr; ++r) {                     // (uniform: every lane evaluates row a's cells and weights)
    for (int m = threadIdx.x; m < M; m += CA_THREADS) g[r * M + m] = 0.0;
    for (int i = 0; i < d; ++i) {
      const double* mesh = meshes + P.mesh_off[i];
      const double xa = x1[(a0 + r) * d + i];
      const int idx = neighbour_index(xa, mesh, P.n_mesh[i], mesh[0], P.inv_delta[i]);
      double va[K + 1];
      bspline_pieces<K>((xa - mesh[idx]) * P.inv_delta[i], va);
      const double* rows = W + (long)(P.off[i] + idx + K) * M;
      for (int m = threadIdx.x; m < M; m += CA_THREADS) {
        double acc = g[r * M + m];
#pragma unroll
        for (int j = 0; j <= K; ++j) acc = fma(va[j], rows[-(long)j * M + m], acc);
        g[r * M + m] = acc;
      }
    }
  }
  __syncthreads();
  const long b_end = ((long)blockIdx.y + 1) * chunk < n2 ? ((long)blockIdx.y + 1) * chunk : n2;
  for (long b = (long)blockIdx.y * chunk + threadIdx.x; b < b_end; b += CA_THREADS) {
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0;
    for (int i = 0; i < d; ++i) {
      const double* mesh = meshes + P.mesh_off[i];
      const double xb = x2[b * d + i];
      const int idx = neighbour_index(xb, mesh, P.n_mesh[i], mesh[0], P.inv_delta[i]);
      double vb[K + 1];
      bspline_pieces<K>((xb - mesh[idx]) * P.inv_delta[i], vb);
      const int col = P.off[i] + idx + K;
      const int kind = P.kind[i];
      const double v = P.v[i], inv_l = P.inv_l[i];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r < nr) {
          double q = 0.0;
#pragma unroll
          for (int j = 0; j <= K; ++j) q = fma(vb[j], g[r * M + col - j], q);
          acc[r] += matern_a(kind, v, inv_l, xs[r * ASVGP_ADDITIVE_COV_MAX_D + i], xb) + q;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (r < nr) cov[(a0 + r) * ldc + b] = acc[r];
  }
}

template <int K>
static int launch_cov_additive(const double* x1, long n1, const double* x2, long n2, const double* meshes, const AddDims& P, int M,
                               const double* W, double* cov, long ldc, hipStream_t st) {
  const size_t row_bytes = sizeof(double) * (size_t)M;
  const int R = (CA_ROWS * row_bytes <= CA_LDS_PREF) ? CA_ROWS : 1;
  const size_t lds = R * row_bytes;
  const long gx = (n1 + R - 1) / R;
  // column chunks: enough workgroups to fill the device when n1 is small (each chunk forms its rows' g_a again)
  long gy = (1024 + gx - 1) / gx;
  const long gy_max = (n2 + CA_THREADS - 1) / CA_THREADS;
  if (gy > gy_max) gy = gy_max;
  if (gy < 1) gy = 1;
  const long chunk = (n2 + gy - 1) / gy;
  gy = (n2 + chunk - 1) / chunk;
  if (gx > 0x7fffffff || gy > 65535) { set_error("predict_cov_additive: n1 = %ld, n2 = %ld too large for one launch", n1, n2); return ASVGP_ERR_UNSUPPORTED; }
  auto kern = R == CA_ROWS ? predict_cov_additive_kernel<K, CA_ROWS> : predict_cov_additive_kernel<K, 1>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) { set_error("predict_cov_additive: hipFuncSetAttribute: %s", hipGetErrorString(e)); return ASVGP_ERR_LDS_CAPACITY; }
  hipLaunchKernelGGL(kern, dim3((unsigned)gx, (unsigned)gy), dim3(CA_THREADS), lds, st, x1, n1, x2, n2, meshes, P, M, W, chunk, cov, ldc);
  return check_launch("predict_cov_additive");
}

constexpr int CC_THREADS = 256;

// the cell of x in dimension i and its k + 1 weights phi_i^(p) (x), times (1 / delta_i)^p; returns the row of w[0] (rows row - r, r = 0..K)
template <int K, int P>
__device__ __forceinline__ long cell_weights(const double* __restrict__ meshes, const AddDims& D, int i, double x, double (&w)[K + 1]) {
  const double* mesh = meshes + D.mesh_off[i];
  const double inv_delta = D.inv_delta[i];
  const int idx = neighbour_index(x, mesh, D.n_mesh[i], mesh[0], inv_delta);
  bspline_pieces<K, P>((x - mesh[idx]) * inv_delta, w);
  if (P) {
#pragma unroll
    for (int r = 0; r <= K; ++r) w[r] *= inv_delta;
  }
  return (long)D.off[i] + idx + K;
}

template <int K, int P>
__global__ __launch_bounds__(CC_THREADS) void predict_components_additive_kernel(const double* __restrict__ X, long n,
                                                                                 const double* __restrict__ meshes, AddDims D, long M,
                                                                                 const double* __restrict__ alpha,
                                                                                 const double* __restrict__ W, double* __restrict__ mean,
                                                                                 double* __restrict__ cov) {
  const long a = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (a >= n) return;
  const int d = D.d;
  const double* x = X + a * d;
  double* cov_a = cov + a * d * d;
  for (int i = 0; i < d; ++i) {
    double wi[K + 1];
    const long ri = cell_weights<K, P>(meshes, D, i, x[i], wi);
    double mu = 0.0;
#pragma unroll
    for (int r = 0; r <= K; ++r) mu = fma(wi[r], alpha[ri - r], mu);
    mean[a * d + i] = mu;
    for (int j = 0; j <= i; ++j) {
      double wj[K + 1];
      const long cj = cell_weights<K, P>(meshes, D, j, x[j], wj);
      double blk[K + 1][K + 1];                      // blk[r][s] = W[ri - r, cj - s]: every load issued before the first use
#pragma unroll
      for (int r = 0; r <= K; ++r) {
        const double* row = W + (ri - r) * M + cj - K;
#pragma unroll
        for (int s = 0; s <= K; ++s) blk[r][s] = row[K - s];
      }
      double q = 0.0;
#pragma unroll
      for (int r = 0; r <= K; ++r) {
        double t = 0.0;
#pragma unroll
        for (int s = 0; s <= K; ++s) t = fma(blk[r][s], wj[s], t);
        q = fma(wi[r], t, q);
      }
      if (j == i) {
        const double v = D.v[i], il = D.inv_l[i];
        q += P == 0 ? v : (D.kind[i] == ASVGP_MATERN32 ? 3.0 : 5.0 / 3.0) * v * il * il;
      }
      cov_a[i * d + j] = q;                          // (one value for both halves: symmetric bit for bit)
      cov_a[j * d + i] = q;
    }
  }
}

template <int K>
static int launch_components_additive(const double* X, long n, const double* meshes, const AddDims& D, long M, int deriv,
                                      const double* alpha, const double* W, double* mean, double* cov, hipStream_t st) {
  const long gx = (n + CC_THREADS - 1) / CC_THREADS;
  if (gx > 0x7fffffff) { set_error("predict_components_additive: n = %ld too large for one launch", n); return ASVGP_ERR_UNSUPPORTED; }
  auto kern = deriv ? predict_components_additive_kernel<K, 1> : predict_components_additive_kernel<K, 0>;
  hipLaunchKernelGGL(kern, dim3((unsigned)gx), dim3(CC_THREADS), 0, st, X, n, meshes, D, M, alpha, W, mean, cov);
  return check_launch("predict_components_additive");
}

}  // namespace asvgp

using namespace asvgp;

// handle: accepted like asvgp_predict_cov_1d's (NULL = the process default); the kernel keeps no per-handle state
extern "C" int asvgp_predict_cov_additive(asvgp_handle_t handle, const double* x1, int64_t n1, const double* x2, int64_t n2, int d,
                                          const double* meshes, const int64_t* n_mesh, const double* delta, const int64_t* m, int order,
                                          const int* kind, const double* variance, const double* lengthscale, const double* W,
                                          double* cov, int64_t ldc, asvgp_stream_t stream) {
  (void)handle;
  if (!x1 || !x2 || !meshes || !n_mesh || !delta || !m || !kind || !variance || !lengthscale || !W || !cov || n1 < 0 || n2 < 0 ||
      ldc < n2 || d < 1) {
    set_error("predict_cov_additive: bad argument");
    return ASVGP_ERR_BAD_ARG;
  }
  if (int st = check_additive_dims("predict_cov_additive", d, n_mesh, delta, m, order, kind, variance, lengthscale)) return st;
  size_t M = 0;
  bool huge = false;                                 // (an m_i alone beyond the plan: the sum is not formed, so it cannot overflow)
  for (int i = 0; i < d; ++i) {
    if ((size_t)m[i] > CA_LDS_MAX) huge = true;
    else M += (size_t)m[i];
  }
  if (huge || sizeof(double) * M > CA_LDS_MAX) {
    if (huge) set_error("predict_cov_additive: a row of W does not fit the kernel's LDS plan");
    else set_error("predict_cov_additive: a row of W (M_tot = %ld) does not fit the kernel's LDS plan", (long)M);
    return ASVGP_ERR_UNSUPPORTED;
  }
  if (n1 == 0 || n2 == 0) return ASVGP_OK;
  const AddDims P = make_dims(d, n_mesh, delta, m, kind, variance, lengthscale);
  hipStream_t st = as_stream(stream);
  const int Mt = (int)M;
  switch (order) {
    case 1: return launch_cov_additive<1>(x1, n1, x2, n2, meshes, P, Mt, W, cov, ldc, st);
    case 2: return launch_cov_additive<2>(x1, n1, x2, n2, meshes, P, Mt, W, cov, ldc, st);
    case 3: return launch_cov_additive<3>(x1, n1, x2, n2, meshes, P, Mt, W, cov, ldc, st);
    case 4: return launch_cov_additive<4>(x1, n1, x2, n2, meshes, P, Mt, W, cov, ldc, st);
    case 5: return launch_cov_additive<5>(x1, n1, x2, n2, meshes, P, Mt, W, cov, ldc, st);
    default: return launch_cov_additive<6>(x1, n1, x2, n2, meshes, P, Mt, W, cov, ldc, st);
  }
}

// components (deriv = 0) or gradient (deriv = 1) of the additive posterior, per point: mean (n, d), cov (n, d, d)
extern "C" int asvgp_predict_components_additive(asvgp_handle_t handle, const double* X, int64_t n, int d, const double* meshes,
                                                 const int64_t* n_mesh, const double* delta, const int64_t* m, int order, const int* kind,
                                                 const double* variance, const double* lengthscale, int deriv, const double* alpha,
                                                 const double* W, double* mean, double* cov, asvgp_stream_t stream) {
  (void)handle;
  if (!X || !meshes || !n_mesh || !delta || !m || !kind || !variance || !lengthscale || !alpha || !W || !mean || !cov || n < 0 ||
      d < 1 || deriv < 0 || deriv > 1) {
    set_error("predict_components_additive: bad argument");
    return ASVGP_ERR_BAD_ARG;
  }
  if (int st = check_additive_dims("predict_components_additive", d, n_mesh, delta, m, order, kind, variance, lengthscale)) return st;
  if (deriv)
    for (int i = 0; i < d; ++i)
      if (kind[i] == ASVGP_MATERN12) {
        set_error("predict_components_additive: dimension %d is Matern-1/2, which has no mean-square derivative (its k''(0) is unbounded); "
                  "the gradient needs Matern-3/2 or Matern-5/2", i);
        return ASVGP_ERR_UNSUPPORTED;
      }
  int64_t M = 0;                                     // (M_tot, and the smaller mesh offsets, travel as int)
  for (int i = 0; i < d; ++i) {
    if (m[i] > 0x7fffffff - M) {
      set_error("predict_components_additive: M_tot above 2^31 - 1 (dimension %d: m = %ld)", i, (long)m[i]);
      return ASVGP_ERR_UNSUPPORTED;
    }
    M += m[i];
  }
  if (n == 0) return ASVGP_OK;
  const AddDims P = make_dims(d, n_mesh, delta, m, kind, variance, lengthscale);
  hipStream_t st = as_stream(stream);
  switch (order) {
    case 1: return launch_components_additive<1>(X, n, meshes, P, M, deriv, alpha, W, mean, cov, st);
    case 2: return launch_components_additive<2>(X, n, meshes, P, M, deriv, alpha, W, mean, cov, st);
    case 3: return launch_components_additive<3>(X, n, meshes, P, M, deriv, alpha, W, mean, cov, st);
    case 4: return launch_components_additive<4>(X, n, meshes, P, M, deriv, alpha, W, mean, cov, st);
    case 5: return launch_components_additive<5>(X, n, meshes, P, M, deriv, alpha, W, mean, cov, st);
    default: return launch_components_additive<6>(X, n, meshes, P, M, deriv, alpha, W, mean, cov, st);
  }
}
