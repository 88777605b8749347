// Posterior cross-covariance of the additive model (asvgp_predict_cov_additive):
//   cov[a, b] = sum_i k_i(x1_ai, x2_bi) + phi(x1_a)^T W phi(x2_b),   W = P^-1 - blockdiag(K_1^-1 .. K_d^-1)   (M_tot x M_tot, dense)
// phi(x) = [phi_1(x_1); ..; phi_d(x_d)] has k + 1 contiguous non-zeros per block, rows off_i + idx_i + k - j, so per row a the product
// g_a = phi(x1_a)^T W is a combination of d (k + 1) rows of W, formed once per workgroup in the LDS from coalesced reads (the plan of
// posterior_cov.hip); the x2 points are swept across the lanes, and for every one of them each dimension's cell and k + 1 B-spline
// weights are contracted with k + 1 LDS reads of g_a per row, that dimension's Matern closed form added in fp64, and the rows of cov
// stored coalesced.  The per-dimension scalars travel in a by-value kernel argument (no copy, no allocation, no per-handle state).
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
  if (d > ASVGP_ADDITIVE_COV_MAX_D) {
    set_error("predict_cov_additive: d = %d above the maximum %d", d, (int)ASVGP_ADDITIVE_COV_MAX_D);
    return ASVGP_ERR_UNSUPPORTED;
  }
  for (int i = 0; i < d; ++i)
    if (!(delta[i] > 0.0) || !(variance[i] > 0.0) || !(lengthscale[i] > 0.0)) {
      set_error("predict_cov_additive: bad argument (dimension %d: delta %g, variance %g, lengthscale %g)", i, delta[i], variance[i],
                lengthscale[i]);
      return ASVGP_ERR_BAD_ARG;
    }
  if (order < 1 || order > ASVGP_MAX_ORDER) { set_error("predict_cov_additive: order %d unsupported", order); return ASVGP_ERR_UNSUPPORTED; }
  for (int i = 0; i < d; ++i)
    if (kind[i] < ASVGP_MATERN12 || kind[i] > ASVGP_MATERN52) {
      set_error("predict_cov_additive: kernel kind %d of dimension %d unsupported", kind[i], i);
      return ASVGP_ERR_UNSUPPORTED;
    }
  for (int i = 0; i < d; ++i)
    if (m[i] < order + 1 || n_mesh[i] != m[i] - order + 1) {
      set_error("predict_cov_additive: bad argument (dimension %d: n_mesh = %ld, m = %ld, order %d)", i, (long)n_mesh[i], (long)m[i], order);
      return ASVGP_ERR_BAD_ARG;
    }
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
