// Posterior cross-covariance of the 1-D model (asvgp_predict_cov_1d):
//   cov[a, b] = k(x1_a, x2_b) + phi(x1_a)^T W_dense phi(x2_b),   W_dense = P^-1 - Kuu^-1 (asvgp_posterior_cov_prepare_1d)
// phi has k + 1 contiguous non-zeros (rows idx + k - i, i = 0..k), so per row a the product g_a = phi(x1_a)^T W_dense is a combination of
// k + 1 rows of W_dense, formed once per workgroup in the LDS from coalesced reads; the x2 points are swept across the lanes, each one's
// cell and k + 1 B-spline weights evaluated as the predict kernel does (phi_pass.hip predict_point), contracted with k + 1 LDS reads of
// g_a per row, the Matern closed form added in fp64, and the rows of cov stored coalesced.
#include "asvgp_common.hpp"

namespace asvgp {

constexpr int COV_THREADS = 256;
constexpr int COV_ROWS = 4;                          // rows a per workgroup when R * M doubles fit COV_LDS_PREF
constexpr size_t COV_LDS_PREF = 64 * 1024;           // two workgroups per CU
constexpr size_t COV_LDS_MAX = 156 * 1024;           // one row alone may take up to this

// k(x, x') of gpflow's Matern kernels, r = |x - x'| / l
__device__ __forceinline__ double matern(int kind, double v, double inv_l, double x, double y) {
  const double r = fabs(x - y) * inv_l;
  if (kind == ASVGP_MATERN12) return v * exp(-r);
  if (kind == ASVGP_MATERN32) {
    const double sr = 1.7320508075688772 * r;
    return v * (1.0 + sr) * exp(-sr);
  }
  const double sr = 2.23606797749979 * r;
  return v * (1.0 + sr + (5.0 / 3.0) * r * r) * exp(-sr);
}

// d^P/dx^P d^Q/dx'^Q k(x, x') for P, Q in {0, 1}, tau = x - x', r = |tau|, a = sqrt(3)/l or sqrt(5)/l (Matern-3/2 / 5/2 only when P + Q > 0):
//   Matern-3/2:  d_x' k = v a^2 tau e^-ar,                d_x d_x' k = v a^2 (1 - ar) e^-ar
//   Matern-5/2:  d_x' k = (v a^2 / 3) tau (1 + ar) e^-ar,  d_x d_x' k = (v a^2 / 3)(1 + ar - a^2 r^2) e^-ar,   d_x k = -d_x' k
template <int P, int Q>
__device__ __forceinline__ double matern_deriv(int kind, double v, double inv_l, double x, double y) {
  if (P == 0 && Q == 0) return matern(kind, v, inv_l, x, y);
  const double tau = x - y;
  const bool m32 = kind == ASVGP_MATERN32;
  const double a = (m32 ? 1.7320508075688772 : 2.23606797749979) * inv_l;
  const double ar = a * fabs(tau);
  const double c = (m32 ? v : v * (1.0 / 3.0)) * a * a * exp(-ar);
  if (P == 1 && Q == 1) return m32 ? c * (1.0 - ar) : c * (1.0 + ar - ar * ar);
  const double d = m32 ? c * tau : c * tau * (1.0 + ar);    // d_x' k
  return Q == 1 ? d : -d;
}

// P, Q: derivative orders of the x1 and the x2 side (asvgp_predict_cov_deriv_1d): phi^(P)(x1_a)^T W_dense phi^(Q)(x2_b) + the Matern
// derivative above; (0, 0) is asvgp_predict_cov_1d.
template <int K, int R, int P = 0, int Q = 0>
__global__ __launch_bounds__(COV_THREADS) void predict_cov_kernel(const double* __restrict__ x1, long n1, const double* __restrict__ x2,
                                                                  long n2, const double* __restrict__ mesh, int n_mesh, double inv_delta,
                                                                  int M, const double* __restrict__ Wd, int kind, double v, double inv_l,
                                                                  long chunk, double* __restrict__ cov, long ldc) {
  extern __shared__ double g[];                      // g[r * M + m] = (phi(x1_{a0 + r})^T W_dense)[m]
  const long a0 = (long)blockIdx.x * R;
  const int nr = (n1 - a0 < R) ? (int)(n1 - a0) : R;
  const double m0 = mesh[0];
  double xa[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    xa[r] = r < nr ? x1[a0 + r] : 0.0;
    if (r < nr) {                                    // (uniform: every lane evaluates row a's cell and weights)
      const int idx = neighbour_index(xa[r], mesh, n_mesh, m0, inv_delta);
      double va[K + 1];
      bspline_pieces<K, P>((xa[r] - mesh[idx]) * inv_delta, va);
      if (P) {
#pragma unroll
        for (int i = 0; i <= K; ++i) va[i] *= inv_delta;
      }
      for (int m = threadIdx.x; m < M; m += COV_THREADS) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i <= K; ++i) acc = fma(va[i], Wd[(long)(idx + K - i) * M + m], acc);
        g[r * M + m] = acc;
      }
    }
  }
  __syncthreads();
  const long b_end = ((long)blockIdx.y + 1) * chunk < n2 ? ((long)blockIdx.y + 1) * chunk : n2;
  for (long b = (long)blockIdx.y * chunk + threadIdx.x; b < b_end; b += COV_THREADS) {
    const double xb = x2[b];
    const int idx = neighbour_index(xb, mesh, n_mesh, m0, inv_delta);
    double vb[K + 1];
    bspline_pieces<K, Q>((xb - mesh[idx]) * inv_delta, vb);
    if (Q) {
#pragma unroll
      for (int i = 0; i <= K; ++i) vb[i] *= inv_delta;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (r < nr) {
        double q = 0.0;
#pragma unroll
        for (int i = 0; i <= K; ++i) q = fma(vb[i], g[r * M + idx + K - i], q);
        cov[(a0 + r) * ldc + b] = matern_deriv<P, Q>(kind, v, inv_l, xa[r], xb) + q;
      }
    }
  }
}

template <int K, int R>
static decltype(&predict_cov_kernel<K, R>) cov_kernel_for(int p, int q) {
  if (p == 0) return q == 0 ? predict_cov_kernel<K, R, 0, 0> : predict_cov_kernel<K, R, 0, 1>;
  return q == 0 ? predict_cov_kernel<K, R, 1, 0> : predict_cov_kernel<K, R, 1, 1>;
}

// (p, q) = (0, 0): asvgp_predict_cov_1d; otherwise asvgp_predict_cov_deriv_1d (the caller has checked kind)
template <int K>
static int launch_cov(const double* x1, long n1, const double* x2, long n2, const double* mesh, int n_mesh, double delta, int M,
                      const double* Wd, int kind, double v, double l, int p, int q, double* cov, long ldc, hipStream_t st,
                      const char* what) {
  const size_t row_bytes = sizeof(double) * (size_t)M;
  const int R = (COV_ROWS * row_bytes <= COV_LDS_PREF) ? COV_ROWS : 1;
  const size_t lds = R * row_bytes;
  const long gx = (n1 + R - 1) / R;
  // column chunks: enough workgroups to fill the device when n1 is small (each chunk forms its rows' g_a again)
  long gy = (1024 + gx - 1) / gx;
  const long gy_max = (n2 + COV_THREADS - 1) / COV_THREADS;
  if (gy > gy_max) gy = gy_max;
  if (gy < 1) gy = 1;
  const long chunk = (n2 + gy - 1) / gy;
  gy = (n2 + chunk - 1) / chunk;
  if (gx > 0x7fffffff || gy > 65535) { set_error("%s: n1 = %ld, n2 = %ld too large for one launch", what, n1, n2); return ASVGP_ERR_UNSUPPORTED; }
  auto kern = R == COV_ROWS ? cov_kernel_for<K, COV_ROWS>(p, q) : cov_kernel_for<K, 1>(p, q);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) { set_error("%s: hipFuncSetAttribute: %s", what, hipGetErrorString(e)); return ASVGP_ERR_LDS_CAPACITY; }
  hipLaunchKernelGGL(kern, dim3((unsigned)gx, (unsigned)gy), dim3(COV_THREADS), lds, st, x1, n1, x2, n2, mesh, n_mesh, 1.0 / delta, M, Wd,
                     kind, v, 1.0 / l, chunk, cov, ldc);
  return check_launch(what);
}

// the argument checks and order dispatch of both entry points
static int predict_cov_entry(const double* x1, int64_t n1, const double* x2, int64_t n2, const double* mesh, int64_t n_mesh, double delta,
                             int order, int64_t M, const double* W_dense, int kind, double variance, double lengthscale, int p, int q,
                             double* cov, int64_t ldc, asvgp_stream_t stream, const char* what) {
  if (!x1 || !x2 || !mesh || !W_dense || !cov || n1 < 0 || n2 < 0 || ldc < n2 || !(delta > 0.0) || !(variance > 0.0) ||
      !(lengthscale > 0.0) || p < 0 || p > 1 || q < 0 || q > 1) {
    set_error("%s: bad argument", what);
    return ASVGP_ERR_BAD_ARG;
  }
  if (order < 1 || order > ASVGP_MAX_ORDER) { set_error("%s: order %d unsupported", what, order); return ASVGP_ERR_UNSUPPORTED; }
  if (kind < ASVGP_MATERN12 || kind > ASVGP_MATERN52) { set_error("%s: kernel kind %d unsupported", what, kind); return ASVGP_ERR_UNSUPPORTED; }
  if ((p || q) && kind == ASVGP_MATERN12) {
    set_error("%s: Matern-1/2 has no mean-square derivative (its k''(0) is unbounded); derivatives need Matern-3/2 or Matern-5/2", what);
    return ASVGP_ERR_UNSUPPORTED;
  }
  if (M < order + 1 || n_mesh != M - order + 1) { set_error("%s: bad argument (n_mesh = %ld, M = %ld, order %d)", what, (long)n_mesh, (long)M, order); return ASVGP_ERR_BAD_ARG; }
  if (sizeof(double) * (size_t)M > COV_LDS_MAX) {
    set_error("%s: a row of W_dense (M = %ld) does not fit the kernel's LDS plan", what, (long)M);
    return ASVGP_ERR_UNSUPPORTED;
  }
  if (n1 == 0 || n2 == 0) return ASVGP_OK;
  hipStream_t st = as_stream(stream);
  switch (order) {
    case 1: return launch_cov<1>(x1, n1, x2, n2, mesh, (int)n_mesh, delta, (int)M, W_dense, kind, variance, lengthscale, p, q, cov, ldc, st, what);
    case 2: return launch_cov<2>(x1, n1, x2, n2, mesh, (int)n_mesh, delta, (int)M, W_dense, kind, variance, lengthscale, p, q, cov, ldc, st, what);
    case 3: return launch_cov<3>(x1, n1, x2, n2, mesh, (int)n_mesh, delta, (int)M, W_dense, kind, variance, lengthscale, p, q, cov, ldc, st, what);
    case 4: return launch_cov<4>(x1, n1, x2, n2, mesh, (int)n_mesh, delta, (int)M, W_dense, kind, variance, lengthscale, p, q, cov, ldc, st, what);
    case 5: return launch_cov<5>(x1, n1, x2, n2, mesh, (int)n_mesh, delta, (int)M, W_dense, kind, variance, lengthscale, p, q, cov, ldc, st, what);
    default: return launch_cov<6>(x1, n1, x2, n2, mesh, (int)n_mesh, delta, (int)M, W_dense, kind, variance, lengthscale, p, q, cov, ldc, st, what);
  }
}

}  // namespace asvgp

using namespace asvgp;

// handle: accepted like asvgp_predict_1d_h's (NULL = the process default); the kernel keeps no per-handle state and the call never touches it
extern "C" int asvgp_predict_cov_1d(asvgp_handle_t handle, const double* x1, int64_t n1, const double* x2, int64_t n2, const double* mesh,
                                    int64_t n_mesh, double delta, int order, int64_t M, const double* W_dense, int kind, double variance,
                                    double lengthscale, double* cov, int64_t ldc, asvgp_stream_t stream) {
  (void)handle;
  return predict_cov_entry(x1, n1, x2, n2, mesh, n_mesh, delta, order, M, W_dense, kind, variance, lengthscale, 0, 0, cov, ldc, stream,
                           "predict_cov_1d");
}

// cov[f^(p)(x1_a), f^(q)(x2_b)]: the same kernel with derivative orders (p, q) in {0, 1}^2
extern "C" int asvgp_predict_cov_deriv_1d(asvgp_handle_t handle, const double* x1, int64_t n1, const double* x2, int64_t n2,
                                          const double* mesh, int64_t n_mesh, double delta, int order, int64_t M, const double* W_dense,
                                          int kind, double variance, double lengthscale, int p, int q, double* cov, int64_t ldc,
                                          asvgp_stream_t stream) {
  (void)handle;
  return predict_cov_entry(x1, n1, x2, n2, mesh, n_mesh, delta, order, M, W_dense, kind, variance, lengthscale, p, q, cov, ldc, stream,
                           "predict_cov_deriv_1d");
}
