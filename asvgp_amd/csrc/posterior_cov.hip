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

template <int K, int R>
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
      bspline_pieces<K>((xa[r] - mesh[idx]) * inv_delta, va);
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
    bspline_pieces<K>((xb - mesh[idx]) * inv_delta, vb);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (r < nr) {
        double q = 0.0;
#pragma unroll
        for (int i = 0; i <= K; ++i) q = fma(vb[i], g[r * M + idx + K - i], q);
        cov[(a0 + r) * ldc + b] = matern(kind, v, inv_l, xa[r], xb) + q;
      }
    }
  }
}

template <int K>
static int launch_cov(const double* x1, long n1, const double* x2, long n2, const double* mesh, int n_mesh, double delta, int M,
                      const double* Wd, int kind, double v, double l, double* cov, long ldc, hipStream_t st) {
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
  if (gx > 0x7fffffff || gy > 65535) { set_error("predict_cov_1d: n1 = %ld, n2 = %ld too large for one launch", n1, n2); return ASVGP_ERR_UNSUPPORTED; }
  auto kern = R == COV_ROWS ? predict_cov_kernel<K, COV_ROWS> : predict_cov_kernel<K, 1>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) { set_error("predict_cov_1d: hipFuncSetAttribute: %s", hipGetErrorString(e)); return ASVGP_ERR_LDS_CAPACITY; }
  hipLaunchKernelGGL(kern, dim3((unsigned)gx, (unsigned)gy), dim3(COV_THREADS), lds, st, x1, n1, x2, n2, mesh, n_mesh, 1.0 / delta, M, Wd,
                     kind, v, 1.0 / l, chunk, cov, ldc);
  return check_launch("predict_cov_1d");
}

}  // namespace asvgp

using namespace asvgp;

// handle: accepted like asvgp_predict_1d_h's (NULL = the process default); the kernel keeps no per-handle state and the call never touches it
extern "C" int asvgp_predict_cov_1d(asvgp_handle_t handle, const double* x1, int64_t n1, const double* x2, int64_t n2, const double* mesh,
                                    int64_t n_mesh, double delta, int order, int64_t M, const double* W_dense, int kind, double variance,
                                    double lengthscale, double* cov, int64_t ldc, asvgp_stream_t stream) {
  (void)handle;
  if (!x1 || !x2 || !mesh || !W_dense || !cov || n1 < 0 || n2 < 0 || ldc < n2 || !(delta > 0.0) || !(variance > 0.0) ||
      !(lengthscale > 0.0)) {
    set_error("predict_cov_1d: bad argument");
    return ASVGP_ERR_BAD_ARG;
  }
  if (order < 1 || order > ASVGP_MAX_ORDER) { set_error("predict_cov_1d: order %d unsupported", order); return ASVGP_ERR_UNSUPPORTED; }
  if (kind < ASVGP_MATERN12 || kind > ASVGP_MATERN52) { set_error("predict_cov_1d: kernel kind %d unsupported", kind); return ASVGP_ERR_UNSUPPORTED; }
  if (M < order + 1 || n_mesh != M - order + 1) { set_error("predict_cov_1d: bad argument (n_mesh = %ld, M = %ld, order %d)", (long)n_mesh, (long)M, order); return ASVGP_ERR_BAD_ARG; }
  if (sizeof(double) * (size_t)M > COV_LDS_MAX) {
    set_error("predict_cov_1d: a row of W_dense (M = %ld) does not fit the kernel's LDS plan", (long)M);
    return ASVGP_ERR_UNSUPPORTED;
  }
  if (n1 == 0 || n2 == 0) return ASVGP_OK;
  hipStream_t st = as_stream(stream);
  switch (order) {
    case 1: return launch_cov<1>(x1, n1, x2, n2, mesh, (int)n_mesh, delta, (int)M, W_dense, kind, variance, lengthscale, cov, ldc, st);
    case 2: return launch_cov<2>(x1, n1, x2, n2, mesh, (int)n_mesh, delta, (int)M, W_dense, kind, variance, lengthscale, cov, ldc, st);
    case 3: return launch_cov<3>(x1, n1, x2, n2, mesh, (int)n_mesh, delta, (int)M, W_dense, kind, variance, lengthscale, cov, ldc, st);
    case 4: return launch_cov<4>(x1, n1, x2, n2, mesh, (int)n_mesh, delta, (int)M, W_dense, kind, variance, lengthscale, cov, ldc, st);
    case 5: return launch_cov<5>(x1, n1, x2, n2, mesh, (int)n_mesh, delta, (int)M, W_dense, kind, variance, lengthscale, cov, ldc, st);
    default: return launch_cov<6>(x1, n1, x2, n2, mesh, (int)n_mesh, delta, (int)M, W_dense, kind, variance, lengthscale, cov, ldc, st);
  }
}
