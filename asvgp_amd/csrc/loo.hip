// Closed-form leave-one-out predictions of GPR_1d (asvgp_loo_1d): one streaming pass over the TRAINING rows.
//
// The posterior is a Gaussian linear model in the inducing features, so removing row i is a rank-one downdate of
// P = Kuu + Phi W Phi^T / s.  With phi = phi(x_i), whose k+1 non-zeros are contiguous,
//   g  = phi^T P^-1 phi            (the (k+1) x (k+1) window of band(P^-1))
//   h  = w_i g / s                 (leverage, 0 <= h < 1; w_i = 1 without weights)
//   mu = phi^T alpha,   var = v + phi^T W phi   (the ordinary posterior of asvgp_predict_1d)
//   mean of f(x_i) given all rows but i:  (mu - h y_i) / (1 - h)
//   its variance:                          var + g h / (1 - h)
//   log p(y_i | y_-i) = sum_d log N(y_id | that mean, that variance + s / w_i)
// A row with w_i = 0 is already absent (h = 0): the ordinary prediction, noise variance s, left out of the scores.  Nothing is clamped.
//
// Per point the kernel evaluates the B-spline pieces once and forms the D dot products and BOTH quadratic forms in one walk of the window.
// Staged plan (N >= 65 536): alpha, the mesh and W / band(P^-1) INTERLEAVED (one 16-byte LDS read brings both entries of a band position) are
// copied into the LDS once per workgroup.  Tables that do not fit whole (k = 4, D = 1: M > 1696) are split into up to 4 (orders 5, 6: 2)
// ranges of mesh cells, one per blockIdx.y: every range's workgroups stride over all rows and take the rows of their cells, so a row is
// served by exactly one workgroup and x / y / w are read once per range.  Otherwise, and below 65 536 rows, the tables are read through
// the caches.  HBM: 24 B in per point and range (16 B unweighted), 8 (D + 2) B out when every per-row output is asked for, nothing of
// size N out for the scores alone.
// Scores [#{w > 0}, sum logdens, sum_i sum_d (y - mean)^2, max h] are reduced in a fixed order and without floating-point atomics: DPP sums per
// wavefront, the wavefronts of a workgroup in index order into one record of the workspace, the records by a one-wavefront launch.
#include "asvgp_common.hpp"
#include "handle.hpp"

namespace asvgp {

constexpr size_t LOO_LDS_BUDGET = 160 * 1024 - 512;
constexpr long LOO_STAGE_MIN_N = 65536;      // below it a workgroup would stage more table bytes than it streams
constexpr int LOO_RECORD = 4;                // [n_pos, sum logdens, sum squared error, max leverage]
constexpr int LOO_MAX_BLOCKS = 1024;         // records in the workspace: one per workgroup
constexpr long LOO_WRAP_N = 262144;          // a grid of at most this many threads per cell range: beyond it the grid-stride loop wraps
constexpr int LOO_SCRATCH = 64;              // 16 wavefronts x LOO_RECORD

struct LooArgs {
  const double* x; const double* y; const double* w; long N; int D;
  const double* mesh; int n_mesh; double inv_delta; int M;
  const double* alpha; const double* W; const double* Pinv;
  double variance, noise;
  double* mean; double* var; double* logdens; double* partials;
  int cpc;                                   // staged plan: mesh cells per range (blockIdx.y); a range's tables span cpc + K columns
};

// NaN-sticky maximum: a leverage that is NaN must reach max h, whatever comes after it
__device__ __forceinline__ double loo_max(double a, double b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }

// halves of phi^T W phi and phi^T P^-1 phi on the (k+1) x (k+1) window: phi_i sits on row c + K - i (predict_point's walk), c the first column
// of the window.  Staged: entry [d][c] of both bands is one double2 of the interleaved table; else two lower bands (k+1, M) in global memory.
template <int K, bool STAGE>
__device__ __forceinline__ void loo_windows(const double (&v)[K + 1], const double2* T, const double* W, const double* Pi, int c, int ld,
                                            double& qw, double& qp) {
  qw = 0.0; qp = 0.0;
#pragma unroll
  for (int i = 0; i <= K; ++i) {
    const int e = c + K - i;
    const double2 dg = STAGE ? T[e] : make_double2(W[e], Pi[e]);
    double aw = 0.5 * v[i] * dg.x, ap = 0.5 * v[i] * dg.y;     // diagonal terms (halved, doubled by the caller)
#pragma unroll
    for (int j = i + 1; j <= K; ++j) {                         // row_j < row_i: band[d = j - i][row_j]
      const int o = (j - i) * ld + c + K - j;
      const double2 b = STAGE ? T[o] : make_double2(W[o], Pi[o]);
      aw = fma(v[j], b.x, aw);
      ap = fma(v[j], b.y, ap);
    }
    qw = fma(v[i], aw, qw);
    qp = fma(v[i], ap, qp);
  }
}

constexpr int loo_staged_threads(int K) { return K >= 5 ? 512 : 1024; }   // (orders 5 and 6 spill at 128 registers per lane)

template <int K, bool STAGE>
__global__ __launch_bounds__(STAGE ? loo_staged_threads(K) : 256) void loo_kernel(const LooArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];   // (the interleaved table is read 16 bytes at a time)
  const int M = a.M, D = a.D;
  // this workgroup's cells [cell0, cell1) and table columns [cell0, cell0 + cols); not staged: everything
  const int ncell = a.n_mesh - 1;
  const int cell0 = STAGE ? (int)blockIdx.y * a.cpc : 0;
  const int cell1 = STAGE ? (cell0 + a.cpc < ncell ? cell0 + a.cpc : ncell) : ncell;
  const int cols = STAGE ? a.cpc + K : M;
  // STAGE is a template parameter so that the table pointers are LDS pointers at compile time (see predict_kernel)
  const double2* T = reinterpret_cast<const double2*>(lds);
  const double* alpha = STAGE ? lds + 2 * (K + 1) * cols : a.alpha;
  const double* mesh = STAGE ? lds + 2 * (K + 1) * cols + cols * D : a.mesh;
  double* scratch = STAGE ? lds + 2 * (K + 1) * cols + cols * D + a.n_mesh : lds;
  if (STAGE) {
    double2* t2 = reinterpret_cast<double2*>(lds);
    double* ta = lds + 2 * (K + 1) * cols;
    double* tm = ta + cols * D;
#pragma unroll
    for (int d = 0; d <= K; ++d)
      for (int c = threadIdx.x; c < cols; c += blockDim.x) {
        const int gc = cell0 + c;                              // (the last range may be short: columns past M - 1 are never read)
        t2[d * cols + c] = gc < M ? make_double2(a.W[d * M + gc], a.Pinv[d * M + gc]) : make_double2(0.0, 0.0);
      }
    for (int e = threadIdx.x; e < cols * D; e += blockDim.x) {
      const long ge = (long)cell0 * D + e;
      ta[e] = ge < (long)M * D ? a.alpha[ge] : 0.0;
    }
#pragma unroll 2
    for (int e = threadIdx.x; e < a.n_mesh; e += blockDim.x) tm[e] = a.mesh[e];
    __syncthreads();
  }
  const double m0 = mesh[0];
  const double inv_noise = 1.0 / a.noise;
  const bool weighted = a.w != nullptr;
  double cnt = 0.0, sld = 0.0, ssq = 0.0, mxh = 0.0;
  const long stride = (long)gridDim.x * blockDim.x;
  long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  double xn = 0.0, wn = 1.0, yn = 0.0;
  if (p < a.N) { xn = a.x[p]; if (weighted) wn = a.w[p]; if (D == 1) yn = a.y[p]; }
  for (; p < a.N; p += stride) {
    const double xv = xn, wv = wn, y0 = yn;
    const long pn = p + stride;
    if (pn < a.N) { xn = a.x[pn]; if (weighted) wn = a.w[pn]; if (D == 1) yn = a.y[pn]; }   // the next row in flight under the table work
    const int idx = neighbour_index(xv, mesh, a.n_mesh, m0, a.inv_delta);
    if (STAGE && (idx < cell0 || idx >= cell1)) continue;      // another range's row
    const double t = (xv - mesh[idx]) * a.inv_delta;
    double v[K + 1];
    bspline_pieces<K>(t, v);
    const int c = idx - cell0;
    double qw, qp;
    loo_windows<K, STAGE>(v, T, a.W, a.Pinv, c, cols, qw, qp);
    const double var0 = fma(2.0, qw, a.variance);   // ordinary posterior variance
    const double g = 2.0 * qp;
    const double h = wv * g * inv_noise;
    const double om = 1.0 - h;
    const double vloo = var0 + g * (h / om);
    double sq = 0.0;
    for (int d = 0; d < D; ++d) {
      double mu = 0.0;
#pragma unroll
      for (int i = 0; i <= K; ++i) mu = fma(v[i], alpha[(long)(c + K - i) * D + d], mu);
      const double yv = (D == 1) ? y0 : a.y[p * D + d];
      const double m = (mu - h * yv) / om;
      if (a.mean) a.mean[p * D + d] = m;
      const double r = yv - m;
      sq = fma(r, r, sq);
    }
    const bool pos = wv > 0.0;
    const double s2 = vloo + (pos ? a.noise / wv : a.noise);
    const double ld = -0.5 * ((double)D * log(6.283185307179586 * s2) + sq / s2);
    if (a.var) a.var[p] = vloo;
    if (a.logdens) a.logdens[p] = ld;
    if (pos) { cnt += 1.0; sld += ld; ssq += sq; mxh = loo_max(mxh, h); }
  }
  if (!a.partials) return;
  // fixed order: DPP sums inside the wavefront, the wavefronts of the workgroup in index order, the workgroups in loo_scores_kernel
  cnt = wave_sum_dpp(cnt); sld = wave_sum_dpp(sld); ssq = wave_sum_dpp(ssq);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mxh = loo_max(mxh, __shfl_xor(mxh, off, 64));
  const int lane = threadIdx.x & 63, wf = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if (lane == 0) { double* r = scratch + wf * LOO_RECORD; r[0] = cnt; r[1] = sld; r[2] = ssq; r[3] = mxh; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
    for (int q = 0; q < nw; ++q) {
      const double* r = scratch + q * LOO_RECORD;
      r0 += r[0]; r1 += r[1]; r2 += r[2]; r3 = loo_max(r3, r[3]);
    }
    double* out = a.partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * LOO_RECORD;
    out[0] = r0; out[1] = r1; out[2] = r2; out[3] = r3;
  }
}

// scores = the G workgroup records in a fixed order (one wavefront: lane l takes records l, l + 64, ... in turn)
__global__ __launch_bounds__(64) void loo_scores_kernel(const double* __restrict__ partials, int G, double* __restrict__ scores) {
  const int lane = threadIdx.x;
  double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
  for (int g = lane; g < G; g += 64) {
    const double* r = partials + (size_t)g * LOO_RECORD;
    r0 += r[0]; r1 += r[1]; r2 += r[2]; r3 = loo_max(r3, r[3]);
  }
  r0 = wave_sum_dpp(r0); r1 = wave_sum_dpp(r1); r2 = wave_sum_dpp(r2);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) r3 = loo_max(r3, __shfl_xor(r3, off, 64));
  if (lane == 0) { scores[0] = r0; scores[1] = r1; scores[2] = r2; scores[3] = r3; }
}

template <int K>
static int launch_loo(LooArgs a, double* scores, hipStream_t st) {
  // staged plan: the fewest cell ranges whose tables fit the LDS, while every workgroup keeps a record of its own in the workspace
  constexpr int ST = loo_staged_threads(K);
  constexpr int max_ranges = LOO_MAX_BLOCKS / (int)(LOO_WRAP_N / ST);
  const int ncell = a.n_mesh - 1;
  int ranges = 0;
  size_t staged_bytes = 0;
  if (a.N >= LOO_STAGE_MIN_N)
    for (int c = 1; c <= max_ranges && c <= ncell && !ranges; ++c) {
      const int cpc = (ncell + c - 1) / c;
      const size_t cols = (size_t)cpc + K;
      staged_bytes = sizeof(double) * (2 * (K + 1) * cols + cols * (size_t)a.D + (size_t)a.n_mesh + LOO_SCRATCH);
      if (staged_bytes <= LOO_LDS_BUDGET) { ranges = c; a.cpc = cpc; }
    }
  const bool stage = ranges > 0;
  const int threads = stage ? ST : 256;
  long blocks = (a.N + threads - 1) / threads;
  if (blocks > LOO_WRAP_N / threads) blocks = LOO_WRAP_N / threads;
  static_assert(LOO_WRAP_N / 256 <= LOO_MAX_BLOCKS && max_ranges >= 1, "one record per workgroup");
  const size_t lds_bytes = stage ? staged_bytes : sizeof(double) * LOO_SCRATCH;
  auto kern = stage ? loo_kernel<K, true> : loo_kernel<K, false>;
  if (stage) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) { set_error("loo_1d: hipFuncSetAttribute(%zu B LDS): %s", lds_bytes, hipGetErrorString(e)); return ASVGP_ERR_LDS_CAPACITY; }
  }
  const int gy = stage ? ranges : 1;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)gy), dim3(threads), lds_bytes, st, a);
  if (scores) hipLaunchKernelGGL(loo_scores_kernel, dim3(1), dim3(64), 0, st, a.partials, (int)blocks * gy, scores);
  return check_launch("loo_1d");
}

}  // namespace asvgp

using namespace asvgp;

extern "C" size_t asvgp_loo_workspace_bytes(int64_t M, int order, int64_t D) {
  if (M < 1 || order < 1 || order > ASVGP_MAX_ORDER || D < 1) return 0;
  return sizeof(double) * (size_t)LOO_MAX_BLOCKS * LOO_RECORD;
}

extern "C" int asvgp_loo_1d(asvgp_handle_t handle, const double* x, const double* y, const double* w, int64_t N, int64_t D, const double* mesh,
                            int64_t n_mesh, double delta, int order, int64_t M, const double* alpha, const double* W, const double* Pinv_band,
                            double variance, double noise_variance, double* mean, double* var, double* logdens, double* scores,
                            void* workspace, size_t workspace_bytes, asvgp_stream_t stream) {
  (void)handle;   // accepted like asvgp_predict_deriv_1d's (NULL = the process default): the kernel keeps no per-handle state
  if (((!x || !y) && N > 0) || !mesh || !alpha || !W || !Pinv_band || N < 0 || D < 1 || M < 1 || !(delta > 0.0) || !(variance > 0.0) ||
      !(noise_variance > 0.0)) {
    set_error("loo_1d: bad argument");
    return ASVGP_ERR_BAD_ARG;
  }
  if (!mean && !var && !logdens && !scores) { set_error("loo_1d: bad argument (no output asked for: mean, var, logdens and scores are all NULL)"); return ASVGP_ERR_BAD_ARG; }
  if (order < 1 || order > ASVGP_MAX_ORDER) { set_error("loo_1d: order %d unsupported", order); return ASVGP_ERR_UNSUPPORTED; }
  if (n_mesh != M - order + 1 || n_mesh < 2) { set_error("loo_1d: bad argument (n_mesh = %ld, M = %ld, order %d)", (long)n_mesh, (long)M, order); return ASVGP_ERR_BAD_ARG; }
  if (M > 0x0fffffff || D > 0x0fffffff || M * D > 0x3fffffff) { set_error("loo_1d: M = %ld, D = %ld too large", (long)M, (long)D); return ASVGP_ERR_UNSUPPORTED; }
  if (!workspace || workspace_bytes < asvgp_loo_workspace_bytes(M, order, D)) {
    set_error("loo_1d: workspace too small (%zu < %zu)", workspace_bytes, asvgp_loo_workspace_bytes(M, order, D));
    return ASVGP_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  if (N == 0) {     // nothing to stream: no launch, the scores of an empty set
    if (scores) {
      hipError_t e = hipMemsetAsync(scores, 0, sizeof(double) * LOO_RECORD, st);
      if (e != hipSuccess) { set_error("loo_1d: hipMemsetAsync: %s", hipGetErrorString(e)); return ASVGP_ERR_HIP; }
    }
    return ASVGP_OK;
  }
  LooArgs a{x, y, w, (long)N, (int)D, mesh, (int)n_mesh, 1.0 / delta, (int)M, alpha, W, Pinv_band, variance, noise_variance,
            mean, var, logdens, scores ? static_cast<double*>(workspace) : nullptr, 0};
  switch (order) {
    case 1: return launch_loo<1>(a, scores, st);
    case 2: return launch_loo<2>(a, scores, st);
    case 3: return launch_loo<3>(a, scores, st);
    case 4: return launch_loo<4>(a, scores, st);
    case 5: return launch_loo<5>(a, scores, st);
    default: return launch_loo<6>(a, scores, st);
  }
}
