// Held-out scores of GPR_1d (asvgp_score_1d): one streaming pass over rows the model has NOT seen.
//
// Per row, with phi = phi(x_i) (k+1 contiguous non-zeros) and the tables of asvgp_posterior_prepare_1d:
//   mu  = phi^T alpha,   var = v + phi^T W phi        (asvgp_predict_1d_h's moments: the cell rule of neighbour_index, predict_point's walk)
//   s2  = var + s / w_i                               (s for a row with w_i = 0; w = NULL: all ones)
//   logdens = sum_d log N(y_id | mu_d, s2)
// scores = [#{w_i > 0}, sum logdens, sum_i sum_d (y_id - mu_id)^2, sum_i sum_d (y_id - mu_id)^2 / s2_i] over the rows with w_i > 0; the fourth
// is the calibration statistic (expectation n D).  A row with w_i = 0 gets its per-row outputs and is left out.  Nothing is clamped: a NaN
// in a counted row reaches the sums.
//
// Launch plan (loo.hip's, with ONE band instead of two).  N >= SCORE_STAGE_MIN_N = 65 536: W, alpha and the mesh are copied into the LDS once
// per workgroup, 8 ((k+1) cols + cols D + n_mesh + 64) bytes with cols = cells + k table columns, within 160 KiB - 512.  k = 4, D = 1: whole
// up to M = 2907 (the headline's M = 2048 takes 115 KB: every row is visited once).  Larger tables are split into up to 4 (orders 5, 6: 2)
// ranges of mesh cells, one per blockIdx.y: every range's workgroups stride over all rows and take the rows of their cells.  Tables that do
// not fit 4 (2) ranges, and every call below 65 536 rows, read the tables through the caches with 256 threads per workgroup.  A grid has at
// most SCORE_WRAP_N = 262 144 threads per range; beyond it the grid-stride loop wraps.  Staged workgroups run 1024 threads (orders 5, 6: 512).
// HBM: 16 B in per row and range (24 B weighted, + 8 (D - 1)), 8 (D + 2) B out with every per-row output, nothing of size N for the scores.
// The scores are reduced in a fixed order and without floating-point atomics: DPP sums per wavefront, the wavefronts of a workgroup in index
// order into one record of the workspace, the records by a one-wavefront launch.  The same call twice returns the same bits, and the
// scores-only call the bits of the per-row call.
#include "asvgp_common.hpp"
#include "handle.hpp"

namespace asvgp {

constexpr size_t SCORE_LDS_BUDGET = 160 * 1024 - 512;
constexpr long SCORE_STAGE_MIN_N = 65536;    // below it a workgroup would stage more table bytes than it streams
constexpr int SCORE_RECORD = 4;              // [n_pos, sum logdens, sum squared error, sum squared error / s2]
constexpr int SCORE_MAX_BLOCKS = 1024;       // records in the workspace: one per workgroup
constexpr long SCORE_WRAP_N = 262144;        // a grid of at most this many threads per cell range
constexpr int SCORE_SCRATCH = 64;            // 16 wavefronts x SCORE_RECORD

struct ScoreArgs {
  const double* x; const double* y; const double* w; long N; int D;
  const double* mesh; int n_mesh; double inv_delta; int M;
  const double* alpha; const double* W;
  double variance, noise;
  double* mean; double* var; double* logdens; double* partials;
  int cpc;                                   // staged plan: mesh cells per range (blockIdx.y); a range's tables span cpc + K columns
};

constexpr int score_staged_threads(int K) { return K >= 5 ? 512 : 1024; }

template <int K, bool STAGE>
__global__ __launch_bounds__(STAGE ? score_staged_threads(K) : 256) void score_kernel(const ScoreArgs a) {
  extern __shared__ double lds[];
  const int M = a.M, D = a.D;
  const int ncell = a.n_mesh - 1;
  const int cell0 = STAGE ? (int)blockIdx.y * a.cpc : 0;
  const int cell1 = STAGE ? (cell0 + a.cpc < ncell ? cell0 + a.cpc : ncell) : ncell;
  const int cols = STAGE ? a.cpc + K : M;
  // STAGE is a template parameter so that the table pointers are LDS pointers at compile time (see predict_kernel)
  const double* W = STAGE ? lds : a.W;
  const double* alpha = STAGE ? lds + (K + 1) * cols : a.alpha;
  const double* mesh = STAGE ? lds + (K + 1) * cols + cols * D : a.mesh;
  double* scratch = STAGE ? lds + (K + 1) * cols + cols * D + a.n_mesh : lds;
  if (STAGE) {
    double* tw = lds;
    double* ta = lds + (K + 1) * cols;
    double* tm = ta + cols * D;
#pragma unroll
    for (int d = 0; d <= K; ++d)
      for (int c = threadIdx.x; c < cols; c += blockDim.x) {
        const int gc = cell0 + c;                              // (the last range may be short: columns past M - 1 are never read)
        tw[d * cols + c] = gc < M ? a.W[d * M + gc] : 0.0;
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
  const bool weighted = a.w != nullptr;
  double cnt = 0.0, sld = 0.0, ssq = 0.0, sch = 0.0;
  const long stride = (long)gridDim.x * blockDim.x;
  long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  // (two rows in flight, loaded unconditionally at clamped indices as predict_poly_kernel does, were measured no faster: 126 - 130 us
  // against 122 - 123 us at N = 10M, M = 2048.  The table work bounds this kernel, not the latency of its loads: DESIGN.md 4.3d.)
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
    double q = 0.0;                                            // predict_point's walk: phi_i sits on row c + K - i
#pragma unroll
    for (int i = 0; i <= K; ++i) {
      double acc = 0.5 * v[i] * W[c + K - i];
#pragma unroll
      for (int j = i + 1; j <= K; ++j) acc = fma(v[j], W[(j - i) * cols + c + K - j], acc);
      q = fma(v[i], acc, q);
    }
    const double var0 = fma(2.0, q, a.variance);
    double sq = 0.0;
    for (int d = 0; d < D; ++d) {
      double mu = 0.0;
#pragma unroll
      for (int i = 0; i <= K; ++i) mu = fma(v[i], alpha[(long)(c + K - i) * D + d], mu);
      const double yv = (D == 1) ? y0 : a.y[p * D + d];
      if (a.mean) a.mean[p * D + d] = mu;
      const double r = yv - mu;
      sq = fma(r, r, sq);
    }
    const bool pos = wv > 0.0;
    const double s2 = var0 + (pos ? a.noise / wv : a.noise);
    const double chi = sq / s2;
    const double ld = -0.5 * ((double)D * log(6.283185307179586 * s2) + chi);
    if (a.var) a.var[p] = var0;
    if (a.logdens) a.logdens[p] = ld;
    if (pos) { cnt += 1.0; sld += ld; ssq += sq; sch += chi; }
  }
  if (!a.partials) return;
  // fixed order: DPP sums inside the wavefront, the wavefronts of the workgroup in index order, the workgroups in score_sum_kernel
  cnt = wave_sum_dpp(cnt); sld = wave_sum_dpp(sld); ssq = wave_sum_dpp(ssq); sch = wave_sum_dpp(sch);
  const int lane = threadIdx.x & 63, wf = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if (lane == 0) { double* r = scratch + wf * SCORE_RECORD; r[0] = cnt; r[1] = sld; r[2] = ssq; r[3] = sch; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
    for (int g = 0; g < nw; ++g) {
      const double* r = scratch + g * SCORE_RECORD;
      r0 += r[0]; r1 += r[1]; r2 += r[2]; r3 += r[3];
    }
    double* out = a.partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * SCORE_RECORD;
    out[0] = r0; out[1] = r1; out[2] = r2; out[3] = r3;
  }
}

// scores = the G workgroup records in a fixed order (one wavefront: lane l takes records l, l + 64, ... in turn)
__global__ __launch_bounds__(64) void score_sum_kernel(const double* __restrict__ partials, int G, double* __restrict__ scores) {
  const int lane = threadIdx.x;
  double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
  for (int g = lane; g < G; g += 64) {
    const double* r = partials + (size_t)g * SCORE_RECORD;
    r0 += r[0]; r1 += r[1]; r2 += r[2]; r3 += r[3];
  }
  r0 = wave_sum_dpp(r0); r1 = wave_sum_dpp(r1); r2 = wave_sum_dpp(r2); r3 = wave_sum_dpp(r3);
  if (lane == 0) { scores[0] = r0; scores[1] = r1; scores[2] = r2; scores[3] = r3; }
}

template <int K>
static int launch_score(ScoreArgs a, double* scores, hipStream_t st) {
  // staged plan: the fewest cell ranges whose tables fit the LDS, while every workgroup keeps a record of its own in the workspace
  constexpr int ST = score_staged_threads(K);
  constexpr int max_ranges = SCORE_MAX_BLOCKS / (int)(SCORE_WRAP_N / ST);
  const int ncell = a.n_mesh - 1;
  int ranges = 0;
  size_t staged_bytes = 0;
  if (a.N >= SCORE_STAGE_MIN_N)
    for (int c = 1; c <= max_ranges && c <= ncell && !ranges; ++c) {
      const int cpc = (ncell + c - 1) / c;
      const size_t cols = (size_t)cpc + K;
      staged_bytes = sizeof(double) * ((K + 1) * cols + cols * (size_t)a.D + (size_t)a.n_mesh + SCORE_SCRATCH);
      if (staged_bytes <= SCORE_LDS_BUDGET) { ranges = c; a.cpc = cpc; }
    }
  const bool stage = ranges > 0;
  const int threads = stage ? ST : 256;
  long blocks = (a.N + threads - 1) / threads;
  if (blocks > SCORE_WRAP_N / threads) blocks = SCORE_WRAP_N / threads;
  static_assert(SCORE_WRAP_N / 256 <= SCORE_MAX_BLOCKS && max_ranges >= 1, "one record per workgroup");
  const size_t lds_bytes = stage ? staged_bytes : sizeof(double) * SCORE_SCRATCH;
  auto kern = stage ? score_kernel<K, true> : score_kernel<K, false>;
  if (stage) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) { set_error("score_1d: hipFuncSetAttribute(%zu B LDS): %s", lds_bytes, hipGetErrorString(e)); return ASVGP_ERR_LDS_CAPACITY; }
  }
  const int gy = stage ? ranges : 1;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)gy), dim3(threads), lds_bytes, st, a);
  if (scores) hipLaunchKernelGGL(score_sum_kernel, dim3(1), dim3(64), 0, st, a.partials, (int)blocks * gy, scores);
  return check_launch("score_1d");
}

}  // namespace asvgp

using namespace asvgp;

extern "C" size_t asvgp_score_workspace_bytes(int64_t M, int order, int64_t D) {
  if (M < 1 || order < 1 || order > ASVGP_MAX_ORDER || D < 1) return 0;
  return sizeof(double) * (size_t)SCORE_MAX_BLOCKS * SCORE_RECORD;
}

extern "C" int asvgp_score_1d(asvgp_handle_t handle, const double* x, const double* y, const double* w, int64_t N, int64_t D, const double* mesh,
                              int64_t n_mesh, double delta, int order, int64_t M, const double* alpha, const double* W, double variance,
                              double noise_variance, double* mean, double* var, double* logdens, double* scores, void* workspace,
                              size_t workspace_bytes, asvgp_stream_t stream) {
  (void)handle;   // accepted like asvgp_loo_1d's (NULL = the process default): the kernel keeps no per-handle state
  if (((!x || !y) && N > 0) || !mesh || !alpha || !W || N < 0 || D < 1 || M < 1 || !(delta > 0.0) || !(variance > 0.0) ||
      !(noise_variance > 0.0)) {
    set_error("score_1d: bad argument");
    return ASVGP_ERR_BAD_ARG;
  }
  if (!mean && !var && !logdens && !scores) { set_error("score_1d: bad argument (no output asked for: mean, var, logdens and scores are all NULL)"); return ASVGP_ERR_BAD_ARG; }
  if (order < 1 || order > ASVGP_MAX_ORDER) { set_error("score_1d: order %d unsupported", order); return ASVGP_ERR_UNSUPPORTED; }
  if (n_mesh != M - order + 1 || n_mesh < 2) { set_error("score_1d: bad argument (n_mesh = %ld, M = %ld, order %d)", (long)n_mesh, (long)M, order); return ASVGP_ERR_BAD_ARG; }
  if (M > 0x0fffffff || D > 0x0fffffff || M * D > 0x3fffffff) { set_error("score_1d: M = %ld, D = %ld too large", (long)M, (long)D); return ASVGP_ERR_UNSUPPORTED; }
  if (!workspace || workspace_bytes < asvgp_score_workspace_bytes(M, order, D)) {
    set_error("score_1d: workspace too small (%zu < %zu)", workspace_bytes, asvgp_score_workspace_bytes(M, order, D));
    return ASVGP_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  if (N == 0) {     // nothing to stream: no launch, the scores of an empty set
    if (scores) {
      hipError_t e = hipMemsetAsync(scores, 0, sizeof(double) * SCORE_RECORD, st);
      if (e != hipSuccess) { set_error("score_1d: hipMemsetAsync: %s", hipGetErrorString(e)); return ASVGP_ERR_HIP; }
    }
    return ASVGP_OK;
  }
  ScoreArgs a{x, y, w, (long)N, (int)D, mesh, (int)n_mesh, 1.0 / delta, (int)M, alpha, W, variance, noise_variance,
              mean, var, logdens, scores ? static_cast<double*>(workspace) : nullptr, 0};
  switch (order) {
    case 1: return launch_score<1>(a, scores, st);
    case 2: return launch_score<2>(a, scores, st);
    case 3: return launch_score<3>(a, scores, st);
    case 4: return launch_score<4>(a, scores, st);
    case 5: return launch_score<5>(a, scores, st);
    default: return launch_score<6>(a, scores, st);
  }
}
