// Per-row scores of GPR_1d in one streaming pass: closed-form leave-one-out predictions over the TRAINING rows (asvgp_loo_1d, LOO = true)
// and held-out scores over rows the model has NOT seen (asvgp_score_1d, LOO = false).  One kernel template, one launch plan.
//
// Per row, with phi = phi(x_i) (k+1 contiguous non-zeros) and the tables of asvgp_posterior_prepare_1d / asvgp_posterior_prepare_loo_1d:
//   mu = phi^T alpha,   var = v + phi^T W phi        (asvgp_predict_1d_h's moments: the cell rule of neighbour_index, predict_point's walk)
// Held-out:
//   s2 = var + s / w_i                               (s for a row with w_i = 0; w = NULL: all ones)
//   logdens = sum_d log N(y_id | mu_d, s2)
//   scores = [#{w_i > 0}, sum logdens, sum_i sum_d (y_id - mu_id)^2, sum_i sum_d (y_id - mu_id)^2 / s2_i] over the rows with w_i > 0; the
//   fourth is the calibration statistic (expectation n D).
// Leave-one-out: the posterior is a Gaussian linear model in the inducing features, so removing row i is a rank-one downdate of
// P = Kuu + Phi W Phi^T / s:
//   g  = phi^T P^-1 phi            (the (k+1) x (k+1) window of band(P^-1), formed in the SAME walk as phi^T W phi)
//   h  = w_i g / s                 (leverage, 0 <= h < 1; w_i = 1 without weights)
//   mean of f(x_i) given all rows but i:  (mu - h y_i) / (1 - h)
//   its variance:                          var + g h / (1 - h)
//   log p(y_i | y_-i) = sum_d log N(y_id | that mean, that variance + s / w_i)
//   scores = [#{w > 0}, sum logdens, sum_i sum_d (y - mean)^2, max h]
// Either way a row with w_i = 0 gets its per-row outputs (leave-one-out: it is already absent, h = 0, the ordinary prediction with noise
// variance s) and is left out of the scores.  Nothing is clamped: a NaN in a counted row reaches the sums, and the maximum is NaN-sticky.
//
// Launch plan.  N >= STAGE_MIN_N = 65 536: the table, alpha and the mesh are copied into the LDS once per workgroup,
// 8 (B (k+1) cols + cols D + n_mesh + 64) bytes with cols = cells + k table columns and B bands, within 160 KiB - 512.  Held-out: B = 1, the
// band of W.  Leave-one-out: B = 2, W and band(P^-1) INTERLEAVED (one 16-byte LDS read brings both entries of a band position).  k = 4, D = 1:
// whole up to M = 2907 held-out (the headline's M = 2048 takes 115 KB: every row is visited once) and up to M = 1696 leave-one-out.  Larger
// tables are split into up to 4 (orders 5, 6: 2) ranges of mesh cells, one per blockIdx.y: every range's workgroups stride over all rows and
// take the rows of their cells, so a row is served by exactly one workgroup and x / y / w are read once per range.  Tables that do not fit
// 4 (2) ranges, and every call below 65 536 rows, read the tables through the caches with 256 threads per workgroup.  A grid has at most
// WRAP_N = 262 144 threads per range; beyond it the grid-stride loop wraps.  Staged workgroups run 1024 threads (orders 5, 6: 512).
// HBM: 16 B in per row and range (24 B weighted, + 8 (D - 1)), 8 (D + 2) B out with every per-row output, nothing of size N for the scores.
// The scores are reduced in a fixed order and without floating-point atomics: DPP sums per wavefront, the wavefronts of a workgroup in index
// order into one record of the workspace, the records by a one-wavefront launch.  The same call twice returns the same bits, and the
// scores-only call the bits of the per-row call.
//
// Third mode (asvgp_weight_grad_1d, WGRAD = true): the derivative of the weighted bound in every weight, on the leave-one-out tables and by
// the leave-one-out plan.  With r_id = y_id - mu_id and var = v + phi^T W phi (W = band(P^-1 - Kuu^-1), so var - g = v - phi^T Kuu^-1 phi):
//   grad_i = 1/2 [ D / w_i - (D g + sum_d r_id^2 + (var - g)) / s ]      (0 for a row with w_i = 0: it is absent from the model)
//   gsum[g] = [#{i in g, w_i > 0}, T_g = sum_{i in g, w_i > 0} w_i grad_i]
// groups = NULL (G = 1): n and T take slots 0 and 1 of the records above, the same fixed order, the same bits twice.  With group labels
// every workgroup keeps 2 G bins behind its tables in the LDS (they count against the staged plan's budget: 16 G bytes, 16 KiB at
// G = 1024), adds its rows with ds_add_f64, stores the bins as one row of the workspace, and group_sums_kernel adds the rows in a fixed
// order: no floating-point atomics to global memory.  n_g is exact (integers in doubles); T_g is reproducible to rounding only, because
// the order of the LDS adds inside a workgroup is not fixed.  A label outside [0, G) indexes nothing: the row is left out of gsum.
#include "asvgp_common.hpp"
#include "handle.hpp"

namespace asvgp {

constexpr size_t LDS_BUDGET = 160 * 1024 - 512;
constexpr long STAGE_MIN_N = 65536;          // below it a workgroup would stage more table bytes than it streams
constexpr int RECORD = 4;                    // [n_pos, sum logdens, sum squared error, max leverage (LOO) or sum squared error / s2]
constexpr int MAX_BLOCKS = 1024;             // records in the workspace: one per workgroup
constexpr long WRAP_N = 262144;              // a grid of at most this many threads per cell range: beyond it the grid-stride loop wraps
constexpr int SCRATCH = 64;                  // 16 wavefronts x RECORD

struct RowArgs {
  const double* x; const double* y; const double* w; long N; int D;
  const double* mesh; int n_mesh; double inv_delta; int M;
  const double* alpha; const double* W;
  double variance, noise;
  double* mean; double* var; double* logdens; double* partials;
  int cpc;                                   // staged plan: mesh cells per range (blockIdx.y); a range's tables span cpc + K columns
  const double* Pinv;                        // leave-one-out only (last: the held-out kernels never load it)
  const int* groups; int G; double* grad;    // weight gradient only: labels (or NULL), bins per workgroup = 2 G, per-row output
};

// slot 3 of a record.  LOO: NaN-sticky maximum (a leverage that is NaN must reach max h, whatever comes after it); held-out: sum
template <bool LOO>
__device__ __forceinline__ double fold3(double a, double b) {
  if constexpr (LOO) return (a != a) ? a : ((b != b) ? b : (a > b ? a : b));
  else return a + b;
}
template <bool LOO>
__device__ __forceinline__ double wave_fold3(double v) {
  if constexpr (LOO) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fold3<true>(v, __shfl_xor(v, off, 64));
    return v;
  } else {
    return wave_sum_dpp(v);
  }
}

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

enum { WG_OFF = 0, WG_RECORD = 1, WG_BINS = 2 };   // weight gradient: off, [n, T] through the records, 2 G bins per workgroup

constexpr int staged_threads(int K) { return K >= 5 ? 512 : 1024; }   // (leave-one-out orders 5 and 6 spill at 128 registers per lane)

template <int K, bool STAGE, bool LOO, int WG = WG_OFF>
__global__ __launch_bounds__(STAGE ? staged_threads(K) : 256) void row_kernel(const RowArgs a) {
  constexpr bool WGRAD = WG != WG_OFF;
  static_assert(LOO || !WGRAD, "the weight gradient reads the leave-one-out tables");
  extern __shared__ __attribute__((aligned(16))) double lds[];   // (the interleaved table is read 16 bytes at a time)
  constexpr int TAB = (LOO ? 2 : 1) * (K + 1);                   // doubles of the staged table per column
  const int M = a.M, D = a.D;
  // this workgroup's cells [cell0, cell1) and table columns [cell0, cell0 + cols); not staged: everything
  const int ncell = a.n_mesh - 1;
  const int cell0 = STAGE ? (int)blockIdx.y * a.cpc : 0;
  const int cell1 = STAGE ? (cell0 + a.cpc < ncell ? cell0 + a.cpc : ncell) : ncell;
  const int cols = STAGE ? a.cpc + K : M;
  // STAGE is a template parameter so that the table pointers are LDS pointers at compile time (see predict_kernel)
  [[maybe_unused]] const double2* T = reinterpret_cast<const double2*>(lds);   // LOO, staged: {W, P^-1}
  [[maybe_unused]] const double* W = STAGE ? lds : a.W;                         // held-out
  const double* alpha = STAGE ? lds + TAB * cols : a.alpha;
  const double* mesh = STAGE ? lds + TAB * cols + cols * D : a.mesh;
  double* scratch = STAGE ? lds + TAB * cols + cols * D + a.n_mesh : lds;
  if (STAGE) {
    double* ta = lds + TAB * cols;
    double* tm = ta + cols * D;
#pragma unroll
    for (int d = 0; d <= K; ++d)
      for (int c = threadIdx.x; c < cols; c += blockDim.x) {
        const int gc = cell0 + c;                              // (the last range may be short: columns past M - 1 are never read)
        if constexpr (LOO)
          reinterpret_cast<double2*>(lds)[d * cols + c] = gc < M ? make_double2(a.W[d * M + gc], a.Pinv[d * M + gc]) : make_double2(0.0, 0.0);
        else
          lds[d * cols + c] = gc < M ? a.W[d * M + gc] : 0.0;
      }
    for (int e = threadIdx.x; e < cols * D; e += blockDim.x) {
      const long ge = (long)cell0 * D + e;
      ta[e] = ge < (long)M * D ? a.alpha[ge] : 0.0;
    }
#pragma unroll 2
    for (int e = threadIdx.x; e < a.n_mesh; e += blockDim.x) tm[e] = a.mesh[e];
    __syncthreads();
  }
  // weight gradient with labels: 2 G bins [n_g, T_g] behind the record scratch, zeroed before the first row
  [[maybe_unused]] double* bins = scratch + SCRATCH;
  if constexpr (WG == WG_BINS) {
    for (int e = threadIdx.x; e < 2 * a.G; e += blockDim.x) bins[e] = 0.0;
    __syncthreads();
  }
  const double m0 = mesh[0];
  [[maybe_unused]] const double inv_noise = 1.0 / a.noise;
  const bool weighted = a.w != nullptr;
  double cnt = 0.0, sld = 0.0, ssq = 0.0, s3 = 0.0;
  const long stride = (long)gridDim.x * blockDim.x;
  long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  // (two rows in flight, loaded unconditionally at clamped indices as predict_poly_kernel does, were measured no faster: 126 - 130 us
  // against 122 - 123 us at N = 10M, M = 2048.  The table work bounds this kernel, not the latency of its loads: DESIGN.md 4.3d.)
  double xn = 0.0, wn = 1.0, yn = 0.0;
  [[maybe_unused]] int labn = 0;                               // bins: the row's label travels with x (loaded at its use, the loop waits on it and on the next row's x, w, y)
  if (p < a.N) { xn = a.x[p]; if (weighted) wn = a.w[p]; if (D == 1) yn = a.y[p]; }
  if constexpr (WG == WG_BINS) { if (p < a.N) labn = a.groups[p]; }
  for (; p < a.N; p += stride) {
    const double xv = xn, wv = wn, y0 = yn;
    [[maybe_unused]] const int lab = labn;
    const long pn = p + stride;
    if (pn < a.N) { xn = a.x[pn]; if (weighted) wn = a.w[pn]; if (D == 1) yn = a.y[pn]; }   // the next row in flight under the table work
    if constexpr (WG == WG_BINS) { if (pn < a.N) labn = a.groups[pn]; }
    const int idx = neighbour_index(xv, mesh, a.n_mesh, m0, a.inv_delta);
    if (STAGE && (idx < cell0 || idx >= cell1)) continue;      // another range's row
    const double t = (xv - mesh[idx]) * a.inv_delta;
    double v[K + 1];
    bspline_pieces<K>(t, v);
    const int c = idx - cell0;
    double q = 0.0;                                            // half of phi^T W phi
    [[maybe_unused]] double h = 0.0, om = 1.0;                 // LOO: leverage and 1 - h
    [[maybe_unused]] double gq = 0.0;                          // WGRAD: g = phi^T P^-1 phi
    double vout;                                               // the variance reported for the row
    if constexpr (LOO) {
      double qp;
      loo_windows<K, STAGE>(v, T, a.W, a.Pinv, c, cols, q, qp);
      const double var0 = fma(2.0, q, a.variance);             // ordinary posterior variance
      const double g = 2.0 * qp;
      if constexpr (WGRAD) {
        gq = g;
        vout = var0;
      } else {
        h = wv * g * inv_noise;
        om = 1.0 - h;
        vout = var0 + g * (h / om);
      }
    } else {                                                   // predict_point's walk: phi_i sits on row c + K - i
#pragma unroll
      for (int i = 0; i <= K; ++i) {
        double acc = 0.5 * v[i] * W[c + K - i];
#pragma unroll
        for (int j = i + 1; j <= K; ++j) acc = fma(v[j], W[(j - i) * cols + c + K - j], acc);
        q = fma(v[i], acc, q);
      }
      vout = fma(2.0, q, a.variance);
    }
    double sq = 0.0;
    const bool pos = wv > 0.0;
    if constexpr (WGRAD) {                                     // slots 0, 1 of the record: n, T = sum w grad
#pragma unroll 1
      for (int d = 0; d < D; ++d) {                            // (not unrolled: four outputs in flight spill at order 4's 128 registers)
        double mu = 0.0;
#pragma unroll
        for (int i = 0; i <= K; ++i) mu = fma(v[i], alpha[(long)(c + K - i) * D + d], mu);
        const double r = ((D == 1) ? y0 : a.y[p * D + d]) - mu;
        sq = fma(r, r, sq);
      }
      const double gr = pos ? 0.5 * ((double)D / wv - ((double)D * gq + sq + (vout - gq)) * inv_noise) : 0.0;
      if (a.grad) a.grad[p] = gr;
      if (pos) {
        if constexpr (WG == WG_BINS) {
          if ((unsigned)lab < (unsigned)a.G) { lds_add(bins + 2 * lab, 1.0); lds_add(bins + 2 * lab + 1, wv * gr); }
        } else {
          cnt += 1.0;
          sld = fma(wv, gr, sld);
        }
      }
    } else {
      for (int d = 0; d < D; ++d) {
        double mu = 0.0;
#pragma unroll
        for (int i = 0; i <= K; ++i) mu = fma(v[i], alpha[(long)(c + K - i) * D + d], mu);
        const double yv = (D == 1) ? y0 : a.y[p * D + d];
        double m = mu;
        if constexpr (LOO) m = (mu - h * yv) / om;
        if (a.mean) a.mean[p * D + d] = m;
        const double r = yv - m;
        sq = fma(r, r, sq);
      }
      const double s2 = vout + (pos ? a.noise / wv : a.noise);
      const double chi = sq / s2;
      const double ld = -0.5 * ((double)D * log(6.283185307179586 * s2) + chi);
      if (a.var) a.var[p] = vout;
      if (a.logdens) a.logdens[p] = ld;
      if (pos) { cnt += 1.0; sld += ld; ssq += sq; s3 = fold3<LOO>(s3, LOO ? h : chi); }
    }
  }
  if (!a.partials) return;
  if constexpr (WG == WG_BINS) {                               // this workgroup's bins: one row of the workspace
    __syncthreads();
    double* out = a.partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)(2 * a.G);
    for (int e = threadIdx.x; e < 2 * a.G; e += blockDim.x) out[e] = bins[e];
    return;
  }
  // fixed order: DPP sums inside the wavefront, the wavefronts of the workgroup in index order, the workgroups in scores_kernel
  cnt = wave_sum_dpp(cnt); sld = wave_sum_dpp(sld); ssq = wave_sum_dpp(ssq); s3 = wave_fold3<LOO>(s3);
  const int lane = threadIdx.x & 63, wf = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if (lane == 0) { double* r = scratch + wf * RECORD; r[0] = cnt; r[1] = sld; r[2] = ssq; r[3] = s3; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
    for (int q = 0; q < nw; ++q) {
      const double* r = scratch + q * RECORD;
      r0 += r[0]; r1 += r[1]; r2 += r[2]; r3 = fold3<LOO>(r3, r[3]);
    }
    double* out = a.partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * RECORD;
    out[0] = r0; out[1] = r1; out[2] = r2; out[3] = r3;
  }
}

// scores = the G workgroup records in a fixed order (one wavefront: lane l takes records l, l + 64, ... in turn)
// (NOUT = 2: the weight gradient's [n, T], which fills slots 0 and 1 only)
template <bool LOO, int NOUT = RECORD>
__global__ __launch_bounds__(64) void scores_kernel(const double* __restrict__ partials, int G, double* __restrict__ scores) {
  const int lane = threadIdx.x;
  double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
  for (int g = lane; g < G; g += 64) {
    const double* r = partials + (size_t)g * RECORD;
    r0 += r[0]; r1 += r[1]; r2 += r[2]; r3 = fold3<LOO>(r3, r[3]);
  }
  r0 = wave_sum_dpp(r0); r1 = wave_sum_dpp(r1); r2 = wave_sum_dpp(r2); r3 = wave_fold3<LOO>(r3);
  if (lane == 0) {
    scores[0] = r0; scores[1] = r1;
    if constexpr (NOUT > 2) { scores[2] = r2; scores[3] = r3; }
  }
}

// gsum = the workgroups' bin rows added in a fixed order.  A workgroup takes 64 consecutive bins (one lane each: a row is read 512
// contiguous bytes at a time); wavefront q adds rows q, q + 16, ... in workgroup order, eight loads in flight, then wavefront 0 adds the
// sixteen slices in index order.  (One thread per bin over all rows in turn took one memory latency per row: 160 us for 512 rows.)
constexpr int SUM_SLICES = 16;
__global__ __launch_bounds__(64 * SUM_SLICES) void group_sums_kernel(const double* __restrict__ partials, int rows, int nbin, double* __restrict__ gsum) {
  __shared__ double slice[SUM_SLICES][64];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane;
  double t = 0.0;
  if (j < nbin) {
#pragma unroll 8
    for (int r = q; r < rows; r += SUM_SLICES) t += partials[(size_t)r * nbin + j];
  }
  slice[q][lane] = t;
  __syncthreads();
  if (q == 0 && j < nbin) {
    double tot = 0.0;
#pragma unroll
    for (int i = 0; i < SUM_SLICES; ++i) tot += slice[i][lane];
    gsum[j] = tot;
  }
}

template <int K, bool LOO, int WG = WG_OFF>
static int launch(RowArgs a, double* scores, hipStream_t st, const char* name) {
  // staged plan: the fewest cell ranges whose tables fit the LDS, while every workgroup keeps a record of its own in the workspace
  constexpr int ST = staged_threads(K);
  constexpr int max_ranges = MAX_BLOCKS / (int)(WRAP_N / ST);
  constexpr int bands = LOO ? 2 : 1;
  const int ncell = a.n_mesh - 1;
  int ranges = 0;
  size_t staged_bytes = 0;
  const size_t bins = WG == WG_BINS ? 2 * (size_t)a.G : 0;     // doubles behind the scratch: part of the LDS budget
  if (a.N >= STAGE_MIN_N)
    for (int c = 1; c <= max_ranges && c <= ncell && !ranges; ++c) {
      const int cpc = (ncell + c - 1) / c;
      const size_t cols = (size_t)cpc + K;
      staged_bytes = sizeof(double) * (bands * (K + 1) * cols + cols * (size_t)a.D + (size_t)a.n_mesh + SCRATCH + bins);
      if (staged_bytes <= LDS_BUDGET) { ranges = c; a.cpc = cpc; }
    }
  const bool stage = ranges > 0;
  const int threads = stage ? ST : 256;
  long blocks = (a.N + threads - 1) / threads;
  if (blocks > WRAP_N / threads) blocks = WRAP_N / threads;
  static_assert(WRAP_N / 256 <= MAX_BLOCKS && max_ranges >= 1, "one record per workgroup");
  const size_t lds_bytes = stage ? staged_bytes : sizeof(double) * (SCRATCH + bins);
  auto kern = stage ? row_kernel<K, true, LOO, WG> : row_kernel<K, false, LOO, WG>;
  if (stage) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) { set_error("%s: hipFuncSetAttribute(%zu B LDS): %s", name, lds_bytes, hipGetErrorString(e)); return ASVGP_ERR_LDS_CAPACITY; }
  }
  const int gy = stage ? ranges : 1;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)gy), dim3(threads), lds_bytes, st, a);
  if constexpr (WG == WG_BINS) {
    hipLaunchKernelGGL(group_sums_kernel, dim3((unsigned)((bins + 63) / 64)), dim3(64 * SUM_SLICES), 0, st, a.partials, (int)blocks * gy, (int)bins, scores);
  } else if constexpr (WG == WG_RECORD) {
    if (scores) hipLaunchKernelGGL((scores_kernel<false, 2>), dim3(1), dim3(64), 0, st, a.partials, (int)blocks * gy, scores);
  } else {
    if (scores) hipLaunchKernelGGL(scores_kernel<LOO>, dim3(1), dim3(64), 0, st, a.partials, (int)blocks * gy, scores);
  }
  return check_launch(name);
}

static size_t workspace_bytes_of(int64_t M, int order, int64_t D) {
  if (M < 1 || order < 1 || order > ASVGP_MAX_ORDER || D < 1) return 0;
  return sizeof(double) * (size_t)MAX_BLOCKS * RECORD;
}

// the argument checks that every entry point shares (Pinv: required by the leave-one-out tables, NULL for the held-out entry)
static int check_row_args(const char* name, const double* x, const double* y, int64_t N, int64_t D, const double* mesh, int64_t n_mesh,
                          double delta, int order, int64_t M, const double* alpha, const double* W, bool need_pinv, const double* Pinv,
                          double variance, double noise_variance, bool any_output, const char* outputs) {
  if (((!x || !y) && N > 0) || !mesh || !alpha || !W || (need_pinv && !Pinv) || N < 0 || D < 1 || M < 1 || !(delta > 0.0) || !(variance > 0.0) ||
      !(noise_variance > 0.0)) {
    set_error("%s: bad argument", name);
    return ASVGP_ERR_BAD_ARG;
  }
  if (!any_output) { set_error("%s: bad argument (no output asked for: %s are all NULL)", name, outputs); return ASVGP_ERR_BAD_ARG; }
  if (order < 1 || order > ASVGP_MAX_ORDER) { set_error("%s: order %d unsupported", name, order); return ASVGP_ERR_UNSUPPORTED; }
  if (n_mesh != M - order + 1 || n_mesh < 2) { set_error("%s: bad argument (n_mesh = %ld, M = %ld, order %d)", name, (long)n_mesh, (long)M, order); return ASVGP_ERR_BAD_ARG; }
  if (M > 0x0fffffff || D > 0x0fffffff || M * D > 0x3fffffff) { set_error("%s: M = %ld, D = %ld too large", name, (long)M, (long)D); return ASVGP_ERR_UNSUPPORTED; }
  return ASVGP_OK;
}

// argument checks, the empty batch and the order switch of both score entry points; name = "loo_1d" (Pinv required) or "score_1d" (Pinv = NULL)
template <bool LOO>
static int row_scores(const char* name, const double* x, const double* y, const double* w, int64_t N, int64_t D, const double* mesh,
                      int64_t n_mesh, double delta, int order, int64_t M, const double* alpha, const double* W, const double* Pinv,
                      double variance, double noise_variance, double* mean, double* var, double* logdens, double* scores, void* workspace,
                      size_t workspace_bytes, asvgp_stream_t stream) {
  if (const int rc = check_row_args(name, x, y, N, D, mesh, n_mesh, delta, order, M, alpha, W, LOO, Pinv, variance, noise_variance,
                                    mean || var || logdens || scores, "mean, var, logdens and scores"))
    return rc;
  if (!workspace || workspace_bytes < workspace_bytes_of(M, order, D)) {
    set_error("%s: workspace too small (%zu < %zu)", name, workspace_bytes, workspace_bytes_of(M, order, D));
    return ASVGP_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  if (N == 0) {     // nothing to stream: no launch, the scores of an empty set
    if (scores) {
      hipError_t e = hipMemsetAsync(scores, 0, sizeof(double) * RECORD, st);
      if (e != hipSuccess) { set_error("%s: hipMemsetAsync: %s", name, hipGetErrorString(e)); return ASVGP_ERR_HIP; }
    }
    return ASVGP_OK;
  }
  RowArgs a{x, y, w, (long)N, (int)D, mesh, (int)n_mesh, 1.0 / delta, (int)M, alpha, W, variance, noise_variance,
            mean, var, logdens, scores ? static_cast<double*>(workspace) : nullptr, 0, Pinv};
  switch (order) {
    case 1: return launch<1, LOO>(a, scores, st, name);
    case 2: return launch<2, LOO>(a, scores, st, name);
    case 3: return launch<3, LOO>(a, scores, st, name);
    case 4: return launch<4, LOO>(a, scores, st, name);
    case 5: return launch<5, LOO>(a, scores, st, name);
    default: return launch<6, LOO>(a, scores, st, name);
  }
}

constexpr int64_t MAX_GROUPS = 1024;         // 2 G bins of 8 bytes per workgroup: 16 KiB of the LDS budget at most

static size_t weight_grad_workspace_bytes_of(int64_t M, int order, int64_t D, int64_t G) {
  if (workspace_bytes_of(M, order, D) == 0 || G < 1 || G > MAX_GROUPS) return 0;
  return sizeof(double) * (size_t)MAX_BLOCKS * (size_t)(2 * G > RECORD ? 2 * G : RECORD);   // a record or a row of 2 G bins per workgroup
}

static int weight_grad(const double* x, const double* y, const double* w, int64_t N, int64_t D, const double* mesh, int64_t n_mesh,
                       double delta, int order, int64_t M, const double* alpha, const double* W, const double* Pinv, double variance,
                       double noise_variance, const int32_t* groups, int64_t G, double* grad, double* gsum, void* workspace,
                       size_t workspace_bytes, asvgp_stream_t stream) {
  const char* name = "weight_grad_1d";
  if (const int rc = check_row_args(name, x, y, N, D, mesh, n_mesh, delta, order, M, alpha, W, true, Pinv, variance, noise_variance,
                                    grad || gsum, "grad and gsum"))
    return rc;
  if (G < 1 || (!groups && G != 1)) { set_error("%s: bad argument (G = %ld%s)", name, (long)G, groups ? "" : ", groups = NULL takes G = 1"); return ASVGP_ERR_BAD_ARG; }
  if (G > MAX_GROUPS) { set_error("%s: G = %ld groups unsupported (at most %ld)", name, (long)G, (long)MAX_GROUPS); return ASVGP_ERR_UNSUPPORTED; }
  if (!workspace || workspace_bytes < weight_grad_workspace_bytes_of(M, order, D, G)) {
    set_error("%s: workspace too small (%zu < %zu)", name, workspace_bytes, weight_grad_workspace_bytes_of(M, order, D, G));
    return ASVGP_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  if (N == 0) {     // nothing to stream: no launch, the sums of an empty set
    if (gsum) {
      hipError_t e = hipMemsetAsync(gsum, 0, sizeof(double) * 2 * (size_t)G, st);
      if (e != hipSuccess) { set_error("%s: hipMemsetAsync: %s", name, hipGetErrorString(e)); return ASVGP_ERR_HIP; }
    }
    return ASVGP_OK;
  }
  RowArgs a{x, y, w, (long)N, (int)D, mesh, (int)n_mesh, 1.0 / delta, (int)M, alpha, W, variance, noise_variance,
            nullptr, nullptr, nullptr, gsum ? static_cast<double*>(workspace) : nullptr, 0, Pinv, gsum ? groups : nullptr, (int)G, grad};
  if (a.groups) switch (order) {                 // (labels without gsum have nothing to fill: a.groups is NULL then)
    case 1: return launch<1, true, WG_BINS>(a, gsum, st, name);
    case 2: return launch<2, true, WG_BINS>(a, gsum, st, name);
    case 3: return launch<3, true, WG_BINS>(a, gsum, st, name);
    case 4: return launch<4, true, WG_BINS>(a, gsum, st, name);
    case 5: return launch<5, true, WG_BINS>(a, gsum, st, name);
    default: return launch<6, true, WG_BINS>(a, gsum, st, name);
  }
  switch (order) {
    case 1: return launch<1, true, WG_RECORD>(a, gsum, st, name);
    case 2: return launch<2, true, WG_RECORD>(a, gsum, st, name);
    case 3: return launch<3, true, WG_RECORD>(a, gsum, st, name);
    case 4: return launch<4, true, WG_RECORD>(a, gsum, st, name);
    case 5: return launch<5, true, WG_RECORD>(a, gsum, st, name);
    default: return launch<6, true, WG_RECORD>(a, gsum, st, name);
  }
}

}  // namespace asvgp

using namespace asvgp;

extern "C" size_t asvgp_loo_workspace_bytes(int64_t M, int order, int64_t D) { return workspace_bytes_of(M, order, D); }
extern "C" size_t asvgp_score_workspace_bytes(int64_t M, int order, int64_t D) { return workspace_bytes_of(M, order, D); }

// handle: accepted like asvgp_predict_deriv_1d's (NULL = the process default): the kernels keep no per-handle state
extern "C" int asvgp_loo_1d(asvgp_handle_t, const double* x, const double* y, const double* w, int64_t N, int64_t D, const double* mesh,
                            int64_t n_mesh, double delta, int order, int64_t M, const double* alpha, const double* W, const double* Pinv_band,
                            double variance, double noise_variance, double* mean, double* var, double* logdens, double* scores,
                            void* workspace, size_t workspace_bytes, asvgp_stream_t stream) {
  return row_scores<true>("loo_1d", x, y, w, N, D, mesh, n_mesh, delta, order, M, alpha, W, Pinv_band, variance, noise_variance, mean, var,
                          logdens, scores, workspace, workspace_bytes, stream);
}

extern "C" int asvgp_score_1d(asvgp_handle_t, const double* x, const double* y, const double* w, int64_t N, int64_t D, const double* mesh,
                              int64_t n_mesh, double delta, int order, int64_t M, const double* alpha, const double* W, double variance,
                              double noise_variance, double* mean, double* var, double* logdens, double* scores, void* workspace,
                              size_t workspace_bytes, asvgp_stream_t stream) {
  return row_scores<false>("score_1d", x, y, w, N, D, mesh, n_mesh, delta, order, M, alpha, W, nullptr, variance, noise_variance, mean, var,
                           logdens, scores, workspace, workspace_bytes, stream);
}

extern "C" size_t asvgp_weight_grad_workspace_bytes(int64_t M, int order, int64_t D, int64_t G) {
  return weight_grad_workspace_bytes_of(M, order, D, G);
}

extern "C" int asvgp_weight_grad_1d(asvgp_handle_t, const double* x, const double* y, const double* w, int64_t N, int64_t D,
                                    const double* mesh, int64_t n_mesh, double delta, int order, int64_t M, const double* alpha,
                                    const double* W, const double* Pinv_band, double variance, double noise_variance, const int32_t* groups,
                                    int64_t G, double* grad, double* gsum, void* workspace, size_t workspace_bytes, asvgp_stream_t stream) {
  return weight_grad(x, y, w, N, D, mesh, n_mesh, delta, order, M, alpha, W, Pinv_band, variance, noise_variance, groups, G, grad, gsum,
                     workspace, workspace_bytes, stream);
}
