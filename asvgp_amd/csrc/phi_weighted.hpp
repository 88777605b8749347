// Weighted Phi pass: the banded sufficient statistics of observations with per-row noise variance s / w_i,
//   A_w = Phi W Phi^T,  b_w = Phi W y,  yy_w = sum w_i y_i^2,   wstats = [sum w, sum_{w>0} log w, #{w > 0}].
// (included by phi_pass.hip behind the unweighted kernels, whose code it does not touch; it shares phi_reduce_kernel and the packed
// [band | Phi y | y^T y] layout, so every consumer of `stats` is served as it is.)
//
// Two kernels; 0 = auto takes the register-moment kernel (phi_sort_weighted.hpp, asvgp_phi_last_algorithm = 16) where it applies - D = 1,
// N >= 2, M <= 2048, 16-byte aligned x / y / w, a mesh that is an exact linspace - and the general kernel otherwise.
// General kernel (asvgp_phi_last_algorithm = 11): the fp64 band scatter of phi_accumulate_kernel with a weight.  Each point's k+1 pieces
// are scaled by w once (u_i = w v_i), the products u_i v_j and u_i y go into the workgroup's LDS image with ds_add_f64; a wavefront whose
// 64 points share one cell (sorted input, where 64 same-address atomics would serialise) sums them on the VALU and commits once.  Any
// order, any M (column chunks), D >= 1, any alignment, float32-linspace meshes: one scalar load per array and point, no vector path.
// The fixed-point images of algorithms 3 and 5 have no weighted form: their scales are compile-time bounds on the products, which w breaks.
//
// HBM: 24 B/point (x, y, w read once, fp64).  A row with w = 0 is absent: it reaches nothing, the row count included.  A negative, NaN
// or infinite weight is reported the way a point outside the mesh is: yy_w = NaN.
#pragma once
#include "phi_sort_weighted.hpp"

namespace asvgp {

constexpr int PW_THREADS = 1024;
constexpr int PW_WCOLS = 4;   // per-workgroup record of the weight sums: [sum w, sum log w, n_pos, unused]

template <int K>
__global__ __launch_bounds__(PW_THREADS) void phi_weighted_kernel(
    const double* __restrict__ x, const double* __restrict__ y, long y_stride, const double* __restrict__ w, long N,
    const double* __restrict__ mesh_g, int n_mesh, double inv_delta, int cell0, int cell1, int ncols, int do_band,
    double* __restrict__ partials, double* __restrict__ wpart, long ppb, double* __restrict__ zero_ptr, long zero_n) {
  extern __shared__ double lds[];
  if (zero_ptr) for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < zero_n; e += (long)gridDim.x * blockDim.x) zero_ptr[e] = 0.0;
  double* band = lds;                      // (K+1) x ncols
  double* rhs = band + (K + 1) * ncols;    // ncols
  double* mesh = rhs + ncols;              // n_mesh
  double* scratch = mesh + n_mesh;         // 16
  const int tid = threadIdx.x, lane = tid & 63;
  const int E = (K + 2) * ncols;
  for (int e = tid; e < E; e += PW_THREADS) lds[e] = 0.0;
  for (int e = tid; e < n_mesh; e += PW_THREADS) mesh[e] = mesh_g[e];
  __syncthreads();
  const double m0 = mesh[0];
  const long beg = (long)blockIdx.x * ppb;
  long end = beg + ppb;
  if (end > N) end = N;
  double yy = 0.0, sw = 0.0, sl = 0.0, np = 0.0;
  // whole wavefronts enter every iteration (the votes and DPP sums below are wave-wide): the bound is on the wave's first point
  for (long base = beg + (tid - lane); base < end; base += PW_THREADS) {
    const long i = base + lane;
    const bool have = i < end;
    const double xv = have ? x[i] : 0.0, wv = have ? w[i] : 0.0, yv = have ? y[i * y_stride] : 0.0;
    const bool wok = wv >= 0.0 && wv < __builtin_inf();             // (NaN fails both)
    yy = wok ? yy : __builtin_nan("");
    const bool live = have && wok && wv > 0.0;
    const int idx = live ? neighbour_index(xv, mesh, n_mesh, m0, inv_delta) : 0;
    const double t = live ? (xv - mesh[idx]) * inv_delta : 0.5;
    const bool inside = t >= -0.02 && t <= 1.02;                    // (as classify(): 2 % for the wobble of float32-linspace meshes; NaN fails)
    yy = inside ? yy : __builtin_nan("");
    const bool in = live && inside && idx >= cell0 && idx < cell1;
    const int idx0 = __builtin_amdgcn_readfirstlane(idx);
    const bool uniform = __all(in && idx == idx0);
    double v[K + 1], u[K + 1];
    bspline_pieces<K>(t, v);
    const double wy = wv * yv;
#pragma unroll
    for (int a = 0; a <= K; ++a) u[a] = wv * v[a];                   // u_a = w v_a, once per point: the products below are u_a v_b and u_a y
    if (in) {
      yy = fma(wy, yv, yy);
      if (do_band) { sw += wv; sl += log(wv); np += 1.0; }           // (first output column only; every point lies in one column chunk)
    }
    if (uniform) {
      const int cb = idx0 - cell0;
#pragma unroll
      for (int a = 0; a <= K; ++a) {
        const double r = wave_sum_dpp(u[a] * yv);
        if (lane == 0) lds_add(rhs + cb + K - a, r);
        if (do_band) {
#pragma unroll
          for (int b = a; b <= K; ++b) {
            const double p = wave_sum_dpp(u[a] * v[b]);
            if (lane == 0) lds_add(band + (b - a) * ncols + cb + K - b, p);
          }
        }
      }
    } else if (in) {
      const int cb = idx - cell0;
#pragma unroll
      for (int a = 0; a <= K; ++a) {
        lds_add(rhs + cb + K - a, u[a] * yv);
        if (do_band) {
#pragma unroll
          for (int b = a; b <= K; ++b) lds_add(band + (b - a) * ncols + cb + K - b, u[a] * v[b]);   // rows idx+K-a >= idx+K-b: sub-diagonal b-a, column of row b
        }
      }
    }
  }
  const double tot = block_sum(yy, scratch);   // (its barriers order the LDS atomics before the flush)
  const double tw = block_sum(sw, scratch), tl = block_sum(sl, scratch), tn = block_sum(np, scratch);
  __syncthreads();
  double* out = partials + (size_t)blockIdx.x * (E + 1);
  for (int e = tid; e < E; e += PW_THREADS) out[e] = lds[e];
  if (tid == 0) {
    out[E] = tot;
    if (do_band) { double* wp = wpart + (size_t)blockIdx.x * PW_WCOLS; wp[0] = tw; wp[1] = tl; wp[2] = tn; wp[3] = 0.0; }
  }
}

// wstats[c] (+)= sum over the G workgroups' records, in a fixed order (one wavefront; bit-reproducible for a given launch shape).
// first = 0: a later column chunk of the same pass adds its rows' share.
__global__ __launch_bounds__(64) void phi_wstats_accumulate_kernel(const double* __restrict__ wpart, int G, double* __restrict__ wstats, int first) {
  const int lane = threadIdx.x;
  double a[3] = {0.0, 0.0, 0.0};
  for (int g = lane; g < G; g += 64)
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] += wpart[(size_t)g * PW_WCOLS + c];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double s = wave_sum_dpp(a[c]);
    if (lane == 0) wstats[c] = first ? s : wstats[c] + s;
  }
}

// 256 partial images, 256 records of the weight sums, 256 column ranges (2 ints) of the register-moment kernel
static size_t phi_weighted_ws_doubles(long M, int order) { return (size_t)PHI_MAX_BLOCKS * ((size_t)(order + 2) * (size_t)M + 1) + (size_t)PHI_MAX_BLOCKS * (PW_WCOLS + 1); }

// Register-moment kernel.  Returns 1 when it does not apply (the conditions of launch_phi_sort, with w) and the caller takes the general kernel.
template <int K>
static int launch_phi_sort_weighted(Handle* h, const double* x, const double* y, const double* w, long N, long D, const double* mesh, long n_mesh,
                                    double delta, long M, double* stats, double* wstats, double* ws, hipStream_t st) {
  if (D != 1 || N < 2 || M > PS_NCELL ||
      ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(w)) & 15) != 0) return 1;
  double step = 0.0, m0 = 0.0, m_last = 0.0;
  if (!handle_mesh_is_linspace(h, mesh, n_mesh, st, &step, &m0, &m_last)) return 1;
  const double amax = fabs(m0) > fabs(m_last) ? fabs(m0) : fabs(m_last);
  const double margin = 16.0 * 2.220446049250313e-16 * amax / delta + 1e-12;   // knot rounding over delta (as launch_phi_sort)
  if (!(margin < 0.125)) return 1;
  constexpr int TP = psw_tile_points<K>();
  // (k = 4: 160 248 of 163 840 bytes.  A table that grows past the LDS must fail the build, not quietly hand the measured shape to kernel 11.)
  static_assert(psw_lds_bytes<K, TP>() <= 160 * 1024 && ps_epilogue_bytes<K>() <= 160 * 1024, "weighted register-moment kernel: LDS plan exceeds 160 KB");
  size_t lds_bytes = psw_lds_bytes<K, TP>();
  if (ps_epilogue_bytes<K>() > lds_bytes) lds_bytes = ps_epilogue_bytes<K>();
  const long nblk = (N + TP * PS_THREADS - 1) / (TP * PS_THREADS);   // at least one tile per workgroup
  const long gmax = (h->phi_blocks > 0 && h->phi_blocks < PHI_MAX_BLOCKS) ? h->phi_blocks : PHI_MAX_BLOCKS;
  const int G = (int)(nblk < 1 ? 1 : (nblk > gmax ? gmax : nblk));
  long ppb = (N + G - 1) / G;
  ppb = (ppb + 1) & ~1L;
  if (ppb > 0x3fffffffL) return 1;                                   // (32-bit pair indices inside a workgroup)
  PswArgs aw;
  PsArgs& a = aw.p;
  a.x = x; a.y = y; a.N = N; a.mesh_g = mesh; a.n_mesh = (int)n_mesh; a.inv_delta = 1.0 / delta; a.M = (int)M;
  a.m0 = m0; a.m_last = m_last; a.step = step; a.smax_fast = 0.5 - margin;
  a.partials = ws; a.ppb = ppb; a.zero_ptr = stats; a.zero_n = (K + 2) * M + 1; a.stamps = nullptr; a.stamps_wave = 0;
  aw.w = w;
  aw.wpart = ws + (size_t)PHI_MAX_BLOCKS * ((size_t)(K + 2) * (size_t)M + 1);
  a.ranges = reinterpret_cast<int*>(aw.wpart + (size_t)PHI_MAX_BLOCKS * PW_WCOLS);   // (2 ints per workgroup: the fourth column's room and more - see phi_weighted_ws_doubles)
  auto kern = phi_sort_weighted_kernel<K, TP>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) { set_error("hipFuncSetAttribute(%zu B LDS): %s", lds_bytes, hipGetErrorString(e)); return ASVGP_ERR_LDS_CAPACITY; }
  const bool prof = h->prof_on && h->prof_n < PROF_RING && (h->prof_calls++ % h->prof_every == 0);
  if (prof) (void)hipEventRecord(h->prof_ev[h->prof_n][0], st);
  hipLaunchKernelGGL(kern, dim3((unsigned)G), dim3(PS_THREADS), lds_bytes, st, aw);
  if (prof) { (void)hipEventRecord(h->prof_ev[h->prof_n][1], st); ++h->prof_n; }
  const int E1 = (int)((K + 2) * M + 1);
  const int gsplit = G >= 64 ? 16 : (G >= 8 ? 4 : 1);
  hipLaunchKernelGGL(phi_reduce_kernel, dim3((E1 + 255) / 256, gsplit), dim3(256), 0, st, a.partials, G, (int)M, K, 0, M, 1L, 0, 1, stats, (const int*)a.ranges);
  hipLaunchKernelGGL(phi_wstats_accumulate_kernel, dim3(1), dim3(64), 0, st, aw.wpart, G, wstats, 1);
  return check_launch("phi_accumulate_1d_weighted (register moments)");
}

template <int K>
static int launch_phi_weighted(Handle* h, const double* x, const double* y, const double* w, long N, long D, const double* mesh, long n_mesh,
                               double delta, long M, double* stats, double* wstats, double* partials, hipStream_t st) {
  { const int rcf = handle_flush_phi_reduce(h, nullptr, st); if (rcf) return rcf; }   // (a reduce parked on this workspace goes out first)
  if (h->phi_algo == 3 || h->phi_algo == 5) {
    set_error("phi_accumulate_1d_weighted: phi algorithm %d accumulates in fixed point, whose scales are bounds on the unweighted products - it has no weighted form (0 or 1)", h->phi_algo);
    return ASVGP_ERR_UNSUPPORTED;
  }
  if (h->phi_algo == 0 || h->phi_algo == 6) {
    const int rc = launch_phi_sort_weighted<K>(h, x, y, w, N, D, mesh, n_mesh, delta, M, stats, wstats, partials, st);
    if (rc != 1) { h->phi_last = 16; return rc; }
    if (h->phi_algo == 6) { set_error("phi_accumulate_1d_weighted: phi algorithm 6 (register moments) needs D == 1, N >= 2, M <= 2048, 16-byte aligned x / y / w and a mesh that is an exact linspace"); return ASVGP_ERR_UNSUPPORTED; }
  }
  h->phi_last = 11;
  const int ncells = (int)n_mesh - 1;
  const int maxc = phi_max_cols(K, n_mesh, false);
  if (maxc < 2 * K + 2) {
    set_error("phi_accumulate_1d_weighted: mesh table (%ld knots) leaves no LDS for the band", n_mesh);
    return ASVGP_ERR_LDS_CAPACITY;
  }
  const int cells_per_chunk = (M <= maxc) ? ncells : (maxc - K);
  const long nblk = (N + PW_THREADS - 1) / PW_THREADS;
  const long gmax = (h->phi_blocks > 0 && h->phi_blocks < PHI_MAX_BLOCKS) ? h->phi_blocks : PHI_MAX_BLOCKS;
  const int G = (int)(nblk < 1 ? 1 : (nblk > gmax ? gmax : nblk));
  long ppb = (N + G - 1) / G;
  ppb = ((ppb + 63) / 64) * 64;
  double* wpart = partials + (size_t)PHI_MAX_BLOCKS * ((size_t)(K + 2) * (size_t)M + 1);
  const long zero_n = (K + 1) * M + M * D + 1;
  bool zeroed = false;   // the first launched kernel zeroes the stats buffer
  for (long dcol = 0; dcol < D; ++dcol) {
    for (int cell0 = 0; cell0 < ncells; cell0 += cells_per_chunk) {
      int cell1 = cell0 + cells_per_chunk;
      if (cell1 > ncells) cell1 = ncells;
      const int ncols = cell1 - cell0 + K;
      const size_t lds_bytes = sizeof(double) * ((size_t)(K + 2) * ncols + n_mesh + 16);
      const int do_band = (dcol == 0);
      auto kern = phi_weighted_kernel<K>;
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
      if (e != hipSuccess) { set_error("hipFuncSetAttribute(%zu B LDS): %s", lds_bytes, hipGetErrorString(e)); return ASVGP_ERR_LDS_CAPACITY; }
      const bool prof = h->prof_on && h->prof_n < PROF_RING && (h->prof_calls++ % h->prof_every == 0);
      if (prof) (void)hipEventRecord(h->prof_ev[h->prof_n][0], st);
      // (the weight sums: every chunk of the first output column writes its share of the rows; summed behind each of those launches)
      hipLaunchKernelGGL(kern, dim3(G), dim3(PW_THREADS), lds_bytes, st, x, y + dcol, (long)D, w, N, mesh, (int)n_mesh, 1.0 / delta, cell0, cell1,
                         ncols, do_band, partials, wpart, ppb, zeroed ? (double*)nullptr : stats, zero_n);
      if (prof) { (void)hipEventRecord(h->prof_ev[h->prof_n][1], st); ++h->prof_n; }
      const int E1 = (K + 2) * ncols + 1;
      const int gsplit = G >= 64 ? 16 : (G >= 8 ? 4 : 1);
      hipLaunchKernelGGL(phi_reduce_kernel, dim3((E1 + 255) / 256, gsplit), dim3(256), 0, st, partials, G, ncols, K, cell0, M, D, (int)dcol, do_band, stats,
                         (const int*)nullptr);
      if (do_band) hipLaunchKernelGGL(phi_wstats_accumulate_kernel, dim3(1), dim3(64), 0, st, wpart, G, wstats, zeroed ? 0 : 1);
      zeroed = true;
    }
  }
  return check_launch("phi_accumulate_1d_weighted");
}

}  // namespace asvgp

using namespace asvgp;

extern "C" size_t asvgp_phi_weighted_workspace_bytes(int64_t M, int order, int64_t D) {
  (void)D;
  if (M <= 0 || order < 1 || order > ASVGP_MAX_ORDER) return 0;
  const size_t own = sizeof(double) * phi_weighted_ws_doubles((long)M, order);
  const size_t base = asvgp_phi_workspace_bytes(M, order, D);   // (never less: a model keeps ONE workspace for both entries)
  return own > base ? own : base;
}

extern "C" int asvgp_phi_accumulate_1d_weighted(asvgp_handle_t handle, const double* x, const double* y, const double* w, int64_t N, int64_t D,
                                                const double* mesh, int64_t n_mesh, double delta, int order, int64_t M, double* stats,
                                                double* wstats, void* workspace, size_t workspace_bytes, asvgp_stream_t stream) {
  if (((!x || !y || !w) && N > 0) || !mesh || !stats || !wstats || N < 0 || D < 1 || M < 1 || !(delta > 0.0)) {
    set_error("phi_accumulate_1d_weighted: bad argument");
    return ASVGP_ERR_BAD_ARG;
  }
  if (order < 1 || order > ASVGP_MAX_ORDER) { set_error("phi_accumulate_1d_weighted: order %d unsupported", order); return ASVGP_ERR_UNSUPPORTED; }
  if (n_mesh != M - order + 1 || n_mesh < 2) { set_error("phi_accumulate_1d_weighted: n_mesh=%ld != M-order+1", (long)n_mesh); return ASVGP_ERR_BAD_ARG; }
  if (M > 0x3fffffff) { set_error("phi_accumulate_1d_weighted: M too large"); return ASVGP_ERR_UNSUPPORTED; }
  if (!workspace || workspace_bytes < asvgp_phi_weighted_workspace_bytes(M, order, D)) {
    set_error("phi_accumulate_1d_weighted: workspace too small (%zu < %zu)", workspace_bytes, asvgp_phi_weighted_workspace_bytes(M, order, D));
    return ASVGP_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  Handle* h = as_handle(handle);
  double* part = static_cast<double*>(workspace);
  switch (order) {
    case 1: return launch_phi_weighted<1>(h, x, y, w, N, D, mesh, n_mesh, delta, M, stats, wstats, part, st);
    case 2: return launch_phi_weighted<2>(h, x, y, w, N, D, mesh, n_mesh, delta, M, stats, wstats, part, st);
    case 3: return launch_phi_weighted<3>(h, x, y, w, N, D, mesh, n_mesh, delta, M, stats, wstats, part, st);
    case 4: return launch_phi_weighted<4>(h, x, y, w, N, D, mesh, n_mesh, delta, M, stats, wstats, part, st);
    case 5: return launch_phi_weighted<5>(h, x, y, w, N, D, mesh, n_mesh, delta, M, stats, wstats, part, st);
    default: return launch_phi_weighted<6>(h, x, y, w, N, D, mesh, n_mesh, delta, M, stats, wstats, part, st);
  }
}
