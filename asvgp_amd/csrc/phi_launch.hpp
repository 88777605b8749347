// Host side of the 1-D Phi pass (asvgp_phi_accumulate_1d, asvgp_phi_accumulate_1d_weighted): which kernel one call launches and in what
// shape, decided from integers and doubles alone BEFORE anything happens, then one straight-line launcher per kernel family.
// (included by phi_pass.hip behind every kernel of the pass: phi_pass.hip, phi_moments.hpp, phi_sort.hpp, phi_sort_weighted.hpp and
// phi_weighted.hpp hold kernels only.)
//
// An entry is: check_phi_args -> flush a reduce still parked on the handle -> plan_phi -> gather the one fact the plan asks for (is the
// mesh an exact linspace: handle_mesh_is_linspace; is x a time series: handle_phi_is_series) and plan again -> refuse, or hand the plan to
// launch_phi_tile_sort | launch_phi_moments | launch_phi_band.  The launchers decide nothing.  asvgp_phi_launch_plan_host shows the same
// plan_phi to the CPU tests.
#pragma once
#include <type_traits>

namespace asvgp {

constexpr size_t PHI_LDS_MAX = 160 * 1024;    // what a workgroup of the tile-sort kernels may ask for (PHI_LDS_BUDGET: the scatter kernels)

// ---- shared rules: each is written here and nowhere else ----------------------------------------------------------------------
// G workgroups of at least `unit` points each - at most the handle's count (asvgp_set_phi_workgroups), else one per CU -, every one
// takes `ppb` consecutive points, a multiple of `round`
struct PhiGrid { int G; long ppb; };
static PhiGrid phi_grid(long N, int blocks, long unit, long round) {
  const long nblk = (N + unit - 1) / unit;
  const long gmax = (blocks > 0 && blocks < PHI_MAX_BLOCKS) ? blocks : PHI_MAX_BLOCKS;
  const int G = (int)(nblk < 1 ? 1 : (nblk > gmax ? gmax : nblk));
  return PhiGrid{G, ((N + G - 1) / G + round - 1) / round * round};
}

// fixed-point exponent: 62 - ceil(log2(points per workgroup)), at most 50 (magic-constant conversion range)
static int phi_s0(long ppb) {
  int lg = 1;
  for (long c = 2; c < ppb; c <<= 1) ++lg;
  return 62 - lg < 50 ? 62 - lg : 50;
}

// columns a band-scatter workgroup holds beside the mesh table, and the LDS of one chunk of ncols columns
static int phi_max_cols(int K, long n_mesh, bool fx) {
  long avail = (long)PHI_LDS_BUDGET - (long)n_mesh * 8 - 16 * 8;
  if (avail <= 0) return 0;
  return (int)(avail / (8 * (K + 2 + (fx ? 1 : 0))));
}
static size_t phi_band_lds_bytes(int K, bool fx, int ncols, long n_mesh) { return sizeof(double) * ((size_t)(K + 2 + (fx ? 1 : 0)) * ncols + n_mesh + 16); }

// the cross-workgroup reduce: grid = (ceil(((K + 2) ncols + 1) / 256), slices of the G partials)
static int phi_reduce_split(int G) { return G >= 64 ? 16 : (G >= 8 ? 4 : 1); }
static void enqueue_phi_reduce(hipStream_t st, const double* partials, int G, int ncols, int K, int cell0, long M, long D, int dcol, int do_band,
                               double* stats, const int* ranges) {
  const int E1 = (K + 2) * ncols + 1;
  hipLaunchKernelGGL(phi_reduce_kernel, dim3((E1 + 255) / 256, phi_reduce_split(G)), dim3(256), 0, st, partials, G, ncols, K, cell0, M, D, dcol, do_band, stats, ranges);
}

// set the LDS attribute, launch G workgroups; timing events (Handle::prof_*) are recorded on the launch stream right around the kernel
template <class Kern, class... Args>
static int phi_launch(Handle* h, hipStream_t st, Kern kern, int G, int threads, size_t lds_bytes, Args... args) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) { set_error("hipFuncSetAttribute(%zu B LDS): %s", lds_bytes, hipGetErrorString(e)); return ASVGP_ERR_LDS_CAPACITY; }
  const bool prof = h->prof_on && h->prof_n < PROF_RING && (h->prof_calls++ % h->prof_every == 0);
  if (prof) (void)hipEventRecord(h->prof_ev[h->prof_n][0], st);
  hipLaunchKernelGGL(kern, dim3((unsigned)G), dim3(threads), lds_bytes, st, args...);
  if (prof) { (void)hipEventRecord(h->prof_ev[h->prof_n][1], st); ++h->prof_n; }
  return ASVGP_OK;
}

// one case per built order: f(std::integral_constant<int, order>)
template <class F>
static int for_phi_order(int order, F&& f) {
  switch (order) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
  }
  return ASVGP_ERR_UNSUPPORTED;
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------
enum PhiNeed { PHI_NEED_NOTHING = 0, PHI_NEED_MESH, PHI_NEED_ORDER };
struct PhiInputs {
  long N, D, M, n_mesh; double delta;
  bool weighted;                       // asvgp_phi_accumulate_1d_weighted
  int algo, blocks; bool defer;        // Handle: phi_algo, phi_blocks, phi_defer
  bool aligned16;                      // x, y (and w) on 16-byte boundaries
  // the two facts that cost a device round trip, < 0 while nobody has asked: the mesh is an exact numpy.linspace (with its end knots and
  // the step as the host rounds it), x is a time series
  int mesh_regular; double mesh_first, mesh_last, mesh_step;
  int series;
};
struct PhiPlan {
  int status; char msg[256];           // != ASVGP_OK: refused, nothing below counts
  int need;                            // PhiNeed: the fact the rules stopped at; give it and plan again
  int kernel;                          // 1 | 3 band scatter (fp64 | fixed point), 5 centred moments, 6 tile sort; weighted: 11 band scatter, 16 register moments
  int series;                          // 6: the instantiation with the time-series front loop
  int shape;                           // 6 / 16: points per thread and tile; 5: plane stride of the moment image
  size_t lds_bytes;                    // dynamic LDS (band scatter: of the widest chunk)
  int G; long ppb;                     // workgroups, points per workgroup
  int s0;                              // fixed-point exponent (3, 5), else -1
  int cells_per_chunk, chunks;         // band scatter: mesh cells per launch, launches per output column (else all cells, 1)
  int launches, reduces, reduce_y;     // kernel launches; reduce launches of this call (0: parked on the handle), their grid.y
  bool defer;
  bool asked_mesh, asked_order;        // which facts a rule on the way depended on
};

// knot rounding (two roundings <= ulp(|knot|)) over delta: how close to a knot the arithmetic cell guess of the tile sort may be trusted
static double phi_knot_margin(const PhiInputs& in) {
  const double amax = fabs(in.mesh_first) > fabs(in.mesh_last) ? fabs(in.mesh_first) : fabs(in.mesh_last);
  return 16.0 * 2.220446049250313e-16 * amax / in.delta + 1e-12;
}

// Which kernel and shape.  Reads its argument only: no HIP call, no handle.  The rules, in order (include/asvgp_hip.h,
// asvgp_set_phi_algorithm): 0 = auto takes the tile sort (6; weighted: 16) where it applies, else the centred moments (5; none with
// weights), else the band scatter (3; weighted: 11); a forced 6 or 5 that does not apply is refused, 1 and 3 are the band scatter.
template <int K>
static PhiPlan plan_phi(const PhiInputs& in) {
  PhiPlan p{};
  p.s0 = -1;
  auto refuse = [&p](int status, const char* fmt, auto... a) { p.status = status; snprintf(p.msg, sizeof(p.msg), fmt, a...); return p; };
  auto ask = [&p](int fact) { p.need = fact; return p; };
  // one streaming launch and one reduce over all M columns (6, 16, 5)
  auto whole = [&](int kernel, int series, int shape, size_t lds, PhiGrid g, bool fixed_point, bool may_defer) {
    p.kernel = kernel; p.series = series; p.shape = shape; p.lds_bytes = lds; p.G = g.G; p.ppb = g.ppb;
    if (fixed_point) p.s0 = phi_s0(g.ppb);
    p.cells_per_chunk = (int)in.n_mesh - 1; p.chunks = 1; p.launches = 1;
    p.defer = may_defer && in.defer;   // the caller enqueues the reduce itself (asvgp_phi_reduce_1d), e.g. on the stream that consumes the statistics
    p.reduces = p.defer ? 0 : 1; p.reduce_y = phi_reduce_split(g.G);
    return p;
  };
  const int algo = in.algo;
  const int ncells = (int)in.n_mesh - 1;
  const char* entry = in.weighted ? "phi_accumulate_1d_weighted" : "phi_accumulate_1d";
  if (in.weighted && (algo == 3 || algo == 5))
    return refuse(ASVGP_ERR_UNSUPPORTED, "%s: phi algorithm %d accumulates in fixed point, whose scales are bounds on the unweighted products - it has no weighted form (0 or 1)", entry, algo);
  const bool streams = in.D == 1 && in.aligned16;   // one output column, 16-byte loads

  // Tile sort (phi_sort.hpp; weighted: the register moments of phi_sort_weighted.hpp): an image of at most 2048 columns, at least one
  // pair of points, a mesh that is an exact numpy.linspace whose knots are not so large against delta that the arithmetic cell guess has
  // no safe margin.  Unweighted, two instantiations: TP points per thread and tile without the time-series front loop (fastest on i.i.d.
  // points), and at most 4 with it (the run sums and the second register set of its prefetch need the room) for an input the order probe
  // - or the caller, asvgp_set_phi_input_order - calls a time series; where that one does not hold the input, the plain one runs.
  if (algo == 0 || algo == 6) {
    bool applies = streams && in.N >= 2 && in.M <= PS_NCELL;
    if (applies) {
      if (in.mesh_regular < 0) return ask(PHI_NEED_MESH);
      p.asked_mesh = true;
      applies = in.mesh_regular != 0 && phi_knot_margin(in) < 0.125;
    }
    if (applies && !in.weighted) {
      if (in.series < 0) return ask(PHI_NEED_ORDER);
      p.asked_order = true;
    }
    if (applies) {
      constexpr int TP = ps_tile_points<K>(), TPS = TP < 4 ? TP : 4, TPW = psw_tile_points<K>();
      // (k = 4: 160 248 of 163 840 bytes.  A table that grows past the LDS must fail the build, not quietly hand the measured shape to kernel 11.)
      static_assert(psw_lds_bytes<K, TPW>() <= PHI_LDS_MAX && ps_epilogue_bytes<K>() <= PHI_LDS_MAX, "weighted register-moment kernel: LDS plan exceeds 160 KB");
      struct { int kernel, series, tp; size_t lds; bool tried; } inst[3] = {
          {16, 0, TPW, psw_lds_bytes<K, TPW>(), in.weighted},
          {6, 1, TPS, ps_lds_bytes<K, TPS, 1>(), !in.weighted && in.series > 0},
          {6, 0, TP, ps_lds_bytes<K, TP, 0>(), !in.weighted}};
      for (const auto& i : inst) {
        if (!i.tried) continue;
        const size_t lds = i.lds > ps_epilogue_bytes<K>() ? i.lds : ps_epilogue_bytes<K>();
        // at least one tile per workgroup; series: whole rows of 64 pairs - only the grid's last workgroup has an incomplete one
        const PhiGrid g = phi_grid(in.N, in.blocks, (long)i.tp * PS_THREADS, i.series ? 128 : 2);
        if (lds > PHI_LDS_MAX || g.ppb > 0x3fffffffL) continue;          // (32-bit pair indices inside a workgroup)
        return whole(i.kernel, i.series, i.tp, lds, g, false, !in.weighted);
      }
    }
    if (algo == 6)
      return in.weighted ? refuse(ASVGP_ERR_UNSUPPORTED, "%s: phi algorithm 6 (register moments) needs D == 1, N >= 2, M <= 2048, 16-byte aligned x / y / w and a mesh that is an exact linspace", entry)
                         : refuse(ASVGP_ERR_UNSUPPORTED, "%s", "phi algorithm 6 (tile sort) needs D == 1, N >= 2, M <= 2048, 16-byte aligned x / y and a mesh that is an exact linspace");
  }

  // Centred moments (phi_moments.hpp): the smallest plane stride that holds the cells and fits the LDS with the Phi y plane.  The mesh
  // fact only chooses between the instantiation that generates its knots and the one that reads the table.
  if (!in.weighted && (algo == 0 || algo == 5)) {
    if (streams && in.N >= 1) {
      if (in.mesh_regular < 0) return ask(PHI_NEED_MESH);
      p.asked_mesh = true;
      const size_t lds[3] = {mq_lds_bytes<K, 512>(in.M), mq_lds_bytes<K, 1024>(in.M), mq_lds_bytes<K, 2048>(in.M)};
      for (int i = 0; i < 3; ++i)
        if (ncells <= (512 << i) && lds[i] <= PHI_LDS_BUDGET)
          return whole(5, 0, 512 << i, lds[i], phi_grid(in.N, in.blocks, 2 * MQ_THREADS, 2 * MQ_THREADS), true, true);
    }
    if (algo == 5) return refuse(ASVGP_ERR_UNSUPPORTED, "%s", "phi algorithm 5 (centred moments) needs D == 1, 16-byte aligned x / y and M small enough for the LDS split");
  }

  // Band scatter (phi_accumulate_kernel, phi_weighted_kernel): any D, alignment, mesh and M - the columns the LDS does not hold beside
  // the mesh table go in chunks of cells, one launch and one reduce per chunk and output column.  Never deferred.
  const bool fx = !in.weighted && algo != 1;
  const int maxc = phi_max_cols(K, in.n_mesh, fx);
  if (maxc < 2 * K + 2) return refuse(ASVGP_ERR_LDS_CAPACITY, "%s: mesh table (%ld knots) leaves no LDS for the band", entry, in.n_mesh);
  p.kernel = in.weighted ? 11 : (fx ? 3 : 1);
  p.cells_per_chunk = (in.M <= maxc) ? ncells : (maxc - K);
  p.chunks = (ncells + p.cells_per_chunk - 1) / p.cells_per_chunk;
  p.lds_bytes = phi_band_lds_bytes(K, fx, p.cells_per_chunk + K, in.n_mesh);
  const PhiGrid g = in.weighted ? phi_grid(in.N, in.blocks, PW_THREADS, 64) : phi_grid(in.N, in.blocks, 2 * PHI_THREADS, 2 * PHI_THREADS);
  p.G = g.G; p.ppb = g.ppb;
  if (fx) p.s0 = phi_s0(g.ppb);
  p.launches = p.reduces = (int)(p.chunks * in.D);
  p.reduce_y = phi_reduce_split(g.G);
  return p;
}

// ---- the fact behind PHI_NEED_ORDER ---------------------------------------------------------------------------------------------
// Is x a time series (sorted / locally sorted)?  Decided once per (pointer, N) from 512 sampled rows (phi_order_probe_kernel); a stale
// verdict - the caller has overwritten the buffer with data of another order - costs speed, never correctness.
static bool handle_phi_is_series(Handle* h, const double* x, long N, double m0, double inv_delta, long n_mesh, hipStream_t st) {
  if (h->phi_order == 1) return false;
  if (h->phi_order == 2) return true;
  for (int i = 0; i < h->n_order_seen; ++i)
    if (h->order_seen[i].ptr == x && h->order_seen[i].n == N) return h->order_seen[i].series != 0;
  int series = 0;
  const int nprobe = 512;
  if (N >= 128L * nprobe) {
    if (!h->order_dev && hipMalloc(&h->order_dev, sizeof(int)) != hipSuccess) h->order_dev = nullptr;
    int cnt = 0;
    if (h->order_dev && hipMemsetAsync(h->order_dev, 0, sizeof(int), st) == hipSuccess) {
      hipLaunchKernelGGL(phi_order_probe_kernel, dim3(nprobe), dim3(64), 0, st, x, N, N / nprobe, nprobe, m0, inv_delta, (int)n_mesh, h->order_dev);
      if (hipMemcpyAsync(&cnt, h->order_dev, sizeof(int), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess)
        series = cnt * 10 >= nprobe * 9 ? 1 : 0;                 // nine rows in ten: the front loop will carry the pass
    }
  }
  if (h->n_order_seen < 8) h->order_seen[h->n_order_seen++] = Handle::OrderSeen{x, N, series};
  return series != 0;
}

// ---- the launchers: each executes an accepted plan ------------------------------------------------------------------------------
struct PhiCall {
  PhiInputs in;
  const double* x; const double* y; const double* w; const double* mesh;
  double* stats; double* wstats;       // wstats: weighted only
  double* ws;                          // 256 partial [band | Phi y | y^T y] images, then `behind`
  hipStream_t st;
  // behind the partials: the moment kernel's overflow planes | the tile sort's column ranges | the weighted kernels' 256 records of the
  // weight sums and, behind those, the register-moment kernel's column ranges (asvgp_phi_[weighted_]workspace_bytes)
  template <int K> double* behind() const { return ws + (size_t)PHI_MAX_BLOCKS * ((size_t)(K + 2) * (size_t)in.M + 1); }
};

template <int K>
static int launch_phi_tile_sort(Handle* h, const PhiCall& c, const PhiPlan& p) {
  const PhiInputs& in = c.in;
  PswArgs aw;
  PsArgs& a = aw.p;
  a.x = c.x; a.y = c.y; a.N = in.N; a.mesh_g = c.mesh; a.n_mesh = (int)in.n_mesh; a.inv_delta = 1.0 / in.delta; a.M = (int)in.M;
  a.m0 = in.mesh_first; a.m_last = in.mesh_last; a.step = in.mesh_step; a.smax_fast = 0.5 - phi_knot_margin(in);
  a.partials = c.ws; a.ppb = p.ppb; a.zero_ptr = c.stats; a.zero_n = (K + 2) * in.M + 1; a.stamps = nullptr; a.stamps_wave = 0;
  aw.w = c.w;
  aw.wpart = c.behind<K>();
  a.ranges = in.weighted ? reinterpret_cast<int*>(aw.wpart + (size_t)PHI_MAX_BLOCKS * PW_WCOLS) : reinterpret_cast<int*>(c.behind<K>());
  constexpr int TP = ps_tile_points<K>(), TPS = TP < 4 ? TP : 4, TPW = psw_tile_points<K>();
  const int rc = in.weighted ? phi_launch(h, c.st, phi_sort_weighted_kernel<K, TPW>, p.G, PS_THREADS, p.lds_bytes, aw)
               : p.series    ? phi_launch(h, c.st, phi_sort_kernel<K, TPS, 0, 1, 1>, p.G, PS_THREADS, p.lds_bytes, a)
                             : phi_launch(h, c.st, phi_sort_kernel<K, TP, 0, 1, 0>, p.G, PS_THREADS, p.lds_bytes, a);
  if (rc) return rc;
  if (!in.weighted) h->phi_last_series = p.series;
  if (p.defer) {
    h->pend = Handle::PendingReduce{a.partials, p.G, (int)in.M, K, c.stats, true, a.ranges};
    return check_launch("phi_accumulate_1d (tile sort, reduce deferred)");
  }
  enqueue_phi_reduce(c.st, a.partials, p.G, (int)in.M, K, 0, in.M, 1L, 0, 1, c.stats, a.ranges);
  if (in.weighted) hipLaunchKernelGGL(phi_wstats_accumulate_kernel, dim3(1), dim3(64), 0, c.st, aw.wpart, p.G, c.wstats, 1);
  return check_launch(in.weighted ? "phi_accumulate_1d_weighted (register moments)" : "phi_accumulate_1d (tile sort)");
}

template <int K, int CS>
static int launch_phi_moments_cs(Handle* h, const PhiCall& c, const PhiPlan& p) {
  const PhiInputs& in = c.in;
  MqArgs a;
  a.x = c.x; a.y = c.y; a.N = in.N; a.mesh_g = c.mesh; a.n_mesh = (int)in.n_mesh; a.inv_delta = 1.0 / in.delta; a.M = (int)in.M; a.step = in.mesh_step;
  a.partials = c.ws; a.ov = c.behind<K>();
  a.ppb = p.ppb; a.zero_ptr = c.stats; a.zero_n = (K + 2) * in.M + 1; a.s0 = p.s0;
  const int rc = phi_launch(h, c.st, in.mesh_regular ? phi_moment_kernel<K, CS, true> : phi_moment_kernel<K, CS, false>, p.G, MQ_THREADS, p.lds_bytes, a);
  if (rc) return rc;
  if (p.defer) {
    h->pend = Handle::PendingReduce{a.partials, p.G, (int)in.M, K, c.stats, true, nullptr};
    return check_launch("phi_accumulate_1d (moments, reduce deferred)");
  }
  enqueue_phi_reduce(c.st, a.partials, p.G, (int)in.M, K, 0, in.M, 1L, 0, 1, c.stats, nullptr);
  return check_launch("phi_accumulate_1d (moments)");
}
template <int K>
static int launch_phi_moments(Handle* h, const PhiCall& c, const PhiPlan& p) {
  return p.shape == 512 ? launch_phi_moments_cs<K, 512>(h, c, p) : p.shape == 1024 ? launch_phi_moments_cs<K, 1024>(h, c, p) : launch_phi_moments_cs<K, 2048>(h, c, p);
}

// the (k+1)(k+2)/2 + (k+1) products of every point go straight into the workgroup's LDS band image, chunk by chunk of cells
template <int K>
static int launch_phi_band(Handle* h, const PhiCall& c, const PhiPlan& p) {
  const PhiInputs& in = c.in;
  const bool fx = p.kernel == 3, weighted = p.kernel == 11;
  const int ncells = (int)in.n_mesh - 1;
  const long M = in.M, D = in.D;
  const double inv_delta = 1.0 / in.delta;
  const long zero_n = (K + 1) * M + M * D + 1;
  const bool vec = D == 1 && in.aligned16;
  bool zeroed = false;   // the first launched kernel zeroes the stats buffer
  for (long dcol = 0; dcol < D; ++dcol) {
    for (int cell0 = 0; cell0 < ncells; cell0 += p.cells_per_chunk) {
      const int cell1 = cell0 + p.cells_per_chunk < ncells ? cell0 + p.cells_per_chunk : ncells;
      const int ncols = cell1 - cell0 + K;
      const size_t lds_bytes = phi_band_lds_bytes(K, fx, ncols, in.n_mesh);
      const int do_band = (dcol == 0);
      double* zero_ptr = zeroed ? nullptr : c.stats;
      int rc;
      if (weighted) {
        rc = phi_launch(h, c.st, phi_weighted_kernel<K>, p.G, PW_THREADS, lds_bytes, c.x, c.y + dcol, D, c.w, in.N, c.mesh, (int)in.n_mesh, inv_delta, cell0, cell1,
                        ncols, do_band, c.ws, c.behind<K>(), p.ppb, zero_ptr, zero_n);
      } else {
        auto kern = fx ? (vec ? phi_accumulate_kernel<K, true, true> : phi_accumulate_kernel<K, false, true>)
                       : (vec ? phi_accumulate_kernel<K, true, false> : phi_accumulate_kernel<K, false, false>);
        rc = phi_launch(h, c.st, kern, p.G, PHI_THREADS, lds_bytes, c.x, c.y + dcol, D, in.N, c.mesh, (int)in.n_mesh, inv_delta, cell0, cell1, ncols, do_band, c.ws,
                        p.ppb, zero_ptr, zero_n, p.s0);
      }
      if (rc) return rc;
      enqueue_phi_reduce(c.st, c.ws, p.G, ncols, K, cell0, M, D, (int)dcol, do_band, c.stats, nullptr);
      // (the weight sums: every chunk of the first output column writes its share of the rows; summed behind each of those launches)
      if (weighted && do_band) hipLaunchKernelGGL(phi_wstats_accumulate_kernel, dim3(1), dim3(64), 0, c.st, c.behind<K>(), p.G, c.wstats, zeroed ? 0 : 1);
      zeroed = true;
    }
  }
  return check_launch(weighted ? "phi_accumulate_1d_weighted" : "phi_accumulate_1d");
}

// flush -> plan -> fact -> plan -> refuse or dispatch
template <int K>
static int run_phi(Handle* h, PhiCall& c) {
  // a reduce still parked on this handle (deferred mode, e.g. the per-dimension calls of an additive model share one handle and one
  // partials workspace) goes out now, stream-ordered before this pass overwrites the partials
  { const int rcf = handle_flush_phi_reduce(h, nullptr, c.st); if (rcf) return rcf; }
  PhiInputs& in = c.in;
  PhiPlan p = plan_phi<K>(in);
  if (p.need == PHI_NEED_MESH) {
    in.mesh_regular = handle_mesh_is_linspace(h, c.mesh, in.n_mesh, c.st, &in.mesh_step, &in.mesh_first, &in.mesh_last) ? 1 : 0;
    p = plan_phi<K>(in);
  }
  if (p.need == PHI_NEED_ORDER) {
    in.series = handle_phi_is_series(h, c.x, in.N, in.mesh_first, 1.0 / in.delta, in.n_mesh, c.st) ? 1 : 0;
    p = plan_phi<K>(in);
  }
  if (p.status) { set_error("%s", p.msg); return p.status; }
  h->phi_last = p.kernel;
  switch (p.kernel) {
    case 6: case 16: return launch_phi_tile_sort<K>(h, c, p);
    case 5: return launch_phi_moments<K>(h, c, p);
    default: return launch_phi_band<K>(h, c, p);
  }
}

// 256 partial images, 256 records of the weight sums, 256 column ranges (2 ints) of the register-moment kernel
static size_t phi_weighted_ws_doubles(long M, int order) { return (size_t)PHI_MAX_BLOCKS * ((size_t)(order + 2) * (size_t)M + 1) + (size_t)PHI_MAX_BLOCKS * (PW_WCOLS + 1); }

// what both entries and the host plan check of (order, M, n_mesh) - and of the pointers, `ok`
static int check_phi_args(const char* entry, bool ok, int order, int64_t M, int64_t n_mesh) {
  if (!ok) { set_error("%s: bad argument", entry); return ASVGP_ERR_BAD_ARG; }
  if (order < 1 || order > ASVGP_MAX_ORDER) { set_error("%s: order %d unsupported", entry, order); return ASVGP_ERR_UNSUPPORTED; }
  if (n_mesh != M - order + 1 || n_mesh < 2) { set_error("%s: n_mesh=%ld != M-order+1", entry, (long)n_mesh); return ASVGP_ERR_BAD_ARG; }
  if (M > 0x3fffffff) { set_error("%s: M too large", entry); return ASVGP_ERR_UNSUPPORTED; }
  return ASVGP_OK;
}

// the body of both C entries (unweighted: w = wstats = NULL)
static int phi_entry(const char* entry, bool weighted, asvgp_handle_t handle, const double* x, const double* y, const double* w, int64_t N, int64_t D,
                     const double* mesh, int64_t n_mesh, double delta, int order, int64_t M, double* stats, double* wstats, void* workspace,
                     size_t workspace_bytes, asvgp_stream_t stream) {
  const bool ok = !(((!x || !y || (weighted && !w)) && N > 0) || !mesh || !stats || (weighted && !wstats) || N < 0 || D < 1 || M < 1 || !(delta > 0.0));
  const int rc = check_phi_args(entry, ok, order, M, n_mesh);
  if (rc) return rc;
  const size_t need = weighted ? asvgp_phi_weighted_workspace_bytes(M, order, D) : asvgp_phi_workspace_bytes(M, order, D);
  if (!workspace || workspace_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", entry, workspace_bytes, need); return ASVGP_ERR_WORKSPACE; }
  Handle* h = as_handle(handle);
  const uintptr_t bits = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(w);
  PhiCall c{PhiInputs{(long)N, (long)D, (long)M, (long)n_mesh, delta, weighted, h->phi_algo, h->phi_blocks, h->phi_defer, (bits & 15) == 0, -1, 0.0, 0.0, 0.0, -1},
            x, y, w, mesh, stats, wstats, static_cast<double*>(workspace), as_stream(stream)};
  return for_phi_order(order, [&](auto k) { return run_phi<decltype(k)::value>(h, c); });
}

int handle_flush_phi_reduce(Handle* h, const double* stats, hipStream_t st) {
  if (!h->pend.valid) return ASVGP_OK;                 // nothing deferred (the accumulate call has reduced already)
  if (stats && stats != h->pend.stats) return ASVGP_OK;
  const Handle::PendingReduce p = h->pend;
  h->pend.valid = false;
  enqueue_phi_reduce(st, p.partials, p.G, p.M, p.K, 0, (long)p.M, 1L, 0, 1, p.stats, p.ranges);
  return check_launch("phi_reduce_1d");
}

}  // namespace asvgp

using namespace asvgp;

extern "C" size_t asvgp_phi_workspace_bytes(int64_t M, int order, int64_t D) {
  (void)D;
  if (M <= 0 || order < 1 || order > ASVGP_MAX_ORDER) return 0;
  // 256 partial [band | Phi y | y^T y] images; the centred-moment kernel adds a per-workgroup fp64 plane for out-of-scale y
  const size_t band = (size_t)PHI_MAX_BLOCKS * ((size_t)(order + 2) * (size_t)M + 1);
  const size_t mom = band + (size_t)PHI_MAX_BLOCKS * (size_t)M;   // + the per-workgroup fp64 plane for out-of-scale y
  return sizeof(double) * (band > mom ? band : mom);
}

extern "C" size_t asvgp_phi_weighted_workspace_bytes(int64_t M, int order, int64_t D) {
  (void)D;
  if (M <= 0 || order < 1 || order > ASVGP_MAX_ORDER) return 0;
  const size_t own = sizeof(double) * phi_weighted_ws_doubles((long)M, order);
  const size_t base = asvgp_phi_workspace_bytes(M, order, D);   // (never less: a model keeps ONE workspace for both entries)
  return own > base ? own : base;
}

extern "C" int asvgp_phi_accumulate_1d(asvgp_handle_t handle, const double* x, const double* y, int64_t N, int64_t D, const double* mesh,
                                       int64_t n_mesh, double delta, int order, int64_t M, double* stats,
                                       void* workspace, size_t workspace_bytes, asvgp_stream_t stream) {
  return phi_entry("phi_accumulate_1d", false, handle, x, y, nullptr, N, D, mesh, n_mesh, delta, order, M, stats, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int asvgp_phi_accumulate_1d_weighted(asvgp_handle_t handle, const double* x, const double* y, const double* w, int64_t N, int64_t D,
                                                const double* mesh, int64_t n_mesh, double delta, int order, int64_t M, double* stats,
                                                double* wstats, void* workspace, size_t workspace_bytes, asvgp_stream_t stream) {
  return phi_entry("phi_accumulate_1d_weighted", true, handle, x, y, w, N, D, mesh, n_mesh, delta, order, M, stats, wstats, workspace, workspace_bytes, stream);
}

extern "C" int asvgp_phi_last_algorithm(asvgp_handle_t handle) { return as_handle(handle)->phi_last; }

extern "C" int asvgp_phi_reduce_1d(asvgp_handle_t handle, asvgp_stream_t stream) {
  return handle_flush_phi_reduce(as_handle(handle), nullptr, as_stream(stream));
}

// Host-only: the plan the two entries above would make for these inputs - the same plan_phi, no handle, no device
extern "C" int asvgp_phi_launch_plan_host(int phi_algorithm, int phi_workgroups, int deferred_reduce, int weighted, int64_t N, int64_t D, int64_t M, int order,
                                          int64_t n_mesh, double delta, int aligned16, int mesh_regular, double mesh_first, double mesh_last, int series,
                                          int64_t* plan16_host) {
  const bool ok = plan16_host && N >= 0 && D >= 1 && M >= 1 && delta > 0.0 && phi_workgroups >= 0 && phi_workgroups <= PHI_MAX_BLOCKS &&
                  (phi_algorithm == 0 || phi_algorithm == 1 || phi_algorithm == 3 || phi_algorithm == 5 || phi_algorithm == 6);
  const int rc = check_phi_args("phi_launch_plan_host", ok, order, M, n_mesh);
  if (rc) { if (plan16_host) { for (int i = 1; i < 16; ++i) plan16_host[i] = 0; plan16_host[0] = rc; } return rc; }
  const PhiInputs in{(long)N, (long)D, (long)M, (long)n_mesh, delta, weighted != 0, phi_algorithm, phi_workgroups, deferred_reduce != 0, aligned16 != 0,
                     mesh_regular != 0 ? 1 : 0, mesh_first, mesh_last, (mesh_last - mesh_first) / (double)(n_mesh - 1), series != 0 ? 1 : 0};
  PhiPlan p{};
  (void)for_phi_order(order, [&](auto k) { p = plan_phi<decltype(k)::value>(in); return 0; });
  const int64_t f[16] = {p.status, p.kernel, p.series, p.shape, (int64_t)p.lds_bytes, p.G, p.ppb, p.chunks, p.cells_per_chunk, p.launches, p.reduces, p.reduce_y,
                         p.s0, p.asked_mesh, p.asked_order, 0};
  for (int i = 0; i < 16; ++i) plan16_host[i] = f[i];
  if (p.status) set_error("%s", p.msg);
  return p.status;
}
