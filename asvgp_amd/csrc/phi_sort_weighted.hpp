// Weighted Phi pass, register-moment design (asvgp_phi_last_algorithm = 16): phi_sort_kernel (phi_sort.hpp, whose helpers, tables and
// phase structure it shares and whose code it does not touch) with a weight per point.  Per cell
//   S_p = sum w s^p (p = 0..2k; S_0 is now a floating sum and one more accumulator per cell),  T_p = sum w y s^p (p = 0..k)
// in the registers of the thread that owns the cell; the MomTab epilogue turns them into the band / rhs entries exactly as for w = 1
// (S_0 takes the place of the integer count).  Beside them per thread: sum w y^2, sum w, sum log w, the number of rows with w > 0.
// What travels through the LDS per point: the 16-byte record (s, w y) of the unweighted kernel - same ds_write_b128 / ds_read_b128 -
// plus w in a PLANE of its own behind the records (8 bytes at the same sorted position): 24 bytes per point, but neither a 24-byte
// record (three 8-byte LDS instructions each way, or a 32-byte one that does not fit) nor a change to the record walk.  Tile: 4 points
// per thread (k <= 4; 2 above): 4096 x 24 B = 96 KB beside the 24 KB of count planes - 6 points (144 KB) do not fit the 160 KB.
// A row with w = 0 is dropped where the cell is searched (it takes no rank, reaches nothing); a negative, NaN or infinite weight counts
// like a point outside the mesh (NaN yy_w).  No time-series front loop: sorted input goes through the general loop, whose heavy-cell
// path (whole wavefronts sum a cell's run) carries it.
#pragma once

namespace asvgp {

struct PswArgs {
  PsArgs p;                // as the unweighted kernel (stamps / stamps_wave unused)
  const double* w;         // N weights
  double* wpart;           // [workgroup][4]: sum w, sum log w, rows with w > 0, unused
};

template <int K> constexpr int psw_tile_points() { return K <= 4 ? 4 : 2; }
template <int K, int TP> constexpr size_t psw_lds_bytes() {
  return (size_t)(TP * PS_THREADS + 1) * 16 + (size_t)3 * PS_NCELL * 4 + 64 * 4 + 64 * 8 +
         (size_t)PS_HROUND * (3 * K + 2) * 8 + (size_t)PS_HLIST * 12 + (size_t)(TP * PS_THREADS + 1) * 8 + (size_t)4 * PS_THREADS * 8;
}

// one point into a cell's weighted moments: S0 += w, S_p += w s^p (p = 1..2K), T_p += (w y) s^p (p = 0..K)
template <int K>
__device__ __forceinline__ void psw_acc(double s, double wy, double w, double& S0, double (&S)[2 * K], double (&Tm)[K + 1]) {
  double pw[K + 1];
  pw[0] = 1.0;
  pw[1] = s;
#pragma unroll
  for (int p = 2; p <= K; ++p) pw[p] = pw[p / 2] * pw[p - p / 2];
  S0 += w;
#pragma unroll
  for (int p = 1; p <= K; ++p) S[p - 1] = fma(w, pw[p], S[p - 1]);
  const double wk = w * pw[K];
#pragma unroll
  for (int p = K + 1; p <= 2 * K; ++p) S[p - 1] = fma(wk, pw[p - K], S[p - 1]);
  Tm[0] += wy;
#pragma unroll
  for (int p = 1; p <= K; ++p) Tm[p] = fma(wy, pw[p], Tm[p]);
}

// ps_own_cell with the weight plane: a lane that has run out reads the (0, 0) record and the weight 0 at slot ZS, which add nothing
template <int K, int ZS>
__device__ __forceinline__ void psw_own_cell(const double2* buf, const double* wpl, unsigned l, unsigned o, double& S0, double (&S)[2 * K],
                                             double (&Tm)[K + 1]) {
  const unsigned nmax = ps_wave_max_u32(l);
  for (unsigned j = 0; j < nmax; ++j) {
    const unsigned at = (j < l) ? o + j : (unsigned)ZS;
    const double2 p = buf[at];
    const double w = wpl[at];
    psw_acc<K>(p.x, p.y, w, S0, S, Tm);
  }
}

// ps_heavy_slices with a weight: slot = [S_1..S_2K | T_0..T_K | S_0]
template <int K>
__device__ __forceinline__ void psw_heavy_slices(const double2* buf, const double* wpl, unsigned hn, unsigned ho, int first, int stride, int lane,
                                                 double* slot) {
  constexpr int NS = 2 * K;
  const unsigned nsl = (hn + 63u) >> 6;
  double S2[NS], T2[K + 1], W2 = 0.0;
#pragma unroll
  for (int q = 0; q < NS; ++q) S2[q] = 0.0;
#pragma unroll
  for (int q = 0; q <= K; ++q) T2[q] = 0.0;
  for (unsigned sl = (unsigned)first; sl < nsl; sl += (unsigned)stride) {
    const unsigned j = sl * 64 + lane;
    if (j < hn) {
      const double2 pt = buf[ho + j];
      psw_acc<K>(pt.x, pt.y, wpl[ho + j], W2, S2, T2);
    }
  }
  if constexpr (NS <= 8) {
    int idx;
    const double t = ps_reduce_scatter8<NS>(S2, lane, idx);
    if (lane < 8 && idx < NS) lds_add(slot + idx, t);
  } else {
#pragma unroll
    for (int q = 0; q < NS; ++q) { const double t = wave_sum_dpp(S2[q]); if (lane == 0) lds_add(slot + q, t); }
  }
  __builtin_amdgcn_sched_barrier(0);
  {
    int idx;
    const double t = ps_reduce_scatter8<K + 1>(T2, lane, idx);
    if (lane < 8 && idx <= K) lds_add(slot + NS + idx, t);
  }
  __builtin_amdgcn_sched_barrier(0);
  {
    const double t = wave_sum_dpp(W2);
    if (lane == 0) lds_add(slot + NS + K + 1, t);
  }
  __builtin_amdgcn_sched_barrier(0);
}

template <int K, int TP>
__global__ __launch_bounds__(PS_THREADS) void phi_sort_weighted_kernel(PswArgs aw) {
  extern __shared__ double lds[];
  static_assert(TP % 2 == 0 && TP * PS_THREADS <= 8192, "tile: rank field is 13 bits");
  const PsArgs& a = aw.p;
  constexpr int T = TP * PS_THREADS;
  constexpr int NS = 2 * K;
  double2* buf = reinterpret_cast<double2*>(lds);                 // T sorted (s, w y) + slot T = (0, 0)
  unsigned* cnt = reinterpret_cast<unsigned*>(buf + T + 1);       // [2][PS_NCELL] per-tile histogram, double-buffered
  unsigned* off = cnt + 2 * PS_NCELL;                             // [PS_NCELL]
  unsigned* wtot = off + PS_NCELL;                                // [16] wave totals of the scan (+ pad)
  double* scratch = reinterpret_cast<double*>(wtot + 64);         // 64 doubles
  constexpr int NSTAT = 3 * K + 2;                                // 2k + (k+1) sums + S_0
  double* hacc = scratch + 64;                                    // [PS_HROUND][NSTAT] hand-over table of the heavy cells
  unsigned* hlist = reinterpret_cast<unsigned*>(hacc + PS_HROUND * NSTAT);   // [PS_HLIST] x (cell, count, offset)
  unsigned* nheavy_p = wtot + 32;                                 // heavy cells of the current tile
  double* wpl = reinterpret_cast<double*>(hlist + 3 * PS_HLIST);  // [T + 1] the weights in cell order, slot T = 0   (8-byte aligned: PS_HLIST is even)
  static_assert((3 * PS_HLIST * 4) % 8 == 0, "weight plane alignment");
  // per-thread sums that are touched once per tile live in the LDS, not in registers held across the owner loops (they cost the k = 4
  // instantiation 13 spilled registers): [4][1024] = sum w y^2, sum w, sum log w, rows with w > 0
  double* tacc = wpl + T + 1;
  if (a.zero_ptr) for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < a.zero_n; e += (long)gridDim.x * blockDim.x) a.zero_ptr[e] = 0.0;
  const int tid0 = threadIdx.x;
  int tid = tid0, lane = tid0 & 63, wv = tid0 >> 6;
  const int n_mesh = a.n_mesh, ncells = n_mesh - 1, M = a.M;
  const double* __restrict__ mesh = a.mesh_g;
  const double inv_delta = a.inv_delta, step = a.step, smax_fast = a.smax_fast;
  const double m0 = a.m0, m_last = a.m_last;
  {
    uint4* z = reinterpret_cast<uint4*>(cnt);
    z[tid] = make_uint4(0u, 0u, 0u, 0u);                          // 2 x 2048 counters = 1024 x 16 B
    if (tid == 0) { buf[T] = make_double2(0.0, 0.0); wpl[T] = 0.0; }
#pragma unroll
    for (int c = 0; c < 4; ++c) tacc[c * PS_THREADS + tid] = 0.0;   // (thread-private slots)
  }
  unsigned nbad = 0;
  auto knot = [&](int i) __attribute__((always_inline)) -> double { return (i == n_mesh - 1) ? m_last : mq_linspace_knot(i, step, m0); };
  // the exact table rule for the rare point within rounding of a knot or outside the mesh (as phi_sort_kernel)
  auto cell_slow = [&](double x, double& s_out, bool& ok) __attribute__((always_inline)) -> int {
    int i = mq_guess(x, m0, inv_delta, n_mesh);                   // clamped to [0, n_mesh - 2]; NaN -> 0
    const double k0 = knot(i);
    const bool down = !(k0 < x) && i > 0;
    const bool up = !down && i < n_mesh - 2 && knot(i + 1) < x;
    i += up ? 1 : (down ? -1 : 0);
    const double lo = knot(i), hi = knot(i + 1);
    const double s = (x - lo) * inv_delta - 0.5;
    ok = (i == 0 || lo < x) && (i == n_mesh - 2 || !(hi < x)) && fabs(s) <= MQ_SMAX;
    s_out = s;
    return i;
  };

  const long beg = (long)blockIdx.x * a.ppb;
  long end = beg + a.ppb;
  if (end > a.N) end = a.N;
  if (end < beg) end = beg;
  const long ubeg = beg >> 1;
  const int npair = (int)((end >> 1) - ubeg);                     // full pairs of this workgroup (beg is even)
  const bool tail = (end & 1) != 0;                               // one odd last point (only the workgroup that reaches N)
  const int nunit = npair + (tail ? 1 : 0);
  const int n_tiles = (nunit + T / 2 - 1) / (T / 2);              // row q2 of tile t: the 1024 pairs t T/2 + q2 1024 + tid
  typedef double ps_nt2 __attribute__((ext_vector_type(2)));
  const ps_nt2* x2 = reinterpret_cast<const ps_nt2*>(a.x) + (npair > 0 ? ubeg : 0);
  const ps_nt2* y2 = reinterpret_cast<const ps_nt2*>(a.y) + (npair > 0 ? ubeg : 0);
  const ps_nt2* w2 = reinterpret_cast<const ps_nt2*>(aw.w) + (npair > 0 ? ubeg : 0);
  const int ulast = npair > 0 ? npair - 1 : 0;

  double xs[TP], ys[TP], ws[TP];
  // unconditional, clamped loads and NO branch around them (see phi_sort_kernel)
  auto load_tile = [&](int tile) __attribute__((always_inline)) {
#pragma unroll
    for (int q2 = 0; q2 < TP / 2; ++q2) {
      int u = tile * (T / 2) + q2 * PS_THREADS + tid;
      u = u < ulast ? u : ulast;
      const ps_nt2 xv = __builtin_nontemporal_load(x2 + u);       // read exactly once: keep the stream out of the L2's LRU order
      const ps_nt2 yv = __builtin_nontemporal_load(y2 + u);
      const ps_nt2 wv2 = __builtin_nontemporal_load(w2 + u);
      xs[2 * q2] = xv.x; xs[2 * q2 + 1] = xv.y; ys[2 * q2] = yv.x; ys[2 * q2 + 1] = yv.y; ws[2 * q2] = wv2.x; ws[2 * q2 + 1] = wv2.y;
    }
  };

  double SA[NS], TA[K + 1], SB[NS], TB[K + 1], W0A = 0.0, W0B = 0.0;
#pragma unroll
  for (int p = 0; p < NS; ++p) { SA[p] = 0.0; SB[p] = 0.0; }
#pragma unroll
  for (int p = 0; p <= K; ++p) { TA[p] = 0.0; TB[p] = 0.0; }
  unsigned n0A = 0, n0B = 0;                                      // rows with w > 0 in the two cells (which columns the partial holds)

  // ---- cell, centred coordinate and weight of the tile held in (xs, ys, ws).  sv = s, yv = w y (ws keeps w until the next tile is
  // loaded, behind the scatter); bit q of valm: point q exists, lies inside the mesh and has a weight > 0.
  double sv[TP], yv[TP];
  int cr[TP];
  unsigned valm = 0;
  auto search_tile = [&](int tile) __attribute__((always_inline)) {
    valm = 0;
    double yy = 0.0, sw = 0.0, sl = 0.0, np = 0.0;
#pragma unroll
    for (int q2 = 0; q2 < TP / 2; ++q2) {
      const int u = tile * (T / 2) + q2 * PS_THREADS + tid;
      double xv[2] = {xs[2 * q2], xs[2 * q2 + 1]};
      double yq[2] = {ys[2 * q2], ys[2 * q2 + 1]};
      double wv2[2] = {ws[2 * q2], ws[2 * q2 + 1]};
      bool val[2] = {u < npair, u < npair};
      if (tail && u == npair) {                                   // the odd last point: a scalar reload by ONE lane of the kernel
        xv[0] = a.x[end - 1]; yq[0] = a.y[end - 1]; wv2[0] = aw.w[end - 1]; ws[2 * q2] = wv2[0]; val[0] = true;
      }
      bool slow = false;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const bool wok = wv2[e] >= 0.0 && wv2[e] < __builtin_inf();       // (NaN fails both)
        if (val[e] && !wok) { ++nbad; val[e] = false; }                   // an invalid weight: reported like a point outside the mesh
        val[e] = val[e] && wv2[e] > 0.0;                                  // w = 0: an absent row
        const double g = floor((xv[e] - m0) * inv_delta);
        const int c = __double2int_rz(g);                         // (v_cvt_i32_f64: saturating; NaN -> 0)
        double u0;
        {
#pragma clang fp contract(off)
          const double t = g * step;                              // numpy.linspace's knot: i * step rounded, THEN + start rounded
          u0 = t + m0;
        }
        const double s = (xv[e] - u0) * inv_delta - 0.5;
        const bool fast = (unsigned)c < (unsigned)ncells && fabs(s) <= smax_fast;
        slow = slow || (val[e] && !fast);
        cr[2 * q2 + e] = c;
        sv[2 * q2 + e] = s;
      }
      if (__any(slow)) {                                          // rare: the exact table rule, per lane
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          bool ok;
          double sq;
          const int c = cell_slow(xv[e], sq, ok);
          cr[2 * q2 + e] = c;
          sv[2 * q2 + e] = sq;
          if (val[e] && !ok) { ++nbad; val[e] = false; }          // outside the mesh (or NaN): reported, never accumulated
        }
      }
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const double wy = wv2[e] * yq[e];
        yv[2 * q2 + e] = wy;
        if (val[e]) { yy = fma(wy, yq[e], yy); sw += wv2[e]; sl += log(wv2[e]); np += 1.0; }
      }
      valm |= (val[0] ? 1u : 0u) << (2 * q2) | (val[1] ? 2u : 0u) << (2 * q2);
      __builtin_amdgcn_sched_barrier(0);
    }
    tacc[tid] += yy; tacc[PS_THREADS + tid] += sw; tacc[2 * PS_THREADS + tid] += sl; tacc[3 * PS_THREADS + tid] += np;
  };

  load_tile(0);
  {   // the host chose this kernel from its copy of the mesh; a table that is NOT that linspace here is reported loudly
    int okm = 1;
    const double last_v = mesh[n_mesh - 1];
    const int i0 = tid < n_mesh - 1 ? tid : 0, i1 = tid + PS_THREADS < n_mesh - 1 ? tid + PS_THREADS : 0;
    const double v0 = mesh[i0], v1 = mesh[i1];
    okm &= (v0 == mq_linspace_knot(i0, step, m0)) ? 1 : 0;
    okm &= (v1 == mq_linspace_knot(i1, step, m0)) ? 1 : 0;
    okm &= (last_v == m_last) ? 1 : 0;
    for (int i = tid + 2 * PS_THREADS; i < n_mesh - 1; i += PS_THREADS) okm &= (mesh[i] == mq_linspace_knot(i, step, m0)) ? 1 : 0;
    if (!okm) ++nbad;
  }
  __syncthreads();
  for (int tile = 0; tile < n_tiles; ++tile) {
    unsigned* cntb = cnt + (tile & 1) * PS_NCELL;
    // the thread index is re-read per tile behind an opaque barrier (see phi_sort_kernel: keeps LDS addresses out of scratch)
    tid = tid0;
    asm volatile("" : "+v"(tid));
    lane = tid & 63;
    wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // ---- P1: cell, centred coordinate, rank inside the cell
    search_tile(tile);
    {
      unsigned rk[TP];
#pragma unroll
      for (int q2 = 0; q2 < TP / 2; ++q2) {                       // all rank atomics of the tile in flight together
        const bool va = (valm >> (2 * q2)) & 1u, vb = (valm >> (2 * q2 + 1)) & 1u;
        const int c0 = __builtin_amdgcn_readfirstlane(cr[2 * q2]);
        if (__all(va && vb && cr[2 * q2] == c0 && cr[2 * q2 + 1] == c0)) {
          // all 128 points of the wave's pair row in ONE cell - one atomic instead of 128 same-address ones
          unsigned base = 0;
          if (lane == 0) base = __hip_atomic_fetch_add(cntb + c0, 128u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
          rk[2 * q2] = base + 2u * (unsigned)lane;
          rk[2 * q2 + 1] = base + 2u * (unsigned)lane + 1u;
        } else {
          rk[2 * q2] = va ? __hip_atomic_fetch_add(cntb + cr[2 * q2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : 0u;
          rk[2 * q2 + 1] = vb ? __hip_atomic_fetch_add(cntb + cr[2 * q2 + 1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : 0u;
        }
      }
#pragma unroll
      for (int q = 0; q < TP; ++q) cr[q] = ((valm >> q) & 1u) ? ((cr[q] << 13) | (int)rk[q]) : -1;
    }
    ps_lds_barrier();
    // ---- P2: exclusive scan of the counts -> off   (thread t scans cells 2t, 2t+1)
    {
      const uint2 c2 = reinterpret_cast<const uint2*>(cntb)[tid];
      const unsigned v = c2.x + c2.y;
      const unsigned inc = ps_wave_scan_incl(v);
      if (lane == 63) wtot[wv] = inc;
      if (tid == 0) *nheavy_p = 0;
      ps_lds_barrier();
      unsigned w = wtot[lane & 15];
      w = ps_dpp_add_u32<0x111, 0xf>(w);
      w = ps_dpp_add_u32<0x112, 0xf>(w);
      w = ps_dpp_add_u32<0x114, 0xf>(w);
      w = ps_dpp_add_u32<0x118, 0xf>(w);                          // lane i < 16: wtot[0] + .. + wtot[i]
      const unsigned basew = (wv == 0) ? 0u : (unsigned)__builtin_amdgcn_readlane((int)w, wv > 0 ? wv - 1 : 0);
      const unsigned ex = basew + inc - v;
      reinterpret_cast<uint2*>(off)[tid] = make_uint2(ex, ex + c2.x);
      if (c2.x > PS_HEAVY || c2.y > PS_HEAVY) {                   // rare: list the heavy cells, flag them for their owners
        if (c2.x > PS_HEAVY) {
          const unsigned hs = __hip_atomic_fetch_add(nheavy_p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          hlist[3 * hs] = 2 * tid; hlist[3 * hs + 1] = c2.x; hlist[3 * hs + 2] = ex;
          cntb[2 * tid] = 0x80000000u | hs;
        }
        if (c2.y > PS_HEAVY) {
          const unsigned hs = __hip_atomic_fetch_add(nheavy_p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          hlist[3 * hs] = 2 * tid + 1; hlist[3 * hs + 1] = c2.y; hlist[3 * hs + 2] = ex + c2.x;
          cntb[2 * tid + 1] = 0x80000000u | hs;
        }
      }
    }
    ps_lds_barrier();
    // ---- P3: (s, w y) and w into cell order
    {
      unsigned pos[TP];
#pragma unroll
      for (int q = 0; q < TP; ++q) pos[q] = off[(cr[q] >> 13) & (PS_NCELL - 1)] + (unsigned)(cr[q] & 8191);
#pragma unroll
      for (int q = 0; q < TP; ++q)
        if (cr[q] >= 0) { buf[pos[q]] = make_double2(sv[q], yv[q]); wpl[pos[q]] = ws[q]; }
    }
    ps_lds_barrier();
    // ---- P4: owners accumulate their two cells' moments (one cell after the other)
    {
      unsigned nA = cntb[tid], nB = cntb[tid + PS_THREADS];
      const unsigned oA = off[tid], oB = off[tid + PS_THREADS];
      const unsigned nheavy = *nheavy_p;
      cntb[tid] = 0; cntb[tid + PS_THREADS] = 0;                  // (owner-exclusive; this buffer is next used two tiles on)
      if (nheavy > 0) {                                           // (workgroup-uniform) sorted / clustered input
        const bool hvA = (nA & 0x80000000u) != 0, hvB = (nB & 0x80000000u) != 0;
        const unsigned slA = nA & 0x7fffffffu, slB = nB & 0x7fffffffu;
        if (hvA) { n0A += hlist[3 * slA + 1]; nA = 0; }
        if (hvB) { n0B += hlist[3 * slB + 1]; nB = 0; }
        for (unsigned r0 = 0; r0 < nheavy; r0 += PS_HROUND) {
          if (tid < PS_HROUND * NSTAT) hacc[tid] = 0.0;
          ps_lds_barrier();
          const unsigned rn = nheavy - r0 < (unsigned)PS_HROUND ? nheavy - r0 : (unsigned)PS_HROUND;
          const int per = rn == 1 ? 16 : (rn == 2 ? 8 : 4), sh_per = rn == 1 ? 4 : (rn == 2 ? 3 : 2);
          for (unsigned hh = 0; hh < rn; ++hh) {
            const unsigned hn = hlist[3 * (r0 + hh) + 1], ho = hlist[3 * (r0 + hh) + 2];
            const bool mine = rn <= 2 ? (wv >> sh_per) == (int)hh : (wv >> 2) == (int)(hh & 3u);
            if (mine && (unsigned)(wv & (per - 1)) < ((hn + 63u) >> 6))
              psw_heavy_slices<K>(buf, wpl, hn, ho, wv & (per - 1), per, lane, hacc + hh * NSTAT);
          }
          ps_lds_barrier();
          if (hvA && slA >= r0 && slA < r0 + PS_HROUND) {
#pragma unroll
            for (int p = 0; p < NS; ++p) SA[p] += hacc[(slA - r0) * NSTAT + p];
#pragma unroll
            for (int p = 0; p <= K; ++p) TA[p] += hacc[(slA - r0) * NSTAT + NS + p];
            W0A += hacc[(slA - r0) * NSTAT + NS + K + 1];
          }
          if (hvB && slB >= r0 && slB < r0 + PS_HROUND) {
#pragma unroll
            for (int p = 0; p < NS; ++p) SB[p] += hacc[(slB - r0) * NSTAT + p];
#pragma unroll
            for (int p = 0; p <= K; ++p) TB[p] += hacc[(slB - r0) * NSTAT + NS + p];
            W0B += hacc[(slB - r0) * NSTAT + NS + K + 1];
          }
          if (r0 + PS_HROUND < nheavy) ps_lds_barrier();
        }
      }
      n0A += nA; n0B += nB;
      load_tile(tile + 1);                                        // the next tile's loads fly under the owner loops (clamped: the last one re-reads the final pair)
      psw_own_cell<K, T>(buf, wpl, nA, oA, W0A, SA, TA);
      psw_own_cell<K, T>(buf, wpl, nB, oB, W0B, SB, TB);
    }
  }

  // ---- epilogue: moments -> band / rhs entries of this workgroup (the LDS image aliases the sort buffers)
  double tot = block_sum(tacc[tid0], scratch);                    // (its barriers also end the last owner phase)
  const double badf = block_sum((double)nbad, scratch + 32);
  const double tw = block_sum(tacc[PS_THREADS + tid0], scratch), tl = block_sum(tacc[2 * PS_THREADS + tid0], scratch + 32),
               tn = block_sum(tacc[3 * PS_THREADS + tid0], scratch);
  __syncthreads();
  double* out = a.partials + (size_t)blockIdx.x * ((size_t)(K + 2) * M + 1);
  int col_lo = 0, col_hi = M - 1;
  if (a.ranges) {   // the columns this workgroup has anything for (as phi_sort_kernel)
    const unsigned mn = n0A ? (unsigned)tid : (n0B ? (unsigned)(tid + PS_THREADS) : 0x7fffffu);
    const unsigned mx = n0B ? (unsigned)(tid + PS_THREADS) + 1u : (n0A ? (unsigned)tid + 1u : 0u);   // (+1: 0 = no cell)
    const unsigned wmn = ps_wave_min_u32(mn), wmx = ps_wave_max_u32(mx);
    if (lane == 0) { wtot[wv] = wmn; wtot[16 + wv] = wmx; }
    __syncthreads();
    const unsigned bmn = ps_wave_min_u32(wtot[lane & 15]), bmx = ps_wave_max_u32(wtot[16 + (lane & 15)]);
    col_lo = bmx ? (int)bmn : 1;
    col_hi = bmx ? (int)bmx - 1 + K : 0;
    if (col_hi > M - 1) col_hi = M - 1;
    if (tid == 0) { a.ranges[2 * blockIdx.x] = col_lo; a.ranges[2 * blockIdx.x + 1] = col_hi; }
    __syncthreads();
  }
  {
    // the MomTab epilogue of phi_sort_kernel, S_0 = sum w in place of the count
    constexpr int IW = PS_THREADS + K;
    double* img = lds;
    auto q_planes = [&](const double (&S)[NS], double s0v, unsigned n0, int slot, int d0, int d1) __attribute__((always_inline)) {
      int pid = 0;
      if (!__any(n0 != 0u)) {
#pragma unroll
        for (int d = d0; d < d1; ++d)
#pragma unroll
          for (int i = 0; i + d <= K; ++i) img[(pid++) * IW + slot] = 0.0;
        return;
      }
#pragma unroll
      for (int d = d0; d < d1; ++d) {
#pragma unroll
        for (int i = 0; i + d <= K; ++i) {
          const int j = i + d, mi = K - j, mj = K - i;             // (mi, mj): the mirror pair, same sub-diagonal
          (void)mj;
          if (mi < i) continue;                                    // written together with its mirror
          double e = MomCoef<K>::tab.pair[i][j][0] * s0v, o = 0.0;
#pragma unroll
          for (int p = 2; p <= NS; p += 2) e = fma(MomCoef<K>::tab.pair[i][j][p], S[p - 1], e);
          if (mi != i) {
#pragma unroll
            for (int p = 1; p <= NS; p += 2) o = fma(MomCoef<K>::tab.pair[i][j][p], S[p - 1], o);
            img[(pid + mi) * IW + slot] = e - o;
          }
          img[(pid + i) * IW + slot] = e + o;
        }
        pid += K + 1 - d;
      }
    };
    auto r_planes = [&](const double (&Tm)[K + 1], int slot, int plane0) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; 2 * i <= K; ++i) {
        double e = 0.0, o = 0.0;
#pragma unroll
        for (int p = 0; p <= K; p += 2) e = fma(MomCoef<K>::tab.single[i][p], Tm[p], e);
        if (2 * i != K) {
#pragma unroll
          for (int p = 1; p <= K; p += 2) o = fma(MomCoef<K>::tab.single[i][p], Tm[p], o);
          img[(plane0 + K - i) * IW + slot] = e - o;
        }
        img[(plane0 + i) * IW + slot] = e + o;
      }
    };
    constexpr int DSPLIT = (K <= 4) ? K + 1 : 2;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int j = half * PS_THREADS + tid;                       // this thread's column (= its cell) in the half
#pragma unroll
      for (int rnd = 0; rnd < (DSPLIT <= K ? 2 : 1); ++rnd) {
        const int d0 = rnd == 0 ? 0 : DSPLIT, d1 = rnd == 0 ? DSPLIT : K + 1;
        if (half == 0) q_planes(SA, W0A, n0A, K + tid, d0, d1); else q_planes(SB, W0B, n0B, K + tid, d0, d1);
        if (tid >= PS_THREADS - K) {                               // the K cells below the half: none (zeros), or the top cells of half A
          const int hs = tid - (PS_THREADS - K);
          if (half == 0) {
            int np = 0;
#pragma unroll
            for (int d = d0; d < d1; ++d) np += K + 1 - d;
            for (int pl = 0; pl < np; ++pl) img[pl * IW + hs] = 0.0;
          } else {
            q_planes(SA, W0A, n0A, hs, d0, d1);
          }
        }
        ps_lds_barrier();
        if (j < M && j >= col_lo && j <= col_hi) {
          int pid = 0;
#pragma unroll
          for (int d = d0; d < d1; ++d) {
            double v = 0.0;
#pragma unroll
            for (int jj = d; jj <= K; ++jj) v += img[(pid + jj - d) * IW + tid + jj];
            __builtin_nontemporal_store((j + d < M) ? v : 0.0, out + (size_t)d * M + j);
            pid += K + 1 - d;
          }
        }
        ps_lds_barrier();
      }
    }
    // rhs: both halves in one round (2 (K+1) planes)
    r_planes(TA, K + tid, 0);
    r_planes(TB, K + tid, K + 1);
    if (tid >= PS_THREADS - K) {
      const int hs = tid - (PS_THREADS - K);
#pragma unroll
      for (int i = 0; i <= K; ++i) img[i * IW + hs] = 0.0;
      r_planes(TA, hs, K + 1);
    }
    ps_lds_barrier();
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int j = half * PS_THREADS + tid;
      if (j < M && j >= col_lo && j <= col_hi) {
        double r = 0.0;
#pragma unroll
        for (int i = 0; i <= K; ++i) r += img[(half * (K + 1) + i) * IW + tid + i];
        __builtin_nontemporal_store(r, out + (size_t)(K + 1) * M + j);
      }
    }
    if (tid == 0) {
      out[(size_t)(K + 2) * M] = (badf > 0.0) ? __builtin_nan("") : tot;   // a point outside the mesh or an invalid weight: loud (NaN yy_w)
      double* wp = aw.wpart + (size_t)blockIdx.x * 4;
      wp[0] = tw; wp[1] = tl; wp[2] = tn; wp[3] = 0.0;
    }
  }
}

}  // namespace asvgp
