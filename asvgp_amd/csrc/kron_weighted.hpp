// Weighted Khatri-Rao Phi pass (d = 2): A_w = Phi W Phi^T as the same block band, b_w = Phi W y, yy_w = sum w y^2 in the layout of
// asvgp_phi_accumulate_kron2d, plus wstats = [sum w, sum_{w>0} log w, #{w > 0}].  (Included by kron.hip behind the unweighted kernels,
// whose code it does not touch; the cell-sorted form shares phi_kron2d_gather_kernel.  Kernels only: the host side of both entries is
// kron_phi_launch.hpp.)
//   per point (asvgp_phi_accumulate_kron2d_weighted):   phi_kron2d_kernel with every product scaled by w; a row with w = 0 is skipped.
//   cell-sorted (asvgp_phi_accumulate_kron2d_sorted_weighted): a cell's share is Phi_c^T diag(w) Phi_c - the A operand of the
//     v_mfma_f64_16x16x4 products is w phi, the B operand phi; w travels beside (x, y) through the wave's LDS buffer (32 B per point).
// A negative, NaN or infinite weight: yy_w = NaN.
#pragma once

namespace asvgp {

__device__ __forceinline__ bool kron_weight_ok(double w) { return w >= 0.0 && w < __builtin_inf(); }   // (NaN fails both)

template <int K>
__global__ __launch_bounds__(256) void phi_kron2d_weighted_kernel(const double* __restrict__ X, const double* __restrict__ y, const double* __restrict__ wt,
                                                                  long N, const double* __restrict__ mesh1, int n1, double id1,
                                                                  int m1, const double* __restrict__ mesh2, int n2, double id2,
                                                                  int m2, double* __restrict__ Ablk, double* __restrict__ rhs,
                                                                  double* __restrict__ yy_out, double* __restrict__ wstats) {
  __shared__ double scratch[16];
  const long Mtot = (long)m1 * m2;
  double yy = 0.0, sw = 0.0, sl = 0.0, np = 0.0;
  for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (long)gridDim.x * blockDim.x) {
    const double wv = wt[n];
    if (!kron_weight_ok(wv)) { yy = __builtin_nan(""); continue; }
    if (wv == 0.0) continue;                                     // an absent row
    const double2 xv = *reinterpret_cast<const double2*>(X + 2 * n);
    const double yv = y[n];
    const int i1 = neighbour_index(xv.x, mesh1, n1, mesh1[0], id1);
    const int i2 = neighbour_index(xv.y, mesh2, n2, mesh2[0], id2);
    double v1[K + 1], v2[K + 1];
    bspline_pieces<K>((xv.x - mesh1[i1]) * id1, v1);
    bspline_pieces<K>((xv.y - mesh2[i2]) * id2, v2);
    yy = fma(wv * yv, yv, yy);
    sw += wv; sl += log(wv); np += 1.0;
#pragma unroll
    for (int a = 0; a <= K; ++a)
#pragma unroll
      for (int b = 0; b <= K; ++b) {
        const double u = wv * (v1[a] * v2[b]);
        const long row = (long)(i1 + K - a) * m2 + (i2 + K - b);
        __hip_atomic_fetch_add(rhs + row, u * yv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int a2 = a; a2 <= K; ++a2)  // d1 = a2 - a >= 0  (row block >= col block)
#pragma unroll
          for (int b2 = 0; b2 <= K; ++b2) {
            const int d1 = a2 - a, d2 = b2 - b;
            if (d1 == 0 && d2 < 0) continue;
            const long col = (long)(i1 + K - a2) * m2 + (i2 + K - b2);
            __hip_atomic_fetch_add(Ablk + (long)kron_off(K, d1, d2) * Mtot + col, u * v1[a2] * v2[b2], __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
          }
      }
  }
  const double tot = block_sum(yy, scratch);
  const double tw = block_sum(sw, scratch), tl = block_sum(sl, scratch), tn = block_sum(np, scratch);
  if (threadIdx.x == 0) {
    if (tot != 0.0) __hip_atomic_fetch_add(yy_out, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tn != 0.0) {
      __hip_atomic_fetch_add(wstats + 0, tw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(wstats + 1, tl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(wstats + 2, tn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// phi_kron2d_mfma_kernel with a weight: see the walk described there.  The weight sums (and the check of the weights) are taken where
// a lane parks ITS OWN point of a chunk - once per point, one log per point -, the weighted Gram matrix on the matrix core.
template <int K>
__global__ __launch_bounds__(64 * KRON_STRIP) void phi_kron2d_mfma_weighted_kernel(
    const double* __restrict__ X, const double* __restrict__ y, const double* __restrict__ wt, const long long* __restrict__ cell_start, int ncell,
    int ncell_pad, const double* __restrict__ mesh1, double id1, const double* __restrict__ mesh2, int n2, double id2,
    double* __restrict__ cellsum, double* __restrict__ yy_out, double* __restrict__ wstats) {
  using KO = KronOut<K>;
  constexpr int NB = (K + 1) * (K + 1), NT = (NB + 15) / 16, NTT = NT * (NT + 1) / 2;
  __shared__ double res[KO::NOUT * KRON_STRIP];
  __shared__ double2 stage_x[64 * KRON_STRIP];
  __shared__ double2 stage_yw[64 * KRON_STRIP];   // (y, w)
  __shared__ double scratch[16];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, ln = lane & 15, lg = lane >> 4;
  double ca[NT][K + 1], cb[NT][K + 1];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int m = 16 * t + ln, a = m / (K + 1), b = m % (K + 1);
#pragma unroll
    for (int q = 0; q <= K; ++q) { ca[t][q] = 0.0; cb[t][q] = 0.0; }
#pragma unroll
    for (int i = 0; i <= K; ++i) {
      if (m < NB && i == a) {
#pragma unroll
        for (int q = 0; q <= K; ++q) ca[t][q] = piece_coef<K, 0>(i, q);
      }
      if (m < NB && i == b) {
#pragma unroll
        for (int q = 0; q <= K; ++q) cb[t][q] = piece_coef<K, 0>(i, q);
      }
    }
  }
  short tgt[NTT][4];
  {
    int qi = 0;
#pragma unroll
    for (int tm = 0; tm < NT; ++tm)
#pragma unroll
      for (int tn = tm; tn < NT; ++tn, ++qi)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = 16 * tm + lg + 4 * i, n = 16 * tn + ln;
          int e = -1;
          if (m < NB && n < NB) {
            const int a = m / (K + 1), b = m % (K + 1), a2 = n / (K + 1), b2 = n % (K + 1);
            if (a < a2 || (a == a2 && b <= b2)) {
              e = 0;                                            // entries before (a, a2, b, b2) in the list order of KronOut
              for (int x = 0; x < a; ++x) e += (K + 1) * (K + 2) / 2 + (K - x) * (K + 1) * (K + 1);
              if (a2 > a) e += (K + 1) * (K + 2) / 2 + (a2 - a - 1) * (K + 1) * (K + 1) + b * (K + 1) + b2;
              else { for (int x = 0; x < b; ++x) e += K + 1 - x; e += b2 - b; }
            }
          }
          tgt[qi][i] = (short)e;
        }
  }
  double2* xs = stage_x + wv * 64;
  double2* yws = stage_yw + wv * 64;
  double yy = 0.0, sw = 0.0, sl = 0.0, npos = 0.0;
  int strip = blockIdx.x;
  auto cell_range = [&](int st, long long& a0, long long& a1) __attribute__((always_inline)) {
    const int c = st * KRON_STRIP + wv;
    const bool in = st * KRON_STRIP < ncell_pad && c < ncell;
    a0 = in ? cell_start[c] : 0;
    a1 = in ? cell_start[c + 1] : 0;
  };
  long long p0, p1e;
  cell_range(strip, p0, p1e);
  double2 xn = make_double2(0.0, 0.0), ywn = xn;
  if (p0 + lane < p1e) { xn = *reinterpret_cast<const double2*>(X + 2 * (p0 + lane)); ywn = make_double2(y[p0 + lane], wt[p0 + lane]); }
  for (; strip * KRON_STRIP < ncell_pad; strip += gridDim.x) {
    const int c0 = strip * KRON_STRIP, c = c0 + wv;
    kron_d4 acc[NTT];
    double r[NT];
#pragma unroll
    for (int q = 0; q < NTT; ++q) acc[q] = kron_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < NT; ++t) r[t] = 0.0;
    long long q0, q1e;                                            // the wave's next cell
    cell_range(strip + gridDim.x, q0, q1e);
    if (p1e > p0) {
      const int i1 = c / (n2 - 1), i2 = c - i1 * (n2 - 1);
      const double u1 = mesh1[i1], u2 = mesh2[i2];
      for (long long base = p0; base < p1e; base += 64) {
        {                                                          // this lane's own point of the chunk (lanes past the cell's end hold zeros)
          const double wq = ywn.y;
          if (!kron_weight_ok(wq)) { yy = __builtin_nan(""); ywn.y = 0.0; }
          else if (wq > 0.0) { sw += wq; sl += log(wq); npos += 1.0; yy = fma(wq * ywn.x, ywn.x, yy); }
        }
        xs[lane] = xn; yws[lane] = ywn;
        {
          const long long nb = base + 64 < p1e ? base + 64 + lane : q0 + lane;      // next chunk of this cell, else the next cell's first
          const long long ne = base + 64 < p1e ? p1e : q1e;
          if (nb < ne) { xn = *reinterpret_cast<const double2*>(X + 2 * nb); ywn = make_double2(y[nb], wt[nb]); }
          else { xn = make_double2(0.0, 0.0); ywn = xn; }
        }
        const int np = (int)(p1e - base < 64 ? p1e - base : 64);
        auto step = [&](int st4, bool masked) __attribute__((always_inline)) {
          const int pi = 4 * st4 + lg;
          const bool ok = !masked || pi < np;
          const double2 xv = xs[pi];
          const double2 yw = yws[pi];
          const double wq = ok ? yw.y : 0.0;
          const double yv = wq > 0.0 ? yw.x : 0.0;                 // (a row with w = 0 is absent, whatever its y)
          const double t1 = (xv.x - u1) * id1, t2 = (xv.y - u2) * id2;
          double phi[NT], phw[NT];
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            double va = ca[t][K], vb = cb[t][K];
#pragma unroll
            for (int q = K - 1; q >= 0; --q) { va = fma(va, t1, ca[t][q]); vb = fma(vb, t2, cb[t][q]); }
            phi[t] = ok ? va * vb : 0.0;
            phw[t] = wq * phi[t];
            r[t] = fma(phw[t], yv, r[t]);
          }
          int qi = 0;
#pragma unroll
          for (int tm = 0; tm < NT; ++tm)
#pragma unroll
            for (int tn = tm; tn < NT; ++tn, ++qi) acc[qi] = __builtin_amdgcn_mfma_f64_16x16x4f64(phw[tm], phi[tn], acc[qi], 0, 0, 0);
        };
        const int nfull = np >> 2;                                  // steps whose four points all exist: no masks
        for (int st4 = 0; st4 < nfull; ++st4) step(st4, false);
        if (np & 3) step(nfull, true);
      }
    } else if (q1e > q0) {
      if (q0 + lane < q1e) { xn = *reinterpret_cast<const double2*>(X + 2 * (q0 + lane)); ywn = make_double2(y[q0 + lane], wt[q0 + lane]); }
      else { xn = make_double2(0.0, 0.0); ywn = xn; }
    }
    p0 = q0; p1e = q1e;
#pragma unroll
    for (int q = 0; q < NTT; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (tgt[q][i] >= 0) res[(int)tgt[q][i] * KRON_STRIP + wv] = acc[q][i];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      double v = r[t];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (lg == 0 && 16 * t + ln < NB) res[(KO::NBAND + 16 * t + ln) * KRON_STRIP + wv] = v;
    }
    __syncthreads();
    for (int idx = tid; idx < KO::NOUT * KRON_STRIP; idx += 64 * KRON_STRIP) {
      const int o = idx / KRON_STRIP, cc = idx % KRON_STRIP;
      cellsum[(size_t)o * ncell_pad + c0 + cc] = res[idx];
    }
    __syncthreads();
  }
  const double tot = block_sum(yy, scratch);
  const double tw = block_sum(sw, scratch), tl = block_sum(sl, scratch), tn = block_sum(npos, scratch);
  if (tid == 0) {
    if (tot != 0.0) __hip_atomic_fetch_add(yy_out, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tn != 0.0) {
      __hip_atomic_fetch_add(wstats + 0, tw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(wstats + 1, tl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(wstats + 2, tn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace asvgp
