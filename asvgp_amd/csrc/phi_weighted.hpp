// Weighted Phi pass: the banded sufficient statistics of observations with per-row noise variance s / w_i,
//   A_w = Phi W Phi^T,  b_w = Phi W y,  yy_w = sum w_i y_i^2,   wstats = [sum w, sum_{w>0} log w, #{w > 0}].
// (included by phi_pass.hip behind the unweighted kernels, whose code it does not touch; it shares phi_reduce_kernel and the packed
// [band | Phi y | y^T y] layout, so every consumer of `stats` is served as it is.  Kernels only: the launch rules and the C entry are
// in phi_launch.hpp, next to the unweighted ones.)
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

}  // namespace asvgp
