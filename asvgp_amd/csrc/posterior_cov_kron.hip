// Full posterior covariance of the 2-D model (GPR_kron):
//   asvgp_kron_dense_inverse   the dense Sigma = P^-1 from the block-bidiagonal factor's G_j = L_{j+1,j} L_jj^-1 and the selected
//                              inverse on the band (SigD, SigS), one-sided or two-sided ("twisted") layout;
//   asvgp_predict_cov_kron2d   cov[a, b] = k1(x1_a1, x2_b1) k2(x1_a2, x2_b2) + phi(x1_a)^T Sigma phi(x2_b)
//                                          - (phi1^T K1^-1 phi1')(phi2^T K2^-1 phi2').
//
// Dense completion.  From Sigma L = L^-T (upper triangular in elimination order), for every block row i eliminated after block
// column j:  Sigma_{i,j} = -Sigma_{i,j+1} G_j.  The seeds Sigma_jj = SigD_j, Sigma_{j+1,j} = SigS_j are copied in unchanged (and SigS_j
// mirrored); the sweep runs j downwards, one launch per step: inside a step every block row is an independent Bb x Bb product on the
// fp64 matrix core (v_mfma_f64_16x16x4), reading Sigma_{i,j+1} straight from the output and writing Sigma_{i,j} and its mirror.
// Super-block (stack s, block b) row r is original index base_s + sgn_s (b Bb + r), valid while lo_s <= b Bb + r < hi_s: padding
// rows read as 0 and are never stored.  Twisted layout: stack 0 = top (padt identity columns, then 0 .. top_end-1), stack 1 = bottom
// reversed (padb identity columns, then M-1 .. h), the separator the last block of both.  Elimination order top interior, bottom
// interior, separator, so (1) stack 1's columns are swept with its later blocks and the separator as rows - (bottom u sep)^2 - then
// (2) stack 0's columns with its later blocks, the separator and every bottom interior block as rows.
#include "asvgp_common.hpp"

namespace asvgp {

struct StackMap {
  long base, lo, hi;
  int sgn;
  __device__ __forceinline__ long orig(int b, int Bb, int r) const {
    const long t = (long)b * Bb + r;
    return (t >= lo && t < hi) ? base + sgn * t : -1;
  }
};

// ---- seeds: SigD_b at (b, b), SigS_b at (b+1, b) and mirrored at (b, b+1), bit for bit.  blockIdx.y = seed block: [0, nd) diagonal
// blocks of stack s0, then the sub-diagonal blocks of stack 0 and of stack 1 (ns0 / ns1 of them).
constexpr int DI_TILE = 64;
__global__ __launch_bounds__(256) void dense_inv_seed_kernel(const double* __restrict__ SigD, const double* __restrict__ SigS, StackMap s0,
                                                             StackMap s1, int Bb, int nd, int ns0, int ns1, long nbS, long M,
                                                             double* __restrict__ Sig) {
  int y = blockIdx.y;
  const double* src;
  StackMap mp;
  int br, bc;
  bool mirror;
  if (y < nd) { src = SigD + (long)y * Bb * Bb; mp = s0; br = bc = y; mirror = false; }
  else if ((y -= nd) < ns0) { src = SigS + (long)y * Bb * Bb; mp = s0; br = y + 1; bc = y; mirror = true; }
  else { y -= ns0; src = SigS + (nbS + y) * Bb * Bb; mp = s1; br = y + 1; bc = y; mirror = true; }
  const long n = (long)Bb * Bb;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
    const int r = (int)(e / Bb), c = (int)(e % Bb);
    const long gr = mp.orig(br, Bb, r), gc = mp.orig(bc, Bb, c);
    if (gr < 0 || gc < 0) continue;
    const double v = src[e];
    Sig[gr * M + gc] = v;
    if (mirror) Sig[gc * M + gr] = v;
  }
}

// ---- one step of the sweep: Sigma_{I, J} = -Sigma_{I, J+1} G_J for the row blocks I of this step (blockIdx.y), one 64 x 64 tile of the
// Bb x Bb product per workgroup (blockIdx.x).  Four waves, 32 x 32 each (2 x 2 MFMA tiles), K in chunks of 32 staged through the LDS;
// the result goes through the LDS once more so that both Sigma_{I,J} and its mirror are stored coalesced.
constexpr int DI_KC = 32;
constexpr int DI_AS = DI_KC + 1;          // LDS strides (odd: bank spread)
constexpr int DI_GS = DI_TILE + 1;
constexpr int DI_LDS = (DI_TILE * DI_AS + DI_KC * DI_GS) > (DI_TILE * DI_GS) ? (DI_TILE * DI_AS + DI_KC * DI_GS) : (DI_TILE * DI_GS);
typedef double di_d4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void dense_inv_step_kernel(const double* __restrict__ G, StackMap cm, int J, StackMap rm_same, int i0_same,
                                                             int n_same, StackMap rm_other, int Bb, long M, double* __restrict__ Sig) {
  __shared__ double lds[DI_LDS];
  double* As = lds;                       // As[r][q]: Sigma_{I, J+1} tile rows, K chunk
  double* Gs = lds + DI_TILE * DI_AS;     // Gs[q][c]: G_J chunk rows, tile columns
  const int nt = (Bb + DI_TILE - 1) / DI_TILE;
  const int tr = blockIdx.x / nt, tc = blockIdx.x % nt;
  const int y = blockIdx.y;
  const StackMap rm = y < n_same ? rm_same : rm_other;
  const int I = y < n_same ? i0_same + y : y - n_same;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ln = lane & 15, lg = lane >> 4;
  const int wr = (w >> 1) * 32, wc = (w & 1) * 32;
  const int r0 = tr * DI_TILE, c0 = tc * DI_TILE;
  // this thread's A rows (8 of them) and their original indices
  const int aq = tid & 31, ar = tid >> 5;  // A tile: column aq of the chunk, rows ar + 8 i
  long arow[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = r0 + ar + 8 * i;
    arow[i] = r < Bb ? rm.orig(I, Bb, r) : -1;
  }
  const int gc = tid & 63, gq = tid >> 6;  // G tile: column gc, chunk rows gq + 4 i
  const bool gcol_ok = c0 + gc < Bb;
  di_d4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = di_d4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < Bb; k0 += DI_KC) {
    const long acol = cm.orig(J + 1, Bb, k0 + aq);
#pragma unroll
    for (int i = 0; i < 8; ++i) As[(ar + 8 * i) * DI_AS + aq] = (arow[i] >= 0 && acol >= 0) ? Sig[arow[i] * M + acol] : 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) Gs[(gq + 4 * i) * DI_GS + gc] = gcol_ok ? G[(long)(k0 + gq + 4 * i) * Bb + c0 + gc] : 0.0;
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < DI_KC; kk += 4) {
      double a[2], b[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        a[t] = As[(wr + 16 * t + ln) * DI_AS + kk + lg];
        b[t] = Gs[(kk + lg) * DI_GS + wc + 16 * t + ln];
      }
#pragma unroll
      for (int ta = 0; ta < 2; ++ta)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) acc[ta][tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ta], b[tb], acc[ta][tb], 0, 0, 0);
    }
    __syncthreads();
  }
  // C tile -> LDS (Cs[r][c]), then stored twice: rows along the lanes of the mirror, columns along the lanes of Sigma_{I,J}
  double* Cs = lds;
#pragma unroll
  for (int ta = 0; ta < 2; ++ta)
#pragma unroll
    for (int tb = 0; tb < 2; ++tb)
#pragma unroll
      for (int i = 0; i < 4; ++i) Cs[(wr + 16 * ta + lg + 4 * i) * DI_GS + wc + 16 * tb + ln] = -acc[ta][tb][i];
  __syncthreads();
  const int sx = tid & 63, sy = tid >> 6;
  const long ox = (c0 + sx < Bb) ? cm.orig(J, Bb, c0 + sx) : -1;   // column of Sigma_{I,J} on the lane
  const long oxr = (r0 + sx < Bb) ? rm.orig(I, Bb, r0 + sx) : -1;  // row of Sigma_{I,J} on the lane (mirror store)
  for (int j = sy; j < DI_TILE; j += 4) {
    const long gr = (r0 + j < Bb) ? rm.orig(I, Bb, r0 + j) : -1;
    if (gr >= 0 && ox >= 0) Sig[gr * M + ox] = Cs[j * DI_GS + sx];
    const long gcm = (c0 + j < Bb) ? cm.orig(J, Bb, c0 + j) : -1;
    if (gcm >= 0 && oxr >= 0) Sig[gcm * M + oxr] = Cs[sx * DI_GS + j];
  }
}

static void launch_step(const double* G, StackMap cm, int J, StackMap rs, int i0, int n_same, StackMap ro, int n_other, int Bb, long M,
                        double* Sig, hipStream_t st) {
  const int nrows = n_same + n_other;
  if (nrows <= 0) return;
  const int nt = (Bb + DI_TILE - 1) / DI_TILE;
  hipLaunchKernelGGL(dense_inv_step_kernel, dim3((unsigned)(nt * nt), (unsigned)nrows), dim3(256), 0, st, G + (long)J * Bb * Bb, cm, J, rs,
                     i0, n_same, ro, Bb, M, Sig);
}

// ---------------------------------------------------------------------------------------------------------
// cross-covariance: per workgroup R rows a; g_a = phi(x1_a)^T Sigma (M_tot doubles: (k+1) runs of k+1 consecutive rows at stride m2)
// and the two 1-D rows u_d = phi_d(x1_ad)^T K_d^-1 in the LDS, the x2 points swept across the lanes.
// ---------------------------------------------------------------------------------------------------------
constexpr int CK_THREADS = 256;
constexpr int CK_ROWS = 4;                           // rows a per workgroup when R (M_tot + m1 + m2) doubles fit CK_LDS_PREF
constexpr size_t CK_LDS_PREF = 64 * 1024;
constexpr size_t CK_LDS_MAX = 156 * 1024;            // one row alone may take up to this (the 1-D kernel's plan)

__device__ __forceinline__ double matern_k(int kind, double v, double inv_l, double x, double y) {
  const double r = fabs(x - y) * inv_l;
  if (kind == ASVGP_MATERN12) return v * exp(-r);
  if (kind == ASVGP_MATERN32) {
    const double sr = 1.7320508075688772 * r;
    return v * (1.0 + sr) * exp(-sr);
  }
  const double sr = 2.23606797749979 * r;
  return v * (1.0 + sr + (5.0 / 3.0) * r * r) * exp(-sr);
}

struct CovDim {
  const double* mesh;
  int n_mesh, m, kind;
  double inv_delta, v, inv_l;
};

template <int K>
__device__ __forceinline__ int cell_weights(const CovDim& d, double x, double (&w)[K + 1]) {
  const int idx = neighbour_index(x, d.mesh, d.n_mesh, d.mesh[0], d.inv_delta);
  bspline_pieces<K>((x - d.mesh[idx]) * d.inv_delta, w);
  return idx;
}

template <int K, int R>
__global__ __launch_bounds__(CK_THREADS) void predict_cov_kron2d_kernel(const double* __restrict__ x1, long n1, const double* __restrict__ x2,
                                                                        long n2, CovDim d1, CovDim d2, const double* __restrict__ Sig,
                                                                        const double* __restrict__ K1i, const double* __restrict__ K2i,
                                                                        long chunk, double* __restrict__ cov, long ldc) {
  extern __shared__ double g[];                      // row r: [g_a (M_tot) | u_1 (m1) | u_2 (m2)]
  const int m1 = d1.m, m2 = d2.m;
  const long Mt = (long)m1 * m2;
  const long RS = Mt + m1 + m2;
  const long a0 = (long)blockIdx.x * R;
  const int nr = (n1 - a0 < R) ? (int)(n1 - a0) : R;
  double xa[R], ya[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    xa[r] = r < nr ? x1[2 * (a0 + r)] : 0.0;
    ya[r] = r < nr ? x1[2 * (a0 + r) + 1] : 0.0;
    if (r < nr) {                                    // (uniform: every lane evaluates row a's cell and weights)
      double v1[K + 1], v2[K + 1];
      const int i1 = cell_weights<K>(d1, xa[r], v1);
      const int i2 = cell_weights<K>(d2, ya[r], v2);
      double* gr = g + r * RS;
      for (long m = threadIdx.x; m < Mt; m += CK_THREADS) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i <= K; ++i) {
          const double* row = Sig + ((long)(i1 + K - i) * m2 + i2 + K) * Mt + m;
          double t = 0.0;
#pragma unroll
          for (int j = 0; j <= K; ++j) t = fma(v2[j], row[-(long)j * Mt], t);
          acc = fma(v1[i], t, acc);
        }
        gr[m] = acc;
      }
      for (int m = threadIdx.x; m < m1 + m2; m += CK_THREADS) {
        double acc = 0.0;
        if (m < m1) {
#pragma unroll
          for (int i = 0; i <= K; ++i) acc = fma(v1[i], K1i[(long)(i1 + K - i) * m1 + m], acc);
        } else {
#pragma unroll
          for (int i = 0; i <= K; ++i) acc = fma(v2[i], K2i[(long)(i2 + K - i) * m2 + (m - m1)], acc);
        }
        gr[Mt + m] = acc;
      }
    }
  }
  __syncthreads();
  const long b_end = ((long)blockIdx.y + 1) * chunk < n2 ? ((long)blockIdx.y + 1) * chunk : n2;
  for (long b = (long)blockIdx.y * chunk + threadIdx.x; b < b_end; b += CK_THREADS) {
    const double xb = x2[2 * b], yb = x2[2 * b + 1];
    double w1[K + 1], w2[K + 1];
    const int j1 = cell_weights<K>(d1, xb, w1);
    const int j2 = cell_weights<K>(d2, yb, w2);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (r < nr) {
        const double* gr = g + r * RS;
        double q = 0.0, q1 = 0.0, q2 = 0.0;
#pragma unroll
        for (int i = 0; i <= K; ++i) {
          const double* row = gr + (long)(j1 + K - i) * m2 + j2 + K;
          double t = 0.0;
#pragma unroll
          for (int j = 0; j <= K; ++j) t = fma(w2[j], row[-j], t);
          q = fma(w1[i], t, q);
          q1 = fma(w1[i], gr[Mt + j1 + K - i], q1);
          q2 = fma(w2[i], gr[Mt + m1 + j2 + K - i], q2);
        }
        const double kk = matern_k(d1.kind, d1.v, d1.inv_l, xa[r], xb) * matern_k(d2.kind, d2.v, d2.inv_l, ya[r], yb);
        cov[(a0 + r) * ldc + b] = kk + q - q1 * q2;
      }
    }
  }
}

template <int K>
static int launch_cov_kron(const double* x1, long n1, const double* x2, long n2, CovDim d1, CovDim d2, const double* Sig,
                           const double* K1i, const double* K2i, double* cov, long ldc, hipStream_t st) {
  const size_t row_bytes = sizeof(double) * ((size_t)d1.m * d2.m + d1.m + d2.m);
  const int R = (CK_ROWS * row_bytes <= CK_LDS_PREF) ? CK_ROWS : 1;
  const size_t lds = R * row_bytes;
  const long gx = (n1 + R - 1) / R;
  // column chunks: enough workgroups to fill the device when n1 is small (each chunk forms its rows' g_a again)
  long gy = (1024 + gx - 1) / gx;
  const long gy_max = (n2 + CK_THREADS - 1) / CK_THREADS;
  if (gy > gy_max) gy = gy_max;
  if (gy < 1) gy = 1;
  const long chunk = (n2 + gy - 1) / gy;
  gy = (n2 + chunk - 1) / chunk;
  if (gx > 0x7fffffff || gy > 65535) { set_error("predict_cov_kron2d: n1 = %ld, n2 = %ld too large for one launch", n1, n2); return ASVGP_ERR_UNSUPPORTED; }
  auto kern = R == CK_ROWS ? predict_cov_kron2d_kernel<K, CK_ROWS> : predict_cov_kron2d_kernel<K, 1>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) { set_error("predict_cov_kron2d: hipFuncSetAttribute: %s", hipGetErrorString(e)); return ASVGP_ERR_LDS_CAPACITY; }
  hipLaunchKernelGGL(kern, dim3((unsigned)gx, (unsigned)gy), dim3(CK_THREADS), lds, st, x1, n1, x2, n2, d1, d2, Sig, K1i, K2i, chunk, cov, ldc);
  return check_launch("predict_cov_kron2d");
}

}  // namespace asvgp

using namespace asvgp;

extern "C" int asvgp_kron_dense_inverse(const double* G, const double* SigD, const double* SigS, int64_t M, int64_t Bb, int twisted,
                                        int64_t nb, int64_t top_end, int64_t padt, int64_t padb, double* Sigma, asvgp_stream_t stream) {
  if (!SigD || !Sigma || M < 1 || Bb < 32 || (twisted != 0 && twisted != 1)) { set_error("kron_dense_inverse: bad argument"); return ASVGP_ERR_BAD_ARG; }
  if (Bb % 32 != 0) { set_error("kron_dense_inverse: Bb = %ld is not a multiple of 32", (long)Bb); return ASVGP_ERR_BAD_ARG; }
  if ((double)M * (double)M > 9.0e18 / 8.0 || Bb > 65536) { set_error("kron_dense_inverse: M = %ld too large", (long)M); return ASVGP_ERR_UNSUPPORTED; }
  if (!twisted) {
    if (nb != (M + Bb - 1) / Bb || top_end != 0 || padt != 0 || padb != 0) {
      set_error("kron_dense_inverse: inconsistent one-sided layout (nb = %ld must be ceil(M / Bb) = %ld, top_end = padt = padb = 0)", (long)nb,
                (long)((M + Bb - 1) / Bb));
      return ASVGP_ERR_BAD_ARG;
    }
  } else if (!(nb >= 2 && top_end >= Bb && top_end <= M && padt >= 0 && padb >= 0 && top_end + padt == nb * Bb &&
               (M - (top_end - Bb)) + padb == nb * Bb)) {
    set_error("kron_dense_inverse: inconsistent twisted layout (nb = %ld, top_end = %ld, padt = %ld, padb = %ld, M = %ld, Bb = %ld)", (long)nb,
              (long)top_end, (long)padt, (long)padb, (long)M, (long)Bb);
    return ASVGP_ERR_BAD_ARG;
  }
  if (nb > 1 && (!G || !SigS)) { set_error("kron_dense_inverse: G / SigS is null"); return ASVGP_ERR_BAD_ARG; }
  hipStream_t st = as_stream(stream);
  const int bb = (int)Bb, n = (int)nb;
  const unsigned sx = (unsigned)((Bb * Bb + 255) / 256 < 1024 ? (Bb * Bb + 255) / 256 : 1024);
  const long BB2 = Bb * Bb;
  if (!twisted) {
    const StackMap s{0, 0, M, +1};
    hipLaunchKernelGGL(dense_inv_seed_kernel, dim3(sx, (unsigned)(2 * n - 1)), dim3(256), 0, st, SigD, SigS, s, s, bb, n, n - 1, 0, (long)(n - 1),
                       (long)M, Sigma);
    for (int J = n - 3; J >= 0; --J) launch_step(G, s, J, s, J + 2, n - J - 2, s, 0, bb, (long)M, Sigma, st);
    return check_launch("kron_dense_inverse");
  }
  const StackMap top{-padt, padt, nb * Bb, +1};
  const StackMap bot{M - 1 + padb, padb, nb * Bb, -1};
  // seeds: every diagonal block of the top stack (the separator included), the bottom stack's interior diagonal blocks, both SigS stacks
  hipLaunchKernelGGL(dense_inv_seed_kernel, dim3(sx, (unsigned)(n + 2 * (n - 1))), dim3(256), 0, st, SigD, SigS, top, bot, bb, n, n - 1, n - 1,
                     (long)(n - 1), (long)M, Sigma);
  hipLaunchKernelGGL(dense_inv_seed_kernel, dim3(sx, (unsigned)(n - 1)), dim3(256), 0, st, SigD + (long)n * BB2, SigS, bot, bot, bb, n - 1, 0, 0,
                     (long)(n - 1), (long)M, Sigma);
  const double* Gt = G;
  const double* Gb = G + (long)(n - 1) * BB2;
  for (int J = n - 3; J >= 0; --J) launch_step(Gb, bot, J, bot, J + 2, n - J - 2, bot, 0, bb, (long)M, Sigma, st);       // (1)
  for (int J = n - 2; J >= 0; --J) launch_step(Gt, top, J, top, J + 2, n - J - 2, bot, n - 1, bb, (long)M, Sigma, st);   // (2)
  return check_launch("kron_dense_inverse");
}

// handle: accepted like asvgp_predict_cov_1d's (NULL = the process default); the kernel keeps no per-handle state
extern "C" int asvgp_predict_cov_kron2d(asvgp_handle_t handle, const double* x1, int64_t n1, const double* x2, int64_t n2, const double* mesh1,
                                        int64_t n_mesh1, double delta1, int64_t m1, const double* mesh2, int64_t n_mesh2, double delta2,
                                        int64_t m2, int order, const double* Sigma, const double* K1inv, const double* K2inv, int kind1,
                                        double variance1, double lengthscale1, int kind2, double variance2, double lengthscale2, double* cov,
                                        int64_t ldc, asvgp_stream_t stream) {
  (void)handle;
  if (!x1 || !x2 || !mesh1 || !mesh2 || !Sigma || !K1inv || !K2inv || !cov || n1 < 0 || n2 < 0 || ldc < n2 || !(delta1 > 0.0) ||
      !(delta2 > 0.0) || !(variance1 > 0.0) || !(lengthscale1 > 0.0) || !(variance2 > 0.0) || !(lengthscale2 > 0.0)) {
    set_error("predict_cov_kron2d: bad argument");
    return ASVGP_ERR_BAD_ARG;
  }
  if (order < 1 || order > ASVGP_MAX_ORDER) { set_error("predict_cov_kron2d: order %d unsupported", order); return ASVGP_ERR_UNSUPPORTED; }
  if (kind1 < ASVGP_MATERN12 || kind1 > ASVGP_MATERN52 || kind2 < ASVGP_MATERN12 || kind2 > ASVGP_MATERN52) {
    set_error("predict_cov_kron2d: kernel kinds %d, %d unsupported", kind1, kind2);
    return ASVGP_ERR_UNSUPPORTED;
  }
  if (m1 < order + 1 || n_mesh1 != m1 - order + 1 || m2 < order + 1 || n_mesh2 != m2 - order + 1) {
    set_error("predict_cov_kron2d: bad argument (n_mesh = %ld / %ld, m = %ld / %ld, order %d)", (long)n_mesh1, (long)n_mesh2, (long)m1, (long)m2, order);
    return ASVGP_ERR_BAD_ARG;
  }
  if (sizeof(double) * ((size_t)m1 * (size_t)m2 + (size_t)m1 + (size_t)m2) > CK_LDS_MAX) {
    set_error("predict_cov_kron2d: a row of Sigma (M_tot = %ld) and the two 1-D rows do not fit the kernel's LDS plan", (long)(m1 * m2));
    return ASVGP_ERR_UNSUPPORTED;
  }
  if (n1 == 0 || n2 == 0) return ASVGP_OK;
  const CovDim d1{mesh1, (int)n_mesh1, (int)m1, kind1, 1.0 / delta1, variance1, 1.0 / lengthscale1};
  const CovDim d2{mesh2, (int)n_mesh2, (int)m2, kind2, 1.0 / delta2, variance2, 1.0 / lengthscale2};
  hipStream_t st = as_stream(stream);
  switch (order) {
    case 1: return launch_cov_kron<1>(x1, n1, x2, n2, d1, d2, Sigma, K1inv, K2inv, cov, ldc, st);
    case 2: return launch_cov_kron<2>(x1, n1, x2, n2, d1, d2, Sigma, K1inv, K2inv, cov, ldc, st);
    case 3: return launch_cov_kron<3>(x1, n1, x2, n2, d1, d2, Sigma, K1inv, K2inv, cov, ldc, st);
    case 4: return launch_cov_kron<4>(x1, n1, x2, n2, d1, d2, Sigma, K1inv, K2inv, cov, ldc, st);
    case 5: return launch_cov_kron<5>(x1, n1, x2, n2, d1, d2, Sigma, K1inv, K2inv, cov, ldc, st);
    default: return launch_cov_kron<6>(x1, n1, x2, n2, d1, d2, Sigma, K1inv, K2inv, cov, ldc, st);
  }
}
