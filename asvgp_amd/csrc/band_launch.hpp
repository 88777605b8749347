// Host side of the four band operators (asvgp_cholesky_band, asvgp_inverse_from_cholesky_band and their two adjoints): which kernel one
// call launches and with what numbers, decided from integers alone BEFORE anything happens, then one launcher per operator that
// executes the plan.  (included by band_ops.hip behind every kernel: band_ops.hip holds the kernels, the element-wise entries,
// asvgp_solve_triang_mat, asvgp_matern_coeffs and asvgp_kuu_assemble.)
//
// An entry is: band_args_ok and its own null checks -> plan_band_op(op, M, k, band_ops_env()) -> refuse, or hand the plan to the
// operator's launcher under dispatch_k.  The launchers decide nothing.  asvgp_band_launch_plan_host shows the same plan_band_op to the
// CPU tests, with the environment as arguments.
#pragma once

namespace asvgp {

// ---- the plan -----------------------------------------------------------------------------------------------------------------
enum BandOp { BAND_CHOL = 0, BAND_INVERSE, BAND_CHOL_VJP, BAND_INVERSE_VJP };
enum BandKernel {
  BAND_SWEEP = 0,      // 64-thread register-window sweep (forward operators)
  BAND_STREAMED,       // lane-uniform register window(s), the band streamed through the LDS in segments (all four)
  BAND_WAVE,           // wave-parallel adjoint, both arrays whole in the LDS
  BAND_SEQUENTIAL      // single-thread adjoint sweep, its arrays in the LDS or in global memory
};
struct BandEnv { bool lds; int seg_blocks; };      // ASVGP_BAND_OPS_LDS != 0; ASVGP_BAND_OPS_SEG_BLOCKS (0: none)
struct BandPlan {
  int status; char msg[160];                       // != ASVGP_OK: refused, nothing below counts
  int kernel, threads;                             // BandKernel; one workgroup of `threads`
  size_t lds_bytes;                                // dynamic LDS, at most BAND_LDS_MAX
  int seg, cap, cap_fq;                            // STREAMED: blocks per segment, columns (rows) the LDS holds, factor doubles it holds (inverse's adjoint only)
  int arrays_in_lds;                               // SEQUENTIAL: the use_lds flag the kernel takes
};
constexpr int BAND_LDS_MAX = 160 * 1024;           // what a workgroup may ask for on gfx950

// The segment rule of the streamed kernels whose LDS holds columns of k+1 doubles: `budget / col_bytes` columns fit; a band of at most
// that many is ONE segment of ceil(M / block) blocks and the LDS holds exactly its M columns; a longer one is walked in segments of as
// many blocks of `block` columns as fit beside the `carry` columns that are staged with a segment without belonging to it.  The test
// override (seg_blocks, from min_override on) shortens the segments, never lengthens them.
struct BandSegments { int seg, cap; };
static BandSegments band_segments(long M, int budget, int col_bytes, int block, int carry, int seg_blocks, int min_override) {
  int cap = budget / col_bytes;
  int seg = M <= cap ? (int)((M + block - 1) / block) : (cap - carry) / block;
  if (seg_blocks >= min_override && seg_blocks < seg) { seg = seg_blocks; cap = seg * block + carry; }
  else if (M <= cap) cap = (int)M;
  return BandSegments{seg, cap};
}

// Which kernel and with what numbers.  Reads its arguments only: no HIP call, no environment.  Per operator the rules run in the
// order written; the first that applies is the plan.
static BandPlan plan_band_op(int op, long M, int k, BandEnv env) {
  BandPlan p{};
  auto refuse = [&p](int status, const char* fmt, auto... a) { p.status = status; snprintf(p.msg, sizeof(p.msg), fmt, a...); return p; };
  auto run = [&p](int kernel, int threads, size_t lds_bytes) { p.kernel = kernel; p.threads = threads; p.lds_bytes = lds_bytes; return p; };
  if (op < BAND_CHOL || op > BAND_INVERSE_VJP) return refuse(ASVGP_ERR_BAD_ARG, "band launch plan: unknown operator %d", op);
  if (k < 1 || k > ASVGP_MAX_BANDWIDTH) return refuse(ASVGP_ERR_UNSUPPORTED, "band launch plan: bandwidth %d outside 1..%d", k, (int)ASVGP_MAX_BANDWIDTH);
  if (M < 1 || M > 0x3fffffff) return refuse(ASVGP_ERR_UNSUPPORTED, "band launch plan: M = %ld outside 1..2^30 - 1", M);
  const int W = k + 1;
  const int sb = env.seg_blocks;

  if (op == BAND_CHOL || op == BAND_INVERSE) {
    // Streamed: whenever the band is longer than the kernel's register window (k+1 columns; the inverse: its first block pair, 2k+1).
    // Budget 156 KiB: the Cholesky kernel keeps a static word (the first bad pivot) beside the dynamic LDS; the inverse - as the parent
    // has it.  The Cholesky walks blocks of k+1 columns and stages the k+1 columns that enter the window behind a segment; the inverse
    // walks blocks of k columns (its window is k x k) and reads ONE column ahead.  An override of 1 block is accepted - as the parent has it.
    const bool chol = op == BAND_CHOL;
    if (env.lds && M > (chol ? W : 2 * k + 1)) {
      const BandSegments s = band_segments(M, 156 * 1024, 8 * W, chol ? W : k, chol ? W : 1, sb, 1);
      p.seg = s.seg; p.cap = s.cap;
      return run(BAND_STREAMED, 256, sizeof(double) * (size_t)W * (size_t)s.cap);
    }
    return run(BAND_SWEEP, 64, 0);
  }

  const bool longer = env.lds && M > 2 * W;        // the streamed adjoints: more than two blocks of k+1 columns - as the parent has it
  const size_t both = sizeof(double) * 2 * (size_t)W * (size_t)M;        // two arrays of the whole band (WAVE, SEQUENTIAL)
  const bool both_fit = both <= (size_t)BAND_LDS_MAX;
  if (op == BAND_CHOL_VJP && longer) {
    // L and the incoming adjoint side by side: 16 (k+1) bytes per column, of the full 160 KiB (no static LDS in the adjoints); blocks
    // and carried columns as in the forward Cholesky.  An override counts from 2 blocks on (1 is ignored) - as the parent has it.
    const BandSegments s = band_segments(M, BAND_LDS_MAX, 16 * W, W, W, sb, 2);
    p.seg = s.seg; p.cap = s.cap;
    return run(BAND_STREAMED, 256, sizeof(double) * 2 * (size_t)s.cap * W);
  }
  if (op == BAND_INVERSE_VJP && longer && k <= 6) {   // (k = 7, 8: the windows and the blocks fetched ahead no longer fit the register file)
    // Two capacities: cap rows of the incoming adjoint (k+1 doubles each) and cap_fq doubles of factors that wave 0 leaves for wave 1.
    // One segment (both arrays of the whole matrix fit, and no override shortens it): the progress counter sits in the slot of
    // (row M - 1 + k, column M - 1), which no column uses.  Several: seg (k+1) + (k+1) rows, seg (k+1) columns of k+1 factors and one
    // more double for the counter - the largest seg with 2 seg (k+1)^2 + (k+1)^2 + 1 doubles in 160 KiB.  Override from 2 blocks on, as above.
    const int nblk = (int)((M + W - 1) / W);
    if (both_fit && !(sb >= 2 && sb < nblk)) { p.seg = nblk; p.cap = (int)M; p.cap_fq = (int)M * W; }
    else {
      const int doubles = BAND_LDS_MAX / (int)sizeof(double);
      p.seg = ((doubles - 1) / W - W) / (2 * W);
      if (sb >= 2 && sb < p.seg) p.seg = sb;
      p.cap = p.seg * W + W;
      p.cap_fq = p.seg * W * W + 1;
    }
    return run(BAND_STREAMED, 256, sizeof(double) * ((size_t)p.cap * W + (size_t)p.cap_fq));
  }
  if (both_fit && W * W <= 64) return run(BAND_WAVE, 256, both);      // one lane per entry of the (k+1) x (k+1) window: k <= 7
  p.arrays_in_lds = both_fit ? 1 : 0;
  return run(BAND_SEQUENTIAL, 256, both_fit ? both : 0);
}

// ---- the launchers: each executes an accepted plan ------------------------------------------------------------------------------
// ASVGP_BAND_OPS_LDS, ASVGP_BAND_OPS_SEG_BLOCKS: read once, at the first call of any of the four operators
static BandEnv band_ops_env() {
  static const BandEnv env = [] {
    const char* lds = getenv("ASVGP_BAND_OPS_LDS");
    const char* seg = getenv("ASVGP_BAND_OPS_SEG_BLOCKS");
    return BandEnv{!(lds && atoi(lds) == 0), seg ? atoi(seg) : 0};
  }();
  return env;
}

// one workgroup of plan.threads with plan.lds_bytes of dynamic LDS.  Every plan asks for at most BAND_LDS_MAX, which gfx950 grants: a
// refused attribute is an error, never another kernel.
template <class Kern, class... Args>
static int band_launch(const BandPlan& p, const char* what, hipStream_t st, Kern kern, Args... args) {
  if (p.lds_bytes > 0) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      set_error("%s: hipFuncSetAttribute(%zu B LDS): %s", what, p.lds_bytes, hipGetErrorString(e));
      return ASVGP_ERR_LDS_CAPACITY;
    }
  }
  hipLaunchKernelGGL(kern, dim3(1), dim3(p.threads), p.lds_bytes, st, args...);
  return check_launch(what);
}
// a plan names a kernel that is not built for this bandwidth (the `if constexpr` guards below): cannot happen after plan_band_op
static int band_not_built(const char* who, const BandPlan& p, int k) {
  set_error("%s: kernel %d of the launch plan is not built for bandwidth %d", who, p.kernel, k);
  return ASVGP_ERR_UNSUPPORTED;
}

template <int K> struct CholLauncher {
  static int run(const BandPlan& p, const double* A, double* L, int M, int* info, hipStream_t st) {
    switch (p.kernel) {
      case BAND_STREAMED: return band_launch(p, "cholesky_band (band in the LDS)", st, cholesky_band_lds_kernel<K>, A, L, M, info, p.seg);
      case BAND_SWEEP: return band_launch(p, "cholesky_band", st, cholesky_band_kernel<K>, A, L, M, info);
    }
    return band_not_built("cholesky_band", p, K);
  }
};
template <int K> struct TakaLauncher {
  static int run(const BandPlan& p, const double* L, double* S, int M, hipStream_t st) {
    switch (p.kernel) {
      case BAND_STREAMED: return band_launch(p, "inverse_from_cholesky_band (band in the LDS)", st, takahashi_lds_kernel<K>, L, S, M, p.seg);
      case BAND_SWEEP: return band_launch(p, "inverse_from_cholesky_band", st, takahashi_kernel<K>, L, S, M);
    }
    return band_not_built("inverse_from_cholesky_band", p, K);
  }
};
template <int K> struct CholVjpLauncher {
  static int run(const BandPlan& p, const double* L, const double* Lbar, double* Kbar, double* work, int M, hipStream_t st) {
    switch (p.kernel) {
      case BAND_STREAMED: return band_launch(p, "cholesky_band_vjp (register window)", st, band_cholesky_vjp_lds_kernel<K>, L, Lbar, Kbar, M, p.seg, p.cap);
      case BAND_WAVE:
        if constexpr ((K + 1) * (K + 1) <= 64) return band_launch(p, "cholesky_band_vjp", st, band_cholesky_vjp_wave_kernel<K>, L, Lbar, Kbar, M);
        break;
      case BAND_SEQUENTIAL: return band_launch(p, "cholesky_band_vjp", st, band_cholesky_vjp_kernel, L, Lbar, Kbar, work, M, K, p.arrays_in_lds);
    }
    return band_not_built("cholesky_band_vjp", p, K);
  }
};
template <int K> struct TakaVjpLauncher {
  static int run(const BandPlan& p, const double* L, const double* S, const double* Sbar, double* Lbar, double* work, int M, hipStream_t st) {
    switch (p.kernel) {
      case BAND_STREAMED:
        if constexpr (K <= 6)
          return band_launch(p, "inverse_from_cholesky_band_vjp (register window)", st, band_takahashi_vjp_lds_kernel<K>, L, S, Sbar, Lbar, work, M, p.seg, p.cap, p.cap_fq);
        break;
      case BAND_WAVE:
        if constexpr ((K + 1) * (K + 1) <= 64) return band_launch(p, "inverse_from_cholesky_band_vjp", st, band_takahashi_vjp_wave_kernel<K>, L, S, Sbar, Lbar, work, M);
        break;
      case BAND_SEQUENTIAL: return band_launch(p, "inverse_from_cholesky_band_vjp", st, band_takahashi_vjp_kernel, L, S, Sbar, Lbar, work, M, K, p.arrays_in_lds);
    }
    return band_not_built("inverse_from_cholesky_band_vjp", p, K);
  }
};

// plan, then refuse or launch (the arguments have passed band_args_ok)
template <template <int> class Launcher, typename... Args>
static int run_band_op(int op, int64_t M, int k, Args... args) {
  const BandPlan p = plan_band_op(op, (long)M, k, band_ops_env());
  if (p.status) { set_error("%s", p.msg); return p.status; }
  return dispatch_k<Launcher>(k, p, args...);
}

}  // namespace asvgp

using namespace asvgp;

extern "C" int asvgp_cholesky_band(const double* K, double* L, int64_t M, int k, int* info, asvgp_stream_t stream) {
  int rc = band_args_ok(K, L, M, k, "cholesky_band");
  if (rc) return rc;
  return run_band_op<CholLauncher>(BAND_CHOL, M, k, K, L, (int)M, info, as_stream(stream));
}

extern "C" int asvgp_inverse_from_cholesky_band(const double* L, double* S, int64_t M, int k, asvgp_stream_t stream) {
  int rc = band_args_ok(L, S, M, k, "inverse_from_cholesky_band");
  if (rc) return rc;
  return run_band_op<TakaLauncher>(BAND_INVERSE, M, k, L, S, (int)M, as_stream(stream));
}

extern "C" int asvgp_cholesky_band_vjp(const double* L, const double* Lbar, double* Kbar, double* work, int64_t M, int k, asvgp_stream_t stream) {
  int rc = band_args_ok(L, Lbar, M, k, "cholesky_band_vjp");
  if (rc) return rc;
  if (!Kbar || !work) { set_error("cholesky_band_vjp: bad argument"); return ASVGP_ERR_BAD_ARG; }
  return run_band_op<CholVjpLauncher>(BAND_CHOL_VJP, M, k, L, Lbar, Kbar, work, (int)M, as_stream(stream));
}

extern "C" int asvgp_inverse_from_cholesky_band_vjp(const double* L, const double* S, const double* Sbar, double* Lbar, double* work, int64_t M,
                                                    int k, asvgp_stream_t stream) {
  int rc = band_args_ok(L, S, M, k, "inverse_from_cholesky_band_vjp");
  if (rc) return rc;
  if (!Sbar || !Lbar || !work) { set_error("inverse_from_cholesky_band_vjp: bad argument"); return ASVGP_ERR_BAD_ARG; }
  return run_band_op<TakaVjpLauncher>(BAND_INVERSE_VJP, M, k, L, S, Sbar, Lbar, work, (int)M, as_stream(stream));
}

// Host-only: the plan the four entries above would make for these inputs - the same plan_band_op, the environment as arguments, no device
extern "C" int asvgp_band_launch_plan_host(int op, int64_t M, int k, int lds, int seg_blocks, int64_t* plan8) {
  if (!plan8) { set_error("band_launch_plan_host: bad argument"); return ASVGP_ERR_BAD_ARG; }
  const BandPlan p = plan_band_op(op, (long)M, k, BandEnv{lds != 0, seg_blocks});
  const int64_t f[8] = {p.status, p.kernel, p.threads, (int64_t)p.lds_bytes, p.seg, p.cap, p.cap_fq, p.arrays_in_lds};
  for (int i = 0; i < 8; ++i) plan8[i] = f[i];
  if (p.status) set_error("%s", p.msg);
  return p.status;
}
