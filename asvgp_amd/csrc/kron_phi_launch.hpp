// Host side of the 2-D (Kronecker) Phi pass - asvgp_phi_accumulate_kron2d, its _weighted, _sorted, _sorted_f32 and _sorted_weighted forms:
// which kernel one call launches and with what numbers, decided from integers alone BEFORE anything happens, then one launcher per
// kernel that executes the plan.  (included by kron.hip last, behind kron_weighted.hpp: kron.hip and kron_weighted.hpp hold the kernels
// of the pass, kron.hip the host code of every other Kronecker entry.)
//
// An entry is: check_kron_phi_args -> plan_kron_phi(..., kron_phi_env(), staging = true) -> gather the one fact the plan asks for (is
// there room for its staging buffer: hipMallocAsync) and plan again without -> refuse, or clear what the plan says and hand it to
// launch_kron_phi_point | launch_kron_phi_cells | launch_kron_phi_mfma.  The launchers decide nothing.  Nothing is written before the
// plan is accepted.  asvgp_kron_phi_launch_plan_host shows the same plan_kron_phi to the CPU tests, with the environment as arguments.
#pragma once

namespace asvgp {

// ---- the plan -----------------------------------------------------------------------------------------------------------------
enum KronPhiForm { KRON_PHI_PER_POINT = 0, KRON_PHI_SORTED };   // points as they come | sorted by cell, with the cell offsets
enum KronPhiKernel {
  KRON_PHI_NONE = 0,   // N = 0: the statistics are cleared, nothing is launched
  KRON_PHI_POINT,      // one thread per point, every product a global atomic (phi_kron2d_kernel, phi_kron2d_weighted_kernel)
  KRON_PHI_CELLS,      // one workgroup per cell, one global atomic per entry and cell (phi_kron2d_cells_kernel; unweighted fp64 only)
  KRON_PHI_MFMA        // one wave per cell on the matrix core into the staging buffer, then the gather (phi_kron2d_mfma[_weighted]_kernel)
};
struct KronPhiEnv { bool atomics; long grid; };      // ASVGP_KRON_PHI_ATOMICS != 0; ASVGP_KRON_PHI_GRID (default 512)
struct KronPhiPlan {
  int status; char msg[160];                         // != ASVGP_OK: refused, nothing below counts
  int kernel, grid, threads;                         // KronPhiKernel; its grid and workgroup
  int gather_grid;                                   // MFMA: workgroups of phi_kron2d_gather_kernel
  size_t staging_bytes;                              // MFMA: the entry-major cell sums, kron_nout(order) doubles per padded cell
  long ncell, ncell_pad;                             // cells of the mesh; rounded up to whole strips of KRON_STRIP (both fit an int)
  bool clear_all;                                    // clear all of stats, else yy only (the gather overwrites every band and rhs entry)
  size_t rhs_off, yy_off;                            // stats = [ Ablk | rhs | yy ]: doubles in front of rhs and of yy
};

// KronOut<K>::NOUT for a run-time order: what one cell leaves in the staging buffer
constexpr int kron_nout(int k) { return (k + 1) * (k + 2) / 2 * (k + 1) * (k + 1) - (k + 1) * (k * (k + 1) / 2) + (k + 1) * (k + 1); }
static_assert(kron_nout(1) == KronOut<1>::NOUT && kron_nout(2) == KronOut<2>::NOUT && kron_nout(3) == KronOut<3>::NOUT &&
              kron_nout(4) == KronOut<4>::NOUT && kron_nout(5) == KronOut<5>::NOUT && kron_nout(6) == KronOut<6>::NOUT, "kron_nout is KronOut's formula");

// Which kernel and with what numbers (the arguments have passed check_kron_phi_args).  Reads its arguments only: no HIP call, no
// environment.  The rules run in the order written; the first that applies is the plan.  `staging`: there is room for the staging buffer.
static KronPhiPlan plan_kron_phi(int form, bool weighted, bool f32, long N, long m1, long m2, long n_mesh1, long n_mesh2, int order, KronPhiEnv env,
                                 bool staging) {
  KronPhiPlan p{};
  auto refuse = [&p](int status, const char* fmt, auto... a) { p.status = status; snprintf(p.msg, sizeof(p.msg), fmt, a...); return p; };
  auto run = [&p](int kernel, long grid, int threads) { p.kernel = kernel; p.grid = (int)grid; p.threads = threads; return p; };
  auto at_most = [](long a, long b) { return a < b ? a : b; };
  const long Mtot = m1 * m2;
  p.rhs_off = (size_t)kron_noff(order) * (size_t)Mtot;
  p.yy_off = p.rhs_off + (size_t)Mtot;
  p.ncell = (n_mesh1 - 1) * (n_mesh2 - 1);
  p.ncell_pad = (p.ncell + KRON_STRIP - 1) / KRON_STRIP * KRON_STRIP;
  p.clear_all = true;
  if (N == 0) return run(KRON_PHI_NONE, 0, 0);
  if (form == KRON_PHI_PER_POINT) return run(KRON_PHI_POINT, at_most((N + 255) / 256, 4096), 256);

  // Sorted.  The matrix-core kernel, always for fp32 storage and for weights (they have no other), for plain fp64 unless the
  // environment asks for the per-cell kernel.  A resident grid: each workgroup walks several strips, the next cell's points in flight.
  const bool only_mfma = weighted || f32;
  if (only_mfma || !env.atomics) {
    if (staging) {
      p.staging_bytes = sizeof(double) * (size_t)kron_nout(order) * (size_t)p.ncell_pad;
      p.gather_grid = (int)at_most(((kron_noff(order) + 1) * Mtot + 255) / 256, 8192);
      p.clear_all = false;
      return run(KRON_PHI_MFMA, at_most(p.ncell_pad / KRON_STRIP, env.grid < 1 ? 1 : env.grid), 64 * KRON_STRIP);
    }
    if (f32) return refuse(ASVGP_ERR_HIP, "phi_accumulate_kron2d_sorted_f32: no room for the staging buffer (%ld cells)", p.ncell);
    if (weighted) return refuse(ASVGP_ERR_HIP, "phi_accumulate_kron2d_sorted_weighted: no room for the staging buffer (%ld cells); the per-point entry needs none", p.ncell);
  }
  return run(KRON_PHI_CELLS, at_most(p.ncell, 4096), 256);   // (it needs no staging buffer)
}

// what all five entries and the host plan check of the integers - and of the pointers and the mesh steps, `ok`, and of X, `aligned`
static int check_kron_phi_args(const char* name, bool ok, bool aligned, const char* align_msg, int64_t N, int64_t m1, int64_t m2, int64_t n_mesh1,
                               int64_t n_mesh2, int order) {
  if (!ok || N < 0 || n_mesh1 != m1 - order + 1 || n_mesh2 != m2 - order + 1 || n_mesh1 < 2 || n_mesh2 < 2) { set_error("%s: bad argument", name); return ASVGP_ERR_BAD_ARG; }
  if (order < 1 || order > ASVGP_MAX_ORDER) { set_error("%s: order %d unsupported", name, order); return ASVGP_ERR_UNSUPPORTED; }
  if (!aligned) { set_error("%s: %s", name, align_msg); return ASVGP_ERR_BAD_ARG; }
  // what the kernels take as int: the four sizes, and the cells rounded up to whole strips
  const struct { const char* what; int64_t v; } ints[4] = {{"m1", m1}, {"m2", m2}, {"n_mesh1", n_mesh1}, {"n_mesh2", n_mesh2}};
  for (const auto& i : ints)
    if (i.v > 0x7fffffff) { set_error("%s: %s = %ld does not fit an int", name, i.what, (long)i.v); return ASVGP_ERR_UNSUPPORTED; }
  const int64_t ncell = (n_mesh1 - 1) * (n_mesh2 - 1);
  if ((ncell + KRON_STRIP - 1) / KRON_STRIP * KRON_STRIP > 0x7fffffff) {
    set_error("%s: %ld cells in strips of %d do not fit an int", name, (long)ncell, KRON_STRIP);
    return ASVGP_ERR_UNSUPPORTED;
  }
  return ASVGP_OK;
}

// ---- the launchers: each executes an accepted plan ------------------------------------------------------------------------------
// ASVGP_KRON_PHI_ATOMICS (the per-cell kernel, for comparison: plain fp64 only), ASVGP_KRON_PHI_GRID (resident workgroups of both
// matrix-core kernels): read once, at the first call of any of the five entries
static KronPhiEnv kron_phi_env() {
  static const KronPhiEnv env = [] {
    const char* atomics = getenv("ASVGP_KRON_PHI_ATOMICS");
    const char* grid = getenv("ASVGP_KRON_PHI_GRID");
    return KronPhiEnv{atomics && atoi(atomics) != 0, grid ? atol(grid) : 512};
  }();
  return env;
}

struct KronPhiCall {
  const void* X; const void* y;                      // double, or float for the fp32-storage entry
  const double* w; long N; const long long* cell_start;
  const double* mesh1; int n1; double id1; int m1;
  const double* mesh2; int n2; double id2; int m2;
  double* Ablk; double* rhs; double* yy; double* wstats;
  double* cellsum;                                   // the staging buffer (MFMA)
  hipStream_t st;
};

static void launch_kron_phi_point(const KronPhiPlan& p, const KronPhiCall& c, int order, bool weighted) {
  const double* X = static_cast<const double*>(c.X);
  const double* y = static_cast<const double*>(c.y);
  KRON_DISPATCH(order, {
    if (weighted)
      hipLaunchKernelGGL(phi_kron2d_weighted_kernel<K>, dim3((unsigned)p.grid), dim3(p.threads), 0, c.st, X, y, c.w, c.N, c.mesh1, c.n1, c.id1, c.m1, c.mesh2, c.n2,
                         c.id2, c.m2, c.Ablk, c.rhs, c.yy, c.wstats);
    else
      hipLaunchKernelGGL(phi_kron2d_kernel<K>, dim3((unsigned)p.grid), dim3(p.threads), 0, c.st, X, y, c.N, c.mesh1, c.n1, c.id1, c.m1, c.mesh2, c.n2, c.id2, c.m2,
                         c.Ablk, c.rhs, c.yy);
  });
}

static void launch_kron_phi_cells(const KronPhiPlan& p, const KronPhiCall& c, int order) {
  KRON_DISPATCH(order, hipLaunchKernelGGL(phi_kron2d_cells_kernel<K>, dim3((unsigned)p.grid), dim3(p.threads), 0, c.st, static_cast<const double*>(c.X),
                                          static_cast<const double*>(c.y), c.cell_start, (int)p.ncell, c.mesh1, c.id1, c.m1, c.mesh2, c.n2, c.id2, c.m2,
                                          c.Ablk, c.rhs, c.yy));
}

template <typename TIN, bool WEIGHTED>
static void launch_kron_phi_mfma(const KronPhiPlan& p, const KronPhiCall& c, int order) {
  const TIN* X = static_cast<const TIN*>(c.X);
  const TIN* y = static_cast<const TIN*>(c.y);
  KRON_DISPATCH(order, {
    if constexpr (WEIGHTED)
      hipLaunchKernelGGL((phi_kron2d_mfma_weighted_kernel<K>), dim3((unsigned)p.grid), dim3(p.threads), 0, c.st, X, y, c.w, c.cell_start, (int)p.ncell,
                         (int)p.ncell_pad, c.mesh1, c.id1, c.mesh2, c.n2, c.id2, c.cellsum, c.yy, c.wstats);
    else
      hipLaunchKernelGGL((phi_kron2d_mfma_kernel<K, TIN>), dim3((unsigned)p.grid), dim3(p.threads), 0, c.st, X, y, c.cell_start, (int)p.ncell, (int)p.ncell_pad,
                         c.mesh1, c.id1, c.mesh2, c.n2, c.id2, c.cellsum, c.yy);
    hipLaunchKernelGGL(phi_kron2d_gather_kernel<K>, dim3((unsigned)p.gather_grid), dim3(256), 0, c.st, c.cellsum, (int)p.ncell_pad, c.n1 - 1, c.n2 - 1, c.m1,
                       c.m2, c.Ablk, c.rhs);
  });
}

// the body of all five C entries (unweighted: w = wstats = NULL; per point: cell_start = NULL): check -> plan -> room for the staging
// buffer, else plan again -> refuse or clear -> launch
static int kron_phi_entry(const char* name, int form, bool weighted, bool f32, const void* X, const void* y, const double* w, int64_t N,
                          const int64_t* cell_start, const double* mesh1, int64_t n_mesh1, double delta1, int64_t m1, const double* mesh2, int64_t n_mesh2,
                          double delta2, int64_t m2, int order, double* stats, double* wstats, asvgp_stream_t stream) {
  const bool sorted = form == KRON_PHI_SORTED;
  const bool ok = !(N > 0 && (!X || !y || (weighted && !w))) && (!sorted || cell_start) && mesh1 && mesh2 && stats && (!weighted || wstats) && delta1 > 0 &&
                  delta2 > 0;
  const bool aligned = (reinterpret_cast<uintptr_t>(X) & (f32 ? 7 : 15)) == 0;
  const char* align_msg = !sorted ? "X must be 16-byte aligned (N,2) row-major"
                          : weighted ? "Xs must be 16-byte aligned (N,2) row-major" : "Xs must be aligned to one (x1, x2) pair, (N,2) row-major";
  const int rc = check_kron_phi_args(name, ok, aligned, align_msg, N, m1, m2, n_mesh1, n_mesh2, order);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  auto plan = [&](bool staging) {
    return plan_kron_phi(form, weighted, f32, (long)N, (long)m1, (long)m2, (long)n_mesh1, (long)n_mesh2, order, kron_phi_env(), staging);
  };
  KronPhiPlan p = plan(true);
  double* cellsum = nullptr;
  if (p.staging_bytes > 0 && hipMallocAsync(reinterpret_cast<void**>(&cellsum), p.staging_bytes, st) != hipSuccess) {
    (void)hipGetLastError();
    cellsum = nullptr;
    p = plan(false);
  }
  if (p.status) { set_error("%s", p.msg); return p.status; }
  const KronPhiCall c{X, y, w, (long)N, reinterpret_cast<const long long*>(cell_start), mesh1, (int)n_mesh1, 1.0 / delta1, (int)m1, mesh2, (int)n_mesh2,
                      1.0 / delta2, (int)m2, stats, stats + p.rhs_off, stats + p.yy_off, wstats, cellsum, st};
  hipError_t e = weighted ? hipMemsetAsync(wstats, 0, 3 * sizeof(double), st) : hipSuccess;
  if (e == hipSuccess) e = p.clear_all ? hipMemsetAsync(stats, 0, (p.yy_off + 1) * sizeof(double), st) : hipMemsetAsync(c.yy, 0, sizeof(double), st);
  if (e != hipSuccess) {
    set_error("hipMemsetAsync: %s", hipGetErrorString(e));
    if (cellsum) (void)hipFreeAsync(cellsum, st);
    return ASVGP_ERR_HIP;
  }
  switch (p.kernel) {
    case KRON_PHI_NONE: return ASVGP_OK;
    case KRON_PHI_POINT: launch_kron_phi_point(p, c, order, weighted); return check_launch(name);
    case KRON_PHI_CELLS: launch_kron_phi_cells(p, c, order); return check_launch(name);
  }
  if (f32) launch_kron_phi_mfma<float, false>(p, c, order);
  else if (weighted) launch_kron_phi_mfma<double, true>(p, c, order);
  else launch_kron_phi_mfma<double, false>(p, c, order);
  (void)hipFreeAsync(cellsum, st);
  return check_launch(weighted ? "phi_accumulate_kron2d_sorted_weighted (matrix-core cell sums + gather)" : "phi_accumulate_kron2d_sorted (matrix-core cell sums + gather)");
}

}  // namespace asvgp

using namespace asvgp;

extern "C" int asvgp_phi_accumulate_kron2d(const double* X, const double* y, int64_t N, const double* mesh1, int64_t n_mesh1, double delta1, int64_t m1,
                                           const double* mesh2, int64_t n_mesh2, double delta2, int64_t m2, int order, double* stats, asvgp_stream_t stream) {
  return kron_phi_entry("phi_accumulate_kron2d", KRON_PHI_PER_POINT, false, false, X, y, nullptr, N, nullptr, mesh1, n_mesh1, delta1, m1, mesh2, n_mesh2, delta2, m2,
                        order, stats, nullptr, stream);
}

extern "C" int asvgp_phi_accumulate_kron2d_weighted(const double* X, const double* y, const double* w, int64_t N, const double* mesh1, int64_t n_mesh1,
                                                    double delta1, int64_t m1, const double* mesh2, int64_t n_mesh2, double delta2, int64_t m2, int order,
                                                    double* stats, double* wstats, asvgp_stream_t stream) {
  return kron_phi_entry("phi_accumulate_kron2d_weighted", KRON_PHI_PER_POINT, true, false, X, y, w, N, nullptr, mesh1, n_mesh1, delta1, m1, mesh2, n_mesh2, delta2, m2,
                        order, stats, wstats, stream);
}

extern "C" int asvgp_phi_accumulate_kron2d_sorted(const double* Xs, const double* ys, int64_t N, const int64_t* cell_start, const double* mesh1, int64_t n_mesh1,
                                                  double delta1, int64_t m1, const double* mesh2, int64_t n_mesh2, double delta2, int64_t m2, int order,
                                                  double* stats, asvgp_stream_t stream) {
  return kron_phi_entry("phi_accumulate_kron2d_sorted", KRON_PHI_SORTED, false, false, Xs, ys, nullptr, N, cell_start, mesh1, n_mesh1, delta1, m1, mesh2, n_mesh2,
                        delta2, m2, order, stats, nullptr, stream);
}

// fp32 STORAGE of the cell-sorted points (BASELINE config 4): 12 B per point streamed, widened exactly, fp64 arithmetic
extern "C" int asvgp_phi_accumulate_kron2d_sorted_f32(const float* Xs, const float* ys, int64_t N, const int64_t* cell_start, const double* mesh1,
                                                      int64_t n_mesh1, double delta1, int64_t m1, const double* mesh2, int64_t n_mesh2, double delta2, int64_t m2,
                                                      int order, double* stats, asvgp_stream_t stream) {
  return kron_phi_entry("phi_accumulate_kron2d_sorted_f32", KRON_PHI_SORTED, false, true, Xs, ys, nullptr, N, cell_start, mesh1, n_mesh1, delta1, m1, mesh2, n_mesh2,
                        delta2, m2, order, stats, nullptr, stream);
}

extern "C" int asvgp_phi_accumulate_kron2d_sorted_weighted(const double* Xs, const double* ys, const double* ws, int64_t N, const int64_t* cell_start,
                                                           const double* mesh1, int64_t n_mesh1, double delta1, int64_t m1, const double* mesh2,
                                                           int64_t n_mesh2, double delta2, int64_t m2, int order, double* stats, double* wstats,
                                                           asvgp_stream_t stream) {
  return kron_phi_entry("phi_accumulate_kron2d_sorted_weighted", KRON_PHI_SORTED, true, false, Xs, ys, ws, N, cell_start, mesh1, n_mesh1, delta1, m1, mesh2, n_mesh2,
                        delta2, m2, order, stats, wstats, stream);
}

// Host-only: the plan the five entries above would make for these inputs - the same integer checks and the same plan_kron_phi, the
// environment and the outcome of the allocation as arguments, no device
extern "C" int asvgp_kron_phi_launch_plan_host(int sorted, int weighted, int f32, int64_t N, int64_t m1, int64_t m2, int64_t n_mesh1, int64_t n_mesh2, int order,
                                               int atomics, int64_t grid, int staging, int64_t* plan12) {
  const bool ok = plan12 && !(f32 && (weighted || !sorted));   // (fp32 storage: the plain sorted entry only)
  const int rc = check_kron_phi_args("kron_phi_launch_plan_host", ok, true, "", N, m1, m2, n_mesh1, n_mesh2, order);
  if (rc) { if (plan12) { for (int i = 1; i < 12; ++i) plan12[i] = 0; plan12[0] = rc; } return rc; }
  const KronPhiPlan p = plan_kron_phi(sorted ? KRON_PHI_SORTED : KRON_PHI_PER_POINT, weighted != 0, f32 != 0, (long)N, (long)m1, (long)m2, (long)n_mesh1,
                                      (long)n_mesh2, order, KronPhiEnv{atomics != 0, (long)grid}, staging != 0);
  const int64_t f[12] = {p.status, p.kernel, p.grid, p.threads, p.gather_grid, (int64_t)p.staging_bytes, p.ncell, p.ncell_pad, p.clear_all,
                         (int64_t)p.rhs_off, (int64_t)p.yy_off, 0};
  for (int i = 0; i < 12; ++i) plan12[i] = f[i];
  if (p.status) set_error("%s", p.msg);
  return p.status;
}
