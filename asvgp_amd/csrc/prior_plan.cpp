// Host half of the prior (Kuu) chain: the FORWARD pass of the block cyclic reduction of bcr.hpp, carried out once per
// hyper-parameter value in long double on the O(log M) DISTINCT nodes of the elimination tree.
//
// Why on the host.  Kuu = sum_t c_t(theta) S_t (inducing_features.py:16-44) with static bands S_t that are Toeplitz away
// from the two boundaries (basis.py:31-45 `_make_banded_matrix`: interior columns constant), so at every level of the
// odd-even elimination all interior nodes are bit-identical: only the first / last one or two differ.  The whole forward
// pass therefore needs ~5 node eliminations per level - a few ten thousand flops, microseconds of scalar work - instead of
// M / k of them.  And it is the forward pass that decides the accuracy of band(Kuu^-1): measured at the BASELINE size
// (M = 2048, cond(Kuu) = 3.5e7, tools/bcr_accuracy.py) fp64 cyclic reduction leaves tr(Kuu^-1 A) 26x further from an 80-bit
// evaluation than the reference's sequential fp64 Cholesky + Takahashi (gpr.py:56-59); with the forward factors computed
// to 64 mantissa bits and the backward (selected inverse) pass in fp64 on the GPU the result is as close as, or closer
// than, the reference's own order in every configuration tried.  GPUs have no 80-bit type and double-double on one wave
// would cost ~10x the level latency; the host's x87 unit does it in the time the Phi pass is in flight.
//
// The plan (symbolic part, once per basis) assigns every node of every level a class by exact comparison of its inputs;
// the numeric part (once per theta) eliminates one representative per class.  A band without that structure (more than
// MAX_CLASSES classes on some level) has no plan and the library falls back to the all-GPU chain.
#include "prior_plan.hpp"

#include <float.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <array>
#include <map>
#include <vector>

namespace asvgp {

namespace {

constexpr int MAXB = 6;            // ASVGP_MAX_ORDER
constexpr int MAX_CLASSES = PRIOR_MAX_CLASSES;    // per level

typedef long double ld;
// The forward pass owes its accuracy (|bound - exact| ~ 3e-11 |bound| at the headline configuration, cond(Kuu) = 3.5e7) to the 64-bit
// mantissa of the x87 extended format.  A toolchain where long double is plain fp64 (or a software quad) must not build this silently.
static_assert(LDBL_MANT_DIG == 64, "prior_plan.cpp needs the 80-bit x87 long double (64-bit mantissa)");
// Tangent arithmetic: double by default (the x87 unit then carries a third of the flops of a (long double, long double) dual number);
// ASVGP_PRIOR_TANGENT_LD=1 in the environment carries the tangents in long double as well (what the
// d / d lengthscale component gains from it at cond(Kuu) ~ 1e9).
template <typename td> struct BlkT { ld v[MAXB][MAXB]; td d[MAXB][MAXB]; };   // value (long double) + tangent d / d lengthscale (td)

struct Level {
  std::vector<std::array<int, 3>> node_in;   // per node class: (D class of i, E class of (a, i), E class of (i, b) or -1)
  std::vector<int> node_count;               // nodes in the class (log-determinant weights)
  std::vector<int> node_rep;                 // a representative node (reports the failing column)
  std::vector<std::array<int, 3>> d_next;    // per D class of the next level: (D class now, node class left or -1, right or -1)
};

}  // namespace

struct PriorPlan {
  int B = 0, n_terms = 0, nb = 0, levels = 0;
  long M = 0;
  std::vector<double> S;                     // host copy of the static bands (n_terms, B + 1, M)
  std::vector<int> d0_rep, e0_rep;           // level-0 classes: representative block of D(n), of E(n) = A[n+1, n]
  std::vector<Level> lv;
  std::vector<int> lvl_off;                  // record offset of every level (+ the root record at the end)
  std::vector<int> node_rec;                 // per block node: record index
  int n_rec = 0;
  long int_lo = 0, int_hi = 0;               // columns [int_lo, int_hi) on which EVERY diagonal of every static term is constant (Toeplitz interior)
  std::vector<double> int_val;               // (n_terms, B + 1): that constant
};

// value of band entry (row, col), row >= col, of static term t; identity padding beyond M (as bcr.hpp band_D / band_E)
static inline double sband(const PriorPlan& p, int t, long row, long col) {
  return p.S[((size_t)t * (p.B + 1) + (size_t)(row - col)) * p.M + col];
}

static void block_key(const PriorPlan& p, int n, bool coupling, std::vector<double>& key) {
  const int B = p.B;
  key.clear();
  for (int r = 0; r < B; ++r)
    for (int c = 0; c < B; ++c) {
      long row, col;
      if (!coupling) { if (c > r) continue; row = (long)n * B + r; col = (long)n * B + c; }
      else { if (r > c) continue; row = (long)(n + 1) * B + r; col = (long)n * B + c; }   // E(n)[r][c], band offset B + r - c <= B
      const bool pad = row >= p.M || col >= p.M;
      key.push_back(pad ? 1.0 : 0.0);
      for (int t = 0; t < p.n_terms; ++t) key.push_back(pad ? 0.0 : sband(p, t, row, col));
    }
}

PriorPlan* prior_plan_create(const double* statics_host, int n_terms, long M, int k, char* err, size_t errlen) {
  auto fail = [&](const char* msg) -> PriorPlan* { if (err && errlen) snprintf(err, errlen, "%s", msg); return nullptr; };
  if (!statics_host || n_terms < 1 || n_terms > ASVGP_MAX_KUU_TERMS || M < 1 || k < 1 || k > MAXB) return fail("prior plan: bad argument");
  PriorPlan* p = new PriorPlan;
  p->B = k; p->n_terms = n_terms; p->M = M; p->nb = (int)((M + k - 1) / k);
  p->S.assign(statics_host, statics_host + (size_t)n_terms * (k + 1) * M);
  const int nb = p->nb;
  while ((1 << p->levels) < nb) ++p->levels;
  // ---- Toeplitz interior: the longest column range around the middle on which every (term, diagonal) is one constant, bit for bit
  {
    const long mid = M / 2;
    long lo = 0, hi = M - k;                  // (columns whose whole band column lies inside the matrix)
    p->int_val.assign((size_t)n_terms * (k + 1), 0.0);
    if (hi > mid && mid >= 0) {
      for (int t = 0; t < n_terms; ++t)
        for (int d = 0; d <= k; ++d) {
          const double* row = p->S.data() + ((size_t)t * (k + 1) + d) * M;
          const double v = row[mid];
          p->int_val[(size_t)t * (k + 1) + d] = v;
          long a = mid, b = mid + 1;
          while (a > 0 && memcmp(&row[a - 1], &v, sizeof(double)) == 0) --a;
          while (b < M - k && memcmp(&row[b], &v, sizeof(double)) == 0) ++b;
          lo = a > lo ? a : lo;
          hi = b < hi ? b : hi;
        }
      if (hi > lo) { p->int_lo = lo; p->int_hi = hi; }
    }
  }
  // ---- level-0 classes by exact comparison of the static blocks
  std::vector<int> cur(nb), dcls(nb), ecls(nb > 1 ? nb - 1 : 0);
  {
    std::map<std::vector<double>, int> dm, em;
    std::vector<double> key;
    for (int n = 0; n < nb; ++n) {
      cur[n] = n;
      block_key(*p, n, false, key);
      auto it = dm.find(key);
      if (it == dm.end()) { it = dm.emplace(key, (int)dm.size()).first; p->d0_rep.push_back(n); }
      dcls[n] = it->second;
      if (n + 1 < nb) {
        block_key(*p, n, true, key);
        auto ie = em.find(key);
        if (ie == em.end()) { ie = em.emplace(key, (int)em.size()).first; p->e0_rep.push_back(n); }
        ecls[n] = ie->second;
      }
    }
    if ((int)dm.size() > MAX_CLASSES || (int)em.size() > MAX_CLASSES) { delete p; return fail("prior plan: the static bands are not Toeplitz-structured"); }
  }
  p->node_rec.assign(nb, -1);
  int rec = 0;
  while (cur.size() > 1) {
    Level L;
    std::map<std::array<int, 3>, int> nm, dn;
    const int n = (int)cur.size();
    std::vector<int> ncls(n, -1);
    for (int j = 1; j < n; j += 2) {
      std::array<int, 3> key{dcls[j], ecls[j - 1], (j + 1 < n) ? ecls[j] : -1};
      auto it = nm.find(key);
      if (it == nm.end()) {
        it = nm.emplace(key, (int)nm.size()).first;
        L.node_in.push_back(key); L.node_count.push_back(0); L.node_rep.push_back(cur[j]);
      }
      ncls[j] = it->second;
      L.node_count[it->second]++;
      p->node_rec[cur[j]] = rec + it->second;
    }
    std::vector<int> ncur, ndcls, necls;
    for (int j = 0; j < n; j += 2) {
      std::array<int, 3> key{dcls[j], (j >= 1) ? ncls[j - 1] : -1, (j + 1 < n) ? ncls[j + 1] : -1};
      auto it = dn.find(key);
      if (it == dn.end()) { it = dn.emplace(key, (int)dn.size()).first; L.d_next.push_back(key); }
      ncur.push_back(cur[j]);
      ndcls.push_back(it->second);
      if (j + 2 < n) necls.push_back(ncls[j + 1]);   // coupling of the survivors (cur[j], cur[j+2]) = fill of the node between
    }
    if ((int)nm.size() > MAX_CLASSES || (int)dn.size() > MAX_CLASSES) { delete p; return fail("prior plan: too many distinct nodes on a level"); }
    p->lvl_off.push_back(rec);
    rec += (int)nm.size();
    p->lv.push_back(std::move(L));
    cur.swap(ncur); dcls.swap(ndcls); ecls.swap(necls);
  }
  p->lvl_off.push_back(rec);      // the root record
  p->node_rec[0] = rec;
  p->n_rec = rec + 1;
  if ((int)p->lv.size() != p->levels) { delete p; return fail("prior plan: level count mismatch"); }
  return p;
}

void prior_plan_destroy(PriorPlan* p) { delete p; }
int prior_plan_mantissa_bits() { return LDBL_MANT_DIG; }
// Kuu for one theta in closed form: kuu_diag[d] = the value of diagonal d on the Toeplitz interior, columns [*lo, *hi); bnd = the
// entries of the boundary columns - left part bnd[d * PRIOR_BND + col] (col < lo), right part bnd[(B + 1) * PRIOR_BND + d * PRIOR_BND +
// (col - hi)] (col >= hi; entries below the matrix are 0).  All formed with the rounding sequence of inducing_features.py:12-44 (this
// file is compiled with -ffp-contract=off): bit for bit what the device assembly writes.  *hi <= *lo: no usable interior (a boundary
// wider than PRIOR_BND columns, or no Toeplitz structure) - the caller keeps the assembled band.
bool prior_plan_interior(const PriorPlan* p) {
  return p->int_hi > p->int_lo && p->int_lo <= PRIOR_BND && p->M - p->int_hi <= PRIOR_BND && p->B + 1 <= PRIOR_BND_DIAGS;
}
void prior_plan_interior_kuu(const PriorPlan* p, const double* coef, double* kuu_diag, long* lo, long* hi, double* bnd) {
  const int B = p->B;
  const long M = p->M;
  *lo = 0; *hi = 0;
  if (!prior_plan_interior(p)) return;
  auto entry = [&](int d, long col) -> double {
    if (col + d >= M) return 0.0;
    const double* S = p->S.data();
    double acc = coef[0] * S[((size_t)0 * (B + 1) + d) * M + col];
    for (int t = 1; t < p->n_terms; ++t) acc = acc + coef[t] * S[((size_t)t * (B + 1) + d) * M + col];
    return acc;
  };
  for (int d = 0; d <= B; ++d) {
    kuu_diag[d] = entry(d, p->int_lo);
    for (long col = 0; col < PRIOR_BND; ++col) {
      bnd[(size_t)d * PRIOR_BND + col] = col < p->int_lo ? entry(d, col) : 0.0;
      const long cr = p->int_hi + col;
      bnd[(size_t)(PRIOR_BND_DIAGS + d) * PRIOR_BND + col] = cr < M ? entry(d, cr) : 0.0;
    }
  }
  *lo = p->int_lo; *hi = p->int_hi;
}
int prior_plan_nrec(const PriorPlan* p) { return p->n_rec; }
int prior_plan_nb(const PriorPlan* p) { return p->nb; }
long prior_plan_M(const PriorPlan* p) { return p->M; }
int prior_plan_k(const PriorPlan* p) { return p->B; }
int prior_plan_terms(const PriorPlan* p) { return p->n_terms; }
const int* prior_plan_node_rec(const PriorPlan* p) { return p->node_rec.data(); }
size_t prior_plan_table_doubles(const PriorPlan* p) {
  return PRIOR_TAB_HEADER + (size_t)2 * p->n_rec * prior_rec_fields(p->B);
}

// Device image of the plan for the all-GPU forward pass (prior_dd.hip): the symbolic class maps as ints, the static-band entries of
// the level-0 representative blocks as doubles.  ints: [0] B, [1] n_terms, [2] levels, [3] n_rec, [4] level-0 D classes, [5] level-0 E
// classes, [6] offset of the per-level headers, [7] total ints, [8] offset of the D entry codes, [9] of the E entry codes; a level
// header is 8 ints [node classes, D classes of the next level, offset of node_in (4 ints per class: D class, E class (a, i), E class
// (i, b) or -1, node count), offset of the representative nodes, offset of d_next (3 ints per class), first record, 0, 0].
// Entry codes (per level-0 class, B x B, row-major): 0 = sum of coef[t] * entry[t], 1 = the constant 1 (identity padding), 2 = 0.
// doubles: D entries [class][r][c][term] (lower triangle filled), then E entries [class][r][c][term] (r <= c filled).
size_t prior_plan_image_ints(const PriorPlan* p) {
  size_t n = 16 + (size_t)8 * p->levels;
  for (const Level& L : p->lv) n += L.node_in.size() * 5 + L.d_next.size() * 3;
  n += (p->d0_rep.size() + p->e0_rep.size()) * (size_t)p->B * p->B;
  return n;
}
size_t prior_plan_image_doubles(const PriorPlan* p) { return (p->d0_rep.size() + p->e0_rep.size()) * (size_t)p->B * p->B * p->n_terms; }
void prior_plan_image(const PriorPlan* pp, int* ints, double* dbls) {
  const PriorPlan& p = *pp;
  const int B = p.B, BB = B * B, nt = p.n_terms;
  size_t at = 16 + (size_t)8 * p.levels;
  for (int i = 0; i < 16; ++i) ints[i] = 0;
  ints[0] = B; ints[1] = nt; ints[2] = p.levels; ints[3] = p.n_rec; ints[4] = (int)p.d0_rep.size(); ints[5] = (int)p.e0_rep.size(); ints[6] = 16;
  for (int l = 0; l < p.levels; ++l) {
    const Level& L = p.lv[l];
    int* h = ints + 16 + 8 * l;
    h[0] = (int)L.node_in.size(); h[1] = (int)L.d_next.size(); h[5] = p.lvl_off[l]; h[6] = h[7] = 0;
    h[2] = (int)at;
    for (size_t q = 0; q < L.node_in.size(); ++q) { for (int i = 0; i < 3; ++i) ints[at++] = L.node_in[q][i]; ints[at++] = L.node_count[q]; }
    h[3] = (int)at;
    for (size_t q = 0; q < L.node_rep.size(); ++q) ints[at++] = L.node_rep[q];
    h[4] = (int)at;
    for (size_t q = 0; q < L.d_next.size(); ++q) for (int i = 0; i < 3; ++i) ints[at++] = L.d_next[q][i];
  }
  ints[8] = (int)at;
  size_t dat = 0;
  for (size_t q = 0; q < p.d0_rep.size(); ++q) {
    const int n = p.d0_rep[q];
    for (int r = 0; r < B; ++r)
      for (int c = 0; c < B; ++c) {
        const long row = (long)n * B + r, col = (long)n * B + c;
        const bool use = c <= r && row < p.M;
        ints[at++] = use ? 0 : ((r == c) ? 1 : 2);                 // (c > r: the device reads the mirrored entry)
        for (int t = 0; t < nt; ++t) dbls[dat++] = use ? sband(p, t, row, col) : 0.0;
      }
  }
  ints[9] = (int)at;
  for (size_t q = 0; q < p.e0_rep.size(); ++q) {
    const int n = p.e0_rep[q];
    for (int r = 0; r < B; ++r)
      for (int c = 0; c < B; ++c) {
        const long row = (long)(n + 1) * B + r, col = (long)n * B + c;
        const bool use = r <= c && row < p.M;
        ints[at++] = use ? 0 : 2;
        for (int t = 0; t < nt; ++t) dbls[dat++] = use ? sband(p, t, row, col) : 0.0;
      }
  }
  ints[7] = (int)at;
  (void)BB;
}

// Kuu / dKuu entry in fp64 with the reference's rounding sequence (inducing_features.py:16-44; the same sequence as
// kuu_assemble_kernel / elbo_prepare_kernel: products and sums rounded one by one, no contraction - this file is built
// with -ffp-contract=off), so the blocks factorised here are bit-identical to the device's Kuu band.
static inline void kuu_entry(const PriorPlan& p, const double* c, const double* dc, long row, long col, double& kv, double& dv) {
  double acc = c[0] * sband(p, 0, row, col);
  double dacc = dc[0] * sband(p, 0, row, col);
  for (int t = 1; t < p.n_terms; ++t) {
    const double s = sband(p, t, row, col);
    const double a = c[t] * s, b = dc[t] * s;
    acc = acc + a;
    dacc = dacc + b;
  }
  kv = acc; dv = dacc;
}

template <typename td>
static int prior_plan_eval_t(const PriorPlan* pp, const double* coef, const double* dcoef, double* tab) {
  typedef BlkT<td> Blk;
  // Values in long double; tangents (d / d lengthscale: the gradient is gated at 1e-6) in double from the rounded values -
  // two separate recurrences, so the x87 unit carries a third of the flops of a (long double, long double) dual number.
  const PriorPlan& p = *pp;
  const int B = p.B, W = prior_rec_fields(B), R = p.n_rec;
  double* val = tab + PRIOR_TAB_HEADER;
  double* tan = val + (size_t)R * W;
  memset(tab, 0, sizeof(double) * PRIOR_TAB_HEADER);
  // (fixed-size scratch: no heap traffic on the per-step path)
  Blk bufD[2][MAX_CLASSES], bufE[2][MAX_CLASSES], updA[MAX_CLASSES], updB[MAX_CLASSES];
  Blk* Dv = bufD[0]; Blk* Dn = bufD[1]; Blk* Ev = bufE[0]; Blk* Enew = bufE[1];
  // ---- level-0 blocks of the representatives
  for (size_t q = 0; q < p.d0_rep.size(); ++q) {
    const int n = p.d0_rep[q];
    for (int r = 0; r < B; ++r)
      for (int c = 0; c <= r; ++c) {
        const long row = (long)n * B + r, col = (long)n * B + c;
        double kv = (r == c) ? 1.0 : 0.0, dv = 0.0;                // identity padding
        if (row < p.M) kuu_entry(p, coef, dcoef, row, col, kv, dv);
        Dv[q].v[r][c] = Dv[q].v[c][r] = kv;
        Dv[q].d[r][c] = Dv[q].d[c][r] = dv;
      }
  }
  for (size_t q = 0; q < p.e0_rep.size(); ++q) {
    const int n = p.e0_rep[q];
    for (int r = 0; r < B; ++r)
      for (int c = 0; c < B; ++c) {
        const long row = (long)(n + 1) * B + r, col = (long)n * B + c;
        double kv = 0.0, dv = 0.0;
        if (r <= c && row < p.M) kuu_entry(p, coef, dcoef, row, col, kv, dv);
        Ev[q].v[r][c] = kv; Ev[q].d[r][c] = dv;
      }
  }
  ld logdet = 0.0L;
  td dlogdet = 0.0;
  int bad = 0;
  // Cholesky in place (lower part of D becomes L), inv = 1 / diag(L); then the tangent recurrence on the rounded factor
  auto chol = [&](Blk& D, ld (&inv)[MAXB], td (&Ld)[MAXB][MAXB], td (&invd)[MAXB], td (&dinv)[MAXB], int col0) {
    for (int j = 0; j < B; ++j) {
      ld s = D.v[j][j];
      for (int q = 0; q < j; ++q) s -= D.v[j][q] * D.v[j][q];
      if (!(s > 0.0L) && !bad) bad = col0 + j + 1;
      const ld l = sqrtl(s > 0.0L ? s : 1.0L);
      D.v[j][j] = l;
      inv[j] = 1.0L / l;
      for (int i = j + 1; i < B; ++i) {
        ld t = D.v[i][j];
        for (int q = 0; q < j; ++q) t -= D.v[i][q] * D.v[j][q];
        D.v[i][j] = t * inv[j];
      }
    }
    for (int r = 0; r < B; ++r) for (int c = 0; c < B; ++c) { if (c > r) D.v[r][c] = 0.0L; Ld[r][c] = (td)D.v[r][c]; }
    for (int j = 0; j < B; ++j) {
      invd[j] = (td)inv[j];
      td ds = D.d[j][j];
      for (int q = 0; q < j; ++q) ds -= 2.0 * D.d[j][q] * Ld[j][q];
      const td dl = 0.5 * ds * invd[j];
      D.d[j][j] = dl;
      dinv[j] = -dl * invd[j] * invd[j];
      for (int i = j + 1; i < B; ++i) {
        td dt = D.d[i][j];
        for (int q = 0; q < j; ++q) dt -= D.d[i][q] * Ld[j][q] + Ld[i][q] * D.d[j][q];
        D.d[i][j] = (dt - Ld[i][j] * dl) * invd[j];
      }
    }
    for (int r = 0; r < B; ++r) for (int c = r + 1; c < B; ++c) D.d[r][c] = 0.0;
  };
  // X <- L^-1 X with its tangent
  auto solveL = [&](const Blk& L, const ld (&inv)[MAXB], const td (&Ld)[MAXB][MAXB], const td (&invd)[MAXB], Blk& X) {
    td Xd[MAXB][MAXB];
    for (int c = 0; c < B; ++c)
      for (int i = 0; i < B; ++i) {
        ld t = X.v[i][c];
        for (int q = 0; q < i; ++q) t -= L.v[i][q] * X.v[q][c];
        X.v[i][c] = t * inv[i];
        Xd[i][c] = (td)X.v[i][c];
      }
    for (int c = 0; c < B; ++c)
      for (int i = 0; i < B; ++i) {
        td dt = X.d[i][c];
        for (int q = 0; q < i; ++q) dt -= L.d[i][q] * Xd[q][c] + Ld[i][q] * X.d[q][c];
        X.d[i][c] = (dt - L.d[i][i] * Xd[i][c]) * invd[i];
      }
  };
  auto put = [&](int rec, int f, ld x, td dx) { val[(size_t)rec * W + f] = (double)x; tan[(size_t)rec * W + f] = (double)dx; };
  ld inv[MAXB];
  td Ld[MAXB][MAXB], invd[MAXB], dinv[MAXB];
  for (int l = 0; l < p.levels; ++l) {
    const Level& L = p.lv[l];
    const int nq = (int)L.node_in.size();
    for (int q = 0; q < nq; ++q) {
      const auto& in = L.node_in[q];
      Blk D = Dv[in[0]];
      Blk Ua = Ev[in[1]];                                      // A[i, a] = E(a)
      Blk Ub;                                                  // A[i, b] = E(i)^T
      const bool hasb = in[2] >= 0;
      for (int r = 0; r < B; ++r) for (int c = 0; c < B; ++c) { Ub.v[r][c] = hasb ? Ev[in[2]].v[c][r] : 0.0L; Ub.d[r][c] = hasb ? Ev[in[2]].d[c][r] : 0.0; }
      chol(D, inv, Ld, invd, dinv, L.node_rep[q] * B);
      solveL(D, inv, Ld, invd, Ua);
      if (hasb) solveL(D, inv, Ld, invd, Ub);
      const int rec = p.lvl_off[l] + q;
      td ua[MAXB][MAXB], ub[MAXB][MAXB];
      double prod = 1.0;
      for (int r = 0; r < B; ++r) {
        put(rec, prior_f_I(B) + r, inv[r], dinv[r]);
        prod *= (double)Ld[r][r];                              // (B <= 6 factors between ~1e-4 and ~1e4: no range problem)
        dlogdet += (td)L.node_count[q] * 2.0 * D.d[r][r] * invd[r];
        for (int c = 0; c < B; ++c) {
          put(rec, prior_f_L(B) + r * B + c, D.v[r][c], D.d[r][c]);
          put(rec, prior_f_UA(B) + r * B + c, Ua.v[r][c], Ua.d[r][c]);
          put(rec, prior_f_UB(B) + r * B + c, Ub.v[r][c], Ub.d[r][c]);
          ua[r][c] = (td)Ua.v[r][c]; ub[r][c] = (td)Ub.v[r][c];
        }
      }
      {   // L^-1 (long double) with its tangent d L^-1 = -L^-1 dL L^-1, then G_a^T = U_a^T L^-1, G_b^T = U_b^T L^-1, D^-1 = L^-T L^-1
        ld Li[MAXB][MAXB];
        td Lid[MAXB][MAXB], dLi[MAXB][MAXB], tmp[MAXB][MAXB];
        for (int c = 0; c < B; ++c)
          for (int r = 0; r < B; ++r) {
            ld t = (r == c) ? 1.0L : 0.0L;
            for (int q2 = 0; q2 < r; ++q2) t -= D.v[r][q2] * Li[q2][c];
            Li[r][c] = (r >= c) ? t * inv[r] : 0.0L;
            Lid[r][c] = (td)Li[r][c];
          }
        for (int r = 0; r < B; ++r) for (int c = 0; c < B; ++c) { td t = 0.0; for (int q2 = 0; q2 < B; ++q2) t += D.d[r][q2] * Lid[q2][c]; tmp[r][c] = t; }
        for (int r = 0; r < B; ++r) for (int c = 0; c < B; ++c) { td t = 0.0; for (int q2 = 0; q2 < B; ++q2) t -= Lid[r][q2] * tmp[q2][c]; dLi[r][c] = t; }
        for (int r = 0; r < B; ++r)
          for (int c = 0; c < B; ++c) {
            ld ga = 0.0L, gb = 0.0L, di = 0.0L;
            td dga = 0.0, dgb = 0.0, ddi = 0.0;
            for (int q2 = 0; q2 < B; ++q2) {
              ga += Ua.v[q2][r] * Li[q2][c];
              gb += Ub.v[q2][r] * Li[q2][c];
              di += Li[q2][r] * Li[q2][c];
              dga += Ua.d[q2][r] * Lid[q2][c] + ua[q2][r] * dLi[q2][c];
              dgb += Ub.d[q2][r] * Lid[q2][c] + ub[q2][r] * dLi[q2][c];
              ddi += dLi[q2][r] * Lid[q2][c] + Lid[q2][r] * dLi[q2][c];
            }
            put(rec, prior_f_GAT(B) + r * B + c, ga, dga);
            put(rec, prior_f_GBT(B) + r * B + c, gb, dgb);
            put(rec, prior_f_DINV(B) + r * B + c, di, ddi);
          }
      }
      // log L_jj in double: |log| ~ 10 at 1e-16 relative, times the class count - far below the 1e-9 |ELBO| gate of the bound
      logdet += (ld)L.node_count[q] * 2.0L * (ld)log(prod);
      for (int r = 0; r < B; ++r)
        for (int c = 0; c < B; ++c) {
          ld a = 0.0L, b = 0.0L, e = 0.0L;
          td da = 0.0, db = 0.0, de = 0.0;
          for (int q2 = 0; q2 < B; ++q2) {
            a += Ua.v[q2][r] * Ua.v[q2][c];
            da += Ua.d[q2][r] * ua[q2][c] + ua[q2][r] * Ua.d[q2][c];
            if (hasb) {
              b += Ub.v[q2][r] * Ub.v[q2][c];
              e -= Ub.v[q2][r] * Ua.v[q2][c];                  // A'[b, a] = -Ub^T Ua
              db += Ub.d[q2][r] * ub[q2][c] + ub[q2][r] * Ub.d[q2][c];
              de -= Ub.d[q2][r] * ua[q2][c] + ub[q2][r] * Ua.d[q2][c];
            }
          }
          updA[q].v[r][c] = a; updB[q].v[r][c] = b; Enew[q].v[r][c] = e;
          updA[q].d[r][c] = da; updB[q].d[r][c] = db; Enew[q].d[r][c] = de;
        }
    }
    for (size_t q = 0; q < L.d_next.size(); ++q) {
      const auto& in = L.d_next[q];
      Blk D = Dv[in[0]];
      for (int r = 0; r < B; ++r)
        for (int c = 0; c < B; ++c) {
          if (in[1] >= 0) { D.v[r][c] -= updB[in[1]].v[r][c]; D.d[r][c] -= updB[in[1]].d[r][c]; }   // it was the right neighbour b of the node on its left
          if (in[2] >= 0) { D.v[r][c] -= updA[in[2]].v[r][c]; D.d[r][c] -= updA[in[2]].d[r][c]; }   // ... and the left neighbour a of the node on its right
        }
      Dn[q] = D;
    }
    { Blk* t = Dv; Dv = Dn; Dn = t; t = Ev; Ev = Enew; Enew = t; }
  }
  // ---- root: L_0, Sigma_00 = D_0^-1
  {
    Blk D = Dv[0];
    chol(D, inv, Ld, invd, dinv, 0);
    Blk X;
    for (int r = 0; r < B; ++r) for (int c = 0; c < B; ++c) { X.v[r][c] = (r == c) ? 1.0L : 0.0L; X.d[r][c] = 0.0; }
    solveL(D, inv, Ld, invd, X);
    td Xd[MAXB][MAXB];
    for (int c = 0; c < B; ++c)                                // X <- L^-T X
      for (int i = B - 1; i >= 0; --i) {
        ld t = X.v[i][c];
        for (int q = i + 1; q < B; ++q) t -= D.v[q][i] * X.v[q][c];
        X.v[i][c] = t * inv[i];
        Xd[i][c] = (td)X.v[i][c];
      }
    for (int c = 0; c < B; ++c)
      for (int i = B - 1; i >= 0; --i) {
        td dt = X.d[i][c];
        for (int q = i + 1; q < B; ++q) dt -= D.d[q][i] * Xd[q][c] + Ld[q][i] * X.d[q][c];
        X.d[i][c] = (dt - D.d[i][i] * Xd[i][c]) * invd[i];
      }
    const int rec = p.n_rec - 1;
    double prod = 1.0;
    for (int r = 0; r < B; ++r) {
      put(rec, prior_f_I(B) + r, inv[r], dinv[r]);
      prod *= (double)Ld[r][r];
      dlogdet += 2.0 * D.d[r][r] * invd[r];
      for (int c = 0; c < B; ++c) {
        put(rec, prior_f_L(B) + r * B + c, D.v[r][c], D.d[r][c]);
        put(rec, prior_f_UA(B) + r * B + c, X.v[r][c], X.d[r][c]);   // root: the U_a slot carries Sigma_00
        put(rec, prior_f_UB(B) + r * B + c, 0.0L, 0.0);
      }
    }
    logdet += 2.0L * (ld)log(prod);
  }
  // padding rows contribute log(1) = 0; header: [logdet, dlogdet/dl, first failing column + 1, n_rec]
  tab[0] = (double)logdet; tab[1] = (double)dlogdet; tab[2] = (double)bad; tab[3] = (double)R;
  return bad;
}

int prior_plan_eval(const PriorPlan* pp, const double* coef, const double* dcoef, double* tab) {
  static const bool tangent_ld = getenv("ASVGP_PRIOR_TANGENT_LD") && atoi(getenv("ASVGP_PRIOR_TANGENT_LD")) != 0;
  return tangent_ld ? prior_plan_eval_t<long double>(pp, coef, dcoef, tab) : prior_plan_eval_t<double>(pp, coef, dcoef, tab);
}

}  // namespace asvgp
