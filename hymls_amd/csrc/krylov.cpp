// krylov.cpp -- the native Krylov solver of include/hymls_mi_solver.h (the reference's HYMLS::BaseSolver,
// src/HYMLS_BaseSolver.cpp:104-397, without Belos): restarted GMRES(m) and preconditioned CG on device vectors, with
// the preconditioner and the operator of a computed hymls_mi handle (LevelSolver::apply_inverse_mv / matvec, on the
// handle's stream).  The iteration is that of hymls_amd/solver.py step for step, so both take the same number of
// iterations: classical Gram-Schmidt applied twice, Givens rotations and the small triangular solve on the host,
// convergence relative to the first residual of the solve.
//
// One GMRES iteration on one GPU: ApplyInverse, K x, the three orthogonalisation passes with their device reductions
// (krylov_hip.hip), the normalisation of the new basis column, and one device-to-host copy of (h1 + h2, ||w||) -- the
// single synchronisation of the iteration.  Sharded handles add a host all-sum (rank order) after every pass.
//
// FP32 basis storage (hymls_mi_solver_set_basis_storage(s, 32), compressed-basis GMRES): the basis columns are floats,
// every other vector and every sum stays FP64.  Column k is widened into t for ApplyInverse and K x, the three passes
// orthogonalise the FP64 w in place against the float columns, and w / ||w|| is formed in FP64 and rounded once into
// column k + 1.  A cycle ends early at KRY_F32_CYCLE_THETA, and only an explicitly computed residual ends the solve.
//
// Bordered systems [K V; W' C] [x; s] = [b; t] (hymls_mi_solver_solve_bordered, the reference's HYMLS::BorderedSolver):
// the Krylov vectors are the augmented vectors of n + m entries with the border scalars in the tail of the same device
// array, so every launcher above runs on n + m rows and the inner product is that of the reference's BorderedVector.  Only
// the two hooks differ: the operator is K x followed by dev::kry_border_product (under HYMLS_MI_BORDERED_SOLVER: the
// test-only simulators without that launcher leave the macro out and the entry returns -99), the preconditioner is
// LevelSolver::apply_inverse_bordered with T read from and S written to the tail.  One GPU.
#include "../../include/hymls_mi_solver.h"
#include "capi_internal.hpp"
#include "krylov.hpp"
#include <cmath>
#include <limits>

using namespace hymls;

// FP32 basis: a cycle ends as soon as the Givens estimate has fallen to theta times the residual the cycle started from.
// Inside one cycle a float basis cannot reduce the residual by much more than 1e-7: beyond that the estimate keeps falling
// while the true residual stalls.  Iterations to the tolerance on the numpy oracle (CGS2 GMRES(250), right preconditioned;
// FP64 basis -> FP32 basis with theta = 1e-5), tolerances 1e-8 / 1e-10 / 1e-12:
//   Stokes-C 16^3, Skew, sx 8, 1 level:   89 -> 95,   109 -> 115,  135 -> 141   (without the rule at 1e-8: 116, at 1e-10: 159)
//   Stokes-C 16^3, Skew, sx 4, 2 levels:  89 -> 95,   110 -> 116,  139 -> 143   (without the rule at 1e-12: 284)
//   Laplace 32^3, sx 4, 2 levels:         27 -> 28,   34 -> 34,    40 -> 42
// theta = 1e-4 or 1e-6 stays within 3 iterations of these.
static constexpr double KRY_F32_CYCLE_THETA = 1e-5;

struct hymls_mi_solver {
  hymls_mi_t* h = nullptr;
  hymls_mi_solver_params p{};
  std::string err;
  int its = 0;
  double achieved = std::numeric_limits<double>::quiet_NaN();
  int restarts = 0;                // Arnoldi cycles of the last column after its first one
  int basis_bits = 64;             // hymls_mi_solver_set_basis_storage: storage of the GMRES basis from the next solve on
  // device memory, allocated at the first solve and kept (grown when the row count or the restart length grows)
  int64_t n = 0, ld = 0;           // rows of this rank, leading dimension of the basis (multiple of 16 doubles)
  int m_alloc = 0;                 // basis columns allocated
  int bits_alloc = 64;             // storage the basis was allocated for
  double* V = nullptr;             // [(m + 1) * ld]; FP32 storage: the same allocation holds float[(m + 1) * ld]
  double* vec = nullptr;           // 7 vectors of ld: x, r, w, t, p, prev, staged b
  double* work = nullptr;          // reduction scratch (dev::KryWork)
  double* bc = nullptr;            // bordered solves: the device copy of C (HYMLS_MI_SOLVER_MAX_BORDER^2 doubles)
  dev::KryWork ws{};
  bool have_prev = false;
  bool profiling = false;
  double secs[4] = {0, 0, 0, 0};
  dev::KryTimer* timer = nullptr;
};

namespace {

struct Run {
  hymls_mi_solver* s;
  LevelSolver* L;
  const Comm* comm;
  int64_t n, ld;
  bool dist;
  double *x, *r, *w, *t, *p, *prev, *bst;
  // bordered solve (bm > 0): n counts the augmented rows, nh of them are the rows of K and the last bm the border scalars
  int64_t nh = 0;
  int bm = 0;
  const double* dC = nullptr;      // device copy of C
  std::vector<double> bt, bs;      // host T and S of one bordered ApplyInverse

  void mark(int phase, bool begin) { if (s->profiling) dev::kry_mark(s->timer, phase, begin); }
  // the two hooks of the iteration; with a border: M^{-1} [in; T] = [out; S] with T and S in the tails, and
  // [K V; W' C] in = K in(0:nh) followed by the border product
  void prec(const double* in, double* out) {
    mark(1, true);
    if (bm == 0) {
      L->apply_inverse_mv(in, n, out, n, 1);
    } else {
      dev::d2h(bt.data(), in + nh, bm * sizeof(double));
      L->apply_inverse_bordered(in, bt.data(), out, bs.data());
      dev::h2d(out + nh, bs.data(), bm * sizeof(double));
    }
    mark(1, false);
  }
  void matvec(const double* in, double* out) {
    mark(2, true);
    L->matvec(in, out);
#ifdef HYMLS_MI_BORDERED_SOLVER
    if (bm > 0) dev::kry_border_product(nh, bm, L->border_v(), nh, L->border_w(), nh, dC, in, out, s->ws);
#endif
    mark(2, false);
  }

  double allsum(double v) {
    if (!dist) return v;
    std::vector<double> a{v};
    comm->allsum(a);
    return a[0];
  }
  double dot(const double* a, const double* b) {
    dev::kry_dot(n, a, b, s->ws);
    double v = 0;
    dev::d2h(&v, s->ws.out, sizeof v);
    return allsum(v);
  }
  double norm(const double* a) { return std::sqrt(dot(a, a)); }

  // w <- (I - V V^T)^2 w over the k columns of V, written to dst; hk[0..k) = h1 + h2, hk[k] = ||dst||
  template <class BT>
  void orthogonalize(int k, const BT* Vb, int64_t ldv, double* wv, double* dst, double* hk) {
    orthogonalize_step(s->ws, comm, dist, n, k, Vb, ldv, wv, dst, hk);
  }
  template <class BT>   // BT: element type of the basis (float only under HYMLS_MI_F32_BASIS)
  static void orthogonalize_step(const dev::KryWork& ws, const Comm* comm, bool dist, int64_t n, int k, const BT* Vb,
                                 int64_t ldv, double* wv, double* dst, double* hk) {
    dev::kry_pass_a(n, k, Vb, ldv, wv, ws);
    std::vector<double> h1, h2;
    if (dist) {
      h1.resize(k);
      dev::d2h(h1.data(), ws.h1, k * sizeof(double));
      comm->allsum(h1);
      dev::h2d(ws.h1, h1.data(), k * sizeof(double));
    }
    dev::kry_pass_b(n, k, Vb, ldv, wv, ws);
    if (dist) {
      h2.resize(k);
      dev::d2h(h2.data(), ws.h2, k * sizeof(double));
      comm->allsum(h2);
      dev::h2d(ws.h2, h2.data(), k * sizeof(double));
    }
    dev::kry_pass_c(n, k, Vb, ldv, wv, dst, ws);
    if (dist) {
      std::vector<double> ss(1);
      dev::d2h(ss.data(), ws.out + k + 1, sizeof(double));
      comm->allsum(ss);
      const double nrm = std::sqrt(ss[0]);
      dev::h2d(ws.out + k, &nrm, sizeof nrm);
      for (int j = 0; j < k; j++) hk[j] = h1[j] + h2[j];
      hk[k] = nrm;
    }
  }

  // restarted GMRES (solver.py: Solver._gmres); x holds the start vector.  BT = double: the FP64 basis.  BT = float:
  // the FP32 basis, where the Givens estimate only ends a cycle (at the tolerance, or at KRY_F32_CYCLE_THETA times the
  // cycle's first residual) and the explicit residual at the top of the next cycle decides; rel is then always explicit
  template <class BT>
  void gmres(const double* b, int& its, double& rel, int& restarts) {
    constexpr bool F32 = sizeof(BT) == 4;
    const hymls_mi_solver_params& P = s->p;
    const int m = std::min(P.num_blocks, P.max_iters);
    const bool right = P.right != 0;
    BT* V = (BT*)s->V;
    its = 0;
    restarts = 0;
    rel = std::numeric_limits<double>::infinity();
    double beta0 = -1.0;
    std::vector<double> H, cs, sn, g, hk(dev::KRY_KMAX + 2), y;
    // FP32 basis: the loop is left only at its top, after an explicit residual (one more than the cycles allowed)
    for (int cycle = 0; cycle <= P.max_restarts + (F32 ? 1 : 0); cycle++) {
      if (its > 0 || dot(x, x) > 0.0) {
        matvec(x, t);
        mark(3, true); dev::kry_sub(n, b, t, r); mark(3, false);
      } else {
        dev::d2d(r, b, n * sizeof(double));
      }
      double* rr = r;
      if (!right) { prec(r, w); rr = w; }
      const double beta = norm(rr);
      if (beta0 < 0) beta0 = beta;
      if (beta0 == 0.0) { rel = 0.0; return; }
      rel = beta / beta0;
      if (rel <= P.tol || its >= P.max_iters || cycle > P.max_restarts) break;
      if (cycle > 0) restarts++;
      mark(3, true); first_column(rr, beta, V); mark(3, false);
      H.assign((size_t)(m + 1) * m, 0.0);   // H[i + (m + 1) * k]
      cs.assign(m, 0.0); sn.assign(m, 0.0); g.assign(m + 1, 0.0);
      g[0] = beta;
      auto Hk = [&](int i, int k) -> double& { return H[(size_t)i + (size_t)(m + 1) * k]; };
      int k_used = 0;
      for (int k = 0; k < m; k++) {
        arnoldi_product(V + (int64_t)k * ld, right);
        mark(3, true);
        new_column(k, V, hk.data());
        if (!dist) dev::d2h(hk.data(), s->ws.out, (k + 2) * sizeof(double));
        mark(3, false);
        for (int i = 0; i <= k + 1; i++) Hk(i, k) = hk[i];
        for (int i = 0; i < k; i++) {
          const double tt = cs[i] * Hk(i, k) + sn[i] * Hk(i + 1, k);
          Hk(i + 1, k) = -sn[i] * Hk(i, k) + cs[i] * Hk(i + 1, k);
          Hk(i, k) = tt;
        }
        const double d = std::hypot(Hk(k, k), Hk(k + 1, k));
        cs[k] = Hk(k, k) / d; sn[k] = Hk(k + 1, k) / d;
        Hk(k, k) = d; Hk(k + 1, k) = 0.0;
        g[k + 1] = -sn[k] * g[k]; g[k] = cs[k] * g[k];
        its++; k_used = k + 1;
        rel = std::fabs(g[k + 1]) / beta0;
        if (rel <= P.tol || its >= P.max_iters) break;
        if (F32 && std::fabs(g[k + 1]) <= KRY_F32_CYCLE_THETA * beta) break;
      }
      // y = H(0:k_used, 0:k_used) \ g, upper triangular
      y.assign(k_used, 0.0);
      for (int i = k_used - 1; i >= 0; i--) {
        double v = g[i];
        for (int j = i + 1; j < k_used; j++) v -= Hk(i, j) * y[j];
        y[i] = v / Hk(i, i);
      }
      dev::h2d(s->ws.h1, y.data(), k_used * sizeof(double));
      if (right) {
        mark(3, true); dev::zero(t, n * sizeof(double)); dev::kry_update(n, k_used, V, ld, s->ws.h1, t); mark(3, false);
        prec(t, w);
        mark(3, true); dev::kry_add(n, w, x); mark(3, false);
      } else {
        mark(3, true); dev::kry_update(n, k_used, V, ld, s->ws.h1, x); mark(3, false);
      }
      if (!F32 && (rel <= P.tol || its >= P.max_iters)) break;
    }
  }

  // the pieces of an Arnoldi step that differ between the two basis storages
  void first_column(const double* rr, double beta, double* V) { dev::kry_div(n, rr, beta, V); }
  void arnoldi_product(const double* vk, bool right) {
    if (right) { prec(vk, t); matvec(t, w); }
    else { matvec(vk, t); prec(t, w); }
  }
  void new_column(int k, double* V, double* hk) {
    double* vn = V + (int64_t)(k + 1) * ld;
    orthogonalize(k + 1, V, ld, w, vn, hk);
    dev::kry_scale_by(n, vn, s->ws.out + k + 1);   // V[k + 1] = w / ||w|| where ||w|| > 0
  }
#ifdef HYMLS_MI_F32_BASIS
  void first_column(const double* rr, double beta, float* V) { dev::kry_round_div(n, rr, beta, V); }
  void arnoldi_product(const float* vk, bool right) {
    mark(3, true); dev::kry_widen(n, vk, t); mark(3, false);   // p is free in GMRES: the second FP64 vector of the product
    if (right) { prec(t, p); matvec(p, w); }
    else { matvec(t, p); prec(p, w); }
  }
  void new_column(int k, float* V, double* hk) {
    orthogonalize(k + 1, V, ld, w, w, hk);
    dev::kry_round_scale_by(n, w, s->ws.out + k + 1, V + (int64_t)(k + 1) * ld);   // (float)(w / ||w||)
  }
#endif

  // preconditioned CG (solver.py: Solver._cg)
  void cg(const double* b, int& its, double& rel) {
    const hymls_mi_solver_params& P = s->p;
    double* z = w;
    double* q = t;
    if (dot(x, x) > 0.0) {
      matvec(x, t);
      mark(3, true); dev::kry_sub(n, b, t, r); mark(3, false);
    } else {
      dev::d2d(r, b, n * sizeof(double));
    }
    prec(r, z);
    dev::d2d(p, z, n * sizeof(double));
    double rz = dot(r, z);
    const double r0 = norm(r);
    its = 0;
    rel = 1.0;
    if (r0 == 0.0) { rel = 0.0; return; }
    while (its < P.max_iters) {
      matvec(p, q);
      const double alpha = rz / dot(p, q);
      mark(3, true);
      dev::kry_cg_xr(n, alpha, p, q, x, r, s->ws);
      double rr = 0;
      dev::d2h(&rr, s->ws.out, sizeof rr);
      mark(3, false);
      its++;
      rel = std::sqrt(allsum(rr)) / r0;
      if (rel <= P.tol) break;
      prec(r, z);
      const double rz_new = dot(r, z);
      mark(3, true); dev::kry_cg_p(n, rz_new / rz, z, p); mark(3, false);
      rz = rz_new;
    }
  }
};

uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

void check_params(const hymls_mi_solver_params& p) {
  HYMLS_CHECK(p.method == 0 || p.method == 1, -2, "Krylov Method must be GMRES (0) or CG (1)");
  HYMLS_CHECK(p.initial_vector >= 0 && p.initial_vector <= 2, -2, "Initial Vector must be Zero (0), Random (1) or Previous (2)");
  HYMLS_CHECK(p.max_iters >= 0 && p.max_restarts >= 0, -2, "Maximum Iterations and Maximum Restarts must not be negative");
  HYMLS_CHECK(p.method == 1 || (p.num_blocks >= 1 && p.num_blocks <= HYMLS_MI_SOLVER_MAX_BLOCKS), -2,
              "Num Blocks must lie in 1..256");
}

void free_buffers(hymls_mi_solver* s) {
  dev::free(s->V); dev::free(s->vec); dev::free(s->work); dev::free(s->bc);
  s->V = s->vec = s->work = s->bc = nullptr;
  s->n = s->ld = 0; s->m_alloc = 0; s->have_prev = false;
}

}  // namespace

#define SOLVER_BEGIN                           \
  try {                                        \
    HandleView hv_ = handle_view(s->h);        \
    dev::bind(hv_.ctx);
#define SOLVER_END                                                          \
  }                                                                         \
  catch (const hymls::Error& e) { s->err = e.what(); return e.code; }       \
  catch (const std::exception& e) { s->err = e.what(); return -3; }

extern "C" {

void hymls_mi_solver_default_params(hymls_mi_solver_params* p) {
  if (!p) return;
  p->method = 0;
  p->initial_vector = 0;
  p->right = 1;
  p->tol = 1e-8;
  p->max_iters = 500;
  p->num_blocks = 250;
  p->max_restarts = 20;
  p->seed = 1234;
}

int hymls_mi_solver_create(hymls_mi_solver_t** out, hymls_mi_t* h, const hymls_mi_solver_params* p) {
  if (!out || !h) return -2;
  *out = nullptr;
  hymls_mi_solver* s = new hymls_mi_solver();
  s->h = h;
  if (p) s->p = *p; else hymls_mi_solver_default_params(&s->p);
  *out = s;
  SOLVER_BEGIN
  check_params(s->p);
  s->timer = dev::kry_timer_create();
  SOLVER_END
  return 0;
}

int hymls_mi_solver_set_params(hymls_mi_solver_t* s, const hymls_mi_solver_params* p) {
  if (!s || !p) return -2;
  try { check_params(*p); }
  catch (const hymls::Error& e) { s->err = e.what(); return e.code; }
  s->p = *p;
  return 0;
}

int hymls_mi_solver_set_tolerance(hymls_mi_solver_t* s, double tol) {
  if (!s) return -2;
  s->p.tol = tol;
  return 0;
}

}  // extern "C"

namespace {
// The columns of one solve call on a computed handle.  bm = 0: K X(:, c) = B(:, c), c < nvec.  bm > 0 (the border of the
// handle, nvec = 1): the augmented system; B and X hold the nh rows of K, T and S (host, bm values, either may be null)
// the border part.  Returns 0, or -1 when a column did not reach the tolerance; errors are thrown.
int solve_columns(hymls_mi_solver* s, const HandleView& hv_, int bm, const double* B, int64_t ldb, const double* T, double* X,
                  int64_t ldx, double* S, int nvec, int on_device) {
  int status = 0;
  LevelSolver* L = hv_.top;
  const int64_t nh = L->num_owned();
  const int64_t n = nh + bm;       // rows of the Krylov vectors
  const bool gm = s->p.method == 0;
  const int m = gm ? std::min(s->p.num_blocks, std::max(s->p.max_iters, 1)) : 0;
  // buffers: grown when the problem or the restart length grows; the "Previous" solution survives only if n is unchanged
  if (n != s->n) {
    dev::sync();
    free_buffers(s);
    s->n = n;
    s->ld = std::max<int64_t>(16, (n + 15) / 16 * 16);
    s->vec = (double*)dev::alloc((size_t)7 * s->ld * sizeof(double));
    s->work = (double*)dev::alloc(dev::kry_work_doubles() * sizeof(double));
    s->ws.part = s->work;
    s->ws.h1 = s->ws.part + (size_t)dev::KRY_MAXGRID * dev::KRY_KMAX;
    s->ws.h2 = s->ws.h1 + dev::KRY_KMAX;
    s->ws.out = s->ws.h2 + dev::KRY_KMAX;
  }
  if (gm && (m > s->m_alloc || s->basis_bits != s->bits_alloc)) {
    dev::sync();
    dev::free(s->V);
    s->V = nullptr;
    s->m_alloc = 0;
    s->V = (double*)dev::alloc((size_t)(m + 1) * s->ld * (s->basis_bits / 8));
    s->m_alloc = m;
    s->bits_alloc = s->basis_bits;
  }
  Run R{s, L, hv_.comm, n, s->ld, hv_.comm->distributed()};
  R.nh = nh;
  if (bm > 0) {
    if (!s->bc) s->bc = (double*)dev::alloc((size_t)HYMLS_MI_SOLVER_MAX_BORDER * HYMLS_MI_SOLVER_MAX_BORDER * sizeof(double));
    dev::h2d(s->bc, L->border_c(), (size_t)bm * bm * sizeof(double));
    R.bm = bm;
    R.dC = s->bc;
    R.bt.assign(bm, 0.0);
    R.bs.assign(bm, 0.0);
  }
  double* v = s->vec;
  R.x = v; R.r = v + s->ld; R.w = v + 2 * s->ld; R.t = v + 3 * s->ld; R.p = v + 4 * s->ld;
  R.prev = v + 5 * s->ld; R.bst = v + 6 * s->ld;
  std::vector<double> rnd;
  if (s->p.initial_vector == 1) {
    const ivec& gids = L->owned_gids();
    rnd.resize(n);
    for (int64_t i = 0; i < n; i++) {
      // (border scalar j: the global row id that follows the rows of K)
      const uint64_t u = splitmix64(s->p.seed ^ splitmix64(i < nh ? (uint64_t)gids[i] : (uint64_t)(L->size() + (i - nh))));
      rnd[i] = (double)(u >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
    }
  }
  for (int c = 0; c < nvec; c++) {
    const double* b = B + (int64_t)c * ldb;
    if (bm > 0) {                // the augmented right-hand side [b; t] is always staged
      if (on_device) dev::d2d(R.bst, b, nh * sizeof(double));
      else dev::h2d(R.bst, b, nh * sizeof(double));
      if (T) dev::h2d(R.bst + nh, T, bm * sizeof(double));
      else dev::zero(R.bst + nh, bm * sizeof(double));
      b = R.bst;
    } else if (!on_device) { dev::h2d(R.bst, b, n * sizeof(double)); b = R.bst; }
    if (s->p.initial_vector == 1) dev::h2d(R.x, rnd.data(), n * sizeof(double));
    else if (s->p.initial_vector == 2 && s->have_prev) dev::d2d(R.x, R.prev, n * sizeof(double));
    else dev::zero(R.x, n * sizeof(double));
    R.mark(0, true);
    int its = 0, restarts = 0;
    double rel = 0;
    bool solved = false;
    if (bm > 0 && s->p.initial_vector == 2 && s->have_prev) {
      // bordered solve from the "Previous" solution: if that vector already solves this system to the tolerance, measured
      // as the true residual over the right-hand side (what a "Zero" start measures), there is nothing to iterate.
      // Otherwise the iteration runs as ever, relative to its own first residual
      const double nrm_b = R.norm(b);
      R.matvec(R.x, R.t);
      R.mark(3, true); dev::kry_sub(n, b, R.t, R.r); R.mark(3, false);
      const double nrm_r = R.norm(R.r);
      if (nrm_r <= s->p.tol * nrm_b) { rel = nrm_b > 0.0 ? nrm_r / nrm_b : 0.0; solved = true; }
    }
    if (solved) {}
    else if (!gm) R.cg(b, its, rel);
#ifdef HYMLS_MI_F32_BASIS
    else if (s->basis_bits == 32) R.gmres<float>(b, its, rel, restarts);
#endif
    else R.gmres<double>(b, its, rel, restarts);
    R.mark(0, false);
    s->its = its;
    s->restarts = restarts;
    s->achieved = rel;
    dev::d2d(R.prev, R.x, n * sizeof(double));
    s->have_prev = true;
    if (on_device) dev::d2d(X + (int64_t)c * ldx, R.x, nh * sizeof(double));
    else dev::d2h(X + (int64_t)c * ldx, R.x, nh * sizeof(double));
    if (bm > 0 && S) dev::d2h(S, R.x + nh, bm * sizeof(double));
    if (!(rel <= s->p.tol)) status = -1;
  }
  if (s->profiling) dev::kry_collect(s->timer, s->secs);
  else dev::sync();
  if (status) {
    char buf[128];
    std::snprintf(buf, sizeof buf, "Krylov solver did not converge: %d iterations, relative residual %.3e", s->its, s->achieved);
    s->err = buf;
  }
  return status;
}
}  // namespace

extern "C" {

int hymls_mi_solver_solve(hymls_mi_solver_t* s, const double* B, int64_t ldb, double* X, int64_t ldx, int nvec, int on_device) {
  if (!s) return -2;
  int status = 0;
  SOLVER_BEGIN
  HYMLS_CHECK(hv_.computed && hv_.top, -1, "The preconditioner has not yet been computed.");
  HYMLS_CHECK(hv_.top->border_size() == 0, -2, "the native solver does not solve bordered systems");
  HYMLS_CHECK(nvec >= 0 && (nvec == 0 || (B && X)), -2, "solve: null B or X");
  check_params(s->p);
  const int64_t n = hv_.top->num_owned();
  HYMLS_CHECK(nvec <= 1 || (ldb >= n && ldx >= n), -2, "solve: leading dimension smaller than the number of rows");
  status = solve_columns(s, hv_, 0, B, ldb, nullptr, X, ldx, nullptr, nvec, on_device);
  SOLVER_END
  return status;
}

int hymls_mi_solver_solve_bordered(hymls_mi_solver_t* s, const double* B, const double* T, double* X, double* S, int on_device) {
  if (!s) return -2;
  int status = 0;
  SOLVER_BEGIN
#ifndef HYMLS_MI_BORDERED_SOLVER
  (void)B; (void)T; (void)X; (void)S; (void)on_device; (void)status;
  throw hymls::Error(-99, "this build has no border product kernel (a test-only simulator without it)");
#else
  HYMLS_CHECK(hv_.computed && hv_.top, -1, "The preconditioner has not yet been computed.");
  HYMLS_CHECK(!hv_.comm->distributed(), -99, "solve_bordered: one GPU only (sharded handles are not supported)");
  HYMLS_CHECK(B && X, -2, "solve_bordered: null B or X");
  check_params(s->p);
  const int bm = hv_.top->border_size();
  const int64_t n = hv_.top->num_owned();
  if (bm == 0) {
    status = solve_columns(s, hv_, 0, B, n, nullptr, X, n, nullptr, 1, on_device);
  } else {
    HYMLS_CHECK(bm <= HYMLS_MI_SOLVER_MAX_BORDER, -2, "solve_bordered: at most 32 border columns");
    HYMLS_CHECK(s->p.method == 0, -99, "solve_bordered: the bordered operator is indefinite, CG does not apply (use GMRES)");
    status = solve_columns(s, hv_, bm, B, n, T, X, n, S, 1, on_device);
  }
#endif
  SOLVER_END
  return status;
}

int hymls_mi_solver_num_iters(const hymls_mi_solver_t* s) { return s ? s->its : 0; }
double hymls_mi_solver_achieved_tol(const hymls_mi_solver_t* s) { return s ? s->achieved : std::numeric_limits<double>::quiet_NaN(); }

int hymls_mi_solver_num_restarts(const hymls_mi_solver_t* s) { return s ? s->restarts : 0; }

int hymls_mi_solver_set_basis_storage(hymls_mi_solver_t* s, int bits) {
  if (!s) return -2;
  try {
    HYMLS_CHECK(bits == 64 || bits == 32, -2, "basis storage: 64 or 32 bits per basis entry");
#ifndef HYMLS_MI_F32_BASIS
    HYMLS_CHECK(bits == 64, -99, "this build has no FP32 basis kernels (the test-only simulator without them)");
#endif
    s->basis_bits = bits;
  } catch (const hymls::Error& e) { s->err = e.what(); return e.code; }
  return 0;
}
int hymls_mi_solver_basis_storage(const hymls_mi_solver_t* s) { return s ? s->basis_bits : 0; }

int hymls_mi_solver_set_profiling(hymls_mi_solver_t* s, int on) {
  if (!s) return -2;
  SOLVER_BEGIN
  if (s->timer) {
    double junk[4] = {0, 0, 0, 0};
    dev::kry_collect(s->timer, junk);   // drop what was recorded before
  }
  s->profiling = on != 0;
  for (double& t : s->secs) t = 0;
  SOLVER_END
  return 0;
}

double hymls_mi_solver_seconds(const hymls_mi_solver_t* s, int which) {
  if (!s || which < 0 || which > 3) return 0;
  return s->secs[which];
}

int hymls_mi_orthogonalize(hymls_mi_t* h, int64_t n, int32_t k, const double* V, int64_t ldv, double* w, double* hcoef,
                           double* wnorm) {
  if (!h) return -2;
  HandleView hv = handle_view(h);
  try {
    dev::bind(hv.ctx);
    HYMLS_CHECK(n >= 1 && k >= 1 && k <= dev::KRY_KMAX && ldv >= n && V && w && hcoef && wnorm, -2,
                "orthogonalize: need n >= 1, 1 <= k <= 256, ldv >= n and non-null arrays");
    double* work = (double*)dev::alloc(dev::kry_work_doubles() * sizeof(double));
    dev::KryWork ws;
    ws.part = work;
    ws.h1 = work + (size_t)dev::KRY_MAXGRID * dev::KRY_KMAX;
    ws.h2 = ws.h1 + dev::KRY_KMAX;
    ws.out = ws.h2 + dev::KRY_KMAX;
    std::vector<double> hk(k + 1);
    const bool dist = hv.comm->distributed();
    try {
      Run::orthogonalize_step(ws, hv.comm, dist, n, k, V, ldv, w, w, hk.data());
      if (!dist) dev::d2h(hk.data(), ws.out, (k + 1) * sizeof(double));
    } catch (...) { dev::free(work); throw; }
    dev::free(work);
    std::copy(hk.begin(), hk.begin() + k, hcoef);
    *wnorm = hk[k];
  } catch (const hymls::Error& e) { *hv.err = e.what(); return e.code; }
  catch (const std::exception& e) { *hv.err = e.what(); return -3; }
  return 0;
}

int hymls_mi_orthogonalize_f32(hymls_mi_t* h, int64_t n, int32_t k, const float* V, int64_t ldv, double* w, float* vnext,
                               double* hcoef, double* wnorm) {
  if (!h) return -2;
  HandleView hv = handle_view(h);
  try {
#ifndef HYMLS_MI_F32_BASIS
    (void)n; (void)k; (void)V; (void)ldv; (void)w; (void)vnext; (void)hcoef; (void)wnorm;
    throw hymls::Error(-99, "this build has no FP32 basis kernels (the test-only simulator without them)");
#else
    dev::bind(hv.ctx);
    HYMLS_CHECK(n >= 1 && k >= 1 && k <= dev::KRY_KMAX && ldv >= n && V && w && hcoef && wnorm, -2,
                "orthogonalize_f32: need n >= 1, 1 <= k <= 256, ldv >= n and non-null arrays");
    double* work = (double*)dev::alloc(dev::kry_work_doubles() * sizeof(double));
    dev::KryWork ws;
    ws.part = work;
    ws.h1 = work + (size_t)dev::KRY_MAXGRID * dev::KRY_KMAX;
    ws.h2 = ws.h1 + dev::KRY_KMAX;
    ws.out = ws.h2 + dev::KRY_KMAX;
    std::vector<double> hk(k + 1);
    const bool dist = hv.comm->distributed();
    try {
      Run::orthogonalize_step(ws, hv.comm, dist, n, k, V, ldv, w, w, hk.data());
      if (vnext) dev::kry_round_scale_by(n, w, ws.out + k, vnext);
      if (!dist) dev::d2h(hk.data(), ws.out, (k + 1) * sizeof(double));
      else dev::sync();
    } catch (...) { dev::free(work); throw; }
    dev::free(work);
    std::copy(hk.begin(), hk.begin() + k, hcoef);
    *wnorm = hk[k];
#endif
  } catch (const hymls::Error& e) { *hv.err = e.what(); return e.code; }
  catch (const std::exception& e) { *hv.err = e.what(); return -3; }
  return 0;
}

int hymls_mi_border_product(hymls_mi_t* h, int64_t n, int32_t m, const double* V, int64_t ldv, const double* W, int64_t ldw,
                            const double* C, const double* z, double* y) {
  if (!h) return -2;
  HandleView hv = handle_view(h);
  try {
#ifndef HYMLS_MI_BORDERED_SOLVER
    (void)n; (void)m; (void)V; (void)ldv; (void)W; (void)ldw; (void)C; (void)z; (void)y;
    throw hymls::Error(-99, "this build has no border product kernel (a test-only simulator without it)");
#else
    dev::bind(hv.ctx);
    HYMLS_CHECK(n >= 1 && m >= 1 && m <= HYMLS_MI_SOLVER_MAX_BORDER && ldv >= n && ldw >= n && V && W && z && y && z != y, -2,
                "border_product: need n >= 1, 1 <= m <= 32, ldv and ldw >= n and non-null, distinct arrays");
    const int nb = dev::kry_row_grid(n);
    double* work = (double*)dev::alloc(((size_t)nb * m + (size_t)m * m) * sizeof(double));
    dev::KryWork ws{};
    ws.part = work;
    double* dC = nullptr;
    try {
      if (C) { dC = work + (size_t)nb * m; dev::h2d(dC, C, (size_t)m * m * sizeof(double)); }
      dev::kry_border_product(n, m, V, ldv, W, ldw, dC, z, y, ws);
      dev::sync();
    } catch (...) { dev::free(work); throw; }
    dev::free(work);
#endif
  } catch (const hymls::Error& e) { *hv.err = e.what(); return e.code; }
  catch (const std::exception& e) { *hv.err = e.what(); return -3; }
  return 0;
}

const char* hymls_mi_solver_last_error(const hymls_mi_solver_t* s) { return s ? s->err.c_str() : "null solver"; }

void hymls_mi_solver_destroy(hymls_mi_solver_t* s) {
  if (!s) return;
  try {
    dev::bind(handle_view(s->h).ctx);
    dev::sync();
    free_buffers(s);
    dev::kry_timer_destroy(s->timer);
  } catch (...) {}
  delete s;
}

}  // extern "C"
