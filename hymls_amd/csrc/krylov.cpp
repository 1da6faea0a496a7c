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
//
// Lock-step columns (hymls_mi_solver_set_lockstep, under HYMLS_MI_LOCKSTEP_SOLVER): the columns of a solve call in groups of up
// to four that advance together.  Every column has a Run and an Arnoldi state of its own and takes its decisions in the same
// three steps as the single-column solve (Run::cycle_top, record_column, cycle_end); per iteration the active columns share
// one apply_inverse_mv, one matvec_mv, one batched launch chain of the orthogonalisation (krylov.hpp: KryBatch) and one copy
// of their coefficients to the host.  One GPU.  Width 1 does not touch any of it.
//
// Projection vectors (hymls_mi_solver_set_projection, under HYMLS_MI_PROJECTED_SOLVER; the reference's
// BaseSolver::setProjectionVectors with HYMLS::ProjectedOperator): the solve runs in the complement of a small space.  Only
// the two hooks and the start vector change: the operator is (I - BV V') K (I - V BV'), the preconditioner
// M^{-1} (I - BV H^{-1} BV' M^{-1}) with H = BV' M^{-1} BV, and the start vector is projected.  Every projector is one
// dev::kry_oblique_project (krylov.hpp).  The preconditioner has two forms that are equal in exact arithmetic: the literal
// one applies M^{-1} twice as the reference does, the folded one applies it once and subtracts Z (H^{-1} (BV' M^{-1} x))
// with Z = M^{-1} BV formed once per Compute.  One GPU, one column at a time.
//
// Shifted operator (hymls_mi_solver_set_shift and _set_mass_matrix, under HYMLS_MI_SHIFTED_SOLVER; the reference's
// BaseSolver::setShift / SetMassMatrix with HYMLS::ShiftedOperator): with (a, b) != (1, 0) every K x of the solve -- the plain,
// the projected and the bordered operator, the explicit residuals, CG, the lock-step group's product -- is a K x + b B x from
// one dev::kry_shifted_product (Run::product), B the mass matrix or the identity.  The preconditioner stays that of K.
// With (1, 0) nothing changes, whether or not a mass matrix is set.  One GPU.
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
  // results of every column of the last solve call (hymls_mi_solver_column_result)
  struct ColResult { int its; double achieved; int restarts; int converged; };
  std::vector<ColResult> cols;
  // lock-step columns (hymls_mi_solver_set_lockstep): column 0 of a group works in the buffers above, columns 1..width-1 in
  // sets of their own, allocated by the first solve that needs them for the n, restart length and basis storage of that solve
  int lockstep = 1;
  int lk_width = 0, lk_m = 0, lk_bits = 0;
  int64_t lk_n = 0;
  double* lk_V[HYMLS_MI_SOLVER_MAX_LOCKSTEP] = {};      // [1..width): basis
  double* lk_vec[HYMLS_MI_SOLVER_MAX_LOCKSTEP] = {};    // [1..width): 7 vectors
  double* lk_work[HYMLS_MI_SOLVER_MAX_LOCKSTEP] = {};   // [1..width): reduction scratch
  double* lk_out = nullptr;    // [width][KRY_KMAX + 2]: the out areas of all columns in one block, for one copy per step
  double* lk_stage = nullptr;  // [3][width * ld]: the contiguous operands of the batched ApplyInverse and K x
  // projection vectors (hymls_mi_solver_set_projection): one device block, allocated when they are set
  int pm = 0;                      // columns (0: no projection)
  int p_form = 0;                  // preconditioner: 0 folded, 1 literal
  bool p_same = true;              // BV = V: one copy
  int64_t p_n = 0, p_ld = 0;       // rows and leading dimension of V, BV and Z
  double* p_buf = nullptr;         // V, BV (unless BV = V), Z, one work vector, G = H^{-1}, reduction scratch
  double *pV = nullptr, *pBV = nullptr, *pZ = nullptr, *p_tmp = nullptr, *pG = nullptr;
  dev::KryWork pws{};              // part[kry_row_grid(n) * m], h1[m]
  int p_compute = -1;              // hymls_mi_num_compute of the handle when Z and H were formed (-1: not yet)
  // shifted operator a K + b B (hymls_mi_solver_set_shift, hymls_mi_solver_set_mass_matrix): the pair, and the device copy of
  // B in one block (values, rowptr, colind), allocated when B is set; without B the identity
  double sh_a = 1.0, sh_b = 0.0;
  int64_t b_n = 0, b_nnz = 0;
  void* b_buf = nullptr;
  const int32_t *b_rp = nullptr, *b_col = nullptr;
  const double* b_val = nullptr;
};

namespace {

// device scratch of one call, freed when the call ends, by return or by exception
struct Scratch {
  double* p;
  explicit Scratch(size_t doubles) : p((double*)dev::alloc(doubles * sizeof(double))) {}
  ~Scratch() { dev::free(p); }
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
};

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
  dev::KryWork ws{};               // reduction scratch and basis of the column this Run solves (the solver's own, or those of
  double* Vb = nullptr;            // a lock-step column)
  // projection vectors (pm > 0): the solver's device copies, its work vector and the scratch of the projectors
  int pm = 0;
  bool literal = false;
  int64_t pld = 0;
  const double *pV = nullptr, *pBV = nullptr, *pZ = nullptr, *pG = nullptr;
  double* ptmp = nullptr;
  dev::KryWork pws{};
  // shifted operator (shifted: (a, b) != (1, 0)): the pair and the solver's device copy of B (null: the identity)
  bool shifted = false;
  double sa = 1.0, sb = 0.0;
  const int32_t *brp = nullptr, *bcol = nullptr;
  const double* bval = nullptr;

  void mark(int phase, bool begin) { if (s->profiling) dev::kry_mark(s->timer, phase, begin); }
  // out(:, v) = K in(:, v), or (a K + b B) in(:, v) with a shift, on the rows of K; in and out must not overlap
  void product(const double* in, double* out) {
#ifdef HYMLS_MI_SHIFTED_SOLVER
    if (shifted) { product_mv(in, nh, out, nh, 1); return; }
#endif
    L->matvec(in, out);
  }
#ifdef HYMLS_MI_SHIFTED_SOLVER
  // (the lanes per row are those of LevelSolver::matvec, so the row sums of K are bitwise those of K x)
  void product_mv(const double* in, int64_t ldi, double* out, int64_t ldo, int nv) {
    const LevelSolver::DeviceCsr K = L->k_device();
    dev::kry_shifted_product(K.n, K.rowptr, K.col, K.val, -1, brp, bcol, bval, sa, sb, in, ldi, out, ldo, nv);
  }
#endif
  // the seven vectors of a column, in one block of 7 ld doubles
  void bind_vectors(double* v) {
    x = v; r = v + ld; w = v + 2 * ld; t = v + 3 * ld; p = v + 4 * ld; prev = v + 5 * ld; bst = v + 6 * ld;
  }
  // x <- the start vector of a column: random values (rnd), the solution stored by the solve before it, or zero
  void start_vector(const std::vector<double>& rnd, const double* previous) {
    if (s->p.initial_vector == 1) dev::h2d(x, rnd.data(), n * sizeof(double));
    else if (s->p.initial_vector == 2 && s->have_prev) dev::d2d(x, previous, n * sizeof(double));
    else dev::zero(x, n * sizeof(double));
  }
  // the two hooks of the iteration; with a border: M^{-1} [in; T] = [out; S] with T and S in the tails, and
  // [K V; W' C] in = K in(0:nh) followed by the border product
  void prec(const double* in, double* out) {
    mark(1, true);
    if (bm == 0) {
      L->apply_inverse_mv(in, n, out, n, 1);
#ifdef HYMLS_MI_PROJECTED_SOLVER
      // M^{-1} (I - BV H^{-1} BV' M^{-1}) in: with d = H^{-1} (BV' out), literally M^{-1} (in - BV d) as the reference
      // applies it, or folded out - Z d with Z = M^{-1} BV
      if (pm > 0 && literal) {
        dev::kry_proj_coeffs(n, pm, pBV, pld, pG, out, pws);
        dev::kry_proj_update(n, pm, pBV, pld, in, ptmp, pws);
        L->apply_inverse_mv(ptmp, n, out, n, 1);
      } else if (pm > 0) {
        dev::kry_oblique_project(n, pm, pBV, pld, pG, pZ, pld, out, out, pws);
      }
#endif
    } else {
      dev::d2h(bt.data(), in + nh, bm * sizeof(double));
      L->apply_inverse_bordered(in, bt.data(), out, bs.data());
      dev::h2d(out + nh, bs.data(), bm * sizeof(double));
    }
    mark(1, false);
  }
  void matvec(const double* in, double* out) {
    mark(2, true);
#ifdef HYMLS_MI_PROJECTED_SOLVER
    if (pm > 0) {                  // (I - BV V') K (I - V BV') in  (with a shift: a K + b B in the place of K, here and below)
      dev::kry_oblique_project(n, pm, pBV, pld, nullptr, pV, pld, in, ptmp, pws);
      product(ptmp, out);
      dev::kry_oblique_project(n, pm, pV, pld, nullptr, pBV, pld, out, out, pws);
    } else
#endif
    product(in, out);
#ifdef HYMLS_MI_BORDERED_SOLVER
    if (bm > 0) dev::kry_border_product(nh, bm, L->border_v(), nh, L->border_w(), nh, dC, in, out, ws);
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
    dev::kry_dot(n, a, b, ws);
    double v = 0;
    dev::d2h(&v, ws.out, sizeof v);
    return allsum(v);
  }
  double norm(const double* a) { return std::sqrt(dot(a, a)); }

  // w <- (I - V V^T)^2 w over the k columns of V, written to dst; hk[0..k) = h1 + h2, hk[k] = ||dst||
  template <class BT>
  void orthogonalize(int k, const BT* Vb, int64_t ldv, double* wv, double* dst, double* hk) {
    orthogonalize_step(ws, comm, dist, n, k, Vb, ldv, wv, dst, hk);
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
  // cycle's first residual) and the explicit residual at the top of the next cycle decides; rel is then always explicit.
  // The host side of one column is the Arnoldi state below and three steps: cycle_top (explicit residual, first column),
  // record_column (Givens rotations on the coefficients of a new column) and cycle_end (solution update).  gmres() runs
  // them for one column; the lock-step solve runs the same three for every column of a group, so that a column takes
  // the same decisions in both
  struct Arnoldi {
    int m = 0, its = 0, restarts = 0, cycle = 0, k = 0, k_used = 0;
    double rel = std::numeric_limits<double>::infinity(), beta = 0.0, beta0 = -1.0;
    std::vector<double> H, cs, sn, g, hk, y;
    double& Hk(int i, int j) { return H[(size_t)i + (size_t)(m + 1) * j]; }
  };
  void arnoldi_begin(Arnoldi& A) {
    A = Arnoldi();
    A.m = std::min(s->p.num_blocks, s->p.max_iters);
    A.hk.resize(dev::KRY_KMAX + 2);
  }
  // top of cycle A.cycle: false when the solve has ended (A.rel is final), else the first basis column is in place
  template <class BT>
  bool cycle_top(const double* b, Arnoldi& A) {
    constexpr bool F32 = sizeof(BT) == 4;
    const hymls_mi_solver_params& P = s->p;
    const bool right = P.right != 0;
    // FP32 basis: the loop is left only here, after an explicit residual (one more than the cycles allowed)
    if (A.cycle > P.max_restarts + (F32 ? 1 : 0)) return false;
    if (A.its > 0 || dot(x, x) > 0.0) {
      matvec(x, t);
      mark(3, true); dev::kry_sub(n, b, t, r); mark(3, false);
    } else {
      dev::d2d(r, b, n * sizeof(double));
    }
    double* rr = r;
    if (!right) { prec(r, w); rr = w; }
    const double beta = norm(rr);
    A.beta = beta;
    if (A.beta0 < 0) A.beta0 = beta;
    if (A.beta0 == 0.0) { A.rel = 0.0; return false; }
    A.rel = beta / A.beta0;
    if (A.rel <= P.tol || A.its >= P.max_iters || A.cycle > P.max_restarts) return false;
    if (A.cycle > 0) A.restarts++;
    mark(3, true); first_column(rr, beta, (BT*)Vb); mark(3, false);
    const int m = A.m;
    A.H.assign((size_t)(m + 1) * m, 0.0);   // H[i + (m + 1) * k]
    A.cs.assign(m, 0.0); A.sn.assign(m, 0.0); A.g.assign(m + 1, 0.0);
    A.g[0] = beta;
    A.k = 0;
    A.k_used = 0;
    return true;
  }
  // column A.k of the Hessenberg matrix from A.hk[0 .. k + 1]; true when the cycle ends with this column
  template <class BT>
  bool record_column(Arnoldi& A) {
    constexpr bool F32 = sizeof(BT) == 4;
    const hymls_mi_solver_params& P = s->p;
    const int k = A.k;
    std::vector<double>&cs = A.cs, &sn = A.sn, &g = A.g;
    for (int i = 0; i <= k + 1; i++) A.Hk(i, k) = A.hk[i];
    for (int i = 0; i < k; i++) {
      const double tt = cs[i] * A.Hk(i, k) + sn[i] * A.Hk(i + 1, k);
      A.Hk(i + 1, k) = -sn[i] * A.Hk(i, k) + cs[i] * A.Hk(i + 1, k);
      A.Hk(i, k) = tt;
    }
    const double d = std::hypot(A.Hk(k, k), A.Hk(k + 1, k));
    cs[k] = A.Hk(k, k) / d; sn[k] = A.Hk(k + 1, k) / d;
    A.Hk(k, k) = d; A.Hk(k + 1, k) = 0.0;
    g[k + 1] = -sn[k] * g[k]; g[k] = cs[k] * g[k];
    A.its++; A.k_used = k + 1;
    A.rel = std::fabs(g[k + 1]) / A.beta0;
    if (A.rel <= P.tol || A.its >= P.max_iters) return true;
    if (F32 && std::fabs(g[k + 1]) <= KRY_F32_CYCLE_THETA * A.beta) return true;
    A.k = k + 1;
    return A.k >= A.m;
  }
  // the solution update at the end of a cycle; false when the solve has ended
  template <class BT>
  bool cycle_end(Arnoldi& A) {
    constexpr bool F32 = sizeof(BT) == 4;
    const hymls_mi_solver_params& P = s->p;
    const bool right = P.right != 0;
    const int k_used = A.k_used;
    const BT* V = (const BT*)Vb;
    // y = H(0:k_used, 0:k_used) \ g, upper triangular
    std::vector<double>& y = A.y;
    y.assign(k_used, 0.0);
    for (int i = k_used - 1; i >= 0; i--) {
      double v = A.g[i];
      for (int j = i + 1; j < k_used; j++) v -= A.Hk(i, j) * y[j];
      y[i] = v / A.Hk(i, i);
    }
    dev::h2d(ws.h1, y.data(), k_used * sizeof(double));
    if (right) {
      mark(3, true); dev::zero(t, n * sizeof(double)); dev::kry_update(n, k_used, V, ld, ws.h1, t); mark(3, false);
      prec(t, w);
      mark(3, true); dev::kry_add(n, w, x); mark(3, false);
    } else {
      mark(3, true); dev::kry_update(n, k_used, V, ld, ws.h1, x); mark(3, false);
    }
    if (!F32 && (A.rel <= P.tol || A.its >= P.max_iters)) return false;
    A.cycle++;
    return true;
  }
  template <class BT>
  void gmres(const double* b, int& its, double& rel, int& restarts) {
    const bool right = s->p.right != 0;
    BT* V = (BT*)Vb;
    Arnoldi A;
    arnoldi_begin(A);
    while (cycle_top<BT>(b, A)) {
      bool ended = false;
      while (!ended) {
        const int k = A.k;
        arnoldi_product(V + (int64_t)k * ld, right);
        mark(3, true);
        new_column(k, V, A.hk.data());
        if (!dist) dev::d2h(A.hk.data(), ws.out, (k + 2) * sizeof(double));
        mark(3, false);
        ended = record_column<BT>(A);
      }
      if (!cycle_end<BT>(A)) break;
    }
    its = A.its;
    rel = A.rel;
    restarts = A.restarts;
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
    dev::kry_scale_by(n, vn, ws.out + k + 1);   // V[k + 1] = w / ||w|| where ||w|| > 0
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
    dev::kry_round_scale_by(n, w, ws.out + k + 1, V + (int64_t)(k + 1) * ld);   // (float)(w / ||w||)
  }
#endif

  // the start of CG: r = b - K x (b itself where x = 0), z = M^{-1} r in w, p = z;  rz = r . z, r0 = ||r||
  void cg_begin(const double* b, double& rz, double& r0) {
    if (dot(x, x) > 0.0) {
      matvec(x, t);
      mark(3, true); dev::kry_sub(n, b, t, r); mark(3, false);
    } else {
      dev::d2d(r, b, n * sizeof(double));
    }
    prec(r, w);
    dev::d2d(p, w, n * sizeof(double));
    rz = dot(r, w);
    r0 = norm(r);
  }
  // preconditioned CG (solver.py: Solver._cg)
  void cg(const double* b, int& its, double& rel) {
    const hymls_mi_solver_params& P = s->p;
    double* z = w;
    double* q = t;
    double rz = 0, r0 = 0;
    cg_begin(b, rz, r0);
    its = 0;
    rel = 1.0;
    if (r0 == 0.0) { rel = 0.0; return; }
    while (its < P.max_iters) {
      matvec(p, q);
      const double alpha = rz / dot(p, q);
      mark(3, true);
      dev::kry_cg_xr(n, alpha, p, q, x, r, ws);
      double rr = 0;
      dev::d2h(&rr, ws.out, sizeof rr);
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

#ifdef HYMLS_MI_LOCKSTEP_SOLVER
constexpr int LK_MAX = HYMLS_MI_SOLVER_MAX_LOCKSTEP;
constexpr int64_t LK_OUT = dev::KRY_KMAX + 2;   // doubles of one column's out area

void free_lockstep(hymls_mi_solver* s) {
  for (int c = 0; c < LK_MAX; c++) {
    dev::free(s->lk_V[c]); dev::free(s->lk_vec[c]); dev::free(s->lk_work[c]);
    s->lk_V[c] = s->lk_vec[c] = s->lk_work[c] = nullptr;
  }
  dev::free(s->lk_out); dev::free(s->lk_stage);
  s->lk_out = s->lk_stage = nullptr;
  s->lk_width = 0; s->lk_m = 0; s->lk_bits = 0; s->lk_n = 0;
}

// the buffers of columns 1..width-1 next to the solver's own (sized like them), the block of out areas and the staging
// columns.  A failed allocation frees what this attempt took and throws -3: the solver's own buffers are untouched
void ensure_lockstep(hymls_mi_solver* s, int width, bool gm) {
  const bool fits = s->lk_width >= width && s->lk_n == s->n && (!gm || (s->lk_m >= s->m_alloc && s->lk_bits == s->bits_alloc));
  if (fits) return;
  dev::sync();
  free_lockstep(s);
  const size_t basis = gm ? (size_t)(s->m_alloc + 1) * s->ld * (s->bits_alloc / 8) : 0;
  const size_t vecs = (size_t)7 * s->ld * sizeof(double), work = dev::kry_work_doubles() * sizeof(double);
  const size_t outs = (size_t)width * LK_OUT * sizeof(double), stage = (size_t)3 * width * s->ld * sizeof(double);
  const size_t total = (size_t)(width - 1) * (basis + vecs + work) + outs + stage;
  try {
    for (int c = 1; c < width; c++) {
      if (basis) s->lk_V[c] = (double*)dev::alloc(basis);
      s->lk_vec[c] = (double*)dev::alloc(vecs);
      s->lk_work[c] = (double*)dev::alloc(work);
    }
    s->lk_out = (double*)dev::alloc(outs);
    s->lk_stage = (double*)dev::alloc(stage);
  } catch (...) {
    free_lockstep(s);
    char buf[192];
    std::snprintf(buf, sizeof buf, "lock-step solve: could not allocate %zu bytes of device memory for %d columns (the solver "
                  "still works at width 1)", total, width);
    throw hymls::Error(-3, buf);
  }
  s->lk_width = width; s->lk_n = s->n; s->lk_m = gm ? s->m_alloc : 0; s->lk_bits = gm ? s->bits_alloc : 0;
}

// A group of nc <= width consecutive columns that advance together, one Krylov iteration per step.  Every column has a Run
// of its own (vectors, basis, reduction scratch) and takes its decisions in the steps of Run that the single-column solve
// takes them in; what happens once per cycle (explicit residual, first column, solution update) runs through the
// single-column launchers, column by column.  Per iteration the active columns share one ApplyInverse, one K x, one launch
// chain of the orthogonalisation and one copy of their coefficients to the host; a column that has ended leaves the batch.
struct Lockstep {
  hymls_mi_solver* s;
  LevelSolver* L;
  int64_t n, ld;
  int nc = 0;
  Run R[LK_MAX];
  Run::Arnoldi A[LK_MAX];
  const double* b[LK_MAX];
  bool active[LK_MAX];
  int its[LK_MAX];
  double rel[LK_MAX];
  std::vector<double> host;   // the out areas of the group on the host

  double* stage(int which, int j) const { return s->lk_stage + ((size_t)which * s->lk_width + j) * ld; }
  void mark(int phase, bool begin) { R[0].mark(phase, begin); }
  void prec_mv(int which_in, int which_out, int na) {
    mark(1, true);
    L->apply_inverse_mv(stage(which_in, 0), ld, stage(which_out, 0), ld, na);
    mark(1, false);
  }
  void matvec_mv(int which_in, int which_out, int na) {
    mark(2, true);
#ifdef HYMLS_MI_SHIFTED_SOLVER
    // with a shift: K and B are read once per group, and column v has the bits of Run::product on it
    if (R[0].shifted) R[0].product_mv(stage(which_in, 0), ld, stage(which_out, 0), ld, na);
    else
#endif
    L->matvec_mv(stage(which_in, 0), ld, stage(which_out, 0), ld, na);
    mark(2, false);
  }
  // the out areas of columns act[0] .. act[na - 1] (first `count` doubles each) in one copy
  void fetch(const int* act, int na, int64_t count) {
    const int first = act[0], last = act[na - 1];
    dev::d2h(host.data() + first * LK_OUT, s->lk_out + first * LK_OUT, ((size_t)(last - first) * LK_OUT + count) * sizeof(double));
  }

  template <class BT>
  void gmres() {
    constexpr bool F32 = sizeof(BT) == 4;
    const bool right = s->p.right != 0;
    host.assign((size_t)LK_MAX * LK_OUT, 0.0);
    for (int c = 0; c < nc; c++) {
      R[c].arnoldi_begin(A[c]);
      active[c] = R[c].template cycle_top<BT>(b[c], A[c]);
    }
    for (;;) {
      int act[LK_MAX], na = 0;
      for (int c = 0; c < nc; c++) if (active[c]) act[na++] = c;
      if (na == 0) break;
      // the current basis column of every active column, side by side (FP32 basis: widened on the way)
      mark(3, true);
      dev::KryVecBatch vb{};
      vb.nb = na;
      for (int j = 0; j < na; j++) {
        const int c = act[j];
        const BT* vk = (const BT*)R[c].Vb + (int64_t)A[c].k * ld;
        if (F32) { vb.a[j] = vk; vb.y[j] = stage(0, j); }
        else dev::d2d(stage(0, j), vk, n * sizeof(double));
      }
      if (F32) dev::kry_widen_mv(n, vb);
      mark(3, false);
      if (right) { prec_mv(0, 1, na); matvec_mv(1, 2, na); }
      else { matvec_mv(0, 1, na); prec_mv(1, 2, na); }
      // ICGS(2) of column j of the product against the basis of its own column, and the new basis column
      mark(3, true);
      dev::KryBatch B;
      B.nb = na;
      dev::KryVecBatch sb{};
      sb.nb = na;
      int kmax = 0;
      for (int j = 0; j < na; j++) {
        const int c = act[j], kk = A[c].k + 1;
        BT* vn = (BT*)R[c].Vb + (int64_t)kk * ld;
        B.k[j] = kk;
        B.V[j] = R[c].Vb;
        B.w[j] = stage(2, j);
        B.dst[j] = F32 ? stage(2, j) : (double*)vn;
        B.ws[j] = R[c].ws;
        sb.a[j] = stage(2, j);
        sb.y[j] = vn;
        sb.d[j] = R[c].ws.out + kk;
        if (c == act[na - 1]) kmax = kk;
      }
      dev::kry_pass_a_mv(n, ld, B, F32);
      dev::kry_pass_b_mv(n, ld, B, F32);
      dev::kry_pass_c_mv(n, ld, B, F32);
      if (F32) dev::kry_round_scale_by_mv(n, sb);   // (float)(w / ||w||)
      else dev::kry_scale_by_mv(n, sb);             // V[k + 1] = w / ||w|| where ||w|| > 0
      fetch(act, na, kmax + 1);
      mark(3, false);
      for (int j = 0; j < na; j++) {
        const int c = act[j];
        std::copy(host.begin() + c * LK_OUT, host.begin() + c * LK_OUT + A[c].k + 2, A[c].hk.begin());
        if (!R[c].template record_column<BT>(A[c])) continue;
        active[c] = R[c].template cycle_end<BT>(A[c]) && R[c].template cycle_top<BT>(b[c], A[c]);
      }
    }
    for (int c = 0; c < nc; c++) { its[c] = A[c].its; rel[c] = A[c].rel; }
  }

  // preconditioned CG: Run::cg_begin column by column, then the loop of Run::cg with the active columns side by side
  void cg() {
    const hymls_mi_solver_params& P = s->p;
    host.assign((size_t)LK_MAX * LK_OUT, 0.0);
    double rz[LK_MAX], r0[LK_MAX];
    for (int c = 0; c < nc; c++) {
      R[c].cg_begin(b[c], rz[c], r0[c]);
      its[c] = 0;
      rel[c] = 1.0;
      active[c] = true;
      if (r0[c] == 0.0) { rel[c] = 0.0; active[c] = false; }
      else if (!(its[c] < P.max_iters)) active[c] = false;
    }
    for (;;) {
      int act[LK_MAX], na = 0;
      for (int c = 0; c < nc; c++) if (active[c]) act[na++] = c;
      if (na == 0) break;
      dev::KryVecBatch vb{};
      vb.nb = na;
      for (int j = 0; j < na; j++) {
        const int c = act[j];
        dev::d2d(stage(0, j), R[c].p, n * sizeof(double));
        vb.a[j] = R[c].p; vb.b[j] = stage(2, j);            // p . q with q = K p
        vb.part[j] = R[c].ws.part; vb.out[j] = R[c].ws.out;
      }
      matvec_mv(0, 2, na);
      dev::kry_dot_mv(n, vb);
      fetch(act, na, 1);
      mark(3, true);
      for (int j = 0; j < na; j++) {
        const int c = act[j];
        vb.s[j] = rz[c] / host[c * LK_OUT];                // alpha
        vb.y[j] = R[c].x; vb.r[j] = R[c].r;
      }
      dev::kry_cg_xr_mv(n, vb);
      fetch(act, na, 1);
      mark(3, false);
      int cont[LK_MAX], ncont = 0;
      for (int j = 0; j < na; j++) {
        const int c = act[j];
        its[c]++;
        rel[c] = std::sqrt(host[c * LK_OUT]) / r0[c];
        if (rel[c] <= P.tol) active[c] = false;
        else cont[ncont++] = c;
      }
      if (ncont == 0) continue;
      dev::KryVecBatch zb{};
      zb.nb = ncont;
      for (int j = 0; j < ncont; j++) {
        const int c = cont[j];
        dev::d2d(stage(0, j), R[c].r, n * sizeof(double));
        zb.a[j] = R[c].r; zb.b[j] = stage(1, j);            // r . z with z = M^{-1} r
        zb.part[j] = R[c].ws.part; zb.out[j] = R[c].ws.out;
      }
      prec_mv(0, 1, ncont);
      dev::kry_dot_mv(n, zb);
      fetch(cont, ncont, 1);
      mark(3, true);
      for (int j = 0; j < ncont; j++) {
        const int c = cont[j];
        const double rz_new = host[c * LK_OUT];
        zb.s[j] = rz_new / rz[c];
        zb.a[j] = stage(1, j); zb.y[j] = R[c].p;            // p <- z + beta p
        rz[c] = rz_new;
        active[c] = its[c] < P.max_iters;
      }
      dev::kry_cg_p_mv(n, zb);
      mark(3, false);
    }
  }
};
#endif

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

void free_projection(hymls_mi_solver* s) {
  dev::free(s->p_buf);
  s->p_buf = s->pV = s->pBV = s->pZ = s->p_tmp = s->pG = nullptr;
  s->pws = dev::KryWork{};
  s->pm = 0; s->p_n = s->p_ld = 0; s->p_same = true; s->p_compute = -1;
}

void free_mass(hymls_mi_solver* s) {
  dev::free(s->b_buf);
  s->b_buf = nullptr;
  s->b_rp = s->b_col = nullptr;
  s->b_val = nullptr;
  s->b_n = s->b_nnz = 0;
}

// hands the shift and the mass matrix of the solver to a Run; (1, 0) leaves the Run on the plain K x, with or without B
void bind_shift(const hymls_mi_solver* s, Run& R) {
  R.shifted = !(s->sh_a == 1.0 && s->sh_b == 0.0);
  R.sa = s->sh_a; R.sb = s->sh_b;
  R.brp = s->b_rp; R.bcol = s->b_col; R.bval = s->b_val;
}

#ifdef HYMLS_MI_PROJECTED_SOLVER
// hands the projection of the solver to a Run
void bind_projection(const hymls_mi_solver* s, Run& R) {
  R.pm = s->pm; R.literal = s->p_form == 1; R.pld = s->p_ld;
  R.pV = s->pV; R.pBV = s->pBV; R.pZ = s->pZ; R.pG = s->pG; R.ptmp = s->p_tmp; R.pws = s->pws;
}

// Z = M^{-1} BV in groups of up to four columns, H = BV' Z column by column with the dots kernel, and G = H^{-1} from an LU
// factorisation with partial pivoting on the host (H G = I); formed again when the handle has been computed anew
void form_projection(hymls_mi_solver* s, LevelSolver* L) {
  const int m = s->pm;
  const int64_t n = s->p_n, ld = s->p_ld;
  for (int c = 0; c < m; c += 4) L->apply_inverse_mv(s->pBV + c * ld, ld, s->pZ + c * ld, ld, std::min(4, m - c));
  std::vector<double> H((size_t)m * m), G((size_t)m * m, 0.0);
  for (int k = 0; k < m; k++) {
    dev::kry_proj_coeffs(n, m, s->pBV, ld, nullptr, s->pZ + k * ld, s->pws);
    dev::d2h(H.data() + (size_t)k * m, s->pws.h1, m * sizeof(double));
  }
  for (int j = 0; j < m; j++) G[j + (size_t)m * j] = 1.0;
  for (int k = 0; k < m; k++) {
    int piv = k;
    for (int i = k + 1; i < m; i++)
      if (std::fabs(H[i + (size_t)m * k]) > std::fabs(H[piv + (size_t)m * k])) piv = i;
    const double d = H[piv + (size_t)m * k];
    if (d == 0.0 || !std::isfinite(d)) {
      char buf[160];
      std::snprintf(buf, sizeof buf, "projection vectors: H = BV' M^-1 BV is singular (zero pivot in column %d of %d)", k, m);
      throw hymls::Error(-4, buf);
    }
    if (piv != k)
      for (int j = 0; j < m; j++) {
        std::swap(H[k + (size_t)m * j], H[piv + (size_t)m * j]);
        std::swap(G[k + (size_t)m * j], G[piv + (size_t)m * j]);
      }
    for (int i = k + 1; i < m; i++) {
      const double l = H[i + (size_t)m * k] / d;
      if (l == 0.0) continue;
      for (int j = k + 1; j < m; j++) H[i + (size_t)m * j] -= l * H[k + (size_t)m * j];
      for (int j = 0; j < m; j++) G[i + (size_t)m * j] -= l * G[k + (size_t)m * j];
    }
  }
  for (int j = 0; j < m; j++)
    for (int i = m - 1; i >= 0; i--) {
      double v = G[i + (size_t)m * j];
      for (int l = i + 1; l < m; l++) v -= H[i + (size_t)m * l] * G[l + (size_t)m * j];
      G[i + (size_t)m * j] = v / H[i + (size_t)m * i];
    }
  dev::h2d(s->pG, G.data(), (size_t)m * m * sizeof(double));
  s->p_compute = hymls_mi_num_compute(s->h);
}

// the checks of a solve with projection vectors, and Z and H where they are missing or stale (counted as ApplyInverse)
void ready_projection(hymls_mi_solver* s, const HandleView& hv_, Run& R) {
  HYMLS_CHECK(!hv_.comm->distributed(), -99, "solve with projection vectors: one GPU only (sharded handles are not supported)");
  HYMLS_CHECK(s->p_n == hv_.top->num_owned(), -2, "the projection vectors do not have the row count of the handle");
  if (s->p_compute != hymls_mi_num_compute(s->h)) {
    R.mark(1, true);
    try { form_projection(s, hv_.top); } catch (...) { R.mark(1, false); throw; }
    R.mark(1, false);
  }
  bind_projection(s, R);
}
#endif

void free_buffers(hymls_mi_solver* s) {
#ifdef HYMLS_MI_LOCKSTEP_SOLVER
  free_lockstep(s);
#endif
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
    s->ws = dev::kry_work_at(s->work);
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
  bind_shift(s, R);
  HYMLS_CHECK(!R.shifted || !s->b_buf || s->b_n == nh, -2, "the mass matrix does not have the row count of the handle");
  if (bm > 0) {
    if (!s->bc) s->bc = (double*)dev::alloc((size_t)HYMLS_MI_SOLVER_MAX_BORDER * HYMLS_MI_SOLVER_MAX_BORDER * sizeof(double));
    dev::h2d(s->bc, L->border_c(), (size_t)bm * bm * sizeof(double));
    R.bm = bm;
    R.dC = s->bc;
    R.bt.assign(bm, 0.0);
    R.bs.assign(bm, 0.0);
  }
  R.ws = s->ws;
  R.Vb = s->V;
#ifdef HYMLS_MI_PROJECTED_SOLVER
  if (s->pm > 0) ready_projection(s, hv_, R);   // (a bordered solve with projection vectors has been refused before)
#endif
  s->cols.clear();
  R.bind_vectors(s->vec);
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
#ifdef HYMLS_MI_LOCKSTEP_SOLVER
  // lock-step columns: groups of `width` consecutive columns (the bordered solve has one right-hand side and ignores it)
  // and so does a solve with projection vectors: its columns go one after the other
  const int width = bm == 0 && s->pm == 0 ? std::min(s->lockstep, std::max(nvec, 1)) : 1;
  if (width > 1) {
    ensure_lockstep(s, width, gm);
    Lockstep G{s, L, n, s->ld};
    for (int c0 = 0; c0 < nvec; c0 += width) {
      G.nc = std::min(width, nvec - c0);
      for (int c = 0; c < G.nc; c++) {
        Run& Rc = G.R[c];
        Rc = R;
        if (c > 0) {
          Rc.bind_vectors(s->lk_vec[c]);
          Rc.Vb = s->lk_V[c];
          Rc.ws = dev::kry_work_at(s->lk_work[c]);
        }
        Rc.ws.out = s->lk_out + c * LK_OUT;   // the out areas of a group: one block, one copy per step
        const double* b = B + (int64_t)(c0 + c) * ldb;
        if (!on_device) { dev::h2d(Rc.bst, b, n * sizeof(double)); b = Rc.bst; }
        G.b[c] = b;
        // "Previous": every column of the group starts from the solution stored before the group
        Rc.start_vector(rnd, R.prev);
      }
      R.mark(0, true);
      if (!gm) G.cg();
#ifdef HYMLS_MI_F32_BASIS
      else if (s->basis_bits == 32) G.gmres<float>();
#endif
      else G.gmres<double>();
      R.mark(0, false);
      for (int c = 0; c < G.nc; c++) {
        const int restarts = gm ? G.A[c].restarts : 0;
        s->its = G.its[c];
        s->restarts = restarts;
        s->achieved = G.rel[c];
        s->cols.push_back({G.its[c], G.rel[c], restarts, G.rel[c] <= s->p.tol ? 1 : 0});
        if (on_device) dev::d2d(X + (int64_t)(c0 + c) * ldx, G.R[c].x, n * sizeof(double));
        else dev::d2h(X + (int64_t)(c0 + c) * ldx, G.R[c].x, n * sizeof(double));
        if (!(G.rel[c] <= s->p.tol)) status = -1;
      }
      dev::d2d(R.prev, G.R[G.nc - 1].x, n * sizeof(double));   // the group's last column
      s->have_prev = true;
    }
    nvec = 0;   // nothing is left for the column-by-column loop
  }
#endif
  for (int c = 0; c < nvec; c++) {
    const double* b = B + (int64_t)c * ldb;
    if (bm > 0) {                // the augmented right-hand side [b; t] is always staged
      if (on_device) dev::d2d(R.bst, b, nh * sizeof(double));
      else dev::h2d(R.bst, b, nh * sizeof(double));
      if (T) dev::h2d(R.bst + nh, T, bm * sizeof(double));
      else dev::zero(R.bst + nh, bm * sizeof(double));
      b = R.bst;
    } else if (!on_device) { dev::h2d(R.bst, b, n * sizeof(double)); b = R.bst; }
    R.start_vector(rnd, R.prev);
    R.mark(0, true);
#ifdef HYMLS_MI_PROJECTED_SOLVER
    // the start vector in the complement: x0 <- x0 - BV (V' x0) (reference BaseSolver.cpp:339-345)
    if (R.pm > 0) { R.mark(3, true); dev::kry_oblique_project(n, R.pm, R.pV, R.pld, nullptr, R.pBV, R.pld, R.x, R.x, R.pws); R.mark(3, false); }
#endif
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
    s->cols.push_back({its, rel, restarts, rel <= s->p.tol ? 1 : 0});
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

// one ICGS(2) step on caller-owned device arrays (hymls_mi_orthogonalize, _f32): w in place, the coefficients and the norm
// to the host; vnext (FP32 basis only, may be null): the rounded new column (float)(w / ||w||)
template <class BT>
void orthogonalize_one(const HandleView& hv, const char* name, int64_t n, int32_t k, const BT* V, int64_t ldv, double* w,
                       float* vnext, double* hcoef, double* wnorm) {
  dev::bind(hv.ctx);
  HYMLS_CHECK(n >= 1 && k >= 1 && k <= dev::KRY_KMAX && ldv >= n && V && w && hcoef && wnorm, -2,
              std::string(name) + ": need n >= 1, 1 <= k <= 256, ldv >= n and non-null arrays");
  Scratch work(dev::kry_work_doubles());
  const dev::KryWork ws = dev::kry_work_at(work.p);
  std::vector<double> hk(k + 1);
  const bool dist = hv.comm->distributed();
  Run::orthogonalize_step(ws, hv.comm, dist, n, k, V, ldv, w, w, hk.data());
  if constexpr (sizeof(BT) == 4) {
    if (vnext) dev::kry_round_scale_by(n, w, ws.out + k, vnext);
  }
  if (!dist) dev::d2h(hk.data(), ws.out, (k + 1) * sizeof(double));
  else dev::sync();   // (the rounding store has ended before the scratch is freed)
  std::copy(hk.begin(), hk.begin() + k, hcoef);
  *wnorm = hk[k];
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
  HYMLS_CHECK(s->lockstep == 1 || !hv_.comm->distributed(), -99, "solve with lock-step columns: one GPU only (sharded handles are not supported)");
#ifndef HYMLS_MI_LOCKSTEP_SOLVER
  HYMLS_CHECK(s->lockstep == 1, -99, "this build has no batched Krylov launchers (a test-only simulator without them)");
#endif
  HYMLS_CHECK(s->pm == 0 || !hv_.comm->distributed(), -99, "solve with projection vectors: one GPU only (sharded handles are not supported)");
  HYMLS_CHECK((s->sh_a == 1.0 && s->sh_b == 0.0) || !hv_.comm->distributed(), -99,
              "solve with a shift: one GPU only (sharded handles are not supported)");  status = solve_columns(s, hv_, 0, B, ldb, nullptr, X, ldx, nullptr, nvec, on_device);
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
  HYMLS_CHECK(s->pm == 0, -99, "solve_bordered: projection vectors are set (the bordered solve does not combine with them)");
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
    orthogonalize_one(hv, "orthogonalize", n, k, V, ldv, w, nullptr, hcoef, wnorm);
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
    orthogonalize_one(hv, "orthogonalize_f32", n, k, V, ldv, w, vnext, hcoef, wnorm);
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
    Scratch work((size_t)nb * m + (size_t)m * m);
    dev::KryWork ws{};
    ws.part = work.p;
    double* dC = nullptr;
    if (C) { dC = work.p + (size_t)nb * m; dev::h2d(dC, C, (size_t)m * m * sizeof(double)); }
    dev::kry_border_product(n, m, V, ldv, W, ldw, dC, z, y, ws);
    dev::sync();
#endif
  } catch (const hymls::Error& e) { *hv.err = e.what(); return e.code; }
  catch (const std::exception& e) { *hv.err = e.what(); return -3; }
  return 0;
}

#ifndef HYMLS_MI_PROJECTED_SOLVER
#define PROJ_MISSING throw hymls::Error(-99, "this build has no projection kernels (a test-only simulator without them)")
#endif

int hymls_mi_solver_set_projection(hymls_mi_solver_t* s, int64_t n, int32_t m, const double* V, int64_t ldv, const double* BV,
                                   int64_t ldbv, int on_device) {
  if (!s) return -2;
  SOLVER_BEGIN
#ifndef HYMLS_MI_PROJECTED_SOLVER
  (void)n; (void)m; (void)V; (void)ldv; (void)BV; (void)ldbv; (void)on_device;
  PROJ_MISSING;
#else
  if (m == 0 || !V) {              // no projection from the next solve on
    if (s->p_buf) dev::sync();
    free_projection(s);
    return 0;
  }
  HYMLS_CHECK(hv_.top, -1, "set_projection needs an initialized handle (its row count)");
  HYMLS_CHECK(m >= 1 && m <= HYMLS_MI_SOLVER_MAX_PROJECTION, -2, "set_projection: at most 32 projection vectors");
  HYMLS_CHECK(n == hv_.top->num_owned(), -2, "set_projection: n is not the row count of the handle");
  HYMLS_CHECK(ldv >= n && (!BV || ldbv >= n), -2, "set_projection: leading dimension smaller than the number of rows");
  if (s->p_buf) dev::sync();
  free_projection(s);
  const bool same = !BV || (BV == V && ldbv == ldv);
  const int64_t ld = std::max<int64_t>(16, (n + 15) / 16 * 16);
  const int nb = dev::kry_row_grid(n);
  const size_t doubles = (size_t)((same ? 2 : 3) * m + 1) * ld + (size_t)m * m + (size_t)nb * m + dev::KRY_PROJ_MAX;
  try {
    s->p_buf = (double*)dev::alloc(doubles * sizeof(double));
  } catch (...) {
    char buf[192];
    std::snprintf(buf, sizeof buf, "set_projection: could not allocate %zu bytes of device memory for %d projection vectors "
                  "(the solver still works without a projection)", doubles * sizeof(double), (int)m);
    throw hymls::Error(-3, buf);
  }
  s->pV = s->p_buf;
  s->pBV = same ? s->pV : s->pV + (size_t)m * ld;
  s->pZ = s->pBV + (size_t)m * ld;
  s->p_tmp = s->pZ + (size_t)m * ld;
  s->pG = s->p_tmp + ld;
  s->pws.part = s->pG + (size_t)m * m;
  s->pws.h1 = s->pws.part + (size_t)nb * m;
  s->p_same = same; s->p_n = n; s->p_ld = ld;
  try {
    for (int j = 0; j < m; j++) {
      if (on_device) dev::d2d(s->pV + (size_t)j * ld, V + (int64_t)j * ldv, n * sizeof(double));
      else dev::h2d(s->pV + (size_t)j * ld, V + (int64_t)j * ldv, n * sizeof(double));
      if (same) continue;
      if (on_device) dev::d2d(s->pBV + (size_t)j * ld, BV + (int64_t)j * ldbv, n * sizeof(double));
      else dev::h2d(s->pBV + (size_t)j * ld, BV + (int64_t)j * ldbv, n * sizeof(double));
    }
    // the reference's CheckOrthogonal (DenseUtils.cpp:177-199): ||V' BV - I||_inf <= 1e-8, column k of V' BV from the
    // dots kernel.  (A sharded handle has only this rank's rows here; its solve is refused, so the check is left out)
    if (!hv_.comm->distributed()) {
      std::vector<double> M((size_t)m * m);
      for (int k = 0; k < m; k++) {
        dev::kry_proj_coeffs(n, m, s->pV, ld, nullptr, s->pBV + (size_t)k * ld, s->pws);
        dev::d2h(M.data() + (size_t)k * m, s->pws.h1, m * sizeof(double));
      }
      double norm = 0.0;
      for (int i = 0; i < m; i++) {
        double row = 0.0;
        for (int k = 0; k < m; k++) row += std::fabs(M[i + (size_t)m * k] - (i == k ? 1.0 : 0.0));
        norm = std::max(norm, row);
      }
      if (!(norm <= 1e-8)) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "set_projection: the vectors are not orthogonal, ||V' BV - I||_inf = %.3e (at most 1e-8)", norm);
        throw hymls::Error(-2, buf);
      }
    }
  } catch (...) {
    dev::sync();
    free_projection(s);
    throw;
  }
  s->pm = m;
#endif
  SOLVER_END
  return 0;
}

int hymls_mi_solver_num_projection(const hymls_mi_solver_t* s) { return s ? s->pm : 0; }

int hymls_mi_solver_set_projection_form(hymls_mi_solver_t* s, int form) {
  if (!s) return -2;
  try {
#ifndef HYMLS_MI_PROJECTED_SOLVER
    (void)form;
    PROJ_MISSING;
#else
    HYMLS_CHECK(form == 0 || form == 1, -2, "projection form: 0 (folded) or 1 (literal)");
    s->p_form = form;
#endif
  } catch (const hymls::Error& e) { s->err = e.what(); return e.code; }
  return 0;
}

int hymls_mi_solver_apply_projected(hymls_mi_solver_t* s, int which, const double* X, double* Y, int on_device) {
  if (!s) return -2;
  SOLVER_BEGIN
#ifndef HYMLS_MI_PROJECTED_SOLVER
  (void)which; (void)X; (void)Y; (void)on_device;
  PROJ_MISSING;
#else
  HYMLS_CHECK(hv_.computed && hv_.top, -1, "The preconditioner has not yet been computed.");
  HYMLS_CHECK(s->pm > 0, -2, "apply_projected: no projection vectors are set");
  HYMLS_CHECK((which == 0 || which == 1) && X && Y, -2, "apply_projected: which is 0 (operator) or 1 (preconditioner); X and Y non-null");
  const int64_t n = hv_.top->num_owned();
  Run R{s, hv_.top, hv_.comm, n, s->p_ld, hv_.comm->distributed()};
  R.nh = n;
  bind_shift(s, R);
  ready_projection(s, hv_, R);
  Scratch stage((size_t)2 * s->p_ld);   // staged: X may be Y or host memory
  double* buf = stage.p;
  if (on_device) dev::d2d(buf, X, n * sizeof(double));
  else dev::h2d(buf, X, n * sizeof(double));
  if (which == 0) R.matvec(buf, buf + s->p_ld);
  else R.prec(buf, buf + s->p_ld);
  if (on_device) { dev::d2d(Y, buf + s->p_ld, n * sizeof(double)); dev::sync(); }
  else dev::d2h(Y, buf + s->p_ld, n * sizeof(double));
#endif
  SOLVER_END
  return 0;
}

int hymls_mi_oblique_project(hymls_mi_t* h, int64_t n, int32_t m, const double* Q, int64_t ldq, const double* G, const double* P,
                             int64_t ldp, const double* x, double* y) {
  if (!h) return -2;
  HandleView hv = handle_view(h);
  try {
#ifndef HYMLS_MI_PROJECTED_SOLVER
    (void)n; (void)m; (void)Q; (void)ldq; (void)G; (void)P; (void)ldp; (void)x; (void)y;
    PROJ_MISSING;
#else
    dev::bind(hv.ctx);
    HYMLS_CHECK(n >= 1 && m >= 1 && m <= HYMLS_MI_SOLVER_MAX_PROJECTION && ldq >= n && ldp >= n && Q && P && x && y, -2,
                "oblique_project: need n >= 1, 1 <= m <= 32, ldq and ldp >= n and non-null arrays");
    const int nb = dev::kry_row_grid(n);
    Scratch work((size_t)nb * m + (size_t)m * m + dev::KRY_PROJ_MAX);
    dev::KryWork ws{};
    ws.part = work.p;
    ws.h1 = work.p + (size_t)nb * m + (size_t)m * m;
    double* dG = nullptr;
    if (G) { dG = work.p + (size_t)nb * m; dev::h2d(dG, G, (size_t)m * m * sizeof(double)); }
    dev::kry_oblique_project(n, m, Q, ldq, dG, P, ldp, x, y, ws);
    dev::sync();
#endif
  } catch (const hymls::Error& e) { *hv.err = e.what(); return e.code; }
  catch (const std::exception& e) { *hv.err = e.what(); return -3; }
  return 0;
}

#ifndef HYMLS_MI_SHIFTED_SOLVER
#define SHIFT_MISSING throw hymls::Error(-99, "this build has no shifted product kernel (a test-only simulator without it)")
#else
namespace {
// do the nvec columns of n doubles at X (leading dimension ldx) and at Y (ldy) share a byte?
bool columns_overlap(const double* X, int64_t ldx, const double* Y, int64_t ldy, int64_t n, int nvec) {
  const uintptr_t x0 = (uintptr_t)X, x1 = x0 + ((size_t)(nvec - 1) * ldx + n) * sizeof(double);
  const uintptr_t y0 = (uintptr_t)Y, y1 = y0 + ((size_t)(nvec - 1) * ldy + n) * sizeof(double);
  return x0 < y1 && y0 < x1;
}
}  // namespace
#endif

int hymls_mi_solver_set_mass_matrix(hymls_mi_solver_t* s, int64_t n, const int32_t* rowptr, const int32_t* colind,
                                    const double* values, int on_device) {
  if (!s) return -2;
  SOLVER_BEGIN
#ifndef HYMLS_MI_SHIFTED_SOLVER
  (void)n; (void)rowptr; (void)colind; (void)values; (void)on_device;
  SHIFT_MISSING;
#else
  if (s->b_buf) dev::sync();       // whatever follows, the matrix set before is gone
  free_mass(s);
  if (!rowptr) return 0;           // the identity from the next solve on
  HYMLS_CHECK(hv_.top, -1, "set_mass_matrix needs an initialized handle (its row count)");
  HYMLS_CHECK(n == hv_.top->num_owned(), -2, "set_mass_matrix: n is not the row count of the handle");
  // every index is checked on the host before a kernel reads it; device input: rowptr and colind are copied back once
  std::vector<int32_t> hrp, hcol;
  const int32_t* rp = rowptr;
  if (on_device) { hrp.resize(n + 1); dev::d2h(hrp.data(), rowptr, (size_t)(n + 1) * sizeof(int32_t)); rp = hrp.data(); }
  HYMLS_CHECK(rp[0] == 0, -2, "set_mass_matrix: rowptr[0] is not 0");
  for (int64_t i = 0; i < n; i++)
    if (rp[i + 1] < rp[i]) {
      char buf[128];
      std::snprintf(buf, sizeof buf, "set_mass_matrix: rowptr decreases at row %lld (%d after %d)", (long long)i, (int)rp[i + 1], (int)rp[i]);
      throw hymls::Error(-2, buf);
    }
  // (rowptr is int32 and does not decrease, so nnz < 2^31: a larger matrix cannot be expressed and shows as a decrease)
  const int64_t nnz = rp[n];
  HYMLS_CHECK(nnz == 0 || (colind && values), -2, "set_mass_matrix: null colind or values");
  const int32_t* col = colind;
  if (on_device && nnz > 0) { hcol.resize(nnz); dev::d2h(hcol.data(), colind, (size_t)nnz * sizeof(int32_t)); col = hcol.data(); }
  for (int64_t k = 0; k < nnz; k++)
    if (col[k] < 0 || col[k] >= n) {
      char buf[128];
      std::snprintf(buf, sizeof buf, "set_mass_matrix: column %d at entry %lld lies outside [0, %lld)", (int)col[k], (long long)k, (long long)n);
      throw hymls::Error(-2, buf);
    }
  const size_t bytes = (size_t)nnz * (sizeof(double) + sizeof(int32_t)) + (size_t)(n + 1) * sizeof(int32_t);
  try {
    s->b_buf = dev::alloc(bytes);
  } catch (...) {
    char buf[192];
    std::snprintf(buf, sizeof buf, "set_mass_matrix: could not allocate %zu bytes of device memory for the mass matrix (the solver "
                  "is left without one)", bytes);
    throw hymls::Error(-3, buf);
  }
  double* dval = (double*)s->b_buf;
  int32_t* drp = (int32_t*)(dval + nnz);
  int32_t* dcol = drp + (n + 1);
  try {
    if (on_device) {
      dev::d2d(drp, rowptr, (size_t)(n + 1) * sizeof(int32_t));
      if (nnz > 0) { dev::d2d(dcol, colind, (size_t)nnz * sizeof(int32_t)); dev::d2d(dval, values, (size_t)nnz * sizeof(double)); }
    } else {
      dev::h2d(drp, rowptr, (size_t)(n + 1) * sizeof(int32_t));
      if (nnz > 0) { dev::h2d(dcol, colind, (size_t)nnz * sizeof(int32_t)); dev::h2d(dval, values, (size_t)nnz * sizeof(double)); }
    }
    dev::sync();
  } catch (...) {
    free_mass(s);
    throw;
  }
  s->b_rp = drp; s->b_col = dcol; s->b_val = dval;
  s->b_n = n; s->b_nnz = nnz;
#endif
  SOLVER_END
  return 0;
}

int hymls_mi_solver_apply_mass(hymls_mi_solver_t* s, const double* X, int64_t ldx, double* Y, int64_t ldy, int nvec, int on_device) {
  if (!s) return -2;
  SOLVER_BEGIN
#ifndef HYMLS_MI_SHIFTED_SOLVER
  (void)X; (void)ldx; (void)Y; (void)ldy; (void)nvec; (void)on_device;
  SHIFT_MISSING;
#else
  HYMLS_CHECK(hv_.top, -1, "apply_mass needs an initialized handle (its row count)");
  const int64_t n = hv_.top->num_owned();
  HYMLS_CHECK(nvec >= 0 && (nvec == 0 || (X && Y && ldx >= n && ldy >= n)), -2, "apply_mass: need non-null X, Y and ldx, ldy >= n");
  if (nvec == 0) return 0;
  HYMLS_CHECK(!s->b_buf || s->b_n == n, -2, "the mass matrix does not have the row count of the handle");
  if (on_device) {
    HYMLS_CHECK(!columns_overlap(X, ldx, Y, ldy, n, nvec), -2, "apply_mass: X and Y overlap");
    dev::kry_shifted_product((int32_t)n, nullptr, nullptr, nullptr, -1, s->b_rp, s->b_col, s->b_val, 0.0, 1.0, X, ldx, Y, ldy, nvec);
    dev::sync();
  } else {
    Scratch stage((size_t)2 * nvec * n);
    double* buf = stage.p;
    for (int v = 0; v < nvec; v++) dev::h2d(buf + (int64_t)v * n, X + (int64_t)v * ldx, n * sizeof(double));
    dev::kry_shifted_product((int32_t)n, nullptr, nullptr, nullptr, -1, s->b_rp, s->b_col, s->b_val, 0.0, 1.0, buf, n,
                             buf + (int64_t)nvec * n, n, nvec);
    for (int v = 0; v < nvec; v++) dev::d2h(Y + (int64_t)v * ldy, buf + (int64_t)(nvec + v) * n, n * sizeof(double));
  }
#endif
  SOLVER_END
  return 0;
}

int hymls_mi_solver_set_shift(hymls_mi_solver_t* s, double shift_a, double shift_b) {
  if (!s) return -2;
  try {
#ifndef HYMLS_MI_SHIFTED_SOLVER
    (void)shift_a; (void)shift_b;
    SHIFT_MISSING;
#else
    HYMLS_CHECK(std::isfinite(shift_a) && std::isfinite(shift_b), -2, "set_shift: the shifts must be finite");
    HYMLS_CHECK(shift_a != 0.0 || shift_b != 0.0, -2, "set_shift: a = b = 0 is the zero operator");
    s->sh_a = shift_a;
    s->sh_b = shift_b;
#endif
  } catch (const hymls::Error& e) { s->err = e.what(); return e.code; }
  return 0;
}

int hymls_mi_solver_shift(const hymls_mi_solver_t* s, double* shift_a, double* shift_b) {
  if (!s) return -2;
#ifndef HYMLS_MI_SHIFTED_SOLVER
  (void)shift_a; (void)shift_b;
  return -99;
#else
  if (shift_a) *shift_a = s->sh_a;
  if (shift_b) *shift_b = s->sh_b;
  return 0;
#endif
}

int hymls_mi_shifted_product(hymls_mi_t* h, int64_t n, double a, const int32_t* rpA, const int32_t* colA, const double* valA,
                             int64_t nnzA_hint, double b, const int32_t* rpB, const int32_t* colB, const double* valB,
                             const double* X, int64_t ldx, double* Y, int64_t ldy, int nvec) {
  if (!h) return -2;
  HandleView hv = handle_view(h);
  try {
#ifndef HYMLS_MI_SHIFTED_SOLVER
    (void)n; (void)a; (void)rpA; (void)colA; (void)valA; (void)nnzA_hint; (void)b; (void)rpB; (void)colB; (void)valB;
    (void)X; (void)ldx; (void)Y; (void)ldy; (void)nvec;
    SHIFT_MISSING;
#else
    dev::bind(hv.ctx);
    HYMLS_CHECK(n >= 1 && n < ((int64_t)1 << 31) && nvec >= 0, -2, "shifted_product: need 1 <= n < 2^31 and nvec >= 0");
    if (nvec == 0) return 0;
    HYMLS_CHECK(X && Y && ldx >= n && ldy >= n, -2, "shifted_product: need non-null X, Y and ldx, ldy >= n");
    HYMLS_CHECK(a == 0.0 || (rpA && colA && valA), -2, "shifted_product: null arrays of A with a != 0");
    HYMLS_CHECK(!rpB || (colB && valB), -2, "shifted_product: B has a rowptr, but null colind or values");
    HYMLS_CHECK(!columns_overlap(X, ldx, Y, ldy, n, nvec), -2, "shifted_product: X and Y overlap");
    dev::kry_shifted_product((int32_t)n, rpA, colA, valA, nnzA_hint, rpB, colB, valB, a, b, X, ldx, Y, ldy, nvec);
    dev::sync();
#endif
  } catch (const hymls::Error& e) { *hv.err = e.what(); return e.code; }
  catch (const std::exception& e) { *hv.err = e.what(); return -3; }
  return 0;
}

int hymls_mi_solver_set_lockstep(hymls_mi_solver_t* s, int width) {
  if (!s) return -2;
  SOLVER_BEGIN
  HYMLS_CHECK(width >= 1 && width <= HYMLS_MI_SOLVER_MAX_LOCKSTEP, -2, "lock-step columns: 1 to 4");
#ifndef HYMLS_MI_LOCKSTEP_SOLVER
  HYMLS_CHECK(width == 1, -99, "this build has no batched Krylov launchers (a test-only simulator without them)");
#else
  if (width != s->lockstep && s->lk_width > 0) {   // another width: the next solve allocates what it needs
    dev::sync();
    free_lockstep(s);
  }
#endif
  s->lockstep = width;
  SOLVER_END
  return 0;
}
int hymls_mi_solver_lockstep(const hymls_mi_solver_t* s) { return s ? s->lockstep : 0; }

int hymls_mi_solver_column_result(const hymls_mi_solver_t* s, int v, int* iters, double* achieved_tol, int* restarts, int* converged) {
  if (!s || v < 0 || v >= (int)s->cols.size()) return -2;
  const hymls_mi_solver::ColResult& c = s->cols[v];
  if (iters) *iters = c.its;
  if (achieved_tol) *achieved_tol = c.achieved;
  if (restarts) *restarts = c.restarts;
  if (converged) *converged = c.converged;
  return 0;
}

int hymls_mi_matvec_mv(hymls_mi_t* h, const double* X, int64_t ldx, double* Y, int64_t ldy, int nvec, int on_device) {
  if (!h) return -2;
  HandleView hv = handle_view(h);
  try {
#ifndef HYMLS_MI_LOCKSTEP_SOLVER
    (void)X; (void)ldx; (void)Y; (void)ldy; (void)nvec; (void)on_device;
    throw hymls::Error(-99, "this build has no multi-vector K x kernel (a test-only simulator without it)");
#else
    dev::bind(hv.ctx);
    HYMLS_CHECK(hv.computed && hv.top, -1, "matvec_mv needs a computed preconditioner (device copy of K)");
    HYMLS_CHECK(!hv.comm->distributed(), -99, "matvec_mv: one GPU only (sharded handles are not supported)");
    const int64_t n = hv.top->num_owned();
    HYMLS_CHECK(nvec >= 0 && (nvec == 0 || (X && Y && ldx >= n && ldy >= n)), -2, "matvec_mv: need non-null X, Y and ldx, ldy >= n");
    if (nvec == 0) return 0;
    if (on_device) {
      hv.top->matvec_mv(X, ldx, Y, ldy, nvec);
      dev::sync();
    } else {
      Scratch stage((size_t)2 * nvec * n);
      double* buf = stage.p;
      for (int v = 0; v < nvec; v++) dev::h2d(buf + (int64_t)v * n, X + (int64_t)v * ldx, n * sizeof(double));
      hv.top->matvec_mv(buf, n, buf + (int64_t)nvec * n, n, nvec);
      for (int v = 0; v < nvec; v++) dev::d2h(Y + (int64_t)v * ldy, buf + (int64_t)(nvec + v) * n, n * sizeof(double));
    }
#endif
  } catch (const hymls::Error& e) { *hv.err = e.what(); return e.code; }
  catch (const std::exception& e) { *hv.err = e.what(); return -3; }
  return 0;
}

}  // extern "C"

#ifdef HYMLS_MI_LOCKSTEP_SOLVER
namespace {
// nb independent ICGS(2) steps in one launch chain (the orthogonalisation of one lock-step iteration); vnext: FP32 basis only
template <class BT>
void orthogonalize_mv(const HandleView& hv, int64_t n, int32_t nb, const int32_t* k, const BT* V, int64_t ldv, int64_t vstride,
                      double* W, int64_t ldw, float* vnext, int64_t ldn, double* hcoef, int64_t ldh, double* wnorm) {
  constexpr bool F32 = sizeof(BT) == 4;
  dev::bind(hv.ctx);
  HYMLS_CHECK(!hv.comm->distributed(), -99, "orthogonalize_mv: one GPU only (sharded handles are not supported)");
  HYMLS_CHECK(nb >= 1 && nb <= HYMLS_MI_SOLVER_MAX_LOCKSTEP && k && n >= 1 && ldv >= n && ldw >= n && V && W && hcoef && wnorm &&
              (!vnext || ldn >= n), -2, "orthogonalize_mv: need 1 <= nb <= 4, n >= 1, ldv, ldw >= n and non-null arrays");
  int kmax = 0;
  for (int v = 0; v < nb; v++) {
    HYMLS_CHECK(k[v] >= 1 && k[v] <= dev::KRY_KMAX, -2, "orthogonalize_mv: need 1 <= k[v] <= 256");
    kmax = std::max(kmax, (int)k[v]);
  }
  HYMLS_CHECK(ldh >= kmax, -2, "orthogonalize_mv: ldh smaller than the largest k");
  const size_t per = dev::kry_work_doubles();
  Scratch work((size_t)nb * per);
  dev::KryBatch B;
  dev::KryVecBatch sb{};
  B.nb = sb.nb = nb;
  for (int v = 0; v < nb; v++) {
    const dev::KryWork ws = B.ws[v] = dev::kry_work_at(work.p + (size_t)v * per);
    B.k[v] = k[v];
    B.V[v] = V + (int64_t)v * vstride;
    B.w[v] = B.dst[v] = W + (int64_t)v * ldw;
    sb.a[v] = B.w[v];
    sb.y[v] = vnext ? vnext + (int64_t)v * ldn : nullptr;
    sb.d[v] = ws.out + k[v];
  }
  std::vector<double> hk(dev::KRY_KMAX + 1);
  dev::kry_pass_a_mv(n, ldv, B, F32);
  dev::kry_pass_b_mv(n, ldv, B, F32);
  dev::kry_pass_c_mv(n, ldv, B, F32);
  if (F32 && vnext) dev::kry_round_scale_by_mv(n, sb);
  for (int v = 0; v < nb; v++) {
    dev::d2h(hk.data(), B.ws[v].out, (k[v] + 1) * sizeof(double));
    std::copy(hk.begin(), hk.begin() + k[v], hcoef + (int64_t)v * ldh);
    wnorm[v] = hk[k[v]];
  }
}
}  // namespace
#endif

extern "C" {

int hymls_mi_orthogonalize_mv(hymls_mi_t* h, int64_t n, int32_t nb, const int32_t* k, const double* V, int64_t ldv,
                              int64_t vstride, double* W, int64_t ldw, double* hcoef, int64_t ldh, double* wnorm) {
  if (!h) return -2;
  HandleView hv = handle_view(h);
  try {
#ifndef HYMLS_MI_LOCKSTEP_SOLVER
    (void)n; (void)nb; (void)k; (void)V; (void)ldv; (void)vstride; (void)W; (void)ldw; (void)hcoef; (void)ldh; (void)wnorm;
    throw hymls::Error(-99, "this build has no batched Krylov launchers (a test-only simulator without them)");
#else
    orthogonalize_mv<double>(hv, n, nb, k, V, ldv, vstride, W, ldw, nullptr, 0, hcoef, ldh, wnorm);
#endif
  } catch (const hymls::Error& e) { *hv.err = e.what(); return e.code; }
  catch (const std::exception& e) { *hv.err = e.what(); return -3; }
  return 0;
}

int hymls_mi_orthogonalize_mv_f32(hymls_mi_t* h, int64_t n, int32_t nb, const int32_t* k, const float* V, int64_t ldv,
                                  int64_t vstride, double* W, int64_t ldw, float* vnext, int64_t ldn, double* hcoef, int64_t ldh,
                                  double* wnorm) {
  if (!h) return -2;
  HandleView hv = handle_view(h);
  try {
#if !defined(HYMLS_MI_LOCKSTEP_SOLVER) || !defined(HYMLS_MI_F32_BASIS)
    (void)n; (void)nb; (void)k; (void)V; (void)ldv; (void)vstride; (void)W; (void)ldw; (void)vnext; (void)ldn; (void)hcoef; (void)ldh; (void)wnorm;
    throw hymls::Error(-99, "this build has no batched FP32 basis launchers (a test-only simulator without them)");
#else
    orthogonalize_mv<float>(hv, n, nb, k, V, ldv, vstride, W, ldw, vnext, ldn, hcoef, ldh, wnorm);
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
    free_projection(s);
    free_mass(s);
    dev::kry_timer_destroy(s->timer);
  } catch (...) {}
  delete s;
}

}  // extern "C"
