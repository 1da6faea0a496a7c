/* hymls_mi_solver.h -- device-resident Krylov solver on top of a computed hymls_mi handle.
 *
 * The counterpart of the reference's HYMLS::BaseSolver (GMRES or CG through Belos with the HYMLS preconditioner
 * plugged in): K x = b is solved with K applied by hymls_mi_matvec and the preconditioner by ApplyInverse of the same
 * handle.  Every Krylov vector stays in device memory; the Gram-Schmidt orthogonalisation of GMRES runs in HIP kernels
 * and the host sees a handful of scalars per iteration.  The iteration is the one of hymls_amd.Solver (Python):
 * restarted GMRES(m) with classical Gram-Schmidt applied twice and Givens rotations on the host, or preconditioned CG;
 * convergence is relative to the first residual of the solve.
 *
 * Sharded handles (hymls_mi_set_comm / hymls_mi_set_comm_rccl): every rank calls the solver collectively with its
 * owned rows (hymls_mi_owned_rows order); inner products are summed over the ranks in rank order.
 *
 * Kept apart from hymls_mi.h (as the reference keeps HYMLS_BaseSolver.hpp apart from HYMLS_Preconditioner.hpp).
 */
#ifndef HYMLS_MI_SOLVER_H
#define HYMLS_MI_SOLVER_H
#include <stdint.h>
#include "hymls_mi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hymls_mi_solver hymls_mi_solver_t;

typedef struct hymls_mi_solver_params {
  int32_t method;          /* "Krylov Method": 0 GMRES, 1 CG                                   (GMRES) */
  int32_t initial_vector;  /* "Initial Vector": 0 Zero, 1 Random, 2 Previous                   (Zero)  */
  int32_t right;           /* "Left or Right Preconditioning": 1 Right, 0 Left                 (Right) */
  double tol;              /* "Convergence Tolerance", relative to the first residual          (1e-8)  */
  int32_t max_iters;       /* "Maximum Iterations"                                             (500)   */
  int32_t num_blocks;      /* "Num Blocks": GMRES restart length, 1..HYMLS_MI_SOLVER_MAX_BLOCKS (250)  */
  int32_t max_restarts;    /* "Maximum Restarts"                                               (20)    */
  uint64_t seed;           /* "Random": start vector = hash(seed, global row id) in [-1, 1)    (1234)  */
} hymls_mi_solver_params;

#define HYMLS_MI_SOLVER_MAX_BLOCKS 256

void hymls_mi_solver_default_params(hymls_mi_solver_params* p);

/* h: a handle that has been (or will be, before the first solve) computed; K = the matrix of h, M^{-1} = its ApplyInverse.
 * The solver keeps a pointer to h: destroy the solver first. */
int hymls_mi_solver_create(hymls_mi_solver_t** s, hymls_mi_t* h, const hymls_mi_solver_params* p);
/* replaces every parameter (the reference's setParameterList); the "Previous" solution is kept */
int hymls_mi_solver_set_params(hymls_mi_solver_t* s, const hymls_mi_solver_params* p);
int hymls_mi_solver_set_tolerance(hymls_mi_solver_t* s, double tol);

/* Solves K X(:, v) = B(:, v) for v = 0..nvec-1, one column after the other (block size 1), or in lock-step groups
 * (hymls_mi_solver_set_lockstep below).  B, X: column-major with
 * leading dimensions ldb, ldx (>= this rank's row count); device pointers if on_device, else host memory.
 * "Previous" starts each column from the solution of the column (or call) solved before it.
 * Returns 0 when every column converged, -1 when one did not (X then holds the last iterate), < -1 on errors.
 * num_iters / achieved_tol describe the last column. */
int hymls_mi_solver_solve(hymls_mi_solver_t* s, const double* B, int64_t ldb, double* X, int64_t ldx, int nvec, int on_device);
int hymls_mi_solver_num_iters(const hymls_mi_solver_t* s);
double hymls_mi_solver_achieved_tol(const hymls_mi_solver_t* s);
/* Arnoldi cycles of the last column after its first one (GMRES; 0 for CG).  With FP32 basis storage a cycle that was
 * ended early (below) counts as a restart like one that filled the basis, and "Maximum Restarts" bounds both kinds. */
int hymls_mi_solver_num_restarts(const hymls_mi_solver_t* s);

#define HYMLS_MI_SOLVER_MAX_BORDER 32
/* [K V; W' C] [x; s] = [b; t] with the border of the handle (hymls_mi_set_border + Compute) as the border of
 * the operator AND of the preconditioner (reference HYMLS::BorderedSolver::SetBorder).  One right-hand side.
 * B, X: n entries, device or host as on_device says.  T, S: host arrays of m doubles (T NULL: zero; S NULL: dropped).
 * The Krylov vectors are the augmented vectors [x; s] of n + m entries, kept on the device: inner products run over both
 * parts, and convergence is relative to the first residual of the augmented vector.  Left and right preconditioning,
 * restarts, the three initial vectors ("Random": border scalar j = hash(seed, global size + j); "Previous" survives while
 * n + m is unchanged; a "Previous" vector whose true residual is already within tol of the norm of [b; t], as after a
 * repeated solve of the same system, is returned at once with 0 iterations), both basis storages, num_iters / achieved_tol / num_restarts and the phase timing work as for
 * hymls_mi_solver_solve; the border product counts as K x (phase 2).
 * Returns 0, or -1 when the tolerance was not reached (X and S then hold the last iterate).  A handle without a border:
 * the plain solve of one column, S untouched.  -2: more than HYMLS_MI_SOLVER_MAX_BORDER border columns.  -99: method CG
 * (the bordered operator [K V; W' C] is indefinite, so CG does not apply: use GMRES), a sharded handle (one GPU only), or a
 * library built without the border product kernel.  hymls_mi_solver_solve keeps refusing bordered handles with -2. */
int hymls_mi_solver_solve_bordered(hymls_mi_solver_t* s, const double* B, const double* T, double* X, double* S, int on_device);
/* building block (as hymls_mi_orthogonalize): y[0:n) += V z[n:n+m),  y[n+j] = W(:,j)' z[0:n) + sum_l C[j + m l] z[n+l].
 * V, W, z, y device; C host, m x m column-major, may be NULL (zero).  n >= 1, 1 <= m <= HYMLS_MI_SOLVER_MAX_BORDER,
 * ldv, ldw >= n, z and y distinct arrays of n + m entries; otherwise -2.  Sums in a fixed order without atomics: the
 * result is bitwise repeatable.  -99 from a library built without the kernel. */
int hymls_mi_border_product(hymls_mi_t* h, int64_t n, int32_t m, const double* V, int64_t ldv, const double* W, int64_t ldw,
                            const double* C, const double* z, double* y);

/* Storage of the GMRES basis: 64 (default) keeps FP64 columns, 32 stores them as float (compressed-basis GMRES) and
 * halves the memory and the traffic of the orthogonalisation.  Every other vector, every inner product and the
 * Hessenberg matrix stay FP64: a new column is w / ||w|| formed in FP64 and rounded once.  Takes effect with the next
 * solve, which reallocates the basis.  CG ignores it.  Other values return -2; a library built without the FP32 basis
 * kernels returns -99 for 32.
 * With 32 bits the recurrence (Givens) estimate of the residual only ends a cycle: at the tolerance, or as soon as it
 * has fallen to 1e-5 of the residual the cycle started from (a float basis cannot carry a cycle much further).  The
 * solve ends only on the explicitly computed residual b - K x at the top of the next cycle, and achieved_tol and the
 * return status come from that residual, also when the iterations or the restarts run out. */
int hymls_mi_solver_set_basis_storage(hymls_mi_solver_t* s, int bits);
int hymls_mi_solver_basis_storage(const hymls_mi_solver_t* s);

/* Lock-step columns: hymls_mi_solver_solve with width L > 1 takes the nvec columns in groups of L consecutive columns (the
 * last group may be smaller), and the columns of a group advance together, one Krylov iteration per step.  Each column does
 * exactly the arithmetic of its own single-column solve; per step the group shares one ApplyInverse and one K x on its
 * columns side by side (the factors and K are read once for the group), one launch chain of the orthogonalisation whose
 * per-column slices repeat the single-column decomposition, and one copy of the coefficients to the host.  A column that
 * converges, has a zero first residual, or runs out of iterations or restarts leaves the group, and the others go on with
 * a smaller batch; with the FP32 basis the columns may sit at different positions of their cycles.  For the initial
 * vectors "Zero" and "Random", X, the per-column results and the return status are bitwise those of width 1 (the
 * default).  The one difference: with "Previous" every column of a group starts from the solution stored before the
 * group (the last column of the preceding group or call), and the group's last column is stored afterwards.
 * GMRES and CG.  Every column beyond the first has its own basis, seven work vectors and reduction scratch, allocated by
 * the first solve that needs them; a failed allocation returns -3 with the bytes asked for in the message, frees what the
 * attempt took and leaves the solver usable at width 1.  width outside 1..HYMLS_MI_SOLVER_MAX_LOCKSTEP: -2.  One GPU: a
 * solve with width > 1 on a sharded handle returns -99.  hymls_mi_solver_solve_bordered ignores the width.  A library
 * built without the batched launchers (a test-only simulator) returns -99 for width > 1. */
#define HYMLS_MI_SOLVER_MAX_LOCKSTEP 4
int hymls_mi_solver_set_lockstep(hymls_mi_solver_t* s, int width);
int hymls_mi_solver_lockstep(const hymls_mi_solver_t* s);
/* results of column v of the last hymls_mi_solver_solve call (every width; a bordered solve has one column): 0, or -2 for
 * v out of range.  Any of the four pointers may be null.  num_iters / achieved_tol / num_restarts keep describing the
 * last column. */
int hymls_mi_solver_column_result(const hymls_mi_solver_t* s, int v, int* iters, double* achieved_tol, int* restarts,
                                  int* converged);

/* Projection vectors (the reference's HYMLS::BaseSolver::setProjectionVectors with HYMLS::ProjectedOperator): with V and
 * BV set (n x m, V' BV = I), hymls_mi_solver_solve works in the complement of the space they span, as the correction
 * equation of Jacobi-Davidson and the deflated solvers need it:
 *   operator         y = (I - BV V') K (I - V BV') x
 *   preconditioner   y = M^{-1} (I - BV H^{-1} BV' M^{-1}) x,  H = BV' M^{-1} BV
 *   start vector     x0 <- x0 - BV (V' x0), after "Zero", "Random" or "Previous" has produced x0
 * The right-hand side is used as given (the reference hands it to Belos unprojected): pass one with V' b = 0.  GMRES and CG,
 * both basis storages, left and right preconditioning, restarts, achieved_tol and the per-column results work as without a
 * projection (CG: with BV = V and symmetric K and M the projected pair is symmetric).  Each projector is one pass for the m
 * inner products and one for the update, in HIP kernels that sum in a fixed order without atomics.
 * V, BV: column-major, leading dimensions ldv, ldbv >= n, device pointers if on_device, else host memory; the solver keeps
 * device copies of its own (one if BV is NULL, which means BV = V).  m = 0 or V NULL removes the projection, and the solver
 * then takes the path and gives the bits of one that never had it.  -2: m above HYMLS_MI_SOLVER_MAX_PROJECTION, n different
 * from the handle's row count, a leading dimension below n, or ||V' BV - I||_inf > 1e-8 (the reference's CheckOrthogonal;
 * the message holds the norm).  Memory: (2 or 3) m + 1 vectors of n doubles (V, BV, Z below, one work vector), allocated by
 * this call; a failed allocation returns -3 with the bytes asked for in the message and leaves the solver without a
 * projection.
 * The first solve after this call forms Z = M^{-1} BV (ApplyInverse in groups of up to four columns), H = BV' Z and, from an
 * LU factorisation of H with partial pivoting on the host, the dense H^{-1}; a solve after the handle was computed again
 * (hymls_mi_num_compute has changed) forms them again.  A singular H (zero pivot): -4.  A solve on a sharded handle with a
 * projection set returns -99 (one GPU), and so does hymls_mi_solver_solve_bordered.  With a projection set the columns of a
 * solve go one after the other, whatever the lock-step width.  Phase timing: the projectors around K x count as K x
 * (phase 2), those of the preconditioner and forming Z and H as ApplyInverse (phase 1).
 * A library built without the projection kernels (a test-only simulator) returns -99 from all five entries below. */
#define HYMLS_MI_SOLVER_MAX_PROJECTION 32
int hymls_mi_solver_set_projection(hymls_mi_solver_t* s, int64_t n, int32_t m, const double* V, int64_t ldv, const double* BV,
                                   int64_t ldbv, int on_device);
int hymls_mi_solver_num_projection(const hymls_mi_solver_t* s);
/* form of the projected preconditioner: 0 (default) folded, y = M^{-1} x followed by y -= Z (H^{-1} (BV' y)): one ApplyInverse
 * per application; 1 literal, the reference's arithmetic: y = M^{-1} x, d = H^{-1} (BV' y), y = M^{-1} (x - BV d): two.  Both
 * are the same operator in exact arithmetic (M^{-1} (x - BV d) = M^{-1} x - Z d).  Other values: -2. */
int hymls_mi_solver_set_projection_form(hymls_mi_solver_t* s, int form);
/* one vector through the projected operator (which = 0) or the projected preconditioner (which = 1) exactly as the solve
 * applies them (building block, for tests).  X, Y: n entries, device or host as on_device says; Y may be X.  Forms Z and H
 * if the next solve would.  -2 when no projection is set, -1 before Compute.  With a shift set (below), which = 0 applies the
 * shifted projected operator, as the solve does. */
int hymls_mi_solver_apply_projected(hymls_mi_solver_t* s, int which, const double* X, double* Y, int on_device);
/* building block (as hymls_mi_border_product): y = x - P (G (Q' x)).  P, Q: n x m column-major device arrays, x, y device
 * (y may be x); G host, m x m column-major, may be NULL (the identity).  n >= 1, 1 <= m <= HYMLS_MI_SOLVER_MAX_PROJECTION,
 * ldq, ldp >= n; otherwise -2.  Sums in a fixed order without atomics: the result is bitwise repeatable. */
int hymls_mi_oblique_project(hymls_mi_t* h, int64_t n, int32_t m, const double* Q, int64_t ldq, const double* G,
                             const double* P, int64_t ldp, const double* x, double* y);

/* Mass matrix and shifted operator (the reference's HYMLS::BaseSolver::SetMassMatrix / ApplyMass / setShift with
 * HYMLS::ShiftedOperator): with a shift (a, b) other than the default (1, 0), hymls_mi_solver_solve and
 * hymls_mi_solver_solve_bordered solve with
 *   operator         y = a K x + b B x,   B the mass matrix, or the identity when none is set
 * in the place of K x: in the plain operator, inside the projected one, (I - BV V') (a K + b B) (I - V BV'), on the rows of K
 * of the bordered one, in every explicit residual, in CG and in the product of a lock-step group (K and B are read once per
 * group of up to four columns).  This is the system of the Jacobi-Davidson correction equation (setShift(1, -sigma), then
 * set_projection) and of time steppers, (K + sigma B) x = b.  The preconditioner stays ApplyInverse of the handle, the
 * preconditioner of K alone, and so do Z and H of a projection; convergence stays relative to the first residual, and basis
 * storage, left and right preconditioning, restarts, start vectors and per-column results work as without a shift.  The
 * product is one HIP kernel that reads both matrices and writes y once, without atomics (bitwise repeatable), and counts as
 * K x (phase 2) in the phase timing; its row sums of K use the lanes of hymls_mi_matvec.
 * B and the shift are state like the projection vectors: hymls_mi_solver_set_params does not touch them.  With (1, 0) the
 * solver takes the path and gives the bits of one that never had a shift, whether or not a mass matrix is set.  One GPU: a
 * solve with another shift on a sharded handle returns -99; the plain sharded solve is untouched.
 *
 * hymls_mi_solver_set_mass_matrix: B in CSR with n rows and columns, 32-bit rowptr (n + 1 entries) and colind, double values;
 * device pointers if on_device, else host memory; the solver keeps a device copy of its own, 4 (n + 1) + 12 nnz bytes.  The
 * entries of a row are summed in storage order, and duplicates add up.  rowptr NULL removes B (the identity is used).  The
 * entry validates on the host before any kernel reads an index (device input: rowptr and colind are copied back once): -2
 * with a message when n differs from the handle's row count, rowptr[0] != 0, a rowptr entry decreases (which is also how
 * nnz >= 2^31 shows in 32-bit row pointers), a column lies outside [0, n), or colind or values is NULL with nnz > 0.  A
 * failed allocation returns -3 with the bytes asked for in the message.  After any failure the solver has no mass matrix.
 * hymls_mi_solver_apply_mass: Y(:, v) = B X(:, v), v < nvec (column-major, ldx, ldy >= n); Y = X without a mass matrix.
 * nvec = 0: nothing; -2: nvec < 0, a leading dimension below n, null arrays, or device X and Y that overlap.
 * hymls_mi_solver_set_shift: -2 for non-finite values or a = b = 0.  hymls_mi_solver_shift: the pair (either pointer may be
 * null).
 * A library built without the shifted product kernel (a test-only simulator) returns -99 from all five entries below. */
int hymls_mi_solver_set_mass_matrix(hymls_mi_solver_t* s, int64_t n, const int32_t* rowptr, const int32_t* colind,
                                    const double* values, int on_device);
int hymls_mi_solver_apply_mass(hymls_mi_solver_t* s, const double* X, int64_t ldx, double* Y, int64_t ldy, int nvec, int on_device);
int hymls_mi_solver_set_shift(hymls_mi_solver_t* s, double shift_a, double shift_b);
int hymls_mi_solver_shift(const hymls_mi_solver_t* s, double* shift_a, double* shift_b);
/* building block (as hymls_mi_border_product), device pointers: Y(:, v) = a A X(:, v) + b B X(:, v), v < nvec, A and B CSR with
 * n rows, 32-bit indices and double values; rpB NULL: B is the identity.  The caller vouches for the indices of A and B.
 * Lanes per row from nnzA_hint / n (-1: 4 lanes, those of hymls_mi_matvec); b = 0: B is not read; a = 0: A is not read and
 * its arrays may be NULL.  Column v has the bits of the nvec = 1 call on it.  nvec = 0: nothing.  -2: n < 1 or n >= 2^31,
 * nvec < 0, a leading dimension below n, NULL X or Y, NULL arrays of A with a != 0, NULL colB or valB with rpB set, X and Y
 * overlapping. */
int hymls_mi_shifted_product(hymls_mi_t* h, int64_t n, double a, const int32_t* rpA, const int32_t* colA, const double* valA,
                             int64_t nnzA_hint, double b, const int32_t* rpB, const int32_t* colB, const double* valB,
                             const double* X, int64_t ldx, double* Y, int64_t ldy, int nvec);

/* phase timing with events on the stream (adds a synchronisation at the end of every solve while on).
 * which: 0 whole solve, 1 ApplyInverse, 2 K x, 3 orthogonalisation + updates; seconds summed since profiling was
 * switched on. */
int hymls_mi_solver_set_profiling(hymls_mi_solver_t* s, int on);
double hymls_mi_solver_seconds(const hymls_mi_solver_t* s, int which);

/* One ICGS(2) step on device arrays, the building block of the GMRES iteration (for tests and for callers with an
 * Arnoldi process of their own):  w <- (I - V V^T)^2 w over the k columns of V (n rows, leading dimension ldv >= n,
 * 1 <= k <= HYMLS_MI_SOLVER_MAX_BLOCKS).  V and w are device memory; hcoef[k] (= h1 + h2) and *wnorm (= ||w|| after
 * both passes) are host memory.  On a sharded handle n is this rank's row count and the products are summed over the
 * ranks (collective). */
int hymls_mi_orthogonalize(hymls_mi_t* h, int64_t n, int32_t k, const double* V, int64_t ldv, double* w, double* hcoef,
                           double* wnorm);

/* The same step against a basis stored as float (V: device memory, n rows, leading dimension ldv floats).  w is
 * orthogonalised in place in FP64: every product and sum is FP64 on the widened entries.  vnext (device memory, n
 * floats) may be null; otherwise it receives (float)(w / ||w||), the column an FP32-basis GMRES stores next.
 * Returns -99 from a library built without the FP32 basis kernels. */
int hymls_mi_orthogonalize_f32(hymls_mi_t* h, int64_t n, int32_t k, const float* V, int64_t ldv, double* w, float* vnext,
                               double* hcoef, double* wnorm);

/* Building blocks of the lock-step solve.  One GPU: sharded handles return -99 from all three, and so does a library built
 * without the batched launchers.
 * Y(:, v) = K X(:, v), v < nvec (column-major, ldx, ldy >= the row count; device pointers if on_device): K is read once per
 * group of up to four columns, and every column is bitwise equal to hymls_mi_matvec. */
int hymls_mi_matvec_mv(hymls_mi_t* h, const double* X, int64_t ldx, double* Y, int64_t ldy, int nvec, int on_device);
/* nb independent ICGS(2) steps in one launch chain: column v orthogonalises W(:, v) (device, ldw >= n) in place against the
 * k[v] columns of its own basis V + v * vstride (device, leading dimension ldv >= n); hcoef (host) receives k[v] values
 * h1 + h2 at hcoef + v * ldh (ldh >= the largest k), wnorm[v] (host) the norm.  Each column is bitwise equal to
 * hymls_mi_orthogonalize with k[v].  1 <= nb <= HYMLS_MI_SOLVER_MAX_LOCKSTEP, 1 <= k[v] <= HYMLS_MI_SOLVER_MAX_BLOCKS (k: host);
 * otherwise -2. */
int hymls_mi_orthogonalize_mv(hymls_mi_t* h, int64_t n, int32_t nb, const int32_t* k, const double* V, int64_t ldv,
                              int64_t vstride, double* W, int64_t ldw, double* hcoef, int64_t ldh, double* wnorm);
/* the same against float bases (vstride in floats); vnext (device, may be null) receives (float)(W(:, v) / ||W(:, v)||) at
 * vnext + v * ldn (ldn >= n floats), as in hymls_mi_orthogonalize_f32 */
int hymls_mi_orthogonalize_mv_f32(hymls_mi_t* h, int64_t n, int32_t nb, const int32_t* k, const float* V, int64_t ldv,
                                  int64_t vstride, double* W, int64_t ldw, float* vnext, int64_t ldn, double* hcoef,
                                  int64_t ldh, double* wnorm);

const char* hymls_mi_solver_last_error(const hymls_mi_solver_t* s);
void hymls_mi_solver_destroy(hymls_mi_solver_t* s);

#ifdef __cplusplus
}
#endif
#endif /* HYMLS_MI_SOLVER_H */
