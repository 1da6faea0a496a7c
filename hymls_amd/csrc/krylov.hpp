// krylov.hpp -- device launchers of the native Krylov solver (krylov.cpp): the three-pass ICGS(2) orthogonalisation of
// GMRES, the basis update x += V y, and the fused vector passes of CG.  The product implements them in krylov_hip.hip;
// the test-only simulator under tests/krylov_sim implements the same functions with plain loops and the same block
// decomposition, so that both add the same partial sums in the same order.
//
// Reductions are two-stage and fixed-order: stage one writes one partial per workgroup (and per column), stage two
// sums the partials of each column on the device in a fixed tree.  No atomics: results are bitwise reproducible.
// Every launcher runs on dev::stream() of the bound context and does not synchronise.
#pragma once
#include "device.hpp"

namespace hymls {
namespace dev {

constexpr int KRY_KMAX = 256;      // columns of one orthogonalisation (= the largest GMRES restart length)
constexpr int KRY_TILE = 64;       // rows of one basis tile of passes A and B (staged in LDS)
constexpr int KRY_MAXGRID = 2048;  // workgroups of any stage-one pass (partials per column)

// workgroups of the tiled passes A and B: as many as fit on the chip at once (the LDS tile bounds them), each walks the
// tiles of its grid stride; rows of the row passes: 256 per workgroup, grid-stride as well
// (fixed numbers, not queried from the device, so that the partial sums -- and the bits of the result -- do not depend on
// the card: 256 CUs of an MI355X, 160 KiB of LDS each, at most 8 workgroups of 256 threads per CU)
constexpr int KRY_LD_TILE = KRY_TILE + 1;   // LDS column stride of a basis tile (odd: conflict-free row and column reads)
inline size_t kry_tile_lds(int32_t k) { return ((size_t)KRY_LD_TILE * k + KRY_TILE + KRY_KMAX + 4 * KRY_TILE) * sizeof(double); }
inline int kry_tile_grid(int64_t n, int32_t k) {
  const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(8, (int64_t)(160 * 1024) / (int64_t)kry_tile_lds(k)));
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + KRY_TILE - 1) / KRY_TILE, 256 * per_cu));
}
// FP32 basis ("MI Basis Storage" = single): the tile holds floats, the vectors and partial sums next to it stay FP64.
// Column stride 65 floats: a wave stages or reads 64 consecutive floats of one column (32 consecutive dwords per
// 32-lane half: 32 distinct banks), and in the dot loop lane t reads dword 65 t + r, bank (t + r) mod 32: the 32 lanes
// of a half hit 32 distinct banks.  Both access kinds are 4-byte LDS operations, banked modulo 32.
constexpr int KRY_LD_TILE_F32 = KRY_TILE + 1;
inline size_t kry_tile_lds_f32(int32_t k) {
  return (size_t)(KRY_TILE + KRY_KMAX + 4 * KRY_TILE) * sizeof(double) + (size_t)KRY_LD_TILE_F32 * k * sizeof(float);
}
inline int kry_tile_grid_f32(int64_t n, int32_t k) {
  const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(8, (int64_t)(160 * 1024) / (int64_t)kry_tile_lds_f32(k)));
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + KRY_TILE - 1) / KRY_TILE, 256 * per_cu));
}
inline int kry_row_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, KRY_MAXGRID)); }

// scratch of the reductions, device memory (krylov.cpp allocates it with kry_work_doubles() doubles)
struct KryWork {
  double* part;   // [KRY_MAXGRID * KRY_KMAX] stage-one partials
  double* h1;     // [KRY_KMAX] V^T w of pass A
  double* h2;     // [KRY_KMAX] V^T w of pass B
  double* out;    // [KRY_KMAX + 2]: h1 + h2, then ||w|| and ||w||^2 at out[k], out[k + 1]; dot results at out[0]
};
inline size_t kry_work_doubles() { return (size_t)KRY_MAXGRID * KRY_KMAX + 2 * KRY_KMAX + KRY_KMAX + 2; }
// the four areas of a KryWork in one allocation of kry_work_doubles() doubles at base
inline KryWork kry_work_at(double* base) {
  KryWork ws;
  ws.part = base;
  ws.h1 = ws.part + (size_t)KRY_MAXGRID * KRY_KMAX;
  ws.h2 = ws.h1 + KRY_KMAX;
  ws.out = ws.h2 + KRY_KMAX;
  return ws;
}

// pass A: h1 = V^T w over the k columns of V (k <= KRY_KMAX)
void kry_pass_a(int64_t n, int32_t k, const double* V, int64_t ldv, const double* w, const KryWork& ws);
// pass B: w <- w - V h1 (h1 from pass A), then h2 = V^T w of the new w, over the same row tile;  out[j] = h1[j] + h2[j]
void kry_pass_b(int64_t n, int32_t k, const double* V, int64_t ldv, double* w, const KryWork& ws);
// pass C: dst <- w - V h2, out[k + 1] = dst . dst (this rank's rows), out[k] = its square root (dst may be w itself)
void kry_pass_c(int64_t n, int32_t k, const double* V, int64_t ldv, const double* w, double* dst, const KryWork& ws);
// x <- x + V y (y: k device values), the pass-C kernel without the norm
void kry_update(int64_t n, int32_t k, const double* V, int64_t ldv, const double* y, double* x);
// x <- x / *d where *d > 0 (device scalar; the column written by pass C, divided by its norm)
void kry_scale_by(int64_t n, double* x, const double* d);
// y <- x / s
void kry_div(int64_t n, const double* x, double s, double* y);
// r <- b - y
void kry_sub(int64_t n, const double* b, const double* y, double* r);
// y <- y + x
void kry_add(int64_t n, const double* x, double* y);
// out[0] = x . y
void kry_dot(int64_t n, const double* x, const double* y, const KryWork& ws);
// CG: x <- x + alpha p, r <- r - alpha q, out[0] = r . r
void kry_cg_xr(int64_t n, double alpha, const double* p, const double* q, double* x, double* r, const KryWork& ws);
// CG: p <- z + beta p
void kry_cg_p(int64_t n, double beta, const double* z, double* p);

// ---- FP32 basis: the same passes over float columns.  w, h1, h2, every partial and every sum stay FP64; a basis entry
// is widened when it is read.  Implemented by krylov_hip.hip and by the test-only tests/krylov_f32_sim; krylov.cpp
// refers to them only under HYMLS_MI_F32_BASIS, because tests/krylov_sim has none.
void kry_pass_a(int64_t n, int32_t k, const float* V, int64_t ldv, const double* w, const KryWork& ws);
void kry_pass_b(int64_t n, int32_t k, const float* V, int64_t ldv, double* w, const KryWork& ws);
void kry_pass_c(int64_t n, int32_t k, const float* V, int64_t ldv, const double* w, double* dst, const KryWork& ws);
void kry_update(int64_t n, int32_t k, const float* V, int64_t ldv, const double* y, double* x);
// t <- (double) v: the FP64 copy of a basis column that ApplyInverse and K x read
void kry_widen(int64_t n, const float* v, double* t);
// y <- (float)(x / s): the first column of a cycle
void kry_round_div(int64_t n, const double* x, double s, float* y);
// y <- (float)(x / *d) where *d > 0, else (float) x (device scalar): the new column, normalised in FP64 and rounded once
void kry_round_scale_by(int64_t n, const double* x, const double* d, float* y);

// ---- bordered systems [K V; W' C] on the augmented vectors z = [x; s], y (n + m entries each, the border scalars in the
// tail [n, n + m) of the same device array; z and y must not overlap):
//   y[0:n) += V s            (after K x has been written to y[0:n)); per row the sum over j ascending, then one add
//   y[n + j] = W(:, j)' x + sum_l C[j + m l] s_l     (l ascending, added to the finished W' x)
// V, W: n x m column-major device arrays (leading dimensions ldv, ldw >= n), dC: device copy of C or nullptr (zero),
// 1 <= m <= KRY_BORDER_MAX.  The columns are handled KRY_BORDER_CHUNK at a time, one pass over the rows of kry_row_grid(n)
// workgroups per chunk (m <= 8: V, W, x and y are read once, (2 m + 3) n 8 bytes); the W' x partials of every workgroup go
// to ws.part[workgroup * m + j], and one workgroup sums them in the fixed order of the other reductions and writes the
// tail.  Implemented by krylov_hip.hip and by the test-only tests/krylov_border_sim; krylov.cpp refers to it only under
// HYMLS_MI_BORDERED_SOLVER, because the other simulators have none.
constexpr int KRY_BORDER_MAX = 32;
constexpr int KRY_BORDER_CHUNK = 8;
void kry_border_product(int64_t n, int32_t m, const double* V, int64_t ldv, const double* W, int64_t ldw, const double* dC,
                        const double* z, double* y, const KryWork& ws);

// ---- lock-step columns ("MI Lockstep Columns", hymls_mi_solver_set_lockstep): up to KRY_LOCKSTEP_MAX independent
// columns per launch, the column is blockIdx.y.  Every launcher below gives column v bit for bit what its single-column
// launcher above gives with the operands of column v: in krylov_hip.hip both kernels call one device function (kry_*_body),
// and the slice of column v strides by ITS OWN grid (kry_tile_grid(n, k[v]), kry_row_grid(n), vec_grid(n)) and writes that
// many partials, whatever the other columns of the launch need; the launch itself has the largest grid and the largest LDS
// size of the batch, and the workgroups of a column beyond its own grid leave before their first barrier.
// The operand table is a kernel argument (it lives in the kernarg segment, which the
// device reads): no copy per step, and k may change from step to step.  Implemented by krylov_hip.hip and by the
// test-only tests/krylov_lockstep_sim; krylov.cpp refers to them only under HYMLS_MI_LOCKSTEP_SOLVER.
constexpr int KRY_LOCKSTEP_MAX = 4;
struct KryBatch {                      // the columns of one batched orthogonalisation launch
  int32_t nb = 0;                      // columns, 1..KRY_LOCKSTEP_MAX
  int32_t k[KRY_LOCKSTEP_MAX];         // basis columns of column v, 1..KRY_KMAX
  const void* V[KRY_LOCKSTEP_MAX];     // its basis (double or float, as the launcher says), leading dimension ldv
  double* w[KRY_LOCKSTEP_MAX];         // the vector that is orthogonalised (passes A, B in place)
  double* dst[KRY_LOCKSTEP_MAX];       // pass C: dst <- w - V h2 (may be w)
  KryWork ws[KRY_LOCKSTEP_MAX];        // its reduction scratch, laid out as for the single-column launchers
};
void kry_pass_a_mv(int64_t n, int64_t ldv, const KryBatch& b, bool f32);
void kry_pass_b_mv(int64_t n, int64_t ldv, const KryBatch& b, bool f32);
void kry_pass_c_mv(int64_t n, int64_t ldv, const KryBatch& b, bool f32);
struct KryVecBatch {                   // the columns of one batched vector pass
  int32_t nb = 0;
  const void* a[KRY_LOCKSTEP_MAX];     // first input
  const double* b[KRY_LOCKSTEP_MAX];   // second input
  void* y[KRY_LOCKSTEP_MAX];           // output (updated in place where the single-column pass does so)
  double* r[KRY_LOCKSTEP_MAX];         // second output (kry_cg_xr_mv)
  const double* d[KRY_LOCKSTEP_MAX];   // device scalar
  double s[KRY_LOCKSTEP_MAX];          // host scalar
  double* part[KRY_LOCKSTEP_MAX];      // stage-one partials of a reduction
  double* out[KRY_LOCKSTEP_MAX];       // its result
};
void kry_scale_by_mv(int64_t n, const KryVecBatch& b);         // y <- y / *d where *d > 0                    (kry_scale_by)
void kry_round_scale_by_mv(int64_t n, const KryVecBatch& b);   // (float*) y <- (float)(a / *d), or (float) a (kry_round_scale_by)
void kry_widen_mv(int64_t n, const KryVecBatch& b);            // (double*) y <- (double)(const float*) a     (kry_widen)
void kry_dot_mv(int64_t n, const KryVecBatch& b);              // out[0] = a . b                              (kry_dot)
void kry_cg_xr_mv(int64_t n, const KryVecBatch& b);            // y += s a, r -= s b, out[0] = r . r          (kry_cg_xr: p = a, q = b, x = y)
void kry_cg_p_mv(int64_t n, const KryVecBatch& b);             // y <- a + s y                                (kry_cg_p: z = a, p = y)

// ---- projection vectors (hymls_mi_solver_set_projection): y = x - P (G (Q' x)), the one primitive behind the projected
// operator (I - BV V') K (I - V BV') and the projected preconditioner.  P, Q: n x m column-major device arrays (leading
// dimensions ldp, ldq >= n), 1 <= m <= KRY_PROJ_MAX, dG: device m x m column-major or nullptr (the identity); y may be x.
// Three kernels, no atomics, every sum in a fixed order that does not depend on the card:
//   dots    c_j = Q(:, j)' x: one row per thread, grid-stride over kry_row_grid(n) workgroups of 256, the columns in chunks
//           of KRY_PROJ_CHUNK (one launch per chunk, x is read once per chunk: (m + ceil(m / 8)) n 8 bytes), register
//           partials, the fixed tree of the workgroup into ws.part[workgroup * m + j]
//   tail    one workgroup: the partials of each column summed as the other reductions sum them, then
//           d_j = sum_l G[j + m l] c_l (l ascending; d = c without G), written to ws.h1[0..m)
//   update  y_i = x_i - sum_j P[i, j] d_j (j ascending, then one subtraction), one pass over the rows for every m:
//           (m + 2) n 8 bytes
// kry_proj_coeffs is dots + tail, kry_proj_update the update with the d that is in ws.h1 (the literal preconditioner takes
// the coefficients from one vector and updates another), kry_oblique_project both.  ws needs part[kry_row_grid(n) * m] and
// h1[m].  Implemented by krylov_hip.hip and by the test-only tests/krylov_proj_sim; krylov.cpp refers to them only under
// HYMLS_MI_PROJECTED_SOLVER, because the other simulators have none.
constexpr int KRY_PROJ_MAX = 32;
constexpr int KRY_PROJ_CHUNK = 8;
void kry_proj_coeffs(int64_t n, int32_t m, const double* Q, int64_t ldq, const double* dG, const double* x, const KryWork& ws);
void kry_proj_update(int64_t n, int32_t m, const double* P, int64_t ldp, const double* x, double* y, const KryWork& ws);
void kry_oblique_project(int64_t n, int32_t m, const double* Q, int64_t ldq, const double* dG, const double* P, int64_t ldp,
                         const double* x, double* y, const KryWork& ws);

// ---- shifted operator (hymls_mi_solver_set_shift, hymls_mi_solver_set_mass_matrix; the reference's HYMLS::ShiftedOperator):
//   Y(:, v) = a * A X(:, v) + b * B X(:, v),  v < nv;  B (rpB) == nullptr: the identity
// A, B: CSR with 32-bit indices and n rows on the device, X, Y column-major with leading dimensions ldx, ldy >= n; X and Y
// must not overlap.  One kernel reads both matrices and writes Y once.  L = spmv_lanes(n, nnzA_hint) consecutive lanes share
// a row and form two partial sums, sA over the row of A and sB over the row of B, each exactly as k_spmv<L> forms its sum
// (entries rp[row] + lane, step L, ascending, then the __shfl_down tree); lane 0 writes a * sA + b * sB.  Without B, sB is
// x[row]; with b == 0 B is not read and lane 0 writes a * sA; with a == 0 A is not read (its arrays may be null) and lane 0
// writes b * sB.  The columns go in groups of up to four (a lane loads each entry once and keeps the sums of every column of
// the group), and column v has the bits of the nv = 1 call on that column.  The grid is that of spmv() for n and L.  No
// atomics.  Implemented by krylov_hip.hip and by the test-only tests/krylov_shift_sim; krylov.cpp refers to it only under
// HYMLS_MI_SHIFTED_SOLVER, because the other simulators have none.
void kry_shifted_product(int32_t n, const int32_t* rpA, const int32_t* colA, const double* valA, int64_t nnzA_hint,
                         const int32_t* rpB, const int32_t* colB, const double* valB, double a, double b, const double* X,
                         int64_t ldx, double* Y, int64_t ldy, int nv);

// phase timing of a solve: events recorded on the stream (the simulator takes host clock readings)
struct KryTimer;
KryTimer* kry_timer_create();
void kry_timer_destroy(KryTimer* t);
void kry_mark(KryTimer* t, int phase, bool begin);     // phase < 4
void kry_collect(KryTimer* t, double* sum);            // synchronises; adds the seconds of every begin/end pair

}  // namespace dev
}  // namespace hymls
