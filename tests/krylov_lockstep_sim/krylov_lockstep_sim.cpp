// krylov_lockstep_sim.cpp -- TEST-ONLY host versions of the batched (lock-step) launchers of hymls_amd/csrc/krylov.hpp and
// of dev::spmv_mv (hymls_amd/csrc/device.hpp); the product implements them in krylov_hip.hip and device_hip.hip.  A batched
// kernel gives column v the slice its single-column kernel would have computed: the column's own grid as the stride and the
// partial count, the same trees.  On the host that decomposition is the single-column launcher of tests/krylov_sim and
// tests/krylov_f32_sim itself, called with the operands of column v, so every batched launcher here is a plain loop over
// the columns.  What this simulator pins is therefore the host side of the lock-step solve (the per-column state machine,
// the staging, the drop-outs); the batched kernels themselves are pinned on the GPU only.  Every other launcher and the
// timer come from tests/krylov_sim, tests/krylov_f32_sim and tests/krylov_border_sim, compiled unchanged into the same
// library.
#include "krylov.hpp"

namespace hymls {
namespace dev {

namespace {
void check_batch(int nb) { if (nb < 1 || nb > KRY_LOCKSTEP_MAX) throw Error(-2, "batched launch: 1 <= columns <= 4"); }
// as check_batch of krylov_hip.hip: every k is checked before the first column runs, so a refused launch writes nothing
void check_batch(const KryBatch& b) {
  check_batch(b.nb);
  for (int c = 0; c < b.nb; c++)
    if (b.k[c] < 1 || b.k[c] > KRY_KMAX) throw Error(-2, "orthogonalisation: 1 <= k <= 256 columns");
}
}  // namespace

void kry_pass_a_mv(int64_t n, int64_t ldv, const KryBatch& b, bool f32) {
  check_batch(b);
  for (int c = 0; c < b.nb; c++) {
    if (f32) kry_pass_a(n, b.k[c], (const float*)b.V[c], ldv, b.w[c], b.ws[c]);
    else kry_pass_a(n, b.k[c], (const double*)b.V[c], ldv, b.w[c], b.ws[c]);
  }
}
void kry_pass_b_mv(int64_t n, int64_t ldv, const KryBatch& b, bool f32) {
  check_batch(b);
  for (int c = 0; c < b.nb; c++) {
    if (f32) kry_pass_b(n, b.k[c], (const float*)b.V[c], ldv, b.w[c], b.ws[c]);
    else kry_pass_b(n, b.k[c], (const double*)b.V[c], ldv, b.w[c], b.ws[c]);
  }
}
void kry_pass_c_mv(int64_t n, int64_t ldv, const KryBatch& b, bool f32) {
  check_batch(b);
  for (int c = 0; c < b.nb; c++) {
    if (f32) kry_pass_c(n, b.k[c], (const float*)b.V[c], ldv, b.w[c], b.dst[c], b.ws[c]);
    else kry_pass_c(n, b.k[c], (const double*)b.V[c], ldv, b.w[c], b.dst[c], b.ws[c]);
  }
}
void kry_scale_by_mv(int64_t n, const KryVecBatch& b) {
  check_batch(b.nb);
  for (int c = 0; c < b.nb; c++) kry_scale_by(n, (double*)b.y[c], b.d[c]);
}
void kry_round_scale_by_mv(int64_t n, const KryVecBatch& b) {
  check_batch(b.nb);
  for (int c = 0; c < b.nb; c++) kry_round_scale_by(n, (const double*)b.a[c], b.d[c], (float*)b.y[c]);
}
void kry_widen_mv(int64_t n, const KryVecBatch& b) {
  check_batch(b.nb);
  for (int c = 0; c < b.nb; c++) kry_widen(n, (const float*)b.a[c], (double*)b.y[c]);
}
void kry_dot_mv(int64_t n, const KryVecBatch& b) {
  check_batch(b.nb);
  for (int c = 0; c < b.nb; c++) {
    KryWork ws{};
    ws.part = b.part[c]; ws.out = b.out[c];
    kry_dot(n, (const double*)b.a[c], b.b[c], ws);
  }
}
void kry_cg_xr_mv(int64_t n, const KryVecBatch& b) {
  check_batch(b.nb);
  for (int c = 0; c < b.nb; c++) {
    KryWork ws{};
    ws.part = b.part[c]; ws.out = b.out[c];
    kry_cg_xr(n, b.s[c], (const double*)b.a[c], b.b[c], (double*)b.y[c], b.r[c], ws);
  }
}
void kry_cg_p_mv(int64_t n, const KryVecBatch& b) {
  check_batch(b.nb);
  for (int c = 0; c < b.nb; c++) kry_cg_p(n, b.s[c], (const double*)b.a[c], (double*)b.y[c]);
}

// the simulator's spmv() (tests/hostsim/device_sim.cpp) sums a row in index order; so does every column here
void spmv_mv(int32_t nrows, const int32_t* rp, const int32_t* col, const double* val, const double* x, int64_t ldx, double* y,
             int64_t ldy, int nv, double alpha, double beta, int64_t nnz_hint) {
  for (int v = 0; v < nv; v++) spmv(nrows, rp, col, val, x + (int64_t)v * ldx, y + (int64_t)v * ldy, alpha, beta, nnz_hint);
}

}  // namespace dev
}  // namespace hymls
