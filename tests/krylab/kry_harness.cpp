// kry_harness.cpp -- TEST-ONLY driver of the launchers of the native Krylov solver (krylov.hpp: the vector, reduction and update
// passes, the orthogonalisation passes A, B and C, the projection and the border product, and their batched forms) and of
// the multi-vector SpMV (device.hpp: spmv_mv), plain C++ without device code.
//
// One extern "C" function per launcher: bind a context (kstream() is the bound context's stream), upload the arguments,
// call exactly ONE launcher, dev::sync(), download, free.  The same source is linked twice (Makefile): against the
// test-only simulators (tests/hostsim + tests/krylov_*_sim), where a batched launcher is a loop over the single one, and
// against the product library.  So a harness bug shows up on a machine without a GPU first.
//
// Canaries (the scheme of tests/seplab): every output buffer -- the reduction scratch KryWork::part and KryWork::out
// included -- is allocated with a guard tail behind it and filled, tail included, with a signalling-NaN bit pattern before
// the caller's initial content (if any) is copied to its front.  The whole buffer comes back, so the caller checks bit for
// bit that nothing outside the defined output set was written.  Input arrays are uploaded with exactly the length the
// operation may read (no slack): a read past the end is not absorbed by padding of the harness.
//
// Batched entries: every operand kind is ONE flat array, and column c starts at an element offset the caller chooses
// (off[kind * 4 + c]), so that a float column may start at a 4-byte but not 8-byte aligned address and a double column at an
// 8-byte but not 16-byte aligned one.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <vector>
#include "krylov.hpp"
#include "device.hpp"

using namespace hymls;

namespace {

constexpr uint64_t CANARY = 0x7ff4dead5eed5eedULL;   // a signalling NaN no arithmetic produces
constexpr int64_t GUARD_WORDS = 1024;                 // 8 KiB behind every output

dev::Context* g_ctx = nullptr;
void bind() {
  if (!g_ctx) g_ctx = dev::create_context(0);
  dev::bind(g_ctx);
}

// exactly n elements (one element when n = 0, never read)
template <class T>
T* up(const T* h, int64_t n) {
  T* p = (T*)dev::alloc((size_t)std::max<int64_t>(n, 1) * sizeof(T));
  if (n > 0) dev::h2d(p, h, (size_t)n * sizeof(T));
  return p;
}

// an output buffer of `words` 8-byte words (guard tail included) whose first init_bytes come from the host array
struct Out {
  void* d = nullptr; void* h = nullptr; int64_t words = 0;
  Out(void* host, int64_t init_bytes, int64_t words_) : h(host), words(words_) {
    if (words < GUARD_WORDS || init_bytes > (words - GUARD_WORDS) * 8) throw Error(-2, "krylab: output buffer without its guard tail");
    std::vector<uint64_t> fill((size_t)words, CANARY);
    if (init_bytes > 0) std::memcpy(fill.data(), host, (size_t)init_bytes);
    d = dev::alloc((size_t)words * 8);
    dev::h2d(d, fill.data(), (size_t)words * 8);
  }
  template <class T> T* as() { return (T*)d; }
  void back() { dev::d2h(h, d, (size_t)words * 8); }
  ~Out() { dev::free(d); }
  Out(const Out&) = delete;
  Out& operator=(const Out&) = delete;
};

struct Freer {
  std::vector<void*> p;
  template <class T> T* operator()(T* q) { p.push_back((void*)q); return q; }
  ~Freer() { for (void* q : p) dev::free(q); }
};

int fail(const std::exception& e, char* err, int32_t errlen) {
  if (err && errlen > 0) { std::strncpy(err, e.what(), (size_t)errlen - 1); err[errlen - 1] = 0; }
  const Error* he = dynamic_cast<const Error*>(&e);
  return he && he->code != 0 ? he->code : -1;
}

dev::KryWork work(Out& part, Out& out) {
  dev::KryWork ws{};
  ws.part = part.as<double>();
  ws.out = out.as<double>();
  return ws;
}

// entries of a basis of k columns with leading dimension ld that x += V y may read
int64_t basis_len(int64_t n, int32_t k, int64_t ld) { return k > 0 ? (int64_t)(k - 1) * ld + n : 0; }

}  // namespace

#define KRYLAB_TRY try { bind();
#define KRYLAB_END return 0; } catch (const std::exception& e) { return fail(e, err, errlen); }

extern "C" {

int64_t krylab_guard_words() { return GUARD_WORDS; }
uint64_t krylab_canary() { return CANARY; }

// ---- the product's own grid functions and limits (read by the coverage bookkeeping)
int32_t krylab_row_grid(int64_t n) { return dev::kry_row_grid(n); }
int32_t krylab_spmv_lanes(int32_t nrows, int64_t nnz_hint) { return dev::spmv_lanes(nrows, nnz_hint); }
int32_t krylab_maxgrid() { return dev::KRY_MAXGRID; }
int32_t krylab_kmax() { return dev::KRY_KMAX; }
int32_t krylab_lockstep_max() { return dev::KRY_LOCKSTEP_MAX; }

// ---- single-vector launchers
int krylab_sub(int64_t n, const double* b, const double* y, double* r, int64_t r_words, char* err, int32_t errlen) {
  KRYLAB_TRY
  Freer f;
  const double* d_b = f(up(b, n)); const double* d_y = f(up(y, n));
  Out o(r, 0, r_words);
  dev::kry_sub(n, d_b, d_y, o.as<double>());
  dev::sync(); o.back();
  KRYLAB_END
}
int krylab_add(int64_t n, const double* x, double* y, int64_t y_words, char* err, int32_t errlen) {
  KRYLAB_TRY
  Freer f;
  const double* d_x = f(up(x, n));
  Out o(y, n * 8, y_words);
  dev::kry_add(n, d_x, o.as<double>());
  dev::sync(); o.back();
  KRYLAB_END
}
int krylab_div(int64_t n, const double* x, double s, double* y, int64_t y_words, char* err, int32_t errlen) {
  KRYLAB_TRY
  Freer f;
  const double* d_x = f(up(x, n));
  Out o(y, 0, y_words);
  dev::kry_div(n, d_x, s, o.as<double>());
  dev::sync(); o.back();
  KRYLAB_END
}
int krylab_scale_by(int64_t n, double* x, int64_t x_words, const double* d, char* err, int32_t errlen) {
  KRYLAB_TRY
  Freer f;
  const double* d_d = f(up(d, 1));
  Out o(x, n * 8, x_words);
  dev::kry_scale_by(n, o.as<double>(), d_d);
  dev::sync(); o.back();
  KRYLAB_END
}
int krylab_widen(int64_t n, const float* v, double* t, int64_t t_words, char* err, int32_t errlen) {
  KRYLAB_TRY
  Freer f;
  const float* d_v = f(up(v, n));
  Out o(t, 0, t_words);
  dev::kry_widen(n, d_v, o.as<double>());
  dev::sync(); o.back();
  KRYLAB_END
}
int krylab_round_div(int64_t n, const double* x, double s, float* y, int64_t y_words, char* err, int32_t errlen) {
  KRYLAB_TRY
  Freer f;
  const double* d_x = f(up(x, n));
  Out o(y, 0, y_words);
  dev::kry_round_div(n, d_x, s, o.as<float>());
  dev::sync(); o.back();
  KRYLAB_END
}
int krylab_round_scale_by(int64_t n, const double* x, const double* d, float* y, int64_t y_words, char* err, int32_t errlen) {
  KRYLAB_TRY
  Freer f;
  const double* d_x = f(up(x, n)); const double* d_d = f(up(d, 1));
  Out o(y, 0, y_words);
  dev::kry_round_scale_by(n, d_x, d_d, o.as<float>());
  dev::sync(); o.back();
  KRYLAB_END
}
int krylab_dot(int64_t n, const double* x, const double* y, double* part, int64_t part_words, double* out, int64_t out_words,
               char* err, int32_t errlen) {
  KRYLAB_TRY
  Freer f;
  const double* d_x = f(up(x, n)); const double* d_y = f(up(y, n));
  Out op(part, 0, part_words), oo(out, 0, out_words);
  dev::kry_dot(n, d_x, d_y, work(op, oo));
  dev::sync(); op.back(); oo.back();
  KRYLAB_END
}
int krylab_cg_xr(int64_t n, double alpha, const double* p, const double* q, double* x, int64_t x_words, double* r, int64_t r_words,
                 double* part, int64_t part_words, double* out, int64_t out_words, char* err, int32_t errlen) {
  KRYLAB_TRY
  Freer f;
  const double* d_p = f(up(p, n)); const double* d_q = f(up(q, n));
  Out ox(x, n * 8, x_words), orr(r, n * 8, r_words), op(part, 0, part_words), oo(out, 0, out_words);
  dev::kry_cg_xr(n, alpha, d_p, d_q, ox.as<double>(), orr.as<double>(), work(op, oo));
  dev::sync(); ox.back(); orr.back(); op.back(); oo.back();
  KRYLAB_END
}
int krylab_cg_p(int64_t n, double beta, const double* z, double* p, int64_t p_words, char* err, int32_t errlen) {
  KRYLAB_TRY
  Freer f;
  const double* d_z = f(up(z, n));
  Out o(p, n * 8, p_words);
  dev::kry_cg_p(n, beta, d_z, o.as<double>());
  dev::sync(); o.back();
  KRYLAB_END
}
// x <- x + V y in place, as the solver calls it; V has exactly (k - 1) ld + n entries, y has k
int krylab_update_f64(int64_t n, int32_t k, const double* V, int64_t ld, const double* y, double* x, int64_t x_words,
                      char* err, int32_t errlen) {
  KRYLAB_TRY
  Freer f;
  const double* d_V = f(up(V, basis_len(n, k, ld))); const double* d_y = f(up(y, std::max<int32_t>(k, 0)));
  Out o(x, n * 8, x_words);
  dev::kry_update(n, k, d_V, ld, d_y, o.as<double>());
  dev::sync(); o.back();
  KRYLAB_END
}
int krylab_update_f32(int64_t n, int32_t k, const float* V, int64_t ld, const double* y, double* x, int64_t x_words,
                      char* err, int32_t errlen) {
  KRYLAB_TRY
  Freer f;
  const float* d_V = f(up(V, basis_len(n, k, ld))); const double* d_y = f(up(y, std::max<int32_t>(k, 0)));
  Out o(x, n * 8, x_words);
  dev::kry_update(n, k, d_V, ld, d_y, o.as<double>());
  dev::sync(); o.back();
  KRYLAB_END
}

}  // extern "C"

// ---- batched launchers.  Operand kinds (rows of the offset table off[6][4], in elements of the kind's type):
//   0 A   first input   (float for widen_mv, double otherwise)      nA elements in all
//   1 B   second input  (double)                                     nB
//   2 Y   output        (float for round_scale_by_mv, double otherwise; initial content where the pass is in place)
//   3 R   second output (double, cg_xr_mv; initial content)
//   4 P   stage-one partials of column c
//   5 O   the result of column c
// D: nb device scalars (column c reads D[c]), S: the host scalars.  A null array is not uploaded and its pointers stay null.
namespace {

enum { MV_SCALE_BY, MV_ROUND_SCALE_BY, MV_WIDEN, MV_DOT, MV_CG_XR, MV_CG_P };

void run_mv(int which, int64_t n, int32_t nb, const void* A, int64_t nA, const double* B, int64_t nB, void* Y, int64_t y_init,
            int64_t y_words, double* R, int64_t r_init, int64_t r_words, const double* D, const double* S, double* P, int64_t p_words,
            double* O, int64_t o_words, const int64_t* off) {
  Freer f;
  const size_t a_item = which == MV_WIDEN ? 4 : 8, y_item = which == MV_ROUND_SCALE_BY ? 4 : 8;
  const int cols = std::max(0, std::min<int>(nb, dev::KRY_LOCKSTEP_MAX));
  const char* d_A = A ? (const char*)f(up((const char*)A, nA * (int64_t)a_item)) : nullptr;
  const double* d_B = B ? f(up(B, nB)) : nullptr;
  const double* d_D = D ? f(up(D, cols)) : nullptr;
  std::unique_ptr<Out> oy, orr, op, oo;
  if (Y) oy.reset(new Out(Y, y_init, y_words));
  if (R) orr.reset(new Out(R, r_init, r_words));
  if (P) op.reset(new Out(P, 0, p_words));
  if (O) oo.reset(new Out(O, 0, o_words));
  dev::KryVecBatch b{};
  b.nb = nb;                                             // as given: the launcher must refuse 0 and 5
  for (int c = 0; c < cols; c++) {
    b.a[c] = d_A ? d_A + (size_t)off[0 * 4 + c] * a_item : nullptr;
    b.b[c] = d_B ? d_B + off[1 * 4 + c] : nullptr;
    b.y[c] = oy ? (void*)(oy->as<char>() + (size_t)off[2 * 4 + c] * y_item) : nullptr;
    b.r[c] = orr ? orr->as<double>() + off[3 * 4 + c] : nullptr;
    b.d[c] = d_D ? d_D + c : nullptr;
    b.s[c] = S ? S[c] : 0.0;
    b.part[c] = op ? op->as<double>() + off[4 * 4 + c] : nullptr;
    b.out[c] = oo ? oo->as<double>() + off[5 * 4 + c] : nullptr;
  }
  switch (which) {
    case MV_SCALE_BY: dev::kry_scale_by_mv(n, b); break;
    case MV_ROUND_SCALE_BY: dev::kry_round_scale_by_mv(n, b); break;
    case MV_WIDEN: dev::kry_widen_mv(n, b); break;
    case MV_DOT: dev::kry_dot_mv(n, b); break;
    case MV_CG_XR: dev::kry_cg_xr_mv(n, b); break;
    default: dev::kry_cg_p_mv(n, b); break;
  }
  dev::sync();
  if (oy) oy->back();
  if (orr) orr->back();
  if (op) op->back();
  if (oo) oo->back();
}

}  // namespace

#define KRYLAB_MV(name, id)                                                                                                      \
  int krylab_##name(int64_t n, int32_t nb, const void* A, int64_t nA, const double* B, int64_t nB, void* Y, int64_t y_init,      \
                    int64_t y_words, double* R, int64_t r_init, int64_t r_words, const double* D, const double* S, double* P,    \
                    int64_t p_words, double* O, int64_t o_words, const int64_t* off, char* err, int32_t errlen) {                \
    KRYLAB_TRY                                                                                                                   \
    run_mv(id, n, nb, A, nA, B, nB, Y, y_init, y_words, R, r_init, r_words, D, S, P, p_words, O, o_words, off);                  \
    KRYLAB_END                                                                                                                   \
  }

extern "C" {

KRYLAB_MV(scale_by_mv, MV_SCALE_BY)
KRYLAB_MV(round_scale_by_mv, MV_ROUND_SCALE_BY)
KRYLAB_MV(widen_mv, MV_WIDEN)
KRYLAB_MV(dot_mv, MV_DOT)
KRYLAB_MV(cg_xr_mv, MV_CG_XR)
KRYLAB_MV(cg_p_mv, MV_CG_P)

// ---- SpMV: x has exactly nx entries ((nv - 1) ldx + ncols for the multi-vector form), y comes back whole
int krylab_spmv(int32_t nrows, const int32_t* rowptr, const int32_t* col, const double* val, const double* x, int64_t nx, double* y,
                int64_t y_init, int64_t y_words, double alpha, double beta, int64_t nnz_hint, char* err, int32_t errlen) {
  KRYLAB_TRY
  Freer f;
  const int64_t nnz = rowptr[nrows];
  const int32_t* d_rp = f(up(rowptr, (int64_t)nrows + 1)); const int32_t* d_col = f(up(col, nnz));
  const double* d_val = f(up(val, nnz)); const double* d_x = f(up(x, nx));
  Out o(y, y_init * 8, y_words);
  dev::spmv(nrows, d_rp, d_col, d_val, d_x, o.as<double>(), alpha, beta, nnz_hint);
  dev::sync(); o.back();
  KRYLAB_END
}
int krylab_spmv_mv(int32_t nrows, const int32_t* rowptr, const int32_t* col, const double* val, const double* x, int64_t nx, int64_t ldx,
                   double* y, int64_t y_init, int64_t y_words, int64_t ldy, int32_t nv, double alpha, double beta, int64_t nnz_hint,
                   char* err, int32_t errlen) {
  KRYLAB_TRY
  Freer f;
  const int64_t nnz = rowptr[nrows];
  const int32_t* d_rp = f(up(rowptr, (int64_t)nrows + 1)); const int32_t* d_col = f(up(col, nnz));
  const double* d_val = f(up(val, nnz)); const double* d_x = f(up(x, nx));
  Out o(y, y_init * 8, y_words);
  dev::spmv_mv(nrows, d_rp, d_col, d_val, d_x, ldx, o.as<double>(), ldy, nv, alpha, beta, nnz_hint);
  dev::sync(); o.back();
  KRYLAB_END
}

}  // extern "C"

// ---- the orthogonalisation passes A, B, C, single and batched.  Operand kinds (rows of the offset table off[7][4], in
// elements of the kind's type); every kind is ONE flat array and column c starts at off[kind * 4 + c]:
//   0 V    the basis of column c: K[c] columns of n rows, leading dimension ld (float or double).  An input of exactly nV
//          elements, or -- v_words > 0, double only -- an output buffer whose front is the caller's array: pass C with
//          dst = column K[c] of the same basis (mode 2), the way the solver calls it
//   1 W    the vector (output buffer with initial content: pass A must not write it)
//   2 DST  pass C, mode 0: a separate destination (mode 1: dst = w)
//   3 P    KryWork::part of column c      4 H1   KryWork::h1      5 H2   KryWork::h2      6 O   KryWork::out
// P and O are output buffers that start as canary; H1 and H2 are output buffers whose front holds the caller's initial content
// (h1 of pass B, h2 of pass C, and whatever the pass must leave alone).  A single-column entry takes column 0 of K and of the table.  When the launcher refuses, the
// buffers still come back from the device before the error is returned: a refusal must have written nothing.
namespace {

enum { PASS_A, PASS_B, PASS_C };

// sync and download whatever the launcher did, then pass its error on
template <class Launch, class Back>
void launch_and_fetch(Launch launch, Back back) {
  std::exception_ptr ep;
  try { launch(); } catch (...) { ep = std::current_exception(); }
  dev::sync();
  back();
  if (ep) std::rethrow_exception(ep);
}

void run_pass(int which, bool batched, bool f32, int64_t n, int64_t ld, int32_t nb, int32_t mode, const int32_t* K, void* V, int64_t nV,
              int64_t v_words, double* W, int64_t w_init, int64_t w_words, double* DST, int64_t dst_words, double* P,
              int64_t p_words, double* H1, int64_t h1_init, int64_t h1_words, double* H2, int64_t h2_init, int64_t h2_words, double* O,
              int64_t o_words, const int64_t* off) {
  Freer f;
  const size_t v_item = f32 ? 4 : 8;
  if (mode == 2 && (f32 || v_words <= 0)) throw Error(-2, "krylab: dst inside the basis needs a double basis in an output buffer");
  std::unique_ptr<Out> ov, odst;
  const char* d_V = nullptr;
  if (v_words > 0) { ov.reset(new Out(V, nV * 8, v_words)); d_V = ov->as<char>(); }
  else d_V = (const char*)f(up((const char*)V, nV * (int64_t)v_item));
  Out ow(W, w_init, w_words), op(P, 0, p_words), oh1(H1, h1_init, h1_words), oh2(H2, h2_init, h2_words), oo(O, 0, o_words);
  if (DST) odst.reset(new Out(DST, 0, dst_words));
  auto column = [&](int c, const void*& Vc, double*& wc, double*& dc, dev::KryWork& ws) {
    Vc = d_V + (size_t)off[0 * 4 + c] * v_item;
    wc = ow.as<double>() + off[1 * 4 + c];
    dc = mode == 0 ? (odst ? odst->as<double>() + off[2 * 4 + c] : nullptr)
       : mode == 1 ? wc : (double*)(d_V + (size_t)off[0 * 4 + c] * 8) + (int64_t)K[c] * ld;
    ws.part = op.as<double>() + off[3 * 4 + c];
    ws.h1 = oh1.as<double>() + off[4 * 4 + c];
    ws.h2 = oh2.as<double>() + off[5 * 4 + c];
    ws.out = oo.as<double>() + off[6 * 4 + c];
  };
  auto back = [&]() {
    if (ov) ov->back();
    if (odst) odst->back();
    ow.back(); op.back(); oh1.back(); oh2.back(); oo.back();
  };
  if (!batched) {
    const void* Vc; double *wc, *dc; dev::KryWork ws{};
    column(0, Vc, wc, dc, ws);
    const int32_t k = K[0];
    launch_and_fetch([&]() {
      if (f32) {
        if (which == PASS_A) dev::kry_pass_a(n, k, (const float*)Vc, ld, wc, ws);
        else if (which == PASS_B) dev::kry_pass_b(n, k, (const float*)Vc, ld, wc, ws);
        else dev::kry_pass_c(n, k, (const float*)Vc, ld, wc, dc, ws);
      } else {
        if (which == PASS_A) dev::kry_pass_a(n, k, (const double*)Vc, ld, wc, ws);
        else if (which == PASS_B) dev::kry_pass_b(n, k, (const double*)Vc, ld, wc, ws);
        else dev::kry_pass_c(n, k, (const double*)Vc, ld, wc, dc, ws);
      }
    }, back);
    return;
  }
  dev::KryBatch b{};
  b.nb = nb;                                               // as given: the launcher must refuse 0 and 5
  for (int c = 0; c < std::max(0, std::min<int>(nb, dev::KRY_LOCKSTEP_MAX)); c++) {
    b.k[c] = K[c];
    column(c, b.V[c], b.w[c], b.dst[c], b.ws[c]);
  }
  launch_and_fetch([&]() {
    if (which == PASS_A) dev::kry_pass_a_mv(n, ld, b, f32);
    else if (which == PASS_B) dev::kry_pass_b_mv(n, ld, b, f32);
    else dev::kry_pass_c_mv(n, ld, b, f32);
  }, back);
}

}  // namespace

#define KRYLAB_PASS_ARGS                                                                                                         \
  int32_t mode, const int32_t* K, void* V, int64_t nV, int64_t v_words, double* W, int64_t w_init, int64_t w_words, double* DST, \
  int64_t dst_words, double* P, int64_t p_words, double* H1, int64_t h1_init, int64_t h1_words, double* H2,     \
  int64_t h2_init, int64_t h2_words, double* O, int64_t o_words, const int64_t* off, char* err, int32_t errlen
#define KRYLAB_PASS_PASS                                                                                                         \
  mode, K, V, nV, v_words, W, w_init, w_words, DST, dst_words, P, p_words, H1, h1_init, h1_words, H2, h2_init, h2_words, \
  O, o_words, off
#define KRYLAB_PASS(name, id, f32)                                                          \
  int krylab_##name(int64_t n, int64_t ld, KRYLAB_PASS_ARGS) {                              \
    KRYLAB_TRY                                                                              \
    run_pass(id, false, f32, n, ld, 1, KRYLAB_PASS_PASS);                                   \
    KRYLAB_END                                                                              \
  }
#define KRYLAB_PASS_MV(name, id)                                                            \
  int krylab_##name(int64_t n, int64_t ld, int32_t nb, int32_t f32, KRYLAB_PASS_ARGS) {     \
    KRYLAB_TRY                                                                              \
    run_pass(id, true, f32 != 0, n, ld, nb, KRYLAB_PASS_PASS);                              \
    KRYLAB_END                                                                              \
  }

extern "C" {

int32_t krylab_tile_grid(int64_t n, int32_t k) { return dev::kry_tile_grid(n, k); }
int32_t krylab_tile_grid_f32(int64_t n, int32_t k) { return dev::kry_tile_grid_f32(n, k); }
int32_t krylab_tile() { return dev::KRY_TILE; }
int32_t krylab_proj_max() { return dev::KRY_PROJ_MAX; }
int32_t krylab_proj_chunk() { return dev::KRY_PROJ_CHUNK; }
int32_t krylab_border_max() { return dev::KRY_BORDER_MAX; }
int32_t krylab_border_chunk() { return dev::KRY_BORDER_CHUNK; }

KRYLAB_PASS(pass_a_f64, PASS_A, false)
KRYLAB_PASS(pass_a_f32, PASS_A, true)
KRYLAB_PASS(pass_b_f64, PASS_B, false)
KRYLAB_PASS(pass_b_f32, PASS_B, true)
KRYLAB_PASS(pass_c_f64, PASS_C, false)
KRYLAB_PASS(pass_c_f32, PASS_C, true)
KRYLAB_PASS_MV(pass_a_mv, PASS_A)
KRYLAB_PASS_MV(pass_b_mv, PASS_B)
KRYLAB_PASS_MV(pass_c_mv, PASS_C)

// ---- projection vectors.  Q, P: exactly nQ, nP elements; G null: the identity.  ws.part and ws.h1 are output buffers (h1
// with the caller's initial content: the coefficients of proj_update); x null: in place, y's initial content is x
int krylab_proj_coeffs(int64_t n, int32_t m, const double* Q, int64_t nQ, int64_t ldq, const double* G, int64_t nG, const double* x,
                       int64_t nx, double* P, int64_t p_words, double* H1, int64_t h1_init, int64_t h1_words, char* err, int32_t errlen) {
  KRYLAB_TRY
  Freer f;
  const double* d_Q = f(up(Q, nQ)); const double* d_G = G ? f(up(G, nG)) : nullptr; const double* d_x = f(up(x, nx));
  Out op(P, 0, p_words), oh(H1, h1_init, h1_words);
  dev::KryWork ws{};
  ws.part = op.as<double>(); ws.h1 = oh.as<double>();
  launch_and_fetch([&]() { dev::kry_proj_coeffs(n, m, d_Q, ldq, d_G, d_x, ws); }, [&]() { op.back(); oh.back(); });
  KRYLAB_END
}
int krylab_proj_update(int64_t n, int32_t m, const double* Pm, int64_t nP, int64_t ldp, const double* x, int64_t nx, double* Y, int64_t y_init,
                       int64_t y_words, double* H1, int64_t h1_init, int64_t h1_words, char* err, int32_t errlen) {
  KRYLAB_TRY
  Freer f;
  const double* d_P = f(up(Pm, nP)); const double* d_x = x ? f(up(x, nx)) : nullptr;
  Out oy(Y, y_init, y_words), oh(H1, h1_init, h1_words);
  dev::KryWork ws{};
  ws.h1 = oh.as<double>();
  launch_and_fetch([&]() { dev::kry_proj_update(n, m, d_P, ldp, d_x ? d_x : oy.as<double>(), oy.as<double>(), ws); },
                   [&]() { oy.back(); oh.back(); });
  KRYLAB_END
}
int krylab_oblique_project(int64_t n, int32_t m, const double* Q, int64_t nQ, int64_t ldq, const double* G, int64_t nG, const double* Pm,
                           int64_t nP, int64_t ldp, const double* x, int64_t nx, double* Y, int64_t y_init, int64_t y_words, double* P,
                           int64_t p_words, double* H1, int64_t h1_init, int64_t h1_words, char* err, int32_t errlen) {
  KRYLAB_TRY
  Freer f;
  const double* d_Q = f(up(Q, nQ)); const double* d_G = G ? f(up(G, nG)) : nullptr; const double* d_P = f(up(Pm, nP));
  const double* d_x = x ? f(up(x, nx)) : nullptr;
  Out oy(Y, y_init, y_words), op(P, 0, p_words), oh(H1, h1_init, h1_words);
  dev::KryWork ws{};
  ws.part = op.as<double>(); ws.h1 = oh.as<double>();
  launch_and_fetch([&]() { dev::kry_oblique_project(n, m, d_Q, ldq, d_G, d_P, ldp, d_x ? d_x : oy.as<double>(), oy.as<double>(), ws); },
                   [&]() { oy.back(); op.back(); oh.back(); });
  KRYLAB_END
}
// ---- the border product: z (n + m entries) is an output buffer too, so that the caller sees it unchanged; y is an output
// buffer whose first n entries are K x
int krylab_border_product(int64_t n, int32_t m, const double* V, int64_t nV, int64_t ldv, const double* W, int64_t nW, int64_t ldw,
                          const double* C, int64_t nC, double* Z, int64_t z_init, int64_t z_words, double* Y, int64_t y_init, int64_t y_words, double* P,
                          int64_t p_words, char* err, int32_t errlen) {
  KRYLAB_TRY
  Freer f;
  const double* d_V = f(up(V, nV)); const double* d_W = f(up(W, nW)); const double* d_C = C ? f(up(C, nC)) : nullptr;
  Out oz(Z, z_init, z_words), oy(Y, y_init, y_words), op(P, 0, p_words);
  dev::KryWork ws{};
  ws.part = op.as<double>();
  launch_and_fetch([&]() { dev::kry_border_product(n, m, d_V, ldv, d_W, ldw, d_C, oz.as<double>(), oy.as<double>(), ws); },
                   [&]() { oz.back(); oy.back(); op.back(); });
  KRYLAB_END
}

}  // extern "C"
