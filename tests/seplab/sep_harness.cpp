// sep_harness.cpp -- TEST-ONLY driver of the separator-side, vector and table launchers of the device layer (plain C++, no
// device code).
//
// One extern "C" function per launcher of device.hpp: upload the arguments, call exactly ONE dev:: launcher (the pairs
// sblock_transform + sblock_extract and offdiag_count + offdiag_fill are the exceptions), synchronise, download, free.  The
// descriptor tables (BlkD, KeptD) are assembled here from flat arrays and offsets.  The same source is linked twice
// (Makefile): against the host simulator (tests/hostsim) and against the product library, so a harness bug shows up on a
// machine without a GPU first.
//
// Canaries: every output buffer is allocated with a guard tail behind it and filled, tail included, with the NaN bit pattern
// of tests/frontlab before the caller's initial content (if any) is copied to its front.  The whole buffer comes back, so
// the caller checks bit for bit that nothing outside the defined output set was written.  The caller's host array has the
// full length, words = payload + SEPLAB_GUARD_WORDS 8-byte words.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
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
    if (words < GUARD_WORDS || init_bytes > (words - GUARD_WORDS) * 8) throw Error(-2, "seplab: output buffer without its guard tail");
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

// descriptor table from flat arrays: block b has order nb[b], row tile r0[b], entries at binv + boff[b], ids at ids + ioff[b]
std::vector<dev::BlkD> blk_table(int32_t nblk, const int32_t* nb, const int32_t* r0, const int64_t* boff, const int64_t* ioff,
                                 const double* d_binv, const int32_t* d_ids) {
  std::vector<dev::BlkD> t((size_t)nblk);
  for (int32_t b = 0; b < nblk; b++) t[b] = dev::BlkD{d_binv + boff[b], d_ids ? d_ids + ioff[b] : nullptr, nb[b], r0 ? r0[b] : -1};
  return t;
}

}  // namespace

#define SEPLAB_TRY try { bind();
#define SEPLAB_END return 0; } catch (const std::exception& e) { return fail(e, err, errlen); }

extern "C" {

int64_t seplab_guard_words() { return GUARD_WORDS; }
uint64_t seplab_canary() { return CANARY; }

// ---- route predicates (recorded by the coverage bookkeeping)
int32_t seplab_spmv_lanes(int32_t nrows, int64_t nnz_hint) { return dev::spmv_lanes(nrows, nnz_hint); }
int32_t seplab_invert_blocked_order(int32_t nb) { return dev::dense_invert_blocked_order(nb) ? 1 : 0; }
int32_t seplab_kept_fits(int32_t nS, int32_t ngl) { return dev::sblock_kept_fits(nS, ngl) ? 1 : 0; }

// ---- vector kernels
int seplab_gather(int64_t n, const int32_t* idx, const double* src, int64_t nsrc, double* dst, int64_t dst_words, char* err, int32_t errlen) {
  SEPLAB_TRY
  Freer f;
  const int32_t* d_idx = f(up(idx, n)); const double* d_src = f(up(src, nsrc));
  Out o(dst, 0, dst_words);
  dev::gather(n, d_idx, d_src, o.as<double>());
  dev::sync(); o.back();
  SEPLAB_END
}
int seplab_scatter(int64_t n, const int32_t* idx, const double* src, double* dst, int64_t dst_init, int64_t dst_words, int32_t add,
                   char* err, int32_t errlen) {
  SEPLAB_TRY
  Freer f;
  const int32_t* d_idx = f(up(idx, n)); const double* d_src = f(up(src, n));
  Out o(dst, dst_init * 8, dst_words);
  if (add) dev::scatter_add(n, d_idx, d_src, o.as<double>());
  else dev::scatter(n, d_idx, d_src, o.as<double>());
  dev::sync(); o.back();
  SEPLAB_END
}
int seplab_spmv(int32_t nrows, const int32_t* rowptr, const int32_t* col, const double* val, const double* x, int64_t nx, double* y,
                int64_t y_init, int64_t y_words, double alpha, double beta, int64_t nnz_hint, char* err, int32_t errlen) {
  SEPLAB_TRY
  Freer f;
  const int64_t nnz = rowptr[nrows];
  const int32_t* d_rp = f(up(rowptr, (int64_t)nrows + 1)); const int32_t* d_col = f(up(col, nnz));
  const double* d_val = f(up(val, nnz)); const double* d_x = f(up(x, nx));
  Out o(y, y_init * 8, y_words);
  dev::spmv(nrows, d_rp, d_col, d_val, d_x, o.as<double>(), alpha, beta, nnz_hint);
  dev::sync(); o.back();
  SEPLAB_END
}
int seplab_dot(int64_t n, const double* x, const double* y, double* out, char* err, int32_t errlen) {
  SEPLAB_TRY
  Freer f;
  const double* d_x = f(up(x, n)); const double* d_y = f(up(y, n));
  *out = dev::dot(n, d_x, d_y);
  dev::sync();
  SEPLAB_END
}
int seplab_pull_sum(int64_t n, const int64_t* ptr, const int64_t* idx, const double* in, int64_t nin, double* out, int64_t out_words,
                    char* err, int32_t errlen) {
  SEPLAB_TRY
  Freer f;
  const int64_t* d_ptr = f(up(ptr, n + 1)); const int64_t* d_idx = f(up(idx, ptr[n])); const double* d_in = f(up(in, nin));
  Out o(out, 0, out_words);
  dev::pull_sum(n, d_ptr, d_idx, d_in, o.as<double>());
  dev::sync(); o.back();
  SEPLAB_END
}
int seplab_pull_sum_blocks(int64_t blen, int32_t nblk, const int64_t* ptr, const int64_t* base, const double* in, int64_t nin, double* out,
                           int64_t out_words, char* err, int32_t errlen) {
  SEPLAB_TRY
  Freer f;
  const int64_t* d_ptr = f(up(ptr, (int64_t)nblk + 1)); const int64_t* d_base = f(up(base, ptr[nblk])); const double* d_in = f(up(in, nin));
  Out o(out, 0, out_words);
  dev::pull_sum_blocks(blen, nblk, d_ptr, d_base, d_in, o.as<double>());
  dev::sync(); o.back();
  SEPLAB_END
}
int seplab_build_pull_tables(int64_t nrows, const int64_t* rcount, const int32_t* rowptr, const uint64_t* keys, int64_t* ptr, int64_t ptr_words,
                             int64_t* idx, int64_t idx_words, char* err, int32_t errlen) {
  SEPLAB_TRY
  Freer f;
  const int64_t* d_rc = f(up(rcount, nrows + 1)); const int32_t* d_rp = f(up(rowptr, nrows + 1)); const uint64_t* d_keys = f(up(keys, rcount[nrows]));
  Out op(ptr, 0, ptr_words), oi(idx, 0, idx_words);
  dev::build_pull_tables(nrows, d_rc, d_rp, d_keys, op.as<int64_t>(), oi.as<int64_t>());
  dev::sync(); op.back(); oi.back();
  SEPLAB_END
}
// level matrix: nk rows (krow[nk + 1], kcol); src: int32 entries in a buffer of src_words 8-byte words
int seplab_member_sources(int32_t nb, int32_t next, int32_t nent, const int32_t* ext, const int32_t* ent_row, const int32_t* ent_col,
                          int32_t nk, const int32_t* krow, const int32_t* kcol, int32_t* src, int64_t src_words, int32_t* flag,
                          char* err, int32_t errlen) {
  SEPLAB_TRY
  Freer f;
  const int32_t* d_ext = f(up(ext, (int64_t)nb * next)); const int32_t* d_er = f(up(ent_row, nent)); const int32_t* d_ec = f(up(ent_col, nent));
  const int32_t* d_krow = f(up(krow, (int64_t)nk + 1)); const int32_t* d_kcol = f(up(kcol, krow[nk]));
  int32_t* d_flag = f(up(flag, 1));
  Out o(src, 0, src_words);
  dev::member_sources(nb, next, nent, d_ext, d_er, d_ec, d_krow, d_kcol, o.as<int32_t>(), d_flag);
  dev::sync(); o.back();
  dev::d2h(flag, d_flag, sizeof(int32_t));
  SEPLAB_END
}
// offdiag_count, the prefix sum on the host, offdiag_fill.  ncols: length of ta / tb / excl; cap: entries the col / src buffers hold
int seplab_offdiag(int64_t nrows, const int32_t* rows, int32_t nk, const int32_t* krow, const int32_t* kcol, int32_t ncols, const int32_t* ta,
                   const int32_t* tb, const int32_t* excl, int32_t* count, int64_t count_words, int32_t* col, int64_t col_words, int32_t* src,
                   int64_t src_words, int64_t cap, char* err, int32_t errlen) {
  SEPLAB_TRY
  Freer f;
  const int32_t* d_rows = f(up(rows, nrows)); const int32_t* d_krow = f(up(krow, (int64_t)nk + 1)); const int32_t* d_kcol = f(up(kcol, krow[nk]));
  const int32_t* d_ta = f(up(ta, ncols)); const int32_t* d_tb = tb ? f(up(tb, ncols)) : nullptr; const int32_t* d_excl = f(up(excl, ncols));
  Out oc(count, 0, count_words), ocol(col, 0, col_words), osrc(src, 0, src_words);
  dev::offdiag_count(nrows, d_rows, d_krow, d_kcol, d_ta, d_tb, d_excl, oc.as<int32_t>());
  dev::sync(); oc.back();
  std::vector<int32_t> rowptr((size_t)nrows + 1, 0);
  for (int64_t t = 0; t < nrows; t++) {
    if (count[t + 1] < 0 || (int64_t)rowptr[t] + count[t + 1] > cap) throw Error(-2, "seplab: offdiag_count exceeds the expected number of entries");
    rowptr[t + 1] = rowptr[t] + count[t + 1];
  }
  const int32_t* d_rowptr = f(up(rowptr.data(), nrows + 1));
  dev::offdiag_fill(nrows, d_rows, d_krow, d_kcol, d_ta, d_tb, d_excl, d_rowptr, ocol.as<int32_t>(), osrc.as<int32_t>());
  dev::sync(); ocol.back(); osrc.back();
  SEPLAB_END
}

// ---- separator-side kernels
int seplab_ot_apply(int32_t ng, const int32_t* gptr, const double* w, int64_t nw, double* x, int64_t x_init, int64_t x_words, char* err, int32_t errlen) {
  SEPLAB_TRY
  Freer f;
  const int32_t* d_g = f(up(gptr, (int64_t)ng + 1)); const double* d_w = f(up(w, nw));
  Out o(x, x_init * 8, x_words);
  dev::ot_apply(ng, d_g, d_w, o.as<double>());
  dev::sync(); o.back();
  SEPLAB_END
}
// two-pass route: sblock (nbc blocks + guard, transformed in place) and out[b][k] = sblock[b][pick[k]]
int seplab_transform_extract(int32_t nS, int32_t ng, const int32_t* gptr, const double* tv, double* sblock, int64_t sblock_words, int32_t nbc,
                             int64_t npick, const int32_t* pick, double* out, int64_t out_stride, int64_t out_words, char* err, int32_t errlen) {
  SEPLAB_TRY
  Freer f;
  const int32_t* d_g = f(up(gptr, (int64_t)ng + 1)); const double* d_tv = f(up(tv, (int64_t)nbc * nS)); const int32_t* d_pick = f(up(pick, npick));
  Out os(sblock, (int64_t)nbc * nS * nS * 8, sblock_words), oo(out, 0, out_words);
  dev::sblock_transform(nS, ng, d_g, d_tv, os.as<double>(), nbc);
  dev::sblock_extract(nS, npick, d_pick, os.as<double>(), oo.as<double>(), out_stride, nbc);
  dev::sync(); os.back(); oo.back();
  SEPLAB_END
}
int seplab_sblock_kept(int32_t nS, int32_t ngl, const int32_t* gptr, const int32_t* glink, const int32_t* goff, int32_t nlinks, const int64_t* lboff,
                       const int32_t* lblen, const double* tv, const double* sblock, int32_t nbc, double* out, int64_t out_stride, int64_t out_words,
                       char* err, int32_t errlen) {
  SEPLAB_TRY
  Freer f;
  dev::KeptD K{nS, ngl, f(up(gptr, (int64_t)ngl + 1)), f(up(glink, ngl)), f(up(goff, ngl)), f(up(lboff, nlinks)), f(up(lblen, nlinks))};
  const double* d_tv = f(up(tv, (int64_t)nbc * nS)); const double* d_S = f(up(sblock, (int64_t)nbc * nS * nS));
  Out oo(out, 0, out_words);
  dev::sblock_kept(K, d_tv, d_S, oo.as<double>(), out_stride, nbc);
  dev::sync(); oo.back();
  SEPLAB_END
}
int seplab_dense_invert(int32_t nb, int32_t nblk, double* blocks, int64_t blocks_words, int32_t* flag, char* err, int32_t errlen) {
  SEPLAB_TRY
  Freer f;
  int32_t* d_flag = f(up(flag, 1));
  Out o(blocks, (int64_t)nblk * nb * nb * 8, blocks_words);
  dev::dense_invert(nb, nblk, o.as<double>(), d_flag);
  dev::sync(); o.back();
  dev::d2h(flag, d_flag, sizeof(int32_t));
  SEPLAB_END
}
// flat: the blocks one after the other (block b of order nb[b] at boff[b]), inverted in place
int seplab_dense_invert_all(int32_t nblk, const int32_t* nb, const int64_t* boff, double* flat, int64_t flat_init, int64_t flat_words, int32_t max_nb,
                            int32_t* flag, char* err, int32_t errlen) {
  SEPLAB_TRY
  Freer f;
  int32_t* d_flag = f(up(flag, 1));
  Out o(flat, flat_init * 8, flat_words);
  const std::vector<dev::BlkD> t = blk_table(nblk, nb, nullptr, boff, nullptr, o.as<double>(), nullptr);
  const dev::BlkD* d_t = f(dev::upload(t));
  dev::dense_invert_all(nblk, d_t, max_nb, d_flag);
  dev::sync(); o.back();
  dev::d2h(flag, d_flag, sizeof(int32_t));
  SEPLAB_END
}
int seplab_blocks_apply(int32_t nb, int32_t nblk, const double* binv, const int32_t* ids, const double* x, int64_t nx, double* y, int64_t y_words,
                        char* err, int32_t errlen) {
  SEPLAB_TRY
  Freer f;
  const double* d_b = f(up(binv, (int64_t)nblk * nb * nb)); const int32_t* d_ids = f(up(ids, (int64_t)nblk * nb)); const double* d_x = f(up(x, nx));
  Out o(y, 0, y_words);
  dev::blocks_apply(nb, nblk, d_b, d_ids, d_x, o.as<double>());
  dev::sync(); o.back();
  SEPLAB_END
}
int seplab_blocks_apply_all(int32_t nblk, const int32_t* nb, const int32_t* r0, const int64_t* boff, const int64_t* ioff, const double* binv,
                            int64_t nbinv, const int32_t* ids, int64_t nids, int32_t max_nb, const double* x, int64_t nx, double* y, int64_t y_words,
                            char* err, int32_t errlen) {
  SEPLAB_TRY
  Freer f;
  const double* d_b = f(up(binv, nbinv)); const int32_t* d_ids = f(up(ids, nids)); const double* d_x = f(up(x, nx));
  const dev::BlkD* d_t = f(dev::upload(blk_table(nblk, nb, r0, boff, ioff, d_b, d_ids)));
  Out o(y, 0, y_words);
  dev::blocks_apply_all(nblk, d_t, max_nb, d_x, o.as<double>());
  dev::sync(); o.back();
  SEPLAB_END
}
// x: nv columns of leading dimension ldx; y: nv columns of leading dimension ldy (+ guard)
int seplab_blocks_apply_all_mv(int32_t nblk, const int32_t* nb, const int32_t* r0, const int64_t* boff, const int64_t* ioff, const double* binv,
                               int64_t nbinv, const int32_t* ids, int64_t nids, int32_t max_nb, const double* x, int64_t ldx, double* y, int64_t ldy,
                               int32_t nv, int64_t y_words, char* err, int32_t errlen) {
  SEPLAB_TRY
  Freer f;
  const double* d_b = f(up(binv, nbinv)); const int32_t* d_ids = f(up(ids, nids)); const double* d_x = f(up(x, ldx * nv));
  const dev::BlkD* d_t = f(dev::upload(blk_table(nblk, nb, r0, boff, ioff, d_b, d_ids)));
  Out o(y, 0, y_words);
  dev::blocks_apply_all_mv(nblk, d_t, max_nb, d_x, ldx, o.as<double>(), ldy, nv);
  dev::sync(); o.back();
  SEPLAB_END
}
// one row tile [r0, r0 + nrows) of ONE block of order nb whose other rows are zero: rows[r][j] (row-major) are the only entries
// that travel; the nb x nb block exists on the device alone.  ids = identity.  nv = 0: blocks_apply_all, else the _mv form.
int seplab_blocks_apply_tile(int32_t nb, int32_t r0, int32_t nrows, const double* rows, const double* x, int64_t ldx, double* y, int64_t ldy,
                             int32_t nv, int64_t y_words, char* err, int32_t errlen) {
  SEPLAB_TRY
  Freer f;
  const size_t bytes = (size_t)nb * nb * sizeof(double);
  double* d_b = f((double*)dev::alloc(bytes));
  dev::zero(d_b, bytes);
  std::vector<double> colbuf((size_t)nrows);
  for (int32_t j = 0; j < nb; j++) {
    for (int32_t r = 0; r < nrows; r++) colbuf[r] = rows[(int64_t)r * nb + j];
    dev::h2d(d_b + (int64_t)nb * j + r0, colbuf.data(), (size_t)nrows * sizeof(double));
  }
  std::vector<int32_t> ids((size_t)nb);
  for (int32_t j = 0; j < nb; j++) ids[j] = j;
  const int32_t* d_ids = f(dev::upload(ids));
  const double* d_x = f(up(x, ldx * std::max(nv, 1)));
  const dev::BlkD* d_t = f(dev::upload(std::vector<dev::BlkD>{dev::BlkD{d_b, d_ids, nb, r0}}));
  Out o(y, 0, y_words);
  if (nv == 0) dev::blocks_apply_all(1, d_t, nb, d_x, o.as<double>());
  else dev::blocks_apply_all_mv(1, d_t, nb, d_x, ldx, o.as<double>(), ldy, nv);
  dev::sync(); o.back();
  SEPLAB_END
}

}  // extern "C"
