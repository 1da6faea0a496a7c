// fused_harness.cpp -- TEST-ONLY driver of the fused interior solve and its panel layouts (plain C++, no device code).
//
// One exported entry per step (tests/fusedlab/cases.py, through ctypes): plan (analyse_class + BatchedLU::upload), factor
// (BatchedLU::factor_chunk), repack (dev::repack_fronts), storage (dev::demote_panels / dev::round_panels on a class's slab),
// solve (the four dev::interior_solve_fused* launchers), solve_io (FusedIO against the separate vector kernels), demote /
// round (on a caller-given array at chosen misalignments) and transposed (dev::solve_transposed).  Every entry is upload,
// one dev:: call, dev::sync, download; solve_io runs the fused launch and the separate sequence it replaces.  The same
// source is linked twice (Makefile): against the host simulator and against the product library.
//
// Every output buffer on the device is filled with the frontlab NaN canary before the call and has a guard tail that must
// still hold it afterwards.  Every index array is checked on the host first; a failed check returns its error code and
// nothing is launched.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>
#include "precond.hpp"

using namespace hymls;

namespace {

constexpr uint64_t CANARY = 0x7ff4dead5eed5eedULL;   // a signalling NaN no arithmetic produces (tests/frontlab)
constexpr uint32_t CANARY32 = 0x7fa5eed5u;           // the same idea in 4 bytes (FP32 slabs)
constexpr size_t GUARD = 4096;                       // elements behind every output buffer

// error codes of the host-side checks (cases.py: ERRORS)
constexpr int E_EXCEPTION = -1, E_ARG = -10, E_PERM = -11, E_ACOL = -12, E_AROW = -13, E_XOFF = -14, E_FITS = -15;

struct Cls {
  BatchedLU lu;
  int32_t nb = 0;
  int64_t nnz = 0, fs = 0;
  double* slab = nullptr;      // [nb][fs] + guard tail: what lu.batch.factor points to
  double* rounded = nullptr;   // the slab rounded through float (round_panels), same layout
  FusedNeed need{0, 0};
  bool fits = false, factored = false;
};

dev::Context* g_ctx = nullptr;
std::vector<std::unique_ptr<Cls>> g_cls;
std::string g_err;

void bind() {
  if (!g_ctx) g_ctx = dev::create_context(0);
  dev::bind(g_ctx);
}

template <class T, class U>
T* canary_buffer(size_t n, U pattern) {
  static_assert(sizeof(T) == sizeof(U), "pattern of the element's size");
  std::vector<U> h(n + GUARD, pattern);
  T* d = (T*)dev::alloc(h.size() * sizeof(T));
  dev::h2d(d, h.data(), h.size() * sizeof(T));
  return d;
}
double* canary_doubles(size_t n) { return canary_buffer<double>(n, CANARY); }

bool guard_intact(const double* d, size_t n) {
  std::vector<uint64_t> g(GUARD);
  dev::d2h(g.data(), d + n, GUARD * sizeof(double));
  for (uint64_t v : g) if (v != CANARY) return false;
  return true;
}

int fail(int code, const char* what) { g_err = what; return code; }

Cls* get(int32_t c) { return c >= 0 && c < (int32_t)g_cls.size() ? g_cls[c].get() : nullptr; }

// the sub table of a launch: members of planned classes at caller-given offsets of a level vector of n entries
struct Launch {
  std::vector<dev::FusedSub> subs;
  std::vector<dev::PlanD> plans;
  int32_t lds = 0, front = 0, vec = 0;
  int64_t covered = 0;
};
// storage: 0 the FP64 slab, 1 the FP32 slab, 2 the rounded FP64 slab
int make_launch(int32_t nsub, const int32_t* sub_cls, const int32_t* sub_mem, const int32_t* sub_xoff, int32_t storage, int64_t n, Launch& L) {
  std::vector<std::pair<int64_t, int64_t>> blocks;
  for (auto& c : g_cls) L.plans.push_back(c->lu.dplan);
  for (int32_t s = 0; s < nsub; s++) {
    Cls* C = get(sub_cls[s]);
    if (!C || sub_mem[s] < 0 || sub_mem[s] >= C->nb || !C->factored) return fail(E_ARG, "sub table: unknown class or member");
    if (!C->fits) return fail(E_FITS, "fused_solve_fits is false for a class of the launch");
    const int64_t off = (int64_t)sub_mem[s] * C->fs;
    dev::FusedSub fsub{{nullptr}, sub_xoff[s], sub_cls[s]};
    if (storage == 1) { if (!C->lu.factor32) return fail(E_ARG, "no FP32 slab"); fsub.fac32 = C->lu.factor32 + off; }
    else if (storage == 2) { if (!C->rounded) return fail(E_ARG, "no rounded slab"); fsub.fac = C->rounded + off; }
    else fsub.fac = C->slab + off;
    L.subs.push_back(fsub);
    blocks.emplace_back(sub_xoff[s], (int64_t)sub_xoff[s] + C->lu.plan.nI);
    L.lds = std::max(L.lds, C->need.total);
    L.front = std::max(L.front, C->need.fronts);
    L.vec = std::max(L.vec, C->need.total - C->need.fronts);
    L.covered += C->lu.plan.nI;
  }
  std::sort(blocks.begin(), blocks.end());
  for (size_t t = 0; t < blocks.size(); t++) {
    if (blocks[t].first < 0 || blocks[t].second > n) return fail(E_XOFF, "xoff block outside the level vector");
    if (t > 0 && blocks[t].first < blocks[t - 1].second) return fail(E_XOFF, "xoff blocks overlap");
  }
  return 0;
}

template <class F>
int guarded(F body) {
  try {
    bind();
    return body();
  } catch (const std::exception& e) {
    g_err = e.what();
    return E_EXCEPTION;
  }
}

}  // namespace

extern "C" const char* fusedlab_error() { return g_err.c_str(); }

extern "C" int fusedlab_reset() {
  return guarded([&] {
    for (auto& c : g_cls) { dev::free(c->slab); dev::free(c->rounded); c->lu.batch.factor = nullptr; }
    g_cls.clear();
    return 0;
  });
}

// analyse_class and BatchedLU::upload of one class: the extended local CSR (n = nI + nS rows), nb members at offsets
// xoff[nb] of the level vector.  Returns the class id.  info[12] = {nfronts, nlev, factor_size, contrib_size,
// max_level_rows, fused_solve_need total, ... fronts, fused_solve_fits, forward items, backward items, length of fidx,
// scratch_size}.
extern "C" int fusedlab_plan(int32_t nI, int32_t nS, const int32_t* rowptr, const int32_t* col, const int8_t* zero_diag,
                             const int32_t* coord, int32_t nb, const int32_t* xoff, int32_t leaf_size, int32_t max_width,
                             int32_t packed, int64_t* info) {
  return guarded([&] {
    if (nI <= 0 || nb <= 0) return fail(E_ARG, "plan: empty class");
    const int32_t n = nI + nS;
    const int64_t nnz = rowptr[n];
    LocalPattern lp;
    lp.nI = nI; lp.nS = nS;
    lp.rowptr.assign(rowptr, rowptr + n + 1);
    lp.col.assign(col, col + nnz);
    lp.zero_diag.assign(zero_diag, zero_diag + nI);
    lp.coord.assign(coord, coord + 3 * (int64_t)nI);
    auto C = std::make_unique<Cls>();
    BatchedLU& lu = C->lu;
    lu.plan = analyse_class(lp, leaf_size, max_width);
    const ClassPlan& P = lu.plan;
    C->nb = nb; C->nnz = nnz; C->fs = P.factor_size;
    C->need = fused_solve_need(P);
    C->fits = fused_solve_fits(P);
    lu.members.resize(nb);
    lu.h_xoff.assign(xoff, xoff + nb);
    lu.h_src.resize((size_t)nb * nnz);
    for (int32_t b = 0; b < nb; b++) {
      lu.members[b] = b;
      for (int64_t e = 0; e < nnz; e++) lu.h_src[(size_t)b * nnz + e] = (int32_t)(b * nnz + e);
    }
    lu.packed = packed != 0;
    lu.contrib_nv = 1;
    lu.upload((int64_t)1 << 50, nS > 0);
    if (lu.chunk != nb) return fail(E_ARG, "plan: the members do not fit one factorisation pass");
    // the slab with a guard tail takes the place of the one upload() made (which stays owned by lu and unused)
    C->slab = canary_doubles((size_t)nb * C->fs);
    lu.batch.factor = C->slab;
    const int64_t out[12] = {(int64_t)P.fronts.size(), (int64_t)P.levels.size(), P.factor_size, P.contrib_size, P.max_level_rows,
                             C->need.total, C->need.fronts, C->fits ? 1 : 0, (int64_t)P.fw_items.size(), (int64_t)P.bw_items.size(),
                             (int64_t)P.fidx.size(), P.scratch_size};
    std::memcpy(info, out, sizeof out);
    g_cls.push_back(std::move(C));
    return (int)g_cls.size() - 1;
  });
}

// the tables of a planned class: fronts[nfronts][10] = {w, ri, rs, parent, level, c0, idx_off, lp_off, q_off, big},
// fidx, fw_ptr / bw_ptr [nlev + 1], rec_n[forward items] = FwRec::n as uploaded (read back from the device), perm[nI]
extern "C" int fusedlab_tables(int32_t cls, int64_t* fronts, int32_t* fidx, int32_t* fw_ptr, int32_t* bw_ptr, int32_t* rec_n, int32_t* perm) {
  return guarded([&] {
    Cls* C = get(cls);
    if (!C) return fail(E_ARG, "tables: unknown class");
    const ClassPlan& P = C->lu.plan;
    for (size_t s = 0; s < P.fronts.size(); s++) {
      const Front& F = P.fronts[s];
      const int64_t row[10] = {F.w, F.ri, F.rs, F.parent, F.level, F.c0, F.idx_off, F.lp_off, F.q_off, F.big ? 1 : 0};
      std::memcpy(fronts + 10 * s, row, sizeof row);
    }
    std::copy(P.fidx.begin(), P.fidx.end(), fidx);
    std::copy(P.fw_ptr.begin(), P.fw_ptr.end(), fw_ptr);
    std::copy(P.bw_ptr.begin(), P.bw_ptr.end(), bw_ptr);
    std::copy(P.perm.begin(), P.perm.end(), perm);
    std::vector<dev::FwRec> rec(P.fw_items.size());
    if (!rec.empty()) dev::d2h(rec.data(), C->lu.dplan.fw_rec, rec.size() * sizeof(dev::FwRec));
    for (size_t t = 0; t < rec.size(); t++) rec_n[t] = rec[t].n;
    return 0;
  });
}

// BatchedLU::factor_chunk of all members into the canary-filled slab (unpacked panels); slab_out[nb][factor_size].
// info[2] = {flag bits, guard tail intact}
extern "C" int fusedlab_factor(int32_t cls, const double* vals, double* slab_out, int64_t* info) {
  return guarded([&] {
    Cls* C = get(cls);
    if (!C) return fail(E_ARG, "factor: unknown class");
    const size_t nslab = (size_t)C->nb * C->fs;
    std::vector<uint64_t> h(nslab + GUARD, CANARY);
    dev::h2d(C->slab, h.data(), h.size() * sizeof(double));
    double* d_kval = (double*)dev::alloc((size_t)std::max<int64_t>(1, C->nb * C->nnz) * sizeof(double));
    dev::h2d(d_kval, vals, (size_t)C->nb * C->nnz * sizeof(double));
    C->lu.factor_chunk(d_kval, 0, C->nb);
    dev::sync();
    dev::d2h(slab_out, C->slab, nslab * sizeof(double));
    info[0] = C->lu.check_flag();
    info[1] = guard_intact(C->slab, nslab) ? 1 : 0;
    dev::free(d_kval);
    C->factored = true;
    return 0;
  });
}

// dev::repack_fronts of members [b0, b0 + nbc) alone; the whole slab comes down.  info[1] = {guard tail intact}
extern "C" int fusedlab_repack(int32_t cls, int32_t b0, int32_t nbc, double* slab_out, int64_t* info) {
  return guarded([&] {
    Cls* C = get(cls);
    if (!C || !C->factored || b0 < 0 || nbc <= 0 || b0 + nbc > C->nb) return fail(E_ARG, "repack: bad class or members");
    dev::repack_fronts(C->lu.dplan, C->lu.batch, b0, nbc);
    dev::sync();
    const size_t nslab = (size_t)C->nb * C->fs;
    dev::d2h(slab_out, C->slab, nslab * sizeof(double));
    info[0] = guard_intact(C->slab, nslab) ? 1 : 0;
    return 0;
  });
}

// the slab as the caller wants it (upload only) and the layout the solves are told it has
extern "C" int fusedlab_set_slab(int32_t cls, const double* slab, int32_t packed) {
  return guarded([&] {
    Cls* C = get(cls);
    if (!C || !C->factored) return fail(E_ARG, "set_slab: unknown or unfactored class");
    dev::h2d(C->slab, slab, (size_t)C->nb * C->fs * sizeof(double));
    C->lu.packed = packed != 0;
    C->lu.dplan.packed = packed != 0;
    return 0;
  });
}

// what = 1: dev::demote_panels of the slab into the class's FP32 slab; what = 2: a copy of the slab through
// dev::round_panels.  out: the FP32 slab (what = 1, nb * factor_size floats) or the rounded one (doubles).
// info[2] = {FLAG_F32_RANGE raised, guard tail intact}
extern "C" int fusedlab_storage(int32_t cls, int32_t what, void* out, int64_t* info) {
  return guarded([&] {
    Cls* C = get(cls);
    if (!C || !C->factored || (what != 1 && what != 2)) return fail(E_ARG, "storage: bad class or mode");
    const size_t nslab = (size_t)C->nb * C->fs;
    int32_t* d_flag = (int32_t*)dev::alloc(sizeof(int32_t));
    dev::zero(d_flag, sizeof(int32_t));
    if (what == 1) {
      dev::free(C->lu.factor32);
      C->lu.factor32 = canary_buffer<float>(nslab, CANARY32);
      dev::demote_panels((int64_t)nslab, C->slab, C->lu.factor32, d_flag);
      dev::sync();
      dev::d2h(out, C->lu.factor32, nslab * sizeof(float));
      std::vector<uint32_t> g(GUARD);
      dev::d2h(g.data(), C->lu.factor32 + nslab, GUARD * sizeof(float));
      info[1] = std::all_of(g.begin(), g.end(), [](uint32_t v) { return v == CANARY32; }) ? 1 : 0;
    } else {
      dev::free(C->rounded);
      C->rounded = canary_doubles(nslab);
      dev::d2d(C->rounded, C->slab, nslab * sizeof(double));
      dev::round_panels((int64_t)nslab, C->rounded, d_flag);
      dev::sync();
      dev::d2h(out, C->rounded, nslab * sizeof(double));
      info[1] = guard_intact(C->rounded, nslab) ? 1 : 0;
    }
    int32_t fl = 0;
    dev::d2h(&fl, d_flag, sizeof fl);
    dev::free(d_flag);
    info[0] = fl;
    return 0;
  });
}

// kind 0: interior_solve_fused, 1: _f32, 2: _mv, 3: _mv_f32 on x[nv][ldx] (in place; the caller fills the gaps between
// the blocks and behind n with the canary and checks them).  storage as in make_launch (kinds 1 and 3: the FP32 slab).
// info[4] = {guard tail intact, LDS doubles of the launch for one vector, ... of the front descriptors, ... per vector}
extern "C" int fusedlab_solve(int32_t kind, int32_t nsub, const int32_t* sub_cls, const int32_t* sub_mem, const int32_t* sub_xoff,
                              int32_t storage, int64_t n, int32_t nv, int64_t ldx, double* x, int64_t* info) {
  return guarded([&] {
    if (kind < 0 || kind > 3 || nv < 1 || ldx < n || ((kind == 0 || kind == 1) && nv != 1)) return fail(E_ARG, "solve: bad kind, nv or ldx");
    if (kind == 1 || kind == 3) storage = 1; else if (storage == 1) return fail(E_ARG, "solve: the FP32 slab needs an _f32 kind");
    Launch L;
    if (int rc = make_launch(nsub, sub_cls, sub_mem, sub_xoff, storage, n, L)) return rc;
    const size_t len = (size_t)ldx * nv;
    double* d_x = canary_doubles(len);
    dev::h2d(d_x, x, len * sizeof(double));
    dev::FusedSub* d_subs = dev::upload(L.subs);
    dev::PlanD* d_plans = dev::upload(L.plans);
    switch (kind) {
      case 0: dev::interior_solve_fused(nsub, d_subs, d_plans, L.lds, d_x); break;
      case 1: dev::interior_solve_fused_f32(nsub, d_subs, d_plans, L.lds, d_x); break;
      case 2: dev::interior_solve_fused_mv(nsub, d_subs, d_plans, L.vec + L.front, L.front, d_x, ldx, nv); break;
      default: dev::interior_solve_fused_mv_f32(nsub, d_subs, d_plans, L.vec + L.front, L.front, d_x, ldx, nv); break;
    }
    dev::sync();
    dev::d2h(x, d_x, len * sizeof(double));
    info[0] = guard_intact(d_x, len) ? 1 : 0;
    info[1] = L.lds; info[2] = L.front; info[3] = L.vec;
    dev::free(d_x); dev::free(d_subs); dev::free(d_plans);
    return 0;
  });
}

// The two fused launches of a single-vector ApplyInverse and the separate kernels they replace (LevelSolver::
// apply_inverse_mv), on a level vector of n interior rows that the subs cover exactly:
//   (1, 0): x10_fused = A11 \ b[perm]                      against gather, solve
//   (2, 1): user_fused[perm] = z - A11 \ (A x2)            against spmv (row sums by the lanes of nnz_hint), solve, axpby, scatter
// t1_after: the x argument of the (2, 1) launch, which it must not touch.  info[3] = guard tails intact of the three
// fused outputs (x10, user, t1)
extern "C" int fusedlab_solve_io(int32_t nsub, const int32_t* sub_cls, const int32_t* sub_mem, const int32_t* sub_xoff, int32_t n,
                                 int32_t nuser, const int32_t* perm, const int32_t* a_row, const int32_t* a_col, const double* a_val,
                                 int64_t nnz, int32_t nx2, const double* x2, const double* z, const double* b, int32_t a_lanes, int64_t nnz_hint,
                                 double* x10_fused, double* x10_sep, double* user_fused, double* user_sep, double* t1_after,
                                 int64_t* info) {
  return guarded([&] {
    if (n <= 0 || nuser < n || nx2 <= 0) return fail(E_ARG, "solve_io: bad sizes");
    std::vector<char> seen((size_t)nuser, 0);
    for (int32_t i = 0; i < n; i++) {
      if (perm[i] < 0 || perm[i] >= nuser || seen[perm[i]]) return fail(E_PERM, "perm is not a permutation inside the user vector");
      seen[perm[i]] = 1;
    }
    if (a_row[0] != 0) return fail(E_AROW, "a_row does not start at 0");
    for (int32_t i = 0; i < n; i++) if (a_row[i + 1] < a_row[i]) return fail(E_AROW, "a_row is not monotone");
    if (a_row[n] != nnz) return fail(E_AROW, "a_row does not end at nnz");
    for (int64_t e = 0; e < nnz; e++) if (a_col[e] < 0 || a_col[e] >= nx2) return fail(E_ACOL, "a_col outside x2");
    if (dev::spmv_lanes(n, nnz_hint) != a_lanes) return fail(E_ARG, "solve_io: nnz_hint does not select a_lanes");
    Launch L;
    if (int rc = make_launch(nsub, sub_cls, sub_mem, sub_xoff, 0, n, L)) return rc;
    if (L.covered != n) return fail(E_XOFF, "solve_io: the subs do not cover the level vector");
    auto up = [&](const auto* h, size_t cnt) {
      using T = std::remove_const_t<std::remove_pointer_t<decltype(h)>>;
      T* d = (T*)dev::alloc(std::max<size_t>(cnt, 1) * sizeof(T));
      if (cnt) dev::h2d(d, h, cnt * sizeof(T));
      return d;
    };
    int32_t* d_perm = up(perm, n); int32_t* d_arow = up(a_row, (size_t)n + 1); int32_t* d_acol = up(a_col, (size_t)nnz);
    double* d_aval = up(a_val, (size_t)nnz); double* d_x2 = up(x2, nx2); double* d_z = up(z, n); double* d_b = up(b, nuser);
    dev::FusedSub* d_subs = dev::upload(L.subs);
    dev::PlanD* d_plans = dev::upload(L.plans);
    // ---- first solve
    double* d_x = canary_doubles(n);
    dev::FusedIO io1;
    io1.in = 1; io1.b = d_b; io1.perm = d_perm;
    dev::interior_solve_fused(nsub, d_subs, d_plans, L.lds, d_x, &io1);
    dev::sync();
    dev::d2h(x10_fused, d_x, (size_t)n * sizeof(double));
    info[0] = guard_intact(d_x, n) ? 1 : 0;
    double* d_z1 = canary_doubles(n);
    dev::gather(n, d_perm, d_b, d_z1);
    dev::interior_solve_fused(nsub, d_subs, d_plans, L.lds, d_z1);
    dev::sync();
    dev::d2h(x10_sep, d_z1, (size_t)n * sizeof(double));
    // ---- second solve
    double* d_t1 = canary_doubles(n);
    double* d_user = canary_doubles(nuser);
    dev::FusedIO io2;
    io2.in = 2; io2.a_row = d_arow; io2.a_col = d_acol; io2.a_val = d_aval; io2.x2 = d_x2; io2.a_lanes = a_lanes;
    io2.out = 1; io2.z = d_z; io2.user = d_user; io2.perm = d_perm;
    dev::interior_solve_fused(nsub, d_subs, d_plans, L.lds, d_t1, &io2);
    dev::sync();
    dev::d2h(user_fused, d_user, (size_t)nuser * sizeof(double));
    dev::d2h(t1_after, d_t1, (size_t)n * sizeof(double));
    info[1] = guard_intact(d_user, nuser) ? 1 : 0;
    info[2] = guard_intact(d_t1, n) ? 1 : 0;
    double* d_user2 = canary_doubles(nuser);
    double* d_zc = up(z, n);
    dev::spmv(n, d_arow, d_acol, d_aval, d_x2, d_t1, 1.0, 0.0, nnz_hint);
    dev::interior_solve_fused(nsub, d_subs, d_plans, L.lds, d_t1);
    dev::axpby(n, -1.0, d_t1, 1.0, d_zc);
    dev::scatter(n, d_perm, d_zc, d_user2);
    dev::sync();
    dev::d2h(user_sep, d_user2, (size_t)nuser * sizeof(double));
    for (void* p : {(void*)d_perm, (void*)d_arow, (void*)d_acol, (void*)d_aval, (void*)d_x2, (void*)d_z, (void*)d_b, (void*)d_subs,
                    (void*)d_plans, (void*)d_x, (void*)d_z1, (void*)d_t1, (void*)d_user, (void*)d_user2, (void*)d_zc}) dev::free(p);
    return 0;
  });
}

// dev::demote_panels (what = 1) or dev::round_panels (what = 2) of n entries; src starts src_off (0 or 1) doubles and dst
// dst_off (0 .. 3) floats behind a 16-byte boundary.  dst_out[dst_off + n + 64] floats / round_out[src_off + n + 64]
// doubles: the whole buffer from the boundary on, canary before and behind the n entries.  info[1] = {flag}
extern "C" int fusedlab_demote(int32_t what, int64_t n, int32_t src_off, int32_t dst_off, const double* src, float* dst_out,
                               double* round_out, int64_t* info) {
  return guarded([&] {
    if (n <= 0 || src_off < 0 || src_off > 1 || dst_off < 0 || dst_off > 3 || (what != 1 && what != 2)) return fail(E_ARG, "demote: bad arguments");
    constexpr size_t TAIL = 64, ALIGN = 4;   // (ALIGN doubles = 32 bytes)
    auto aligned = [](auto* p) { return (decltype(p))(((uintptr_t)p + 31) / 32 * 32); };
    double* d_src0 = canary_doubles(ALIGN + src_off + n + TAIL);
    double* d_src = aligned(d_src0) + src_off;
    dev::h2d(d_src, src, (size_t)n * sizeof(double));
    int32_t* d_flag = (int32_t*)dev::alloc(sizeof(int32_t));
    dev::zero(d_flag, sizeof(int32_t));
    if (what == 1) {
      float* d_dst0 = canary_buffer<float>(2 * ALIGN + dst_off + n + TAIL, CANARY32);
      float* d_dst = aligned(d_dst0) + dst_off;
      dev::demote_panels(n, d_src, d_dst, d_flag);
      dev::sync();
      dev::d2h(dst_out, d_dst - dst_off, ((size_t)dst_off + n + TAIL) * sizeof(float));
      dev::free(d_dst0);
    } else {
      dev::round_panels(n, d_src, d_flag);
      dev::sync();
      dev::d2h(round_out, d_src - src_off, ((size_t)src_off + n + TAIL) * sizeof(double));
    }
    int32_t fl = 0;
    dev::d2h(&fl, d_flag, sizeof fl);
    info[0] = fl;
    dev::free(d_flag); dev::free(d_src0);
    return 0;
  });
}

// dev::solve_transposed of every member of a class on x[n] (in place, members at the offsets given to plan), with the
// elimination order and the row count LevelSolver::compute_border builds.  info[1] = {guard tail intact}
extern "C" int fusedlab_transposed(int32_t cls, int64_t n, double* x, int64_t* info) {
  return guarded([&] {
    Cls* C = get(cls);
    if (!C || !C->factored) return fail(E_ARG, "transposed: unknown or unfactored class");
    const ClassPlan& P = C->lu.plan;
    std::vector<std::pair<int64_t, int64_t>> blocks;
    for (int32_t o : C->lu.h_xoff) blocks.emplace_back(o, (int64_t)o + P.nI);
    std::sort(blocks.begin(), blocks.end());
    for (size_t t = 0; t < blocks.size(); t++)
      if (blocks[t].first < 0 || blocks[t].second > n || (t > 0 && blocks[t].first < blocks[t - 1].second)) return fail(E_XOFF, "xoff blocks overlap or leave the vector");
    ivec order;
    int32_t rows = 1;
    for (size_t l = 0; l < P.levels.size(); l++) {
      order.insert(order.end(), P.levels[l].begin(), P.levels[l].end());
      order.insert(order.end(), P.big_levels[l].begin(), P.big_levels[l].end());
    }
    for (auto& F : P.fronts) rows = std::max(rows, F.w + F.ri);
    int32_t* d_order = dev::upload(order);
    double* d_x = canary_doubles((size_t)n);
    dev::h2d(d_x, x, (size_t)n * sizeof(double));
    dev::solve_transposed(C->lu.dplan, C->lu.batch, d_order, (int32_t)P.fronts.size(), rows, d_x);
    dev::sync();
    dev::d2h(x, d_x, (size_t)n * sizeof(double));
    info[0] = guard_intact(d_x, (size_t)n) ? 1 : 0;
    dev::free(d_x); dev::free(d_order);
    return 0;
  });
}
