// lvl_harness.cpp -- TEST-ONLY driver of the merged level solve of one pattern class in FP64 and FP32 panel storage (plain
// C++, no device code), in the style of tests/frontlab and tests/fusedlab.
//
// It drives the real host code (precond.cpp: analyse_class, BatchedLU::upload / factor_chunk, MergedSolve::build /
// set_storage / solve) and the launchers of device.hpp (demote_panels, round_panels, solve_*_tasks_mv and their _f32
// forms).  The same source is linked twice (Makefile): against the simulator library of this directory (tests/hostsim +
// tests/f32_sim + lvl_f32_sim.cpp, both macros) and against the product library.
//
// Canaries: the level vectors x and y of a solve are filled with a NaN bit pattern, carry a guard tail, and have ld =
// nb * nI + pad entries per column; the pad and the tails must come back untouched.
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "precond.hpp"

using namespace hymls;

namespace {

constexpr uint64_t CANARY = 0x7ff4dead5eed5eedULL;   // a signalling NaN no arithmetic produces
constexpr size_t GUARD = 4096;                       // doubles behind every level vector

struct Lab {
  BatchedLU lu;
  MergedSolve ms;
  int32_t nb = 0, nI = 0;
  int64_t fs = 0;
  double* slab = nullptr;      // what upload() made: the FP64 panels
  double* rounded = nullptr;   // a copy rounded through float (round_panels)
  dev::PlanD* d_plan = nullptr;
};

dev::Context* g_ctx = nullptr;
std::unique_ptr<Lab> g_lab;
std::string g_err;

template <class F>
int guarded(F body) {
  try {
    if (!g_ctx) g_ctx = dev::create_context(0);
    dev::bind(g_ctx);
    return body();
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}
int fail(int code, const char* what) { g_err = what; return code; }

void drop_lab() {
  if (!g_lab) return;
  g_lab->lu.batch.factor = g_lab->slab;   // (owned by lu)
  dev::free(g_lab->rounded);
  dev::free(g_lab->d_plan);
  g_lab.reset();
}

}  // namespace

extern "C" const char* lvllab_error() { return g_err.c_str(); }

extern "C" int lvllab_reset() {
  return guarded([&] { drop_lab(); return 0; });
}

// analyse_class, BatchedLU::upload, factor_chunk of all nb members and MergedSolve::build of one class: the extended local
// CSR (n = nI + nS rows), nb value sets of nnz entries.  Member b sits at b * nI of the level vector.
// Outputs: slab[nb][factor_size] (unpacked FP64 panels), fronts[nfronts][10] = {w, ri, rs, parent, level, c0, idx_off,
// lp_off, q_off, big} (capacity front_cap), fidx (capacity fidx_cap), perm[nI], info[8] = {nfronts, factor_size, flag
// bits, length of fidx, tasks forward, tasks backward, largest LDS need of a level in doubles, merged_solve_fits}.
// A first call with slab = nullptr only plans and reports the sizes.
extern "C" int lvllab_plan_factor(int32_t nI, int32_t nS, const int32_t* rowptr, const int32_t* col, const int8_t* zero_diag,
                                  const int32_t* coord, int32_t nb, const double* vals, int32_t leaf_size, int32_t max_width,
                                  double* slab, int64_t* fronts, int32_t front_cap, int32_t* fidx, int32_t fidx_cap, int32_t* perm,
                                  int64_t* info) {
  return guarded([&] {
    drop_lab();
    if (nI <= 0 || nb <= 0) return fail(-10, "plan: empty class");
    const int32_t n = nI + nS;
    const int64_t nnz = rowptr[n];
    LocalPattern lp;
    lp.nI = nI; lp.nS = nS;
    lp.rowptr.assign(rowptr, rowptr + n + 1);
    lp.col.assign(col, col + nnz);
    lp.zero_diag.assign(zero_diag, zero_diag + nI);
    lp.coord.assign(coord, coord + 3 * (int64_t)nI);
    auto L = std::make_unique<Lab>();
    BatchedLU& lu = L->lu;
    lu.plan = analyse_class(lp, leaf_size, max_width);
    const ClassPlan& P = lu.plan;
    L->nb = nb; L->nI = nI; L->fs = P.factor_size;
    info[0] = (int64_t)P.fronts.size(); info[1] = P.factor_size; info[3] = (int64_t)P.fidx.size();
    info[7] = merged_solve_fits(P) ? 1 : 0;
    if (!slab) return 0;
    if (!info[7]) return fail(-15, "merged_solve_fits is false for the class");
    if ((int32_t)P.fronts.size() > front_cap || (int32_t)P.fidx.size() > fidx_cap) return fail(-10, "plan: table too small");
    for (size_t s = 0; s < P.fronts.size(); s++) {
      const Front& F = P.fronts[s];
      const int64_t row[10] = {F.w, F.ri, F.rs, F.parent, F.level, F.c0, F.idx_off, F.lp_off, F.q_off, F.big ? 1 : 0};
      std::memcpy(fronts + 10 * s, row, sizeof row);
    }
    std::copy(P.fidx.begin(), P.fidx.end(), fidx);
    std::copy(P.perm.begin(), P.perm.end(), perm);
    lu.members.resize(nb);
    lu.h_xoff.resize(nb);
    lu.h_src.resize((size_t)nb * nnz);
    for (int32_t b = 0; b < nb; b++) {
      lu.members[b] = b;
      lu.h_xoff[b] = b * nI;
      for (int64_t e = 0; e < nnz; e++) lu.h_src[(size_t)b * nnz + e] = (int32_t)(b * nnz + e);
    }
    lu.contrib_nv = dev::NV_MAX;
    lu.upload((int64_t)1 << 50, nS > 0);
    if (lu.chunk != nb) return fail(-10, "plan: the members do not fit one factorisation pass");
    L->slab = lu.batch.factor;
    double* d_kval = (double*)dev::alloc((size_t)std::max<int64_t>(1, nb * nnz) * sizeof(double));
    dev::h2d(d_kval, vals, (size_t)nb * nnz * sizeof(double));
    lu.factor_chunk(d_kval, 0, nb);
    dev::sync();
    dev::free(d_kval);
    info[2] = lu.check_flag();
    dev::d2h(slab, L->slab, (size_t)nb * L->fs * sizeof(double));
    L->ms.build({{0, &L->lu}});
    L->d_plan = dev::upload(std::vector<dev::PlanD>{lu.dplan});
    info[4] = L->ms.fw_off.back(); info[5] = L->ms.bw_off.back();
    int32_t lds = 0;
    for (int32_t v : L->ms.fw_lds) lds = std::max(lds, v);
    for (int32_t v : L->ms.bw_lds) lds = std::max(lds, v);
    info[6] = lds;
    g_lab = std::move(L);
    return 0;
  });
}

// The two storages of the float-rounded panels: dev::demote_panels of the slab into the class's FP32 slab (slab32_out,
// nb * factor_size floats) and a copy of the slab through dev::round_panels (rounded_out, doubles).
// info[2] = {flag bits after the demotion, flag bits after the rounding} (FLAG_F32_RANGE = 4)
extern "C" int lvllab_storage(float* slab32_out, double* rounded_out, int64_t* info) {
  return guarded([&] {
    Lab* L = g_lab.get();
    if (!L) return fail(-10, "storage: nothing planned");
    const int64_t len = (int64_t)L->nb * L->fs;
    BatchedLU& lu = L->lu;
    lu.batch.factor = L->slab;
    lu.hold_factor32();
    dev::zero(lu.batch.flag, 4 * sizeof(int32_t));
    dev::demote_panels(len, L->slab, lu.factor32, lu.batch.flag);
    dev::sync();
    info[0] = lu.check_flag();
    dev::d2h(slab32_out, lu.factor32, (size_t)len * sizeof(float));
    if (!L->rounded) L->rounded = (double*)dev::alloc((size_t)std::max<int64_t>(len, 1) * sizeof(double));
    dev::d2d(L->rounded, L->slab, (size_t)len * sizeof(double));
    dev::zero(lu.batch.flag, 4 * sizeof(int32_t));
    dev::round_panels(len, L->rounded, lu.batch.flag);
    dev::sync();
    info[1] = lu.check_flag();
    dev::d2h(rounded_out, L->rounded, (size_t)len * sizeof(double));
    return 0;
  });
}

// MergedSolve::solve of nv right-hand sides.  storage: 0 the FP64 slab, 1 the FP32 slab (the _f32 launchers), 2 the
// rounded FP64 slab.  rhs[nv][nb * nI] in elimination order (the level vector); x_out[nv][ld], ld = nb * nI + pad: the
// whole vectors as they come back, pad included.  info[2] = {guard tail of x intact, guard tail of y intact}
extern "C" int lvllab_solve(int32_t storage, int32_t nv, int32_t pad, const double* rhs, double* x_out, int64_t* info) {
  return guarded([&] {
    Lab* L = g_lab.get();
    if (!L || nv <= 0 || pad < 0) return fail(-10, "solve: nothing planned or bad sizes");
    BatchedLU& lu = L->lu;
    if (storage == 1) {
      if (!lu.factor32) return fail(-10, "solve: no FP32 slab");
      L->ms.set_storage(32);
    } else {
      if (storage == 2 && !L->rounded) return fail(-10, "solve: no rounded slab");
      lu.batch.factor = storage == 2 ? L->rounded : L->slab;
      L->ms.set_storage(64);
      lu.batch.factor = L->slab;
    }
    const int64_t n = (int64_t)L->nb * L->nI, ld = n + pad;
    const size_t len = (size_t)ld * nv;
    std::vector<uint64_t> h(len + GUARD, CANARY);
    double* d_x = (double*)dev::alloc(h.size() * sizeof(double));
    double* d_y = (double*)dev::alloc(h.size() * sizeof(double));
    dev::h2d(d_y, h.data(), h.size() * sizeof(double));
    for (int32_t v = 0; v < nv; v++) std::memcpy(h.data() + (size_t)v * ld, rhs + (size_t)v * n, (size_t)n * sizeof(double));
    dev::h2d(d_x, h.data(), h.size() * sizeof(double));
    L->ms.solve(L->d_plan, d_x, d_y, ld, nv);
    dev::sync();
    dev::d2h(h.data(), d_x, h.size() * sizeof(double));
    std::memcpy(x_out, h.data(), len * sizeof(double));
    info[0] = 1;
    for (size_t t = len; t < len + GUARD; t++) if (h[t] != CANARY) info[0] = 0;
    dev::d2h(h.data(), d_y, h.size() * sizeof(double));
    info[1] = 1;
    for (size_t t = len; t < len + GUARD; t++) if (h[t] != CANARY) info[1] = 0;
    for (int32_t v = 0; v < nv; v++)                               // (the pad of y as well)
      for (int64_t t = n; t < ld; t++) if (h[(size_t)v * ld + t] != CANARY) info[1] = 0;
    dev::free(d_x);
    dev::free(d_y);
    return 0;
  });
}
