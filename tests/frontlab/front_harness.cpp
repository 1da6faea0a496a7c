// front_harness.cpp -- TEST-ONLY driver of the batched multifrontal LU of one pattern class (plain C++, no device code).
//
// It drives the real host code the way DirectSolver does (precond.cpp: analyse_class, BatchedLU::upload / factor_chunk /
// check_flag / solve, MergedSolve) and hands the separator blocks, the solutions, the flags and the front table back to the
// caller (tests/frontlab/cases.py, through ctypes).  The same source is linked twice (Makefile): against the host simulator
// (tests/hostsim) and against the product library, so a harness bug shows up on a machine without a GPU first.
//
// Canaries: the stream's setup arena is grown by a guard tail and, like the factor slab, filled with a NaN bit pattern
// before every chunk.  Afterwards the guard tail and every slab entry of the members outside the chunk must be unchanged
// (bitwise), every entry outside the fronts' panels must still hold the pattern, and every panel entry of the chunk's
// members must be finite.
#include <cstdint>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>
#include "precond.hpp"

using namespace hymls;

namespace {

constexpr uint64_t CANARY = 0x7ff4dead5eed5eedULL;   // a signalling NaN no arithmetic produces
constexpr size_t GUARD_DOUBLES = (size_t)1 << 17;     // 1 MiB behind the arena's used part

// canary status bits
constexpr int32_t CAN_GUARD = 1;        // the arena's guard tail was written
constexpr int32_t CAN_OTHER = 2;        // a slab entry of a member outside the chunk changed
constexpr int32_t CAN_NONFINITE = 4;    // a panel entry of a factored member is not finite (or was never written)
constexpr int32_t CAN_OUTSIDE = 8;      // a slab entry outside every panel lost the pattern

dev::Context* g_ctx = nullptr;

void fill_canary(void* dptr, size_t ndoubles) {
  if (!ndoubles) return;
  std::vector<uint64_t> h(ndoubles, CANARY);
  dev::h2d(dptr, h.data(), ndoubles * sizeof(uint64_t));
}

}  // namespace

// Inputs: the extended local CSR (n = nI + nS rows), zero-diagonal marks and coordinates of the interior rows, nb value
// sets of nnz entries each, the analysis switches, the members per factorisation pass (0: all), nrhs right-hand sides per
// member (rhs[b][v][nI], local order), merged != 0: solve with MergedSolve where it fits.
// Outputs: sblock[b][nS * nS] (column-major), x[b][v][nI] (local order), info[8] = {nfronts, chunk, merged used,
// flag bits, canary status, factor_size, passes, big fronts}, growth, fronts[nfronts][7] =
// {w, ri, rs, parent, level, big, wide} (capacity front_cap).  Returns 0, or an error code with the message in err.
extern "C" int frontlab_run(int32_t nI, int32_t nS, const int32_t* rowptr, const int32_t* col, const int8_t* zero_diag,
                            const int32_t* coord, int32_t nb, const double* vals, int32_t leaf_size, int32_t max_width,
                            int64_t big_panel_entries, int32_t want_chunk, int32_t nrhs, const double* rhs, int32_t merged,
                            double* sblock, double* x, int64_t* info, double* growth, int32_t* fronts, int32_t front_cap,
                            char* err, int32_t errlen) {
  try {
    if (!g_ctx) g_ctx = dev::create_context(0);
    dev::bind(g_ctx);
    const int32_t n = nI + nS;
    const int64_t nnz = rowptr[n];
    LocalPattern lp;
    lp.nI = nI; lp.nS = nS;
    lp.rowptr.assign(rowptr, rowptr + n + 1);
    lp.col.assign(col, col + nnz);
    lp.zero_diag.assign(zero_diag, zero_diag + nI);
    lp.coord.assign(coord, coord + 3 * (int64_t)nI);
    BatchedLU lu;
    lu.plan = analyse_class(lp, leaf_size, max_width, big_panel_entries);
    const ClassPlan& P = lu.plan;
    const int32_t nf = (int32_t)P.fronts.size();
    HYMLS_CHECK(nf <= front_cap, -2, "front table too small");
    for (int32_t s = 0; s < nf; s++) {
      const Front& F = P.fronts[s];
      const int32_t row[7] = {F.w, F.ri, F.rs, F.parent, F.level, F.big ? 1 : 0, F.wide ? 1 : 0};
      std::memcpy(fronts + 7 * (int64_t)s, row, sizeof row);
    }
    lu.members.resize(nb);
    lu.h_xoff.resize(nb);
    lu.h_src.resize((size_t)nb * nnz);
    for (int32_t b = 0; b < nb; b++) {
      lu.members[b] = b;
      lu.h_xoff[b] = b * nI;
      for (int64_t e = 0; e < nnz; e++) lu.h_src[(size_t)b * nnz + e] = (int32_t)(b * nnz + e);
    }
    lu.contrib_nv = dev::NV_MAX;
    const bool with_sblock = nS > 0;
    const int64_t per = P.scratch_size + (with_sblock ? (int64_t)nS * nS : 0);
    const int64_t budget = want_chunk > 0 ? (int64_t)want_chunk * std::max<int64_t>(per, 1) : (int64_t)1 << 50;
    lu.upload(budget, with_sblock);
    const int32_t chunk = lu.chunk;

    // panel map of one member's slab: 1 inside a front's panels
    const int64_t fs = P.factor_size;
    std::vector<char> in_panel((size_t)std::max<int64_t>(fs, 1), 0);
    for (const Front& F : P.fronts) {
      for (int64_t t = 0; t < (int64_t)(F.w + F.ri) * F.w; t++) in_panel[F.lp_off + t] = 1;
      for (int64_t t = 0; t < (int64_t)F.w * F.ri; t++) in_panel[F.q_off + t] = 1;
    }
    int32_t canary = 0;
    const size_t slab_doubles = (size_t)nb * fs;
    fill_canary(lu.batch.factor, slab_doubles);
    std::vector<uint64_t> slab(slab_doubles, CANARY), after(slab_doubles);

    double* d_kval = (double*)dev::alloc((size_t)std::max<int64_t>(1, nb * nnz) * sizeof(double));
    dev::h2d(d_kval, vals, (size_t)nb * nnz * sizeof(double));
    const size_t need = (size_t)(lu.scratch_need_ + lu.sblock_need_ + lu.tmp_need_);
    int64_t passes = 0;
    for (int32_t b0 = 0; b0 < nb; b0 += chunk) {
      const int32_t nbc = std::min(chunk, nb - b0);
      double* arena = (double*)dev::shared_scratch((need + GUARD_DOUBLES) * sizeof(double));
      fill_canary(arena, need + GUARD_DOUBLES);
      lu.factor_chunk(d_kval, b0, nbc);
      passes++;
      if (nS > 0) dev::d2h(sblock + (int64_t)b0 * nS * nS, lu.batch.sblock, (size_t)nbc * nS * nS * sizeof(double));
      std::vector<uint64_t> guard(GUARD_DOUBLES);
      dev::d2h(guard.data(), arena + need, GUARD_DOUBLES * sizeof(double));
      for (uint64_t g : guard) if (g != CANARY) { canary |= CAN_GUARD; break; }
      dev::d2h(after.data(), lu.batch.factor, slab_doubles * sizeof(double));
      for (int32_t b = 0; b < nb; b++) {
        const bool mine = b >= b0 && b < b0 + nbc;
        const uint64_t* a = after.data() + (size_t)b * fs;
        const uint64_t* s = slab.data() + (size_t)b * fs;
        for (int64_t t = 0; t < fs; t++) {
          if (!mine) { if (a[t] != s[t]) canary |= CAN_OTHER; continue; }
          if (!in_panel[t]) { if (a[t] != CANARY) canary |= CAN_OUTSIDE; continue; }
          double v;
          std::memcpy(&v, &a[t], sizeof v);
          if (!std::isfinite(v)) canary |= CAN_NONFINITE;
        }
      }
      slab.swap(after);
    }
    int32_t flag = lu.check_flag(growth);

    // A11 x = b for every member and right-hand side (level vector: member b at b * nI, elimination order)
    const bool use_merged = merged && merged_solve_fits(P);
    const int64_t ld = (int64_t)nb * nI;
    std::vector<double> z((size_t)std::max<int64_t>(1, ld * nrhs));
    for (int32_t b = 0; b < nb; b++)
      for (int32_t v = 0; v < nrhs; v++)
        for (int32_t i = 0; i < nI; i++) z[(size_t)v * ld + (size_t)b * nI + i] = rhs[((int64_t)b * nrhs + v) * nI + P.perm[i]];
    double* d_x = (double*)dev::alloc(z.size() * sizeof(double));
    dev::h2d(d_x, z.data(), z.size() * sizeof(double));
    int64_t solve_fronts = 0;
    if (use_merged) {
      MergedSolve ms;
      ms.build({{0, &lu}});
      dev::PlanD* d_plan = dev::upload(std::vector<dev::PlanD>{lu.dplan});
      double* d_y = (double*)dev::alloc(z.size() * sizeof(double));
      ms.solve(d_plan, d_x, d_y, ld, nrhs);
      dev::sync();
      dev::free(d_y);
      dev::free(d_plan);
    } else {
      for (int32_t v = 0; v < nrhs; v++) lu.solve(d_x + (size_t)v * ld);
    }
    for (const Front& F : P.fronts) solve_fronts += F.big;
    dev::d2h(z.data(), d_x, z.size() * sizeof(double));
    dev::free(d_x);
    dev::free(d_kval);
    for (int32_t b = 0; b < nb; b++)
      for (int32_t v = 0; v < nrhs; v++)
        for (int32_t i = 0; i < nI; i++) x[((int64_t)b * nrhs + v) * nI + P.perm[i]] = z[(size_t)v * ld + (size_t)b * nI + i];
    info[0] = nf; info[1] = chunk; info[2] = use_merged ? 1 : 0; info[3] = flag; info[4] = canary; info[5] = fs;
    info[6] = passes; info[7] = solve_fronts;
    return 0;
  } catch (const std::exception& e) {
    if (err && errlen > 0) { std::strncpy(err, e.what(), (size_t)errlen - 1); err[errlen - 1] = 0; }
    return -1;
  }
}
