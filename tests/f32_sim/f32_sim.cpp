// TEST-ONLY: plain-loop versions of the launchers FP32 panel storage adds to device.hpp (demote_panels, round_panels and
// the _f32 forms of the fused interior solve), next to tests/hostsim/device_sim.cpp.  The solve is the loop of
// device_sim.cpp's interior_solve_fused with the panels read as float and widened: same loop order, same sums.
// The library keeps pivot-block inverses in its panels, so an input can be finite in FP64 and out of float's range.
#include "device.hpp"
#include <cfloat>
#include <cmath>
#include <vector>

namespace hymls {
namespace dev {

void demote_panels(int64_t n, const double* src, float* dst, int32_t* flag) {
  for (int64_t t = 0; t < n; t++) {
    if (!(std::fabs(src[t]) <= (double)FLT_MAX)) *flag |= FLAG_F32_RANGE;   // (also a NaN)
    dst[t] = (float)src[t];                                                 // round to nearest
  }
}

void round_panels(int64_t n, double* slab, int32_t* flag) {
  for (int64_t t = 0; t < n; t++) {
    if (!(std::fabs(slab[t]) <= (double)FLT_MAX)) *flag |= FLAG_F32_RANGE;
    slab[t] = (double)(float)slab[t];
  }
}

void interior_solve_fused_f32(int32_t nsub, const FusedSub* subs, const PlanD* plans, int32_t, double* x, const FusedIO* iop) {
  const FusedIO io = iop ? *iop : FusedIO();
  std::vector<double> C, Fv, out, Xl;
  for (int b = 0; b < nsub; b++) {
    const PlanD& P = plans[subs[b].cls];
    const int xoff = subs[b].xoff;
    Xl.assign(std::max(P.nI, 1), 0.0);
    for (int i = 0; i < P.nI; i++) {
      if (io.in == 0) Xl[i] = x[xoff + i];
      else if (io.in == 1) Xl[i] = io.b[io.perm[xoff + i]];
      else { double v = 0; for (int e = io.a_row[xoff + i]; e < io.a_row[xoff + i + 1]; e++) v += io.a_val[e] * io.x2[io.a_col[e]]; Xl[i] = v; }
    }
    double* X = Xl.data();
    const float* fac = subs[b].fac32;
    C.assign(std::max(P.contrib_size, 1), 0.0);
    Fv.assign(std::max(P.max_level_rows, 1), 0.0);
    for (int lev = 0; lev < P.nlev; lev++) {
      for (int it = P.fw_ptr[lev]; it < P.fw_ptr[lev + 1]; it++) {
        const FrontD& F = P.fronts[P.fw_items[it] >> 16];
        const int r = P.fw_items[it] & 0xffff;
        double v = r < F.w ? X[F.c0 + r] : 0.0;
        for (int t = P.asm_ptr[F.a_off + r]; t < P.asm_ptr[F.a_off + r + 1]; t++) v += C[P.asm_src[t]];
        if (r < F.w) Fv[F.lf_off + r] = v; else C[F.c_off + r - F.w] = v;
      }
      for (int it = P.fw_ptr[lev]; it < P.fw_ptr[lev + 1]; it++) {
        const FrontD& F = P.fronts[P.fw_items[it] >> 16];
        const int r = P.fw_items[it] & 0xffff, w = F.w, ld = F.w + F.ri;
        const float* Lp = fac + F.lp_off;
        const int kmax = r < w ? r : w;
        double a = 0;
        for (int k = 0; k < kmax; k++) {
          const double l = !P.packed ? Lp[r + (int64_t)ld * k] : (r < w ? Lp[packed_lower(w, r, k)] : Lp[packed_l21(w, F.ri, r - w, k)]);
          a += l * Fv[F.lf_off + k];
        }
        if (r < w) X[F.c0 + r] = Fv[F.lf_off + r] + a; else C[F.c_off + r - w] -= a;
      }
    }
    for (int lev = P.nlev - 1; lev >= 0; lev--) {
      out.assign(P.bw_ptr[lev + 1] - P.bw_ptr[lev], 0.0);
      for (int it = P.bw_ptr[lev]; it < P.bw_ptr[lev + 1]; it++) {
        const FrontD& F = P.fronts[P.bw_items[it] >> 16];
        const int i = P.bw_items[it] & 0xffff, w = F.w, ri = F.ri, ld = w + ri;
        const float* Lp = fac + F.lp_off;
        const float* Q = fac + F.q_off;
        double a = 0;
        for (int k = i; k < w; k++) a += (double)(P.packed ? Lp[packed_upper(w, ri, i, k)] : Lp[i + (int64_t)ld * k]) * X[F.c0 + k];
        for (int k = 0; k < ri; k++) a -= (double)Q[i + (int64_t)w * k] * X[P.fidx[F.idx_off + w + k]];
        out[it - P.bw_ptr[lev]] = a;
      }
      for (int it = P.bw_ptr[lev]; it < P.bw_ptr[lev + 1]; it++) {
        const FrontD& F = P.fronts[P.bw_items[it] >> 16];
        X[F.c0 + (P.bw_items[it] & 0xffff)] = out[it - P.bw_ptr[lev]];
      }
    }
    for (int i = 0; i < P.nI; i++) {
      if (io.out == 0) x[xoff + i] = X[i];
      else io.user[io.perm[xoff + i]] = io.z[xoff + i] - X[i];
    }
  }
}

void interior_solve_fused_mv_f32(int32_t nsub, const FusedSub* subs, const PlanD* plans, int32_t lds_doubles, int32_t, double* x,
                                 int64_t ldx, int nv) {
  for (int v = 0; v < nv; v++) interior_solve_fused_f32(nsub, subs, plans, lds_doubles, x + v * ldx, nullptr);
}

}  // namespace dev
}  // namespace hymls
