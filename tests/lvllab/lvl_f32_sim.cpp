// TEST-ONLY: plain-loop versions of the launchers FP32 storage of the merged level-solve panels adds to device.hpp
// (solve_fwd_tasks_mv_f32 / solve_bwd_tasks_mv_f32), next to tests/hostsim/device_sim.cpp and tests/f32_sim/f32_sim.cpp.
// They are the loops of device_sim.cpp's solve_fwd_tasks / solve_bwd_tasks with the panels read as float and widened: same
// loop order, same sums, so that on this simulator FP32 storage equals FP64 storage of float-rounded panels bit for bit,
// as the HIP kernels do among themselves.
#include "device.hpp"
#include <algorithm>
#include <utility>
#include <vector>

namespace hymls {
namespace dev {

// column v of a group: its own contribution scratch, cstride doubles behind that of column v - 1
static double* contrib_of(const LvlSub& S, int v) { return S.contrib + (int64_t)v * S.cstride; }

static void fwd_f32(const LvlTask* tasks, int32_t ntasks, const LvlSub* subs, const PlanD* plans, const double* x, double* y, int v) {
  // tasks of one level are independent: results first, then the writes (as the workgroups of one launch)
  std::vector<std::pair<double*, double>> writes;
  for (int t = 0; t < ntasks; t++) {
    const LvlTask& T = tasks[t];
    const LvlSub& S = subs[T.sub];
    const PlanD& P = plans[S.cls];
    const FrontD& F = P.fronts[T.front];
    const int w = F.w, rows = F.w + F.ri;
    const double* xb = x + S.xoff;
    double* yb = y + S.xoff;
    double* cb = contrib_of(S, v);
    std::vector<double> a(rows);
    for (int j = 0; j < rows; j++) {
      double val = j < w ? xb[F.c0 + j] : 0.0;
      for (int q = P.asm_ptr[F.a_off + j]; q < P.asm_ptr[F.a_off + j + 1]; q++) val += cb[P.asm_src[q]];
      a[j] = val;
    }
    const float* Lp = S.fac32 + F.lp_off;
    const int i0 = T.r0 < 0 ? 0 : T.r0, i1 = T.r0 < 0 ? rows : std::min(rows, T.r0 + 64);
    for (int i = i0; i < i1; i++) {
      double s = 0;
      for (int k = 0; k < std::min(i, w); k++) s += (double)Lp[i + (int64_t)rows * k] * a[k];
      if (i < w) writes.emplace_back(&yb[F.c0 + i], a[i] + s);
      else writes.emplace_back(&cb[F.c_off + i - w], a[i] - s);
    }
  }
  for (auto& wv : writes) *wv.first = wv.second;
}

static void bwd_f32(const LvlTask* tasks, int32_t ntasks, const LvlSub* subs, const PlanD* plans, const double* y, double* x) {
  std::vector<std::pair<double*, double>> writes;
  for (int t = 0; t < ntasks; t++) {
    const LvlTask& T = tasks[t];
    const LvlSub& S = subs[T.sub];
    const PlanD& P = plans[S.cls];
    const FrontD& F = P.fronts[T.front];
    const int w = F.w, ri = F.ri, ld = w + ri;
    double* xb = x + S.xoff;
    const double* yb = y + S.xoff;
    const float* Lp = S.fac32 + F.lp_off;
    const float* Q = S.fac32 + F.q_off;
    const int i0 = T.r0 < 0 ? 0 : T.r0, i1 = T.r0 < 0 ? w : std::min(w, T.r0 + 64);
    for (int i = i0; i < i1; i++) {
      double s = 0;
      for (int k = i; k < w; k++) s += (double)Lp[i + (int64_t)ld * k] * yb[F.c0 + k];
      for (int k = 0; k < ri; k++) s -= (double)Q[i + (int64_t)w * k] * xb[P.fidx[F.idx_off + w + k]];
      writes.emplace_back(&xb[F.c0 + i], s);
    }
  }
  for (auto& wv : writes) *wv.first = wv.second;
}

void solve_fwd_tasks_mv_f32(const LvlTask* tasks, int32_t ntasks, const LvlSub* subs, const PlanD* plans, int32_t,
                            const double* x, double* y, int64_t ld, int nv) {
  for (int v = 0; v < nv; v++) fwd_f32(tasks, ntasks, subs, plans, x + v * ld, y + v * ld, v);
}
void solve_bwd_tasks_mv_f32(const LvlTask* tasks, int32_t ntasks, const LvlSub* subs, const PlanD* plans, int32_t,
                            const double* y, double* x, int64_t ld, int nv) {
  for (int v = 0; v < nv; v++) bwd_f32(tasks, ntasks, subs, plans, y + v * ld, x + v * ld);
}

}  // namespace dev
}  // namespace hymls
