// krylov_f32_sim.cpp -- TEST-ONLY host versions of the float-basis launchers of hymls_amd/csrc/krylov.hpp (the product
// implements them in krylov_hip.hip).  Plain loops over host memory with the kernels' decomposition: the workgroup grid of
// kry_tile_grid_f32, the same tile and row order, the four quarter sums per row in pass B and the fixed trees of the block
// and column reductions, every product and sum FP64 on the widened float entry.  The FP64 launchers and the timer come
// from tests/krylov_sim/krylov_sim.cpp, compiled unchanged into the same library.
#include "krylov.hpp"
#include <cmath>

namespace hymls {
namespace dev {

namespace {
// the fixed tree of block_sum256 (krylov_hip.hip)
double tree256(double* red) {
  for (int st = 128; st > 0; st >>= 1)
    for (int t = 0; t < st; t++) red[t] += red[t + st];
  return red[0];
}
// stage two: column j of part[nb][k]
double reduce_col(const double* part, int nb, int k, int j) {
  double red[256];
  for (int t = 0; t < 256; t++) {
    double s = 0.0;
    for (int b = t; b < nb; b += 256) s += part[(int64_t)b * k + j];
    red[t] = s;
  }
  return tree256(red);
}
void check_k(int32_t k) { if (k < 1 || k > KRY_KMAX) throw Error(-2, "orthogonalisation: 1 <= k <= 256 columns"); }

template <bool UPD>
void tile_pass(int64_t n, int32_t k, const float* V, int64_t ldv, double* w, const KryWork& ws) {
  check_k(k);
  constexpr int T = KRY_TILE;
  const int nb = kry_tile_grid_f32(n, k);
  const int64_t ntiles = (n + T - 1) / T;
  std::vector<double> acc(k), ws_(T);
  for (int b = 0; b < nb; b++) {
    std::fill(acc.begin(), acc.end(), 0.0);
    for (int64_t tile = b; tile < ntiles; tile += nb) {
      const int64_t r0 = tile * T;
      const int rows = (int)std::min<int64_t>(T, n - r0);
      auto Vs = [&](int j, int r) { return r < rows ? (double)V[(int64_t)j * ldv + r0 + r] : 0.0; };
      for (int r = 0; r < T; r++) ws_[r] = r < rows ? w[r0 + r] : 0.0;
      if (UPD) {
        for (int r = 0; r < T; r++) {
          double q4[4];
          for (int q = 0; q < 4; q++) {
            double s = 0.0;
            for (int j = q; j < k; j += 4) s += Vs(j, r) * ws.h1[j];
            q4[q] = s;
          }
          const double v = ws_[r] - (((q4[0] + q4[1]) + q4[2]) + q4[3]);
          ws_[r] = v;
          if (r < rows) w[r0 + r] = v;
        }
      }
      for (int j = 0; j < k; j++)
        for (int r = 0; r < T; r++) acc[j] += Vs(j, r) * ws_[r];
    }
    for (int j = 0; j < k; j++) ws.part[(int64_t)b * k + j] = acc[j];
  }
  for (int j = 0; j < k; j++) {
    const double s = reduce_col(ws.part, nb, k, j);
    if (UPD) { ws.h2[j] = s; ws.out[j] = ws.h1[j] + s; }
    else ws.h1[j] = s;
  }
}
}  // namespace

void kry_pass_a(int64_t n, int32_t k, const float* V, int64_t ldv, const double* w, const KryWork& ws) {
  tile_pass<false>(n, k, V, ldv, const_cast<double*>(w), ws);
}
void kry_pass_b(int64_t n, int32_t k, const float* V, int64_t ldv, double* w, const KryWork& ws) {
  tile_pass<true>(n, k, V, ldv, w, ws);
}
// grid nb of 256 threads, thread t of block b takes rows b*256 + t + i*nb*256 (k_kry_rows<true, float>)
void kry_pass_c(int64_t n, int32_t k, const float* V, int64_t ldv, const double* w, double* dst, const KryWork& ws) {
  check_k(k);
  const int nb = kry_row_grid(n);
  for (int b = 0; b < nb; b++) {
    double red[256];
    for (int t = 0; t < 256; t++) {
      double ss = 0.0;
      for (int64_t i = (int64_t)b * 256 + t; i < n; i += (int64_t)nb * 256) {
        double s = 0.0;
        for (int j = 0; j < k; j++) s += (double)V[(int64_t)j * ldv + i] * ws.h2[j];
        const double x = w[i] - s;
        dst[i] = x;
        ss += x * x;
      }
      red[t] = ss;
    }
    ws.part[b] = tree256(red);
  }
  double red[256];
  for (int t = 0; t < 256; t++) { double s = 0.0; for (int b = t; b < nb; b += 256) s += ws.part[b]; red[t] = s; }
  const double ss = tree256(red);
  ws.out[k] = std::sqrt(ss);
  ws.out[k + 1] = ss;
}
void kry_update(int64_t n, int32_t k, const float* V, int64_t ldv, const double* y, double* x) {
  if (k < 1) return;
  check_k(k);
  for (int64_t i = 0; i < n; i++) {
    double s = 0.0;
    for (int j = 0; j < k; j++) s += (double)V[(int64_t)j * ldv + i] * y[j];
    x[i] = x[i] + s;
  }
}
void kry_widen(int64_t n, const float* v, double* t) { for (int64_t i = 0; i < n; i++) t[i] = (double)v[i]; }
void kry_round_div(int64_t n, const double* x, double s, float* y) { for (int64_t i = 0; i < n; i++) y[i] = (float)(x[i] / s); }
void kry_round_scale_by(int64_t n, const double* x, const double* d, float* y) {
  const double s = *d;
  const bool pos = s > 0.0;
  for (int64_t i = 0; i < n; i++) y[i] = (float)(pos ? x[i] / s : x[i]);
}

}  // namespace dev
}  // namespace hymls
