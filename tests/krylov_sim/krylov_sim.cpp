// krylov_sim.cpp -- TEST-ONLY host versions of the launchers of hymls_amd/csrc/krylov.hpp (the product implements them in
// krylov_hip.hip).  Plain loops over host memory that follow the kernels' decomposition: the same workgroup grid, the
// same tile and row order inside a workgroup, the same four quarter sums per row in pass B and the same fixed trees of
// the block and column reductions.  So the partial sums are added in the same order as on the GPU, and the solver takes
// the same iterations.
#include "krylov.hpp"
#include <chrono>
#include <cmath>
#include <cstring>

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
int vec_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, KRY_MAXGRID)); }
void check_k(int32_t k) { if (k < 1 || k > KRY_KMAX) throw Error(-2, "orthogonalisation: 1 <= k <= 256 columns"); }

template <bool UPD>
void tile_pass(int64_t n, int32_t k, const double* V, int64_t ldv, double* w, const KryWork& ws) {
  check_k(k);
  constexpr int T = KRY_TILE;
  const int nb = kry_tile_grid(n, k);
  const int64_t ntiles = (n + T - 1) / T;
  std::vector<double> acc(k), ws_(T);
  for (int b = 0; b < nb; b++) {
    std::fill(acc.begin(), acc.end(), 0.0);
    for (int64_t tile = b; tile < ntiles; tile += nb) {
      const int64_t r0 = tile * T;
      const int rows = (int)std::min<int64_t>(T, n - r0);
      auto Vs = [&](int j, int r) { return r < rows ? V[(int64_t)j * ldv + r0 + r] : 0.0; };
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

// one row-per-thread pass: grid nb of 256 threads, thread t of block b takes rows b*256 + t + i*nb*256;
// f(i) returns the row's value, whose square goes into the thread's sum; the block partials are the fixed trees
template <class F>
void row_pass_norm(int64_t n, int nb, double* part, F f) {
  for (int b = 0; b < nb; b++) {
    double red[256];
    for (int t = 0; t < 256; t++) {
      double ss = 0.0;
      for (int64_t i = (int64_t)b * 256 + t; i < n; i += (int64_t)nb * 256) ss += f(i);
      red[t] = ss;
    }
    part[b] = tree256(red);
  }
}
}  // namespace

void kry_pass_a(int64_t n, int32_t k, const double* V, int64_t ldv, const double* w, const KryWork& ws) {
  tile_pass<false>(n, k, V, ldv, const_cast<double*>(w), ws);
}
void kry_pass_b(int64_t n, int32_t k, const double* V, int64_t ldv, double* w, const KryWork& ws) {
  tile_pass<true>(n, k, V, ldv, w, ws);
}
void kry_pass_c(int64_t n, int32_t k, const double* V, int64_t ldv, const double* w, double* dst, const KryWork& ws) {
  check_k(k);
  const int nb = kry_row_grid(n);
  row_pass_norm(n, nb, ws.part, [&](int64_t i) {
    double s = 0.0;
    for (int j = 0; j < k; j++) s += V[(int64_t)j * ldv + i] * ws.h2[j];
    const double x = w[i] - s;
    dst[i] = x;
    return x * x;
  });
  double red[256];
  for (int t = 0; t < 256; t++) { double s = 0.0; for (int b = t; b < nb; b += 256) s += ws.part[b]; red[t] = s; }
  const double ss = tree256(red);
  ws.out[k] = std::sqrt(ss);
  ws.out[k + 1] = ss;
}
void kry_update(int64_t n, int32_t k, const double* V, int64_t ldv, const double* y, double* x) {
  if (k < 1) return;
  check_k(k);
  for (int64_t i = 0; i < n; i++) {
    double s = 0.0;
    for (int j = 0; j < k; j++) s += V[(int64_t)j * ldv + i] * y[j];
    x[i] = x[i] + s;
  }
}
void kry_scale_by(int64_t n, double* x, const double* d) {
  const double s = *d;
  if (!(s > 0.0)) return;
  for (int64_t i = 0; i < n; i++) x[i] = x[i] / s;
}
void kry_div(int64_t n, const double* x, double s, double* y) { for (int64_t i = 0; i < n; i++) y[i] = x[i] / s; }
void kry_sub(int64_t n, const double* b, const double* y, double* r) { for (int64_t i = 0; i < n; i++) r[i] = b[i] - y[i]; }
void kry_add(int64_t n, const double* x, double* y) { for (int64_t i = 0; i < n; i++) y[i] = y[i] + x[i]; }
void kry_dot(int64_t n, const double* x, const double* y, const KryWork& ws) {
  const int nb = vec_grid(n);
  for (int b = 0; b < nb; b++) {
    double red[256];
    for (int t = 0; t < 256; t++) {
      double s = 0.0;
      for (int64_t i = (int64_t)b * 256 + t; i < n; i += (int64_t)nb * 256) s += x[i] * y[i];
      red[t] = s;
    }
    ws.part[b] = tree256(red);
  }
  ws.out[0] = reduce_col(ws.part, nb, 1, 0);
}
void kry_cg_xr(int64_t n, double alpha, const double* p, const double* q, double* x, double* r, const KryWork& ws) {
  const int nb = vec_grid(n);
  row_pass_norm(n, nb, ws.part, [&](int64_t i) {
    x[i] = x[i] + alpha * p[i];
    const double v = r[i] - alpha * q[i];
    r[i] = v;
    return v * v;
  });
  ws.out[0] = reduce_col(ws.part, nb, 1, 0);
}
void kry_cg_p(int64_t n, double beta, const double* z, double* p) { for (int64_t i = 0; i < n; i++) p[i] = z[i] + beta * p[i]; }

struct KryTimer {
  std::vector<std::pair<int, std::chrono::steady_clock::time_point>> log;   // phase, or phase + 4 for an end
};
KryTimer* kry_timer_create() { return new KryTimer(); }
void kry_timer_destroy(KryTimer* t) { delete t; }
void kry_mark(KryTimer* t, int phase, bool begin) { t->log.emplace_back(begin ? phase : phase + 4, std::chrono::steady_clock::now()); }
void kry_collect(KryTimer* t, double* sum) {
  std::chrono::steady_clock::time_point open[4];
  bool have[4] = {false, false, false, false};
  for (auto& e : t->log) {
    if (e.first < 4) { open[e.first] = e.second; have[e.first] = true; }
    else if (have[e.first - 4]) sum[e.first - 4] += std::chrono::duration<double>(e.second - open[e.first - 4]).count();
  }
  t->log.clear();
}

}  // namespace dev
}  // namespace hymls
