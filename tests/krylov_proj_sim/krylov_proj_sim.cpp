// krylov_proj_sim.cpp -- TEST-ONLY host versions of dev::kry_proj_coeffs, dev::kry_proj_update and dev::kry_oblique_project
// (hymls_amd/csrc/krylov.hpp; the product implements them in krylov_hip.hip).  Plain loops over host memory with the kernels'
// decomposition: the columns of Q in chunks of KRY_PROJ_CHUNK, per chunk the grid of kry_row_grid(n) workgroups of 256
// threads with thread t of workgroup b on the rows b * 256 + t + i * grid * 256, the fixed tree of the workgroup sums, the
// one-workgroup second stage that sums the partials of a column as k_kry_reduce does and applies G with l ascending, and the
// row update with j ascending and one subtraction.  Every other launcher and the timer come from the older simulators,
// compiled unchanged into the same library.
#include "krylov.hpp"

namespace hymls {
namespace dev {

namespace {
// the fixed tree of block_sum256 (krylov_hip.hip)
double tree256(double* red) {
  for (int st = 128; st > 0; st >>= 1)
    for (int t = 0; t < st; t++) red[t] += red[t + st];
  return red[0];
}
}  // namespace

void kry_proj_coeffs(int64_t n, int32_t m, const double* Q, int64_t ldq, const double* dG, const double* x, const KryWork& ws) {
  if (n < 1 || m < 1 || m > KRY_PROJ_MAX || ldq < n) throw Error(-2, "oblique projection: n >= 1, 1 <= m <= 32, ldq >= n");
  const int nb = kry_row_grid(n);
  for (int c0 = 0; c0 < m; c0 += KRY_PROJ_CHUNK) {
    const int mc = std::min(KRY_PROJ_CHUNK, m - c0);
    const double* Qc = Q + (int64_t)c0 * ldq;
    for (int b = 0; b < nb; b++) {
      double red[KRY_PROJ_CHUNK][256];
      for (int t = 0; t < 256; t++) {
        double acc[KRY_PROJ_CHUNK] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int64_t i = (int64_t)b * 256 + t; i < n; i += (int64_t)nb * 256) {
          const double xi = x[i];
          for (int j = 0; j < mc; j++) acc[j] += Qc[(int64_t)j * ldq + i] * xi;
        }
        for (int j = 0; j < mc; j++) red[j][t] = acc[j];
      }
      for (int j = 0; j < mc; j++) ws.part[(int64_t)b * m + c0 + j] = tree256(red[j]);
    }
  }
  double cs[KRY_PROJ_MAX];
  for (int j = 0; j < m; j++) {
    double red[256];
    for (int t = 0; t < 256; t++) {
      double sum = 0.0;
      for (int b = t; b < nb; b += 256) sum += ws.part[(int64_t)b * m + j];
      red[t] = sum;
    }
    cs[j] = tree256(red);
  }
  for (int j = 0; j < m; j++) {
    double v = cs[j];
    if (dG) {
      v = 0.0;
      for (int l = 0; l < m; l++) v += dG[j + (int64_t)m * l] * cs[l];
    }
    ws.h1[j] = v;
  }
}

void kry_proj_update(int64_t n, int32_t m, const double* P, int64_t ldp, const double* x, double* y, const KryWork& ws) {
  if (n < 1 || m < 1 || m > KRY_PROJ_MAX || ldp < n) throw Error(-2, "oblique projection: n >= 1, 1 <= m <= 32, ldp >= n");
  double ds[KRY_PROJ_MAX];
  for (int j = 0; j < m; j++) ds[j] = ws.h1[j];
  for (int64_t i = 0; i < n; i++) {
    double s = 0.0;
    for (int j = 0; j < m; j++) s += P[(int64_t)j * ldp + i] * ds[j];
    y[i] = x[i] - s;
  }
}

void kry_oblique_project(int64_t n, int32_t m, const double* Q, int64_t ldq, const double* dG, const double* P, int64_t ldp,
                         const double* x, double* y, const KryWork& ws) {
  if (ldp < n) throw Error(-2, "oblique projection: n >= 1, 1 <= m <= 32, ldp >= n");
  kry_proj_coeffs(n, m, Q, ldq, dG, x, ws);
  kry_proj_update(n, m, P, ldp, x, y, ws);
}

}  // namespace dev
}  // namespace hymls
