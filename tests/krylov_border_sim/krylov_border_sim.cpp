// krylov_border_sim.cpp -- TEST-ONLY host version of dev::kry_border_product (hymls_amd/csrc/krylov.hpp; the product
// implements it in krylov_hip.hip).  Plain loops over host memory with the kernels' decomposition: the columns in chunks
// of KRY_BORDER_CHUNK, per chunk the grid of kry_row_grid(n) workgroups of 256 threads with thread t of workgroup b on
// the rows b * 256 + t + i * grid * 256, the fixed tree of the workgroup sums, and the one-workgroup second stage that
// sums the partials of a column as k_kry_reduce does and adds C s with l ascending.  Every other launcher and the timer
// come from tests/krylov_sim and tests/krylov_f32_sim, compiled unchanged into the same library.
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

void kry_border_product(int64_t n, int32_t m, const double* V, int64_t ldv, const double* W, int64_t ldw, const double* dC,
                        const double* z, double* y, const KryWork& ws) {
  if (n < 1 || m < 1 || m > KRY_BORDER_MAX || ldv < n || ldw < n) throw Error(-2, "border product: n >= 1, 1 <= m <= 32, ldv, ldw >= n");
  const int nb = kry_row_grid(n);
  for (int c0 = 0; c0 < m; c0 += KRY_BORDER_CHUNK) {
    const int mc = std::min(KRY_BORDER_CHUNK, m - c0);
    const double* Vc = V + (int64_t)c0 * ldv;
    const double* Wc = W + (int64_t)c0 * ldw;
    const double* s = z + n + c0;
    for (int b = 0; b < nb; b++) {
      double red[KRY_BORDER_CHUNK][256];
      for (int t = 0; t < 256; t++) {
        double acc[KRY_BORDER_CHUNK] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int64_t i = (int64_t)b * 256 + t; i < n; i += (int64_t)nb * 256) {
          const double xi = z[i];
          double sv = 0.0;
          for (int j = 0; j < mc; j++) {
            sv += Vc[(int64_t)j * ldv + i] * s[j];
            acc[j] += Wc[(int64_t)j * ldw + i] * xi;
          }
          y[i] = y[i] + sv;
        }
        for (int j = 0; j < mc; j++) red[j][t] = acc[j];
      }
      for (int j = 0; j < mc; j++) ws.part[(int64_t)b * m + c0 + j] = tree256(red[j]);
    }
  }
  for (int j = 0; j < m; j++) {
    double red[256];
    for (int t = 0; t < 256; t++) {
      double sum = 0.0;
      for (int b = t; b < nb; b += 256) sum += ws.part[(int64_t)b * m + j];
      red[t] = sum;
    }
    double v = tree256(red);
    if (dC)
      for (int l = 0; l < m; l++) v += dC[j + (int64_t)m * l] * z[n + l];
    y[n + j] = v;
  }
}

}  // namespace dev
}  // namespace hymls
