// krylov_shift_sim.cpp -- TEST-ONLY host version of dev::kry_shifted_product (hymls_amd/csrc/krylov.hpp; the product implements
// it in krylov_hip.hip: k_kry_shifted).  Plain loops over host memory with the kernel's lane decomposition: the L lanes of a
// row, L = spmv_lanes(n, nnzA_hint), each sum the entries rp[row] + lane, step L, ascending, and the partial sums are combined
// in the order of the __shfl_down tree (lane l adds the sum of lane l + off, off = L / 2, L / 4, ..., 1); lane 0 writes.
// Column by column: a column of an nv > 1 call therefore has the bits of its nv = 1 call, as in the kernel.  Every other
// launcher and the timer come from the older simulators, compiled unchanged into the same library.
#include "krylov.hpp"

namespace hymls {
namespace dev {

namespace {
// the sum of one row as the L lanes of k_kry_shifted form it
double lane_sum(int L, const int32_t* rp, const int32_t* col, const double* val, int64_t row, const double* x) {
  double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int e = rp[row + 1];
  for (int lane = 0; lane < L; lane++)
    for (int k = rp[row] + lane; k < e; k += L) s[lane] += val[k] * x[col[k]];
  for (int off = L / 2; off > 0; off >>= 1)
    for (int lane = 0; lane + off < L; lane++) s[lane] += s[lane + off];   // ascending: s[lane + off] is still the old value
  return s[0];
}
}  // namespace

void kry_shifted_product(int32_t n, const int32_t* rpA, const int32_t* colA, const double* valA, int64_t nnzA_hint,
                         const int32_t* rpB, const int32_t* colB, const double* valB, double a, double b, const double* X,
                         int64_t ldx, double* Y, int64_t ldy, int nv) {
  if (n < 1 || nv < 0 || ldx < n || ldy < n || !X || !Y || (a != 0.0 && (!rpA || !colA || !valA)) || (rpB && (!colB || !valB)))
    throw Error(-2, "shifted product: n >= 1, nv >= 0, ldx, ldy >= n, non-null X, Y and arrays of A (unless a = 0)");
  const int L = spmv_lanes(n, nnzA_hint);
  const bool useA = a != 0.0, useB = b != 0.0;
  for (int v = 0; v < nv; v++) {
    const double* x = X + (int64_t)v * ldx;
    double* y = Y + (int64_t)v * ldy;
    for (int64_t row = 0; row < n; row++) {
      const double sA = useA ? lane_sum(L, rpA, colA, valA, row, x) : 0.0;
      const double sB = !useB ? 0.0 : (rpB ? lane_sum(L, rpB, colB, valB, row, x) : x[row]);
      y[row] = !useB ? a * sA : (!useA ? b * sB : a * sA + b * sB);
    }
  }
}

}  // namespace dev
}  // namespace hymls
