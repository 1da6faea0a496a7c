/* capi_solve_shifted.c -- a shifted solve (hymls_mi_solver_set_mass_matrix and hymls_mi_solver_set_shift of
 * include/hymls_mi_solver.h) from plain C (no Python, no torch).  Laplace 8^3, one-level preconditioner, B = a diagonal with
 * entries 1 and 0.5 and a zero on every fourth row, shift (1, sigma) with sigma = 0.1 times the diagonal entry of K.
 * Right-preconditioned GMRES with host buffers; exit 0 when the true residual |b - (K + sigma B) x| / |b|, formed on the host,
 * is below 1e-8, the shift reads back, and ApplyMass gives B b.
 * Build: gcc -O2 -I include tests/capi/capi_solve_shifted.c -o capi_solve_shifted -L hymls_amd -lhymls_mi
 *        -Wl,-rpath,$PWD/hymls_amd -lm */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "hymls_mi_solver.h"

int main(void) {
  const int n = 8;
  int64_t nrows = 0, nnz = 0;
  if (hymls_mi_generate_matrix(0, n, n, n, 0.0, 0.0, &nrows, &nnz, NULL, NULL, NULL)) return 2;
  int32_t* rp = malloc((nrows + 1) * sizeof *rp);
  int32_t* ci = malloc(nnz * sizeof *ci);
  double* va = malloc(nnz * sizeof *va);
  int32_t* brp = malloc((nrows + 1) * sizeof *brp);
  int32_t* bci = malloc(nrows * sizeof *bci);
  double* bva = malloc(nrows * sizeof *bva);
  double *tv = malloc(nrows * sizeof *tv), *b = malloc(nrows * sizeof *b), *x = malloc(nrows * sizeof *x), *y = malloc(nrows * sizeof *y);
  hymls_mi_generate_matrix(0, n, n, n, 0.0, 0.0, &nrows, &nnz, rp, ci, va);
  hymls_mi_generate_testvector(nrows, rp, ci, va, tv);
  hymls_mi_params p;
  hymls_mi_default_params(&p);
  p.nx = p.ny = p.nz = n; p.dim = 3; p.equations = 0; p.sx = 4; p.levels = 1;
  hymls_mi_t* h = NULL;
  int ierr = hymls_mi_create(&h, &p, 0);
  if (ierr) { printf("create: %d %s\n", ierr, hymls_mi_last_error(h)); return 3; }
  if ((ierr = hymls_mi_set_matrix_csr(h, nrows, rp, ci, va)) || (ierr = hymls_mi_set_testvector(h, tv)) || (ierr = hymls_mi_compute(h))) {
    printf("setup: %d %s\n", ierr, hymls_mi_last_error(h));
    return 4;
  }
  double diag = 0.0;
  for (int32_t e = rp[0]; e < rp[1]; e++) if (ci[e] == 0) diag = va[e];
  const double sigma = 0.1 * diag;
  for (int64_t i = 0; i < nrows; i++) { brp[i] = (int32_t)i; bci[i] = (int32_t)i; bva[i] = i % 4 == 3 ? 0.0 : (i % 2 ? 0.5 : 1.0); }
  brp[nrows] = (int32_t)nrows;
  unsigned s = 12345u;
  for (int64_t i = 0; i < nrows; i++) { s = s * 1664525u + 1013904223u; b[i] = (double)(s >> 8) / (double)(1u << 24) * 2.0 - 1.0; }
  hymls_mi_solver_params sp;
  hymls_mi_solver_default_params(&sp);
  sp.tol = 1e-10;
  hymls_mi_solver_t* S = NULL;
  if ((ierr = hymls_mi_solver_create(&S, h, &sp))) { printf("solver: %d %s\n", ierr, hymls_mi_solver_last_error(S)); return 5; }
  bci[3] = (int32_t)nrows;
  if (hymls_mi_solver_set_mass_matrix(S, nrows, brp, bci, bva, 0) != -2) { printf("a column outside [0, n) was accepted\n"); return 7; }
  bci[3] = 3;
  if (hymls_mi_solver_set_shift(S, 0.0, 0.0) != -2) { printf("the zero operator was accepted\n"); return 7; }
  if ((ierr = hymls_mi_solver_set_mass_matrix(S, nrows, brp, bci, bva, 0)) || (ierr = hymls_mi_solver_set_shift(S, 1.0, sigma))) {
    printf("set_mass_matrix / set_shift: %d %s\n", ierr, hymls_mi_solver_last_error(S));
    return 5;
  }
  double sa = 0.0, sb = 0.0;
  if (hymls_mi_solver_shift(S, &sa, &sb) || sa != 1.0 || sb != sigma) return 7;
  if ((ierr = hymls_mi_solver_apply_mass(S, b, nrows, y, nrows, 1, 0))) { printf("apply_mass: %d %s\n", ierr, hymls_mi_solver_last_error(S)); return 6; }
  int ok = 1;
  for (int64_t i = 0; i < nrows; i++) if (y[i] != bva[i] * b[i]) ok = 0;
  if ((ierr = hymls_mi_solver_solve(S, b, nrows, x, nrows, 1, 0))) { printf("solve: %d %s\n", ierr, hymls_mi_solver_last_error(S)); return 6; }
  double bb = 0.0, rr = 0.0;
  for (int64_t i = 0; i < nrows; i++) {
    double r = b[i] - sigma * bva[i] * x[i];
    for (int32_t e = rp[i]; e < rp[i + 1]; e++) r -= va[e] * x[ci[e]];
    bb += b[i] * b[i];
    rr += r * r;
  }
  const double res = sqrt(rr / bb);
  printf("CAPI_SOLVE_SHIFTED GMRES shift (1, %g) iterations %d achieved %.3e true relative residual %.3e\n", sigma,
         hymls_mi_solver_num_iters(S), hymls_mi_solver_achieved_tol(S), res);
  if (!(res < 1e-8)) ok = 0;
  hymls_mi_solver_destroy(S);
  hymls_mi_destroy(h);
  free(rp); free(ci); free(va); free(brp); free(bci); free(bva); free(tv); free(b); free(x); free(y);
  return ok ? 0 : 1;
}
