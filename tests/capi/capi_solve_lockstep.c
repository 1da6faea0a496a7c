/* capi_solve_lockstep.c -- three right-hand sides in lock-step through the native Krylov solver of
 * include/hymls_mi_solver.h from plain C (no Python, no torch).  Laplace 16^3, 2-level preconditioner, right-preconditioned
 * GMRES(50) with host buffers: the three columns are solved at width 1 and at width 3; exit 0 when every column converged,
 * its true relative residual |b - K x| / |b| is below 1e-8, and the two solves agree bit for bit in X and in the
 * per-column results.
 * Build: gcc -O2 -I include tests/capi/capi_solve_lockstep.c -o capi_solve_lockstep -L hymls_amd -lhymls_mi
 *        -Wl,-rpath,$PWD/hymls_amd -lm */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "hymls_mi_solver.h"

int main(void) {
  const int n = 16, nvec = 3;
  int64_t nrows = 0, nnz = 0;
  if (hymls_mi_generate_matrix(0, n, n, n, 0.0, 0.0, &nrows, &nnz, NULL, NULL, NULL)) return 2;
  int32_t* rp = malloc((nrows + 1) * sizeof *rp);
  int32_t* ci = malloc(nnz * sizeof *ci);
  double* va = malloc(nnz * sizeof *va);
  double *tv = malloc(nrows * sizeof *tv), *xe = malloc(nrows * sizeof *xe), *b = calloc(nrows * nvec, sizeof *b);
  double *x1 = malloc(nrows * nvec * sizeof *x1), *x3 = malloc(nrows * nvec * sizeof *x3);
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
  /* column v: b = K x_ex with x_ex random, scaled by 10^-3v so that the columns differ */
  unsigned s = 12345u;
  for (int v = 0; v < nvec; v++) {
    for (int64_t i = 0; i < nrows; i++) { s = s * 1664525u + 1013904223u; xe[i] = ((double)(s >> 8) / (double)(1u << 24) * 2.0 - 1.0) * pow(10.0, -3 * v); }
    for (int64_t i = 0; i < nrows; i++) for (int32_t e = rp[i]; e < rp[i + 1]; e++) b[i + nrows * v] += va[e] * xe[ci[e]];
  }
  hymls_mi_solver_params sp;
  hymls_mi_solver_default_params(&sp);
  sp.tol = 1e-10;
  sp.num_blocks = 50;
  hymls_mi_solver_t* S = NULL;
  if ((ierr = hymls_mi_solver_create(&S, h, &sp))) { printf("solver: %d %s\n", ierr, hymls_mi_solver_last_error(S)); return 5; }
  int its[2][3], rst[2][3], conv[2][3];
  double tol[2][3];
  for (int pass = 0; pass < 2; pass++) {
    if (hymls_mi_solver_set_lockstep(S, pass ? 3 : 1) || hymls_mi_solver_lockstep(S) != (pass ? 3 : 1)) return 6;
    if ((ierr = hymls_mi_solver_solve(S, b, nrows, pass ? x3 : x1, nrows, nvec, 0))) { printf("solve: %d %s\n", ierr, hymls_mi_solver_last_error(S)); return 6; }
    for (int v = 0; v < nvec; v++)
      if (hymls_mi_solver_column_result(S, v, &its[pass][v], &tol[pass][v], &rst[pass][v], &conv[pass][v])) return 7;
    if (hymls_mi_solver_column_result(S, nvec, NULL, NULL, NULL, NULL) != -2) return 7;
  }
  if (hymls_mi_solver_set_lockstep(S, 5) != -2) return 8;
  int ok = memcmp(x1, x3, nrows * nvec * sizeof *x1) == 0;
  for (int v = 0; v < nvec; v++) {
    double rr = 0.0, bb = 0.0;
    for (int64_t i = 0; i < nrows; i++) {
      double r = b[i + nrows * v];
      for (int32_t e = rp[i]; e < rp[i + 1]; e++) r -= va[e] * x3[ci[e] + nrows * v];
      rr += r * r;
      bb += b[i + nrows * v] * b[i + nrows * v];
    }
    const double res = sqrt(rr / bb);
    printf("CAPI_SOLVE_LOCKSTEP column %d: iterations %d restarts %d achieved %.3e converged %d true relative residual %.3e\n", v,
           its[1][v], rst[1][v], tol[1][v], conv[1][v], res);
    ok = ok && res < 1e-8 && conv[1][v] && its[0][v] == its[1][v] && rst[0][v] == rst[1][v] && tol[0][v] == tol[1][v];
  }
  hymls_mi_solver_destroy(S);
  hymls_mi_destroy(h);
  free(rp); free(ci); free(va); free(tv); free(xe); free(b); free(x1); free(x3);
  return ok ? 0 : 1;
}
