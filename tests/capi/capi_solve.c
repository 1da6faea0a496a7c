/* capi_solve.c -- the native Krylov solver of include/hymls_mi_solver.h from plain C (no Python, no torch): what a C /
 * Fortran / cgo host does to solve K x = b.  Laplace 16^3, 2-level preconditioner, right-preconditioned GMRES with host
 * buffers; exit 0 when the true relative residual |b - K x| / |b| is below 1e-8.
 * Build: gcc -O2 -I include tests/capi/capi_solve.c -o capi_solve -L hymls_amd -lhymls_mi -Wl,-rpath,$PWD/hymls_amd -lm */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "hymls_mi_solver.h"

int main(void) {
  const int n = 16;
  int64_t nrows = 0, nnz = 0;
  if (hymls_mi_generate_matrix(0, n, n, n, 0.0, 0.0, &nrows, &nnz, NULL, NULL, NULL)) return 2;
  int32_t* rp = malloc((nrows + 1) * sizeof *rp);
  int32_t* ci = malloc(nnz * sizeof *ci);
  double* va = malloc(nnz * sizeof *va);
  double *tv = malloc(nrows * sizeof *tv), *xe = malloc(nrows * sizeof *xe), *b = calloc(nrows, sizeof *b), *x = malloc(nrows * sizeof *x);
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
  unsigned s = 12345u;
  for (int64_t i = 0; i < nrows; i++) { s = s * 1664525u + 1013904223u; xe[i] = (double)(s >> 8) / (double)(1u << 24) * 2.0 - 1.0; }
  for (int64_t i = 0; i < nrows; i++) for (int32_t e = rp[i]; e < rp[i + 1]; e++) b[i] += va[e] * xe[ci[e]];
  hymls_mi_solver_params sp;
  hymls_mi_solver_default_params(&sp);
  sp.tol = 1e-10;
  sp.num_blocks = 50;
  hymls_mi_solver_t* S = NULL;
  if ((ierr = hymls_mi_solver_create(&S, h, &sp))) { printf("solver: %d %s\n", ierr, hymls_mi_solver_last_error(S)); return 5; }
  if ((ierr = hymls_mi_solver_solve(S, b, nrows, x, nrows, 1, 0))) { printf("solve: %d %s\n", ierr, hymls_mi_solver_last_error(S)); return 6; }
  double rr = 0.0, bb = 0.0;
  for (int64_t i = 0; i < nrows; i++) {
    double r = b[i];
    for (int32_t e = rp[i]; e < rp[i + 1]; e++) r -= va[e] * x[ci[e]];
    rr += r * r;
    bb += b[i] * b[i];
  }
  const double res = sqrt(rr / bb);
  printf("CAPI_SOLVE GMRES iterations %d achieved %.3e true relative residual %.3e\n", hymls_mi_solver_num_iters(S),
         hymls_mi_solver_achieved_tol(S), res);
  hymls_mi_solver_destroy(S);
  hymls_mi_destroy(h);
  free(rp); free(ci); free(va); free(tv); free(xe); free(b); free(x);
  return res < 1e-8 ? 0 : 1;
}
