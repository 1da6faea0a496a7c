/* capi_solve_bordered.c -- a bordered solve of include/hymls_mi_solver.h from plain C (no Python, no torch): the problem of
 * the reference's stokes4_3D.xml.  Stokes-C 8^3, periodic in x, y and z, Skew Cartesian, separator length 4, "Number of
 * Levels" 0, no pinned pressure; the matrix is singular, and its four constant null vectors (one per degree of freedom,
 * scaled by 1 / sqrt(cells)) are the border of the operator and of the preconditioner.  Right-preconditioned GMRES with host
 * buffers through hymls_mi_solver_solve_bordered; exit 0 when it took 1 iteration and the true relative residual
 * |b - K x - V s| / |b| and the relative error are below 5e-11 (the targets of that file).
 * Build: gcc -O2 -I include tests/capi/capi_solve_bordered.c -o capi_solve_bordered -L hymls_amd -lhymls_mi
 *        -Wl,-rpath,$PWD/hymls_amd -lm */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "hymls_mi_solver.h"

int main(void) {
  const int n = 8, dof = 4, m = 4;
  const int64_t nrows = (int64_t)n * n * n * dof;
  int64_t nnz = 0;
  if (hymls_mi_generate_problem_periodic(1, n, n, n, (double)(n * n), 1.0, 0.0, 7, nrows, NULL, &nnz, NULL, NULL, NULL)) return 2;
  int32_t* rp = malloc((nrows + 1) * sizeof *rp);
  int32_t* ci = malloc(nnz * sizeof *ci);
  double* va = malloc(nnz * sizeof *va);
  double *tv = malloc(nrows * sizeof *tv), *xe = malloc(nrows * sizeof *xe), *b = calloc(nrows, sizeof *b), *x = malloc(nrows * sizeof *x);
  double* V = calloc(nrows * m, sizeof *V);
  if (hymls_mi_generate_problem_periodic(1, n, n, n, (double)(n * n), 1.0, 0.0, 7, nrows, NULL, &nnz, rp, ci, va)) return 2;
  hymls_mi_generate_testvector(nrows, rp, ci, va, tv);
  hymls_mi_params p;
  hymls_mi_default_params(&p);
  p.nx = p.ny = p.nz = n; p.dim = 3; p.equations = 1; p.dof = dof; p.sx = 4; p.levels = 0; p.partitioner = 1;
  p.fix_pressure_level = 0;
  p.periodic[0] = p.periodic[1] = p.periodic[2] = 1;
  hymls_mi_t* h = NULL;
  int ierr = hymls_mi_create(&h, &p, 0);
  if (ierr) { printf("create: %d %s\n", ierr, hymls_mi_last_error(h)); return 3; }
  if ((ierr = hymls_mi_set_matrix_csr(h, nrows, rp, ci, va)) || (ierr = hymls_mi_set_testvector(h, tv)) || (ierr = hymls_mi_initialize(h))) {
    printf("setup: %d %s\n", ierr, hymls_mi_last_error(h));
    return 4;
  }
  for (int d = 0; d < dof; d++)
    for (int64_t i = d; i < nrows; i += dof) V[i + nrows * d] = 1.0 / sqrt((double)(nrows / dof));
  if ((ierr = hymls_mi_set_border(h, m, V, nrows, NULL, nrows, NULL)) || (ierr = hymls_mi_compute(h))) {
    printf("border: %d %s\n", ierr, hymls_mi_last_error(h));
    return 4;
  }
  /* x_ex random with the null space projected out, b = K x_ex (the driver of the reference, src/main.cpp:386-409) */
  unsigned s = 12345u;
  for (int64_t i = 0; i < nrows; i++) { s = s * 1664525u + 1013904223u; xe[i] = (double)(s >> 8) / (double)(1u << 24) * 2.0 - 1.0; }
  for (int d = 0; d < dof; d++) {
    double c = 0.0;
    for (int64_t i = d; i < nrows; i += dof) c += V[i + nrows * d] * xe[i];
    for (int64_t i = d; i < nrows; i += dof) xe[i] -= V[i + nrows * d] * c;
  }
  for (int64_t i = 0; i < nrows; i++) for (int32_t e = rp[i]; e < rp[i + 1]; e++) b[i] += va[e] * xe[ci[e]];
  hymls_mi_solver_params sp;
  hymls_mi_solver_default_params(&sp);
  sp.tol = 1e-10;
  sp.max_iters = 5;
  sp.max_restarts = 1;
  hymls_mi_solver_t* S = NULL;
  double sb[4] = {0, 0, 0, 0};
  if ((ierr = hymls_mi_solver_create(&S, h, &sp))) { printf("solver: %d %s\n", ierr, hymls_mi_solver_last_error(S)); return 5; }
  if ((ierr = hymls_mi_solver_solve_bordered(S, b, NULL, x, sb, 0))) { printf("solve: %d %s\n", ierr, hymls_mi_solver_last_error(S)); return 6; }
  if (hymls_mi_solver_solve(S, b, nrows, x, nrows, 1, 0) != -2) { printf("the plain solve accepted a bordered handle\n"); return 7; }
  if ((ierr = hymls_mi_solver_solve_bordered(S, b, NULL, x, sb, 0))) { printf("solve: %d %s\n", ierr, hymls_mi_solver_last_error(S)); return 6; }
  double rr = 0.0, bb = 0.0, ee = 0.0, xx = 0.0;
  for (int64_t i = 0; i < nrows; i++) {
    double r = b[i];
    for (int32_t e = rp[i]; e < rp[i + 1]; e++) r -= va[e] * x[ci[e]];
    for (int j = 0; j < m; j++) r -= V[i + nrows * j] * sb[j];
    rr += r * r;
    bb += b[i] * b[i];
    ee += (x[i] - xe[i]) * (x[i] - xe[i]);
    xx += xe[i] * xe[i];
  }
  const double res = sqrt(rr / bb), err = sqrt(ee / xx);
  const int its = hymls_mi_solver_num_iters(S);
  printf("CAPI_SOLVE_BORDERED GMRES iterations %d achieved %.3e true relative residual %.3e relative error %.3e\n", its,
         hymls_mi_solver_achieved_tol(S), res, err);
  hymls_mi_solver_destroy(S);
  hymls_mi_destroy(h);
  free(rp); free(ci); free(va); free(tv); free(xe); free(b); free(x); free(V);
  return its == 1 && res <= 5e-11 && err <= 5e-11 ? 0 : 1;
}
