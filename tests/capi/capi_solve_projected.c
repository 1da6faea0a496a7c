/* capi_solve_projected.c -- a solve with projection vectors (hymls_mi_solver_set_projection of include/hymls_mi_solver.h)
 * from plain C (no Python, no torch).  Laplace 16^3, 2-level preconditioner, V = the constant vector and the vector that
 * alternates in sign from row to row (both scaled to length 1, orthogonal because the row count is even), BV = V, the
 * right-hand side b = (I - V V') K (I - V V') x_ex.  Right-preconditioned GMRES with host buffers in the folded (default) and
 * in the literal form; exit 0 when in both the projected residual |(I - V V')(b - K x)| / |b| is below 1e-8, |V' x| is
 * below 1e-10 |x|, and the two forms took iteration counts within one of each other.
 * Build: gcc -O2 -I include tests/capi/capi_solve_projected.c -o capi_solve_projected -L hymls_amd -lhymls_mi
 *        -Wl,-rpath,$PWD/hymls_amd -lm */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "hymls_mi_solver.h"

static void project(int64_t n, const double* V, double* r) { /* r <- r - V (V' r), two columns */
  for (int j = 0; j < 2; j++) {
    double c = 0.0;
    for (int64_t i = 0; i < n; i++) c += V[i + n * j] * r[i];
    for (int64_t i = 0; i < n; i++) r[i] -= V[i + n * j] * c;
  }
}

int main(void) {
  const int n = 16, m = 2;
  int64_t nrows = 0, nnz = 0;
  if (hymls_mi_generate_matrix(0, n, n, n, 0.0, 0.0, &nrows, &nnz, NULL, NULL, NULL)) return 2;
  int32_t* rp = malloc((nrows + 1) * sizeof *rp);
  int32_t* ci = malloc(nnz * sizeof *ci);
  double* va = malloc(nnz * sizeof *va);
  double *tv = malloc(nrows * sizeof *tv), *xe = malloc(nrows * sizeof *xe), *b = calloc(nrows, sizeof *b), *x = malloc(nrows * sizeof *x);
  double *r = malloc(nrows * sizeof *r), *V = malloc(nrows * m * sizeof *V);
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
  for (int64_t i = 0; i < nrows; i++) {
    V[i] = 1.0 / sqrt((double)nrows);
    V[i + nrows] = (i % 2 ? -1.0 : 1.0) / sqrt((double)nrows);
  }
  unsigned s = 12345u;
  for (int64_t i = 0; i < nrows; i++) { s = s * 1664525u + 1013904223u; xe[i] = (double)(s >> 8) / (double)(1u << 24) * 2.0 - 1.0; }
  project(nrows, V, xe);
  for (int64_t i = 0; i < nrows; i++) for (int32_t e = rp[i]; e < rp[i + 1]; e++) b[i] += va[e] * xe[ci[e]];
  project(nrows, V, b);
  hymls_mi_solver_params sp;
  hymls_mi_solver_default_params(&sp);
  sp.tol = 1e-10;
  sp.num_blocks = 50;
  hymls_mi_solver_t* S = NULL;
  if ((ierr = hymls_mi_solver_create(&S, h, &sp))) { printf("solver: %d %s\n", ierr, hymls_mi_solver_last_error(S)); return 5; }
  if (hymls_mi_solver_set_projection(S, nrows, m, V, nrows - 1, NULL, 0, 0) != -2) { printf("a leading dimension below n was accepted\n"); return 7; }
  if ((ierr = hymls_mi_solver_set_projection(S, nrows, m, V, nrows, NULL, 0, 0))) { printf("set_projection: %d %s\n", ierr, hymls_mi_solver_last_error(S)); return 5; }
  if (hymls_mi_solver_num_projection(S) != m) return 7;
  int its[2] = {0, 0}, ok = 1;
  for (int form = 0; form < 2; form++) {
    if ((ierr = hymls_mi_solver_set_projection_form(S, form)) || (ierr = hymls_mi_solver_solve(S, b, nrows, x, nrows, 1, 0))) {
      printf("solve: %d %s\n", ierr, hymls_mi_solver_last_error(S));
      return 6;
    }
    double bb = 0.0, xx = 0.0, rr = 0.0, vx = 0.0;
    for (int64_t i = 0; i < nrows; i++) {
      r[i] = b[i];
      for (int32_t e = rp[i]; e < rp[i + 1]; e++) r[i] -= va[e] * x[ci[e]];
      bb += b[i] * b[i];
      xx += x[i] * x[i];
    }
    project(nrows, V, r);
    for (int64_t i = 0; i < nrows; i++) rr += r[i] * r[i];
    for (int j = 0; j < m; j++) {
      double c = 0.0;
      for (int64_t i = 0; i < nrows; i++) c += V[i + nrows * j] * x[i];
      if (fabs(c) > vx) vx = fabs(c);
    }
    its[form] = hymls_mi_solver_num_iters(S);
    const double res = sqrt(rr / bb);
    printf("CAPI_SOLVE_PROJECTED %s GMRES iterations %d achieved %.3e projected relative residual %.3e |V' x| / |x| %.3e\n",
           form ? "literal" : "folded", its[form], hymls_mi_solver_achieved_tol(S), res, vx / sqrt(xx));
    if (!(res < 1e-8) || !(vx <= 1e-10 * sqrt(xx))) ok = 0;
  }
  if (abs(its[0] - its[1]) > 1) ok = 0;
  hymls_mi_solver_destroy(S);
  hymls_mi_destroy(h);
  free(rp); free(ci); free(va); free(tv); free(xe); free(b); free(x); free(r); free(V);
  return ok ? 0 : 1;
}
