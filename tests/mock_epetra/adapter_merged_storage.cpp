// The "Preconditioner" key "MI Merged Factor Storage" through include/hymls_mi_epetra.hpp: SetParameters reads it, the
// handle gets it at Initialize, and ApplyInverse gives the bits of a handle of the C ABI with
// hymls_mi_set_merged_factor_storage(h, 32).  Laplace 16^3 two-level; the test runs this with HYMLS_MI_NO_FUSED_SOLVE=1, so
// that the subdomains are solved on the merged route.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "hymls_mi_epetra.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
  Epetra_SerialComm comm;
  const int n = 16, N = n * n * n;
  Epetra_Map map(N, 0, comm);
  int64_t nrows = 0, nnz = 0;
  hymls_mi_generate_matrix(0, n, n, n, (double)n * n, 1.0, &nrows, &nnz, 0, 0, 0);
  std::vector<int32_t> rp(nrows + 1), ci(nnz);
  std::vector<double> va(nnz);
  hymls_mi_generate_matrix(0, n, n, n, (double)n * n, 1.0, &nrows, &nnz, rp.data(), ci.data(), va.data());
  Teuchos::RCP<Epetra_CrsMatrix> K = Teuchos::rcp(new Epetra_CrsMatrix(Copy, map, 7));
  for (int i = 0; i < nrows; i++) K->InsertGlobalValues(i, rp[i + 1] - rp[i], va.data() + rp[i], ci.data() + rp[i]);
  K->FillComplete();
  Epetra_MultiVector B(map, 2), Y32(map, 2), Y64(map, 2);
  unsigned s = 4711u;
  for (int v = 0; v < 2; v++) for (int i = 0; i < N; i++) { s = s * 1664525u + 1013904223u; B[v][i] = (double)(s >> 8) / (1u << 24) * 2.0 - 1.0; }
  double bytes[2] = {0, 0};
  for (int pass = 0; pass < 2; pass++) {
    Teuchos::RCP<Teuchos::ParameterList> params = Teuchos::rcp(new Teuchos::ParameterList());
    params->sublist("Problem").set("Equations", "Laplace").set("Dimension", 3).set("nx", n).set("ny", n).set("nz", n);
    params->sublist("Preconditioner").set("Separator Length", 4).set("Number of Levels", 1);
    if (pass == 0) params->sublist("Preconditioner").set("MI Merged Factor Storage", "single");
    Teuchos::RCP<HYMLS_MI::Preconditioner> P = Teuchos::rcp(new HYMLS_MI::Preconditioner(K, params));
    REQUIRE(P->Compute() == 0);
    REQUIRE(hymls_mi_merged_factor_storage(P->Handle()) == (pass == 0 ? 32 : 64) && hymls_mi_factor_storage(P->Handle()) == 64);
    bytes[pass] = hymls_mi_apply_bytes(P->Handle(), 10);
    REQUIRE(P->ApplyInverse(B, pass == 0 ? Y32 : Y64) == 0);
    if (pass == 1) {   // the same handle through the C ABI: 64 -> 32
      REQUIRE(hymls_mi_set_merged_factor_storage(P->Handle(), 32) == 0 && !P->IsComputed());
      REQUIRE(P->Compute() == 0);
      Epetra_MultiVector Y(map, 2);
      REQUIRE(P->ApplyInverse(B, Y) == 0);
      int differ64 = 0;
      for (int v = 0; v < 2; v++) for (int i = 0; i < N; i++) { REQUIRE(Y[v][i] == Y32[v][i]); differ64 += Y[v][i] != Y64[v][i]; }
      REQUIRE(differ64 > 0);
    }
    // an unknown value is refused by SetParameters
    params->sublist("Preconditioner").set("MI Merged Factor Storage", "half");
    REQUIRE(P->SetParameters(*params) == -2);
  }
  std::printf("merged panel bytes per ApplyInverse: %.0f (single), %.0f (double)\n", bytes[0], bytes[1]);
  REQUIRE(bytes[1] > 0 && bytes[0] == bytes[1] / 2);
  std::printf("ADAPTER_MERGED_STORAGE_OK\n");
  return 0;
}
