"""Records the fixtures of tests/test_solve_tails_gpu.py: the solutions of the cases of tests/solve_tails_cases.py through
the product library on the GPU, as float64 arrays under tests/golden/solve_tails/.

Run it on the MI355X at the commit whose bits are to be kept (after `make -C hymls_amd/csrc`):

    python tools/record_solve_tails.py [OUT_DIR]

The results depend on the order of the additions in the solve kernels and on the compiler's FMA contraction of
`a += l * f`; after a deliberate change of either (or a compiler that contracts differently) record them again and say so
in the commit."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import solve_tails_cases as st  # noqa: E402

if __name__ == "__main__":
    st.run_all(sys.argv[1] if len(sys.argv) > 1 else st.GOLDEN, "gpu", full=False)
