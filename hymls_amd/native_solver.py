"""ctypes binding of include/hymls_mi_solver.h: the native Krylov solver (GMRES or CG with the HYMLS preconditioner,
the reference's ``HYMLS::BaseSolver``) that lives in the library itself, next to the Python ``hymls_amd.Solver``.

``NativeSolver(P, params)`` reads the same parameter dict as ``Solver`` ({"Solver": {...}} or the sublist itself) and
has the same methods; K is the matrix of the computed preconditioner P and the preconditioner is P's ApplyInverse.
The solver symbols are bound from ``P._lib`` when the first NativeSolver is made, so libraries without them still
load through ``hymls_amd.load_library``.

``NativeBorderedSolver(P, params)`` is the native counterpart of ``hymls_amd.BorderedSolver``: the bordered system
[K V; W' C] [x; s] = [b; t] with the border of P (hymls_mi_solver_solve_bordered).  Its two symbols are bound from a table
of their own when the first NativeBorderedSolver or ``border_product`` is used.

``NativeSolver.setProjectionVectors(V, W)`` is the reference's ``BaseSolver::setProjectionVectors``: the solve then runs in
the complement of a small space (hymls_mi_solver_set_projection).  Its symbols are bound from a third table.

``NativeSolver.SetMassMatrix(B)``, ``ApplyMass(X)`` and ``setShift(a, b)`` are the reference's methods of those names: with a
shift the solve is with a K + b B (hymls_mi_solver_set_shift, the reference's ``HYMLS::ShiftedOperator``).  A fourth table.
"""
import ctypes as C

import numpy as np

from .api import HymlsError

METHODS = {"GMRES": 0, "CG": 1}
STARTS = {"Zero": 0, "Random": 1, "Previous": 2}
BASIS_STORAGE = {"double": 64, "single": 32}    # "MI Basis Storage" (hymls_mi_solver_set_basis_storage)


class _SolverParams(C.Structure):
    _fields_ = [("method", C.c_int32), ("initial_vector", C.c_int32), ("right", C.c_int32), ("tol", C.c_double),
                ("max_iters", C.c_int32), ("num_blocks", C.c_int32), ("max_restarts", C.c_int32), ("seed", C.c_uint64)]


_SIG = {
    "hymls_mi_solver_default_params": (None, [C.POINTER(_SolverParams)]),
    "hymls_mi_solver_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(_SolverParams)]),
    "hymls_mi_solver_set_params": (C.c_int, [C.c_void_p, C.POINTER(_SolverParams)]),
    "hymls_mi_solver_set_tolerance": (C.c_int, [C.c_void_p, C.c_double]),
    "hymls_mi_solver_solve": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int]),
    "hymls_mi_solver_num_iters": (C.c_int, [C.c_void_p]),
    "hymls_mi_solver_achieved_tol": (C.c_double, [C.c_void_p]),
    "hymls_mi_solver_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "hymls_mi_solver_seconds": (C.c_double, [C.c_void_p, C.c_int]),
    "hymls_mi_orthogonalize": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                         C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "hymls_mi_solver_num_restarts": (C.c_int, [C.c_void_p]),
    "hymls_mi_solver_set_basis_storage": (C.c_int, [C.c_void_p, C.c_int]),
    "hymls_mi_solver_basis_storage": (C.c_int, [C.c_void_p]),
    "hymls_mi_orthogonalize_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                             C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "hymls_mi_solver_last_error": (C.c_char_p, [C.c_void_p]),
    "hymls_mi_solver_destroy": (None, [C.c_void_p]),
}


# bound apart from _SIG (bind_bordered): a library may have the solver without the bordered entries
_SIG_BORDERED = {
    "hymls_mi_solver_solve_bordered": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "hymls_mi_border_product": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
}


# bound apart from _SIG as well (bind_lockstep): lock-step columns and their building blocks
_SIG_LOCKSTEP = {
    "hymls_mi_solver_set_lockstep": (C.c_int, [C.c_void_p, C.c_int]),
    "hymls_mi_solver_lockstep": (C.c_int, [C.c_void_p]),
    "hymls_mi_solver_column_result": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double),
                                                C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hymls_mi_matvec_mv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int]),
    "hymls_mi_orthogonalize_mv": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                            C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "hymls_mi_orthogonalize_mv_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                                C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                C.c_void_p]),
}
MAX_LOCKSTEP = 4


# bound apart from _SIG as well (bind_projection): projection vectors and their building blocks
_SIG_PROJECTION = {
    "hymls_mi_solver_set_projection": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                 C.c_int]),
    "hymls_mi_solver_num_projection": (C.c_int, [C.c_void_p]),
    "hymls_mi_solver_set_projection_form": (C.c_int, [C.c_void_p, C.c_int]),
    "hymls_mi_solver_apply_projected": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "hymls_mi_oblique_project": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                           C.c_int64, C.c_void_p, C.c_void_p]),
}
MAX_PROJECTION = 32
PROJECTION_FORMS = {"folded": 0, "literal": 1}    # "MI Projection Form" (hymls_mi_solver_set_projection_form)


# bound apart from _SIG as well (bind_shifted): mass matrix, shift and the shifted product
_SIG_SHIFTED = {
    "hymls_mi_solver_set_mass_matrix": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "hymls_mi_solver_apply_mass": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int]),
    "hymls_mi_solver_set_shift": (C.c_int, [C.c_void_p, C.c_double, C.c_double]),
    "hymls_mi_solver_shift": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "hymls_mi_shifted_product": (C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                           C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                           C.c_int64, C.c_int]),
}


def bind_shifted(lib):
    """declare the mass matrix and shift symbols on a loaded library (once); AttributeError if it lacks one"""
    if not getattr(lib, "_hymls_shifted_bound", False):
        for name, (res, args) in _SIG_SHIFTED.items():
            f = getattr(lib, name)
            f.restype = res
            f.argtypes = args
        lib._hymls_shifted_bound = True
    return lib


def bind_projection(lib):
    """declare the projection symbols on a loaded library (once); AttributeError if it lacks one"""
    if not getattr(lib, "_hymls_projection_bound", False):
        for name, (res, args) in _SIG_PROJECTION.items():
            f = getattr(lib, name)
            f.restype = res
            f.argtypes = args
        lib._hymls_projection_bound = True
    return lib


def bind_lockstep(lib):
    """declare the lock-step symbols on a loaded library (once); AttributeError if it lacks one"""
    if not getattr(lib, "_hymls_lockstep_bound", False):
        for name, (res, args) in _SIG_LOCKSTEP.items():
            f = getattr(lib, name)
            f.restype = res
            f.argtypes = args
        lib._hymls_lockstep_bound = True
    return lib


def bind_bordered(lib):
    """declare the two bordered symbols on a loaded library (once); AttributeError if it lacks one"""
    if not getattr(lib, "_hymls_bordered_bound", False):
        for name, (res, args) in _SIG_BORDERED.items():
            f = getattr(lib, name)
            f.restype = res
            f.argtypes = args
        lib._hymls_bordered_bound = True
    return lib


def bind_solver(lib):
    """declare the solver symbols on a loaded library (once); AttributeError if it lacks one"""
    if not getattr(lib, "_hymls_solver_bound", False):
        for name, (res, args) in _SIG.items():
            f = getattr(lib, name)
            f.restype = res
            f.argtypes = args
        lib._hymls_solver_bound = True
    return lib


def solver_params(params):
    """the C parameter struct from a hymls_amd.Solver parameter dict"""
    sol = params.get("Solver", params)
    it = sol.get("Iterative Solver", {})
    p = _SolverParams()
    method = sol.get("Krylov Method", "GMRES")
    if method not in METHODS:
        raise ValueError("Krylov Method must be GMRES or CG")
    start = sol.get("Initial Vector", "Zero")
    if start not in STARTS:
        raise ValueError("Initial Vector must be Zero, Random or Previous")
    lor = sol.get("Left or Right Preconditioning", "Right")
    if lor not in ("Left", "Right"):
        raise ValueError("Left or Right Preconditioning must be Left or Right")
    p.method, p.initial_vector, p.right = METHODS[method], STARTS[start], int(lor == "Right")
    p.tol = float(it.get("Convergence Tolerance", 1e-8))
    p.max_iters = int(it.get("Maximum Iterations", 500))
    p.num_blocks = int(it.get("Num Blocks", 250))
    p.max_restarts = int(it.get("Maximum Restarts", 20))
    p.seed = int(sol.get("Random Seed", 1234))
    return p


def basis_bits(params):
    """"MI Basis Storage" of the Solver sublist ("double", the default, or "single") as the bits of a basis entry"""
    storage = params.get("Solver", params).get("MI Basis Storage", "double")
    if storage not in BASIS_STORAGE:
        raise ValueError("MI Basis Storage must be double or single")
    return BASIS_STORAGE[storage]


def lockstep_columns(params):
    """"MI Lockstep Columns" of the Solver sublist (1, the default, to 4): the columns of a multi-column solve that advance
    together (hymls_mi_solver_set_lockstep)"""
    width = int(params.get("Solver", params).get("MI Lockstep Columns", 1))
    if not 1 <= width <= MAX_LOCKSTEP:
        raise ValueError("MI Lockstep Columns must lie in 1..%d" % MAX_LOCKSTEP)
    return width


def projection_form(params):
    """"MI Projection Form" of the Solver sublist: "folded" (one ApplyInverse per application of the projected
    preconditioner) or "literal" (the reference's two); None when the key is absent"""
    form = params.get("Solver", params).get("MI Projection Form")
    if form is not None and form not in PROJECTION_FORMS:
        raise ValueError("MI Projection Form must be folded or literal")
    return form


def _colmajor(A):
    """(pointer, leading dimension, on_device, keep-alive) of an (n, m) numpy array or torch tensor as a column-major block"""
    if hasattr(A, "data_ptr"):
        At = A.reshape(A.shape[0], -1).t().contiguous()       # (m, n) row-major: the columns one after the other
        return At.data_ptr(), At.shape[1], 1, At
    Ac = np.asfortranarray(np.asarray(A, dtype=np.float64).reshape(np.shape(A)[0], -1))
    return Ac.ctypes.data, Ac.shape[0], 0, Ac


class NativeSolver:
    """K x = b with the library's own Krylov loop; P: a computed hymls_amd.Preconditioner (sharded or not)."""

    def __init__(self, P, params=None):
        self._P = P
        self._lib = bind_solver(P._lib)
        self._s = C.c_void_p()
        self._params = solver_params(params or {})
        bits = basis_bits(params or {})
        width = lockstep_columns(params or {})
        form = projection_form(params or {})
        ierr = self._lib.hymls_mi_solver_create(C.byref(self._s), P._h, C.byref(self._params))
        if not ierr:
            ierr = self._lib.hymls_mi_solver_set_basis_storage(self._s, bits)
        if not ierr and width != 1:
            ierr = bind_lockstep(self._lib).hymls_mi_solver_set_lockstep(self._s, width)
        if not ierr and form is not None:
            ierr = bind_projection(self._lib).hymls_mi_solver_set_projection_form(self._s, PROJECTION_FORMS[form])
        if ierr:
            msg = self._lib.hymls_mi_solver_last_error(self._s).decode() if self._s else "create failed"
            self.close()
            raise HymlsError(ierr, msg)

    def _check(self, ierr):
        if ierr:
            raise HymlsError(ierr, self._lib.hymls_mi_solver_last_error(self._s).decode())

    # --- reference API (as hymls_amd.Solver)
    def setParameterList(self, params):
        """replaces every parameter; a "Previous" start still uses the last solution"""
        p = solver_params(params)
        bits = basis_bits(params)
        self._check(self._lib.hymls_mi_solver_set_params(self._s, C.byref(p)))
        self._params = p
        self._check(self._lib.hymls_mi_solver_set_basis_storage(self._s, bits))
        width = lockstep_columns(params)
        if width != 1 or getattr(self._lib, "_hymls_lockstep_bound", False):
            self._check(bind_lockstep(self._lib).hymls_mi_solver_set_lockstep(self._s, width))
        form = projection_form(params)
        if form is not None:
            self._check(bind_projection(self._lib).hymls_mi_solver_set_projection_form(self._s, PROJECTION_FORMS[form]))

    def setProjectionVectors(self, V, W=None):
        """the solve works in the complement of span(V): operator (I - W V') K (I - V W'), preconditioner
        M^-1 (I - W H^-1 W' M^-1) with H = W' M^-1 W, projected start vector (the reference's setProjectionVectors; W is
        its BV, None means W = V).  V, W: (n, m) numpy arrays or torch device tensors with V' W = I, m <= 32; the solver
        keeps device copies.  V=None removes the projection.  Pass right-hand sides with V' b = 0."""
        lib = bind_projection(self._lib)
        if V is None:
            self._check(lib.hymls_mi_solver_set_projection(self._s, self._P._n, 0, None, 0, None, 0, 0))
            return
        vp, ldv, dev_v, keep_v = _colmajor(V)
        m = keep_v.shape[0] if dev_v else keep_v.shape[1]
        wp, ldw, dev_w, keep_w = (None, 0, dev_v, None) if W is None else _colmajor(W)
        if dev_w != dev_v or (keep_w is not None and tuple(keep_w.shape) != tuple(keep_v.shape)):
            raise ValueError("V and W must be of one kind (numpy or torch) and one shape")
        self._check(lib.hymls_mi_solver_set_projection(self._s, ldv, m, vp, ldv, wp, ldw, dev_v))

    def getNumProjection(self):
        return bind_projection(self._lib).hymls_mi_solver_num_projection(self._s)

    def applyProjected(self, which, X):
        """one vector through the projected operator (which = 0) or the projected preconditioner (which = 1) as the solve
        applies them (hymls_mi_solver_apply_projected); X: torch tensor on the device or numpy array of n entries"""
        lib = bind_projection(self._lib)
        if hasattr(X, "data_ptr"):
            Y = X.new_empty(X.shape)
            self._check(lib.hymls_mi_solver_apply_projected(self._s, which, X.contiguous().data_ptr(), Y.data_ptr(), 1))
            return Y
        Xc = np.ascontiguousarray(X, dtype=np.float64)
        Y = np.empty_like(Xc)
        self._check(lib.hymls_mi_solver_apply_projected(self._s, which, Xc.ctypes.data, Y.ctypes.data, 0))
        return Y

    def SetMassMatrix(self, B):
        """the mass matrix B of the shifted operator a K + b B (the reference's SetMassMatrix; hymls_mi_solver_set_mass_matrix):
        a scipy sparse matrix of the size of K, converted to CSR with 32-bit indices as it is stored (duplicates add up);
        the solver keeps a device copy.  B=None removes it, and the identity is used."""
        lib = bind_shifted(self._lib)
        if B is None:
            self._check(lib.hymls_mi_solver_set_mass_matrix(self._s, self._P._n, None, None, None, 0))
            return
        Bc = B.tocsr()
        if Bc.shape[0] != Bc.shape[1]:
            raise ValueError("the mass matrix must be square")
        if Bc.nnz >= 2 ** 31:
            raise ValueError("the mass matrix has 2^31 or more entries")
        rp = np.ascontiguousarray(Bc.indptr, dtype=np.int32)
        ci = np.ascontiguousarray(Bc.indices, dtype=np.int32)
        va = np.ascontiguousarray(Bc.data, dtype=np.float64)
        self._check(lib.hymls_mi_solver_set_mass_matrix(self._s, Bc.shape[0], rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0))

    def ApplyMass(self, X):
        """B X (the reference's ApplyMass; X itself without a mass matrix).  X: torch tensor on the device, (n,) or (nvec, n),
        or numpy array in host memory, (n,) or (n, nvec), as in ApplyInverse"""
        lib = bind_shifted(self._lib)
        n = self._P._n
        if hasattr(X, "data_ptr"):
            Xc = X.contiguous()
            assert Xc.shape[-1] == n
            Y = Xc.new_empty(Xc.shape)
            nvec = 1 if Xc.dim() == 1 else Xc.shape[0]
            self._check(lib.hymls_mi_solver_apply_mass(self._s, Xc.data_ptr(), n, Y.data_ptr(), n, nvec, 1))
            return Y
        Xc = np.asfortranarray(np.asarray(X, dtype=np.float64))
        assert Xc.shape[0] == n
        Y = np.empty_like(Xc, order="F")
        nvec = 1 if Xc.ndim == 1 else Xc.shape[1]
        self._check(lib.hymls_mi_solver_apply_mass(self._s, Xc.ctypes.data, n, Y.ctypes.data, n, nvec, 0))
        return Y

    def setShift(self, a, b):
        """the solve is with a K + b B instead of K (the reference's setShift; B: SetMassMatrix, else the identity); the
        preconditioner stays that of K.  (1, 0), the default, is the plain solve"""
        self._check(bind_shifted(self._lib).hymls_mi_solver_set_shift(self._s, float(a), float(b)))

    def getShift(self):
        a, b = C.c_double(), C.c_double()
        self._check(bind_shifted(self._lib).hymls_mi_solver_shift(self._s, C.byref(a), C.byref(b)))
        return a.value, b.value

    def SetTolerance(self, tol):
        self._check(self._lib.hymls_mi_solver_set_tolerance(self._s, float(tol)))

    def getNumIter(self):
        return self._lib.hymls_mi_solver_num_iters(self._s)

    def achievedTol(self):
        return self._lib.hymls_mi_solver_achieved_tol(self._s)

    def getNumRestarts(self):
        """Arnoldi cycles of the last column after its first one (with "MI Basis Storage" = "single" the cycles that
        were ended early count too)"""
        return self._lib.hymls_mi_solver_num_restarts(self._s)

    def getBasisStorage(self):
        return {v: k for k, v in BASIS_STORAGE.items()}[self._lib.hymls_mi_solver_basis_storage(self._s)]

    def getLockstep(self):
        """the columns of a multi-column solve that advance together ("MI Lockstep Columns")"""
        return bind_lockstep(self._lib).hymls_mi_solver_lockstep(self._s)

    def getColumnResults(self):
        """one dict per column of the last ApplyInverse: iterations, achieved_tol, restarts, converged"""
        lib = bind_lockstep(self._lib)
        out = []
        its, tol, rst, conv = C.c_int(), C.c_double(), C.c_int(), C.c_int()
        while lib.hymls_mi_solver_column_result(self._s, len(out), C.byref(its), C.byref(tol), C.byref(rst), C.byref(conv)) == 0:
            out.append({"iterations": its.value, "achieved_tol": tol.value, "restarts": rst.value, "converged": bool(conv.value)})
        return out

    def ApplyInverse(self, B, X=None):
        """solve K X = B.  B: torch tensor on the device (n,) or (nvec, n) (float64, contiguous), or a numpy array (n,)
        or (n, nvec) in host memory.  Returns X.  Raises RuntimeError if a column did not reach the tolerance (X then
        holds the last iterate)."""
        n = self._P._n
        if hasattr(B, "data_ptr"):
            import torch
            assert B.dtype == torch.float64 and B.is_contiguous() and B.shape[-1] == n
            if X is None:
                X = torch.empty_like(B)
            assert X.is_contiguous() and X.shape == B.shape and X.dtype == torch.float64
            nvec = 1 if B.dim() == 1 else B.shape[0]
            ierr = self._lib.hymls_mi_solver_solve(self._s, B.data_ptr(), n, X.data_ptr(), n, nvec, 1)
            out = X
        else:
            Bc = np.asfortranarray(np.asarray(B, dtype=np.float64))
            assert Bc.shape[0] == n
            Xc = np.empty_like(Bc, order="F")
            nvec = 1 if Bc.ndim == 1 else Bc.shape[1]
            ierr = self._lib.hymls_mi_solver_solve(self._s, Bc.ctypes.data, n, Xc.ctypes.data, n, nvec, 0)
            if X is not None:
                X[...] = Xc
                out = X
            else:
                out = Xc
        if ierr == -1:
            raise RuntimeError(self._lib.hymls_mi_solver_last_error(self._s).decode())
        self._check(ierr)
        return out

    # --- measurements
    def set_profiling(self, on=True):
        self._check(self._lib.hymls_mi_solver_set_profiling(self._s, int(on)))

    def seconds(self, which=0):
        """0 whole solve, 1 ApplyInverse, 2 K x, 3 orthogonalisation and vector updates (summed since set_profiling)"""
        return self._lib.hymls_mi_solver_seconds(self._s, which)

    def close(self):
        # the solver lives inside P's handle context: nothing to free once P is closed
        if self._s and self._P._h:
            self._lib.hymls_mi_solver_destroy(self._s)
        self._s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NativeBorderedSolver(NativeSolver):
    """[K V; W' C] [x; s] = [b; t] with the library's own GMRES on the augmented vectors [x; s] (the interface of
    hymls_amd.BorderedSolver); the border is the one of P, for the operator and for the preconditioner.  One GPU."""

    def __init__(self, P, params=None):
        super().__init__(P, params)
        bind_bordered(self._lib)

    def SetBorder(self, V, W=None, C=None):
        """sets the border of P; call P.Compute() afterwards (as in the reference).  V=None removes it."""
        return self._P.SetBorder(V, W, C)

    def ApplyInverse(self, B, T=None, X=None, S=None):
        """returns (X, S).  B: torch tensor on the device or numpy array, (n,) float64; T: array-like (m,), default 0.
        X (same kind as B) and S (numpy, (m,)) may be given to receive the result.  Raises RuntimeError if the tolerance
        was not reached (X and S, where given, then hold the last iterate).  Without a border: the plain solve, S empty."""
        n, m = self._P._n, getattr(self._P, "_m", 0)
        Tc = None if T is None or m == 0 else np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(m))
        Sc = np.zeros(m)
        tp, sp = (Tc.ctypes.data if Tc is not None else None), (Sc.ctypes.data if m else None)
        if hasattr(B, "data_ptr"):
            import torch
            assert B.dtype == torch.float64 and B.is_contiguous() and B.dim() == 1 and B.shape[0] == n
            if X is None:
                X = torch.empty_like(B)
            assert X.is_contiguous() and X.shape == B.shape and X.dtype == torch.float64
            ierr = self._lib.hymls_mi_solver_solve_bordered(self._s, B.data_ptr(), tp, X.data_ptr(), sp, 1)
            out = X
        else:
            Bc = np.ascontiguousarray(np.asarray(B, dtype=np.float64))
            assert Bc.shape == (n,)
            Xc = np.empty_like(Bc)
            ierr = self._lib.hymls_mi_solver_solve_bordered(self._s, Bc.ctypes.data, tp, Xc.ctypes.data, sp, 0)
            if X is not None and ierr in (0, -1):
                X[...] = Xc
                out = X
            else:
                out = Xc
        if S is not None and ierr in (0, -1):
            S[...] = Sc
            Sc = S
        if ierr == -1:
            raise RuntimeError(self._lib.hymls_mi_solver_last_error(self._s).decode())
        self._check(ierr)
        return out, Sc


def border_product(P, n, m, V, ldv, W, ldw, C_, z, y):
    """the border product of the bordered operator (hymls_mi_border_product) on device arrays: y[0:n) += V z[n:n+m) and
    y[n+j] = W(:,j)' z[0:n) + sum_l C[j, l] z[n+l].  V, W (column-major, leading dimensions ldv, ldw), z, y: torch tensors
    (device memory; host memory with the test-only simulator) or None; C_: (m, m) array-like or None (zero)."""
    lib = bind_bordered(P._lib)
    Cm = None if C_ is None else np.asfortranarray(np.asarray(C_, dtype=np.float64))
    ptr = lambda a: a.data_ptr() if a is not None else None
    ierr = lib.hymls_mi_border_product(P._h, n, m, ptr(V), ldv, ptr(W), ldw, Cm.ctypes.data if Cm is not None else None,
                                       ptr(z), ptr(y))
    if ierr:
        raise HymlsError(ierr, lib.hymls_mi_last_error(P._h).decode())


def shifted_product(P, n, a, A, b, B, X, ldx, Y, ldy, nvec, nnz_hint=-1):
    """Y(:, v) = a A X(:, v) + b B X(:, v), v < nvec (hymls_mi_shifted_product) on device arrays.  A, B: (rowptr, colind, values)
    triples of torch tensors (int32, int32, float64; device memory, host memory with the test-only simulator) or None (A: only
    with a = 0; B: the identity); X, Y: torch tensors, column-major with leading dimensions ldx, ldy, not overlapping.
    nnz_hint: the nnz of A, from which the lanes per row follow (-1: 4 lanes)."""
    lib = bind_shifted(P._lib)
    ptr = lambda t: t.data_ptr() if t is not None else None
    pa, pb = [ptr(t) for t in (A or (None,) * 3)], [ptr(t) for t in (B or (None,) * 3)]
    ierr = lib.hymls_mi_shifted_product(P._h, n, a, pa[0], pa[1], pa[2], nnz_hint, b, pb[0], pb[1], pb[2], ptr(X), ldx, ptr(Y), ldy, nvec)
    if ierr:
        raise HymlsError(ierr, lib.hymls_mi_last_error(P._h).decode())


def oblique_project(P, n, m, Q, ldq, G, Pm, ldp, x, y):
    """y = x - Pm (G (Q' x)) (hymls_mi_oblique_project) on device arrays.  Q, Pm (column-major, leading dimensions ldq, ldp),
    x, y: torch tensors (device memory; host memory with the test-only simulator) or None; y may be x; G: (m, m) array-like
    or None (the identity)."""
    lib = bind_projection(P._lib)
    Gm = None if G is None else np.asfortranarray(np.asarray(G, dtype=np.float64))
    ptr = lambda a: a.data_ptr() if a is not None else None
    ierr = lib.hymls_mi_oblique_project(P._h, n, m, ptr(Q), ldq, Gm.ctypes.data if Gm is not None else None, ptr(Pm), ldp,
                                        ptr(x), ptr(y))
    if ierr:
        raise HymlsError(ierr, lib.hymls_mi_last_error(P._h).decode())


def matvec_mv(P, X, ldx, Y, ldy, nvec):
    """Y(:, v) = K X(:, v), v < nvec (hymls_mi_matvec_mv): K is read once per group of up to four columns.  X, Y: torch
    tensors (device memory; host memory with the test-only simulator) or numpy arrays in host memory, column-major with
    leading dimensions ldx, ldy."""
    lib = bind_lockstep(P._lib)
    on_device = hasattr(X, "data_ptr")
    ptr = (lambda a: a.data_ptr()) if on_device else (lambda a: a.ctypes.data)
    ierr = lib.hymls_mi_matvec_mv(P._h, ptr(X), ldx, ptr(Y), ldy, nvec, int(on_device))
    if ierr:
        raise HymlsError(ierr, lib.hymls_mi_last_error(P._h).decode())
    return Y


def _orthogonalize_mv(P, f32, n, ks, V, ldv, vstride, W, ldw, vnext, ldn):
    lib = bind_lockstep(P._lib)
    nb = len(ks)
    kk = np.ascontiguousarray(ks, dtype=np.int32)
    ldh = max(int(kk.max()), 1) if nb else 1
    h = np.zeros((max(nb, 1), ldh))
    nrm = np.zeros(max(nb, 1))
    ptr = lambda a: a.data_ptr() if a is not None else None
    if f32:
        ierr = lib.hymls_mi_orthogonalize_mv_f32(P._h, n, nb, kk.ctypes.data, ptr(V), ldv, vstride, ptr(W), ldw, ptr(vnext), ldn,
                                                 h.ctypes.data, ldh, nrm.ctypes.data)
    else:
        ierr = lib.hymls_mi_orthogonalize_mv(P._h, n, nb, kk.ctypes.data, ptr(V), ldv, vstride, ptr(W), ldw, h.ctypes.data, ldh,
                                             nrm.ctypes.data)
    if ierr:
        raise HymlsError(ierr, lib.hymls_mi_last_error(P._h).decode())
    return [h[v, :kk[v]].copy() for v in range(nb)], nrm[:nb]


def orthogonalize_mv(P, n, ks, V, ldv, vstride, W, ldw):
    """len(ks) independent ICGS(2) steps in one launch chain (hymls_mi_orthogonalize_mv): column v of W (leading dimension
    ldw) is orthogonalised in place against the ks[v] columns of its own basis V[v * vstride:] (leading dimension ldv).
    Returns ([h1 + h2 of column v], norms); each column has the bits of ``orthogonalize``."""
    return _orthogonalize_mv(P, False, n, ks, V, ldv, vstride, W, ldw, None, 0)


def orthogonalize_mv_f32(P, n, ks, V, ldv, vstride, W, ldw, vnext=None, ldn=0):
    """the same against float bases (hymls_mi_orthogonalize_mv_f32); vnext (optional float32 tensor, leading dimension ldn)
    receives float32(W(:, v) / ||W(:, v)||)."""
    return _orthogonalize_mv(P, True, n, ks, V, ldv, vstride, W, ldw, vnext, ldn)


def orthogonalize(P, n, k, V, ldv, w):
    """one ICGS(2) step of the library (hymls_mi_orthogonalize) on device arrays: w <- (I - V V^T)^2 w in place over
    the k columns of V (column-major, leading dimension ldv).  V, w: torch tensors (device memory; host memory with the
    test-only simulator).  Returns (h1 + h2 as a numpy array of k values, ||w||)."""
    lib = bind_solver(P._lib)
    h = np.zeros(k)
    nrm = C.c_double()
    ierr = lib.hymls_mi_orthogonalize(P._h, n, k, V.data_ptr(), ldv, w.data_ptr(), h.ctypes.data_as(C.POINTER(C.c_double)),
                                      C.byref(nrm))
    if ierr:
        raise HymlsError(ierr, lib.hymls_mi_last_error(P._h).decode())
    return h, nrm.value


def orthogonalize_f32(P, n, k, V, ldv, w, vnext=None):
    """the same step against a float basis (hymls_mi_orthogonalize_f32): V a float32 tensor, w a float64 tensor that is
    orthogonalised in place in FP64, vnext (optional float32 tensor of n entries) receives float32(w / ||w||).
    Returns (h1 + h2, ||w||)."""
    lib = bind_solver(P._lib)
    h = np.zeros(k)
    nrm = C.c_double()
    ierr = lib.hymls_mi_orthogonalize_f32(P._h, n, k, V.data_ptr(), ldv, w.data_ptr(),
                                          vnext.data_ptr() if vnext is not None else None,
                                          h.ctypes.data_as(C.POINTER(C.c_double)), C.byref(nrm))
    if ierr:
        raise HymlsError(ierr, lib.hymls_mi_last_error(P._h).decode())
    return h, nrm.value
