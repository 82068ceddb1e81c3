"""CPU-side (-m "not gpu") checks of the pivoted-LU entry points: argument validation happens on the host side of the C ABI before
any launch; the header, the library and the ctypes table agree on the new names; the plugin's HipLUSolver is a th.LUDenseSolver
for the reference's isinstance whitelists (where the reference imports)."""
import ctypes
import os
import sys

import pytest

from tests.conftest import ROOT
from tests.test_cabi_and_host import declared_symbols, lib_path  # noqa: F401  (lib_path: the session fixture that builds)

LU_NAMES = ["thx_lu_factor", "thx_lu_solve", "thx_lu_solve_backward", "thx_lu_solve_forward"]
REF = os.environ.get("THX_REFERENCE_ROOT", "/root/reference")
needs_reference = pytest.mark.skipif(not os.path.isdir(REF), reason="needs /root/reference")


def test_bad_arguments_to_lu_factor_are_refused_before_any_launch(lib_path):  # noqa: F811
    from theseus_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    two = ctypes.c_void_p(4096)
    rc = lib.thx_lu_factor(None, 32, 6, 1, 1, None, 0, 1e-8, None, None, None, 0, None)
    assert rc != 0 and b"null pointer" in lib.thx_last_error()
    rc = lib.thx_lu_factor(one, 33, 6, 1, 1, None, 0, 1e-8, two, one, one, 0, None)        # ld % 32 != 0
    assert rc != 0 and b"ld" in lib.thx_last_error()
    rc = lib.thx_lu_factor(one, 32, 6, 1, 1, None, 0, 1e-8, two, one, one, 7, None)        # bad dtype
    assert rc != 0 and b"dtype" in lib.thx_last_error()
    n = _lib.THX_LU_MAX_N + 1
    rc = lib.thx_lu_factor(one, (n + 31) // 32 * 32, n, 1, 0, None, 0, 1e-8, two, one, one, 0, None)   # n above the limit
    assert rc != 0 and b"limit" in lib.thx_last_error() and str(_lib.THX_LU_MAX_N).encode() in lib.thx_last_error()
    assert _lib.THX_LU_MAX_N >= 3072
    rc = lib.thx_lu_factor(one, 32, 6, 1, 1, None, 0, 1e-8, one, one, one, 0, None)        # LU aliases the source
    assert rc != 0 and b"alias" in lib.thx_last_error()
    # the solves
    rc = lib.thx_lu_solve(one, 32, 6, 1, None, one, one, 6, 0, None)
    assert rc != 0 and b"null pointer" in lib.thx_last_error()
    rc = lib.thx_lu_solve_forward(one, 32, 6, 1, one, one, one, 5, 0, None)                # ldv < n
    assert rc != 0 and b"ldv" in lib.thx_last_error()
    rc = lib.thx_lu_solve_backward(one, 32, 6, 1, one, one, 6, 7, None)
    assert rc != 0 and b"dtype" in lib.thx_last_error()
    rc = lib.thx_lu_solve(one, 32, n, 1, one, one, one, n, 0, None)
    assert rc != 0


def test_header_library_and_ctypes_table_agree_on_the_lu_names(lib_path):  # noqa: F811
    from theseus_amd import _lib
    assert [s for s in declared_symbols() if s.startswith("thx_lu_")] == LU_NAMES
    assert [s for s in _lib.EXPORTED_SYMBOLS if s.startswith("thx_lu_")] == LU_NAMES
    lib = ctypes.CDLL(lib_path)
    assert all(hasattr(lib, s) for s in LU_NAMES)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(s in doc for s in LU_NAMES)


def test_lu_solver_is_exported_with_the_cholesky_solvers_constructor():
    import inspect
    import theseus_amd as th
    from theseus_amd.linear_solver import HipCholeskyCore, HipLUCore
    assert th.LUDenseSolver is th.HipLUSolver and issubclass(th.HipLUSolver, HipLUCore)
    assert list(inspect.signature(th.HipLUSolver.__init__).parameters) == \
        list(inspect.signature(th.HipCholeskySolver.__init__).parameters)
    # the surface the loops and the autograd nodes call on the Cholesky core
    for name in ("factorize", "_substitute", "solve_with_factor", "factor_snapshot", "solve_with_snapshot", "check_info",
                 "singular_mask", "dropped_mask", "post_singular_warning", "_solve"):
        assert callable(getattr(HipLUCore, name)) and callable(getattr(HipCholeskyCore, name)), name
    with pytest.raises(RuntimeError, match="HipLUSolver only works with theseus_amd.HipLinearization"):
        th.HipLUSolver(th.Objective(), linearization_cls=dict)


@pytest.fixture(scope="module")
def ref():
    for p in (os.path.join(ROOT, "oracle", "stubs"), REF, REF + "/torchlie", REF + "/torchkin"):
        if p not in sys.path:
            sys.path.append(p)
    import warnings
    warnings.filterwarnings("ignore")
    import theseus as th
    import theseus_amd.plugin as thp
    return th, thp


def _tiny_objective(th):
    import torch
    obj = th.Objective(dtype=torch.float64)
    a = th.Vector(tensor=torch.zeros(2, 3, dtype=torch.float64), name="a")
    t = th.Vector(tensor=torch.ones(2, 3, dtype=torch.float64), name="t")
    obj.add(th.Difference(a, t, th.ScaleCostWeight(torch.tensor(1.0, dtype=torch.float64)), name="d"))
    return obj


@needs_reference
@pytest.mark.reference
def test_plugin_lu_solver_passes_the_reference_whitelists(ref):
    from tests.oracle_kernels import OracleKernels
    th, thp = ref
    obj = _tiny_objective(th)
    solver = thp.HipLUSolver(obj, linearization_kwargs=dict(kernels=OracleKernels()))
    assert isinstance(solver, th.LUDenseSolver) and not isinstance(solver, th.CholeskyDenseSolver)
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=thp.HipLUSolver, linearization_kwargs=dict(kernels=OracleKernels()))
    assert isinstance(opt.linear_solver, thp.HipLUSolver)
    # levenberg_marquardt.py:16-32,82-87: both damping variants are whitelisted by isinstance on the solver, at construction
    assert opt._allows_ellipsoidal and opt._allows_adaptive


@needs_reference
@pytest.mark.reference
def test_plugin_lu_solver_rejects_a_foreign_linearization(ref):
    th, thp = ref
    with pytest.raises(RuntimeError, match="HipLUSolver only works with theseus_amd.plugin.HipLinearization"):
        thp.HipLUSolver(_tiny_objective(th), linearization_cls=th.DenseLinearization)
