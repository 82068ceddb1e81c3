"""CPU-side (-m "not gpu") checks of thx_ba_reduce_multi / thx_ba_backsub_multi: declared, exported, bound and documented; every
bad argument refused on the host before any launch, by its message; a HipSchurSolver on a kernel set without the two kernels keeps
refusing blocks of right-hand sides."""
import ctypes
import os

import pytest
import torch

from tests.test_cabi_and_host import ROOT, declared_symbols, lib_path  # noqa: F401  (the session fixture that builds)

NAMES = ("thx_ba_reduce_multi", "thx_ba_backsub_multi")
ARGS = dict(thx_ba_reduce_multi=("s", "B", "W", "Hinv", "rhs", "x", "nrhs", "ldv", "bstride", "which", "dtype", "stream"),
            thx_ba_backsub_multi=("s", "B", "W", "Hinv", "x", "nrhs", "ldv", "bstride", "which", "dtype", "stream"))


@pytest.mark.parametrize("name", NAMES)
def test_entry_point_is_declared_exported_bound_and_refuses_bad_arguments(lib_path, name):  # noqa: F811
    from theseus_amd import _lib
    lib = _lib.load()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert name in declared_symbols() and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and name in doc
    p = ctypes.c_void_p(4096)
    s = _lib.BAStructure()
    s.num_cams, s.num_points, s.num_obs = 2, 3, 4          # n = 21
    ok = dict(s=ctypes.byref(s), B=2, W=p, Hinv=p, rhs=p, x=p, nrhs=5, ldv=21, bstride=105, which=0, dtype=0, stream=None)

    def refused(text, **kw):
        a = dict(ok, **kw)
        return getattr(lib, name)(*[a[k] for k in ARGS[name]]) == -1 and lib.thx_last_error().startswith(name.encode()) and \
            text in lib.thx_last_error()
    for arg in ("s", "W", "Hinv", "rhs", "x"):
        if arg in ARGS[name]:
            assert refused(b"null pointer", **{arg: None}), arg
    assert refused(b"B>0", B=0)
    assert refused(b"nrhs < 1", nrhs=0) and refused(b"nrhs < 1", nrhs=-4)
    assert refused(b"ldv < n", ldv=20)
    assert refused(b"bstride < nrhs * ldv", bstride=104) and refused(b"bstride < nrhs * ldv", ldv=2 ** 62, bstride=2 ** 63 - 1)
    assert refused(b"which", which=-1) and refused(b"which", which=3)
    assert refused(b"dtype", dtype=7)
    assert refused(b"grid limit", B=64 * 65536, nrhs=1, bstride=21)


def test_a_kernel_set_without_the_kernels_leaves_the_solver_refusing():
    import theseus_amd as th
    from tests.oracle_kernels import OracleKernels
    from theseus_amd.kernels import HipKernels
    from theseus_amd.utils.synthetic_ba import make_ba_objective
    assert all(hasattr(HipKernels, k) and not hasattr(OracleKernels, k) for k in ("ba_reduce_multi", "ba_backsub_multi"))
    K = OracleKernels()
    obj, info = make_ba_objective(3, 6, 2, device="cpu", kernels=K)
    solver = th.HipSchurSolver(obj, linearization_kwargs=dict(kernels=K))
    assert solver._apply_multi is None
    for call in (lambda: solver.sample_deltas(3), lambda: solver.marginal_covariance(["Cam0"]),
                 lambda: solver.solve_multi_with_factor(torch.zeros(2, 1, info["n"], dtype=torch.float64))):
        with pytest.raises(NotImplementedError, match="HipCholeskySolver"):
            call()
