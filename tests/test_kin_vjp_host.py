"""CPU-side (-m "not gpu") checks of the inverse-kinematics fused backward (csrc/kin_vjp_kernels.hip: thx_kin_vjp): its argument
checks through ctypes, and the gate that keeps a kernel set without the kernel on the torch path.  GPU twin:
tests/test_gpu_kin_vjp.py."""
import ctypes

import pytest

from tests.helpers import load_golden
from tests.kin_common import FIXTURES
from tests.test_cabi_and_host import lib_path  # noqa: F401  (the session fixture that builds)
from tests.test_kin_host import _lm, check_implicit_gradients

ORDER = ("terms", "n_terms", "paths", "n_paths", "x", "ldx", "n", "dof", "u", "ldu", "m", "j_total", "rec", "rec_stride", "plan",
         "grad_out", "B", "dtype", "eps", "stream")
PLAN = (2, 5, 0, 0, 0, 0, 4096, 4096, None, None, 60, 0)   # two tensors, five pairs, no grids


def test_bad_arguments_are_refused_before_any_launch(lib_path):  # noqa: F811
    from theseus_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    plan = _lib.Traj2GradPlan(*PLAN)
    ok = dict(terms=p, n_terms=4, paths=p, n_paths=9, x=p, ldx=7, n=7, dof=7, u=p, ldu=7, m=23, j_total=161, rec=p, rec_stride=28,
              plan=ctypes.pointer(plan), grad_out=p, B=2, dtype=0, eps=_lib.LieEps(1e-6, 1e-3, 1e-6), stream=None)

    def refused(needle, **kw):
        a = dict(ok, **kw)
        rc = lib.thx_kin_vjp(*[a[k] for k in ORDER])
        return rc == -1 and needle in lib.thx_last_error() and b"thx_kin_vjp" in lib.thx_last_error()
    for name in ("terms", "paths", "x", "u", "rec", "plan", "grad_out", "eps"):
        assert refused(b"null pointer", **{name: None}), name
    for name in ("terms", "paths", "x", "u", "rec", "grad_out"):
        assert refused(b"aligned", **{name: ctypes.c_void_p(4098)}), name
    assert refused(b"aligned", u=ctypes.c_void_p(4100), dtype=1) and refused(b"aligned", rec=ctypes.c_void_p(4100))   # 8 bytes
    assert refused(b"dtype", dtype=7) and refused(b"dtype", dtype=-1)
    assert refused(b"n_terms", n_terms=0) and refused(b"batch", B=0) and refused(b"batch", B=-3)
    assert refused(b"dof < 1", dof=0) and refused(b"n < dof", n=6) and refused(b"ldx < n", ldx=6) and refused(b"ldu < n", ldu=6)
    assert refused(b"n_paths", n_paths=-1) and refused(b"m < 1", m=0) and refused(b"j_total < dof", j_total=6)
    assert refused(b"rec_stride", rec_stride=27) and refused(b"rec_stride", rec_stride=17, dof=1, n=1, ldx=1, ldu=1)
    assert refused(b"grid limit", n_terms=2 ** 31 - 1, B=2 ** 31 - 1)
    for field, value, needle in (("n_grids", 1, b"no grids"), ("tensors", None, b"null pointer in the plan"), ("pairs", 4098, b"aligned"),
                                 ("out_elems", 0, b"size in the plan"), ("n_pairs", -1, b"size in the plan"),
                                 ("n_grids", -1, b"size in the plan")):
        bad = _lib.Traj2GradPlan(*PLAN)
        setattr(bad, field, value)
        assert refused(needle, plan=ctypes.pointer(bad)), field


@pytest.mark.parametrize("fixture", FIXTURES)
def test_a_kernel_set_without_the_kernel_stays_on_the_torch_path(fixture, monkeypatch):
    """KinOracleKernels has no kin_vjp: the differentiated assemble(graph=True) evaluates the torch classes (counted here) and
    reproduces the fixture's gradients.  The gate is hasattr, never a fallback after a failure."""
    import theseus_amd as th
    from tests.kin_oracle_kernels import KinOracleKernels
    from theseus_amd.kinematics import PackedKinematics
    K = KinOracleKernels()
    assert not hasattr(K, "kin_vjp") and PackedKinematics.fused_backward and hasattr(th.HipKernels, "kin_vjp")
    calls = {"n": 0}
    real = th.eb.LinkPoseCost.jacobians

    def counted(self):
        calls["n"] += 1
        return real(self)
    monkeypatch.setattr(th.eb.LinkPoseCost, "jacobians", counted)
    g = load_golden(fixture)
    _, opt, leaves, sol, _ = _lm(th, g, K, backward_mode="implicit")
    packed = opt.linear_solver.linearization.packed
    assert type(packed).__name__ == "PackedKinematics" and packed._VJP_KERNEL == "kin_vjp" and calls["n"] >= 1
    check_implicit_gradients(g, leaves, sol)
