"""CPU-side (-m "not gpu") checks of the SE2 planner's fused backward (csrc/trajse2_vjp_kernels.hip: thx_trajse2_vjp): its argument
checks through ctypes, and the gate that keeps a kernel set without the kernel on the torch path.  GPU twin:
tests/test_gpu_trajse2_vjp.py."""
import ctypes

import pytest

from tests.helpers import load_golden
from tests.test_cabi_and_host import lib_path  # noqa: F401  (the session fixture that builds)
from tests.test_push2_host import check_implicit_gradients
from tests.test_trajse2_host import _lm
from tests.trajse2_common import FIXTURES

ORDER = ("terms", "n_terms", "x", "V", "u", "ldu", "m", "j_total", "rec", "plan", "grad_out", "grid_work", "B", "dtype", "eps", "stream")


def test_bad_arguments_are_refused_before_any_launch(lib_path):  # noqa: F811
    from theseus_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    plan = _lib.Traj2GradPlan(2, 5, 1, 3, 42, 0, 4096, 4096, 4096, 4096, 60, 84)
    ok = dict(terms=p, n_terms=3, x=p, V=12, u=p, ldu=36, m=12, j_total=40, rec=p, plan=ctypes.pointer(plan), grad_out=p,
              grid_work=p, B=2, dtype=0, eps=_lib.SE2Eps(1e-6, 1e-3), stream=None)

    def refused(needle, **kw):
        a = dict(ok, **kw)
        rc = lib.thx_trajse2_vjp(*[a[k] for k in ORDER])
        return rc == -1 and needle in lib.thx_last_error() and b"thx_trajse2_vjp" in lib.thx_last_error()
    for name in ("terms", "x", "u", "rec", "plan", "grad_out", "eps"):
        assert refused(b"null pointer", **{name: None}), name
    for name in ("terms", "x", "u", "rec", "grad_out", "grid_work"):
        assert refused(b"aligned", **{name: ctypes.c_void_p(4098)}), name
    assert refused(b"aligned", u=ctypes.c_void_p(4100), dtype=1)   # fp64 needs 8 bytes
    assert refused(b"aligned", x=ctypes.c_void_p(4104)) and refused(b"aligned", x=ctypes.c_void_p(4112), dtype=1)   # one record
    assert refused(b"dtype", dtype=7) and refused(b"dtype", dtype=-1)
    assert refused(b"n_terms", n_terms=0) and refused(b"batch", B=0) and refused(b"batch", B=-3)
    assert refused(b"V < 1", V=0) and refused(b"ldu < 3 V", ldu=35) and refused(b"j_total < 3", j_total=2) and refused(b"m < 1", m=0)
    assert refused(b"grid limit", n_terms=2 ** 31 - 1, B=2 ** 31 - 1)
    for field, value, needle in (("tensors", None, b"null pointer in the plan"), ("grid_terms", None, b"null pointer in the plan"),
                                 ("pairs", 4098, b"aligned"), ("out_elems", 0, b"size in the plan"), ("n_grids", -1, b"size in the plan")):
        bad = _lib.Traj2GradPlan(2, 5, 1, 3, 42, 0, 4096, 4096, 4096, 4096, 60, 84)
        setattr(bad, field, value)
        assert refused(needle, plan=ctypes.pointer(bad)), field
    assert refused(b"null pointer in the plan", grid_work=None)   # (a plan with a grid needs its work buffer)


@pytest.mark.parametrize("fixture", FIXTURES)
def test_a_kernel_set_without_the_kernel_stays_on_the_torch_path(fixture, monkeypatch):
    """TrajSE2OracleKernels has no trajse2_vjp: the differentiated assemble(graph=True) evaluates the torch classes (counted here) and
    reproduces the fixture's gradients.  The gate is hasattr, never a fallback after a failure."""
    import theseus_amd as th
    from tests.trajse2_oracle_kernels import TrajSE2OracleKernels
    from theseus_amd.planning_se2 import PackedTrajectorySE2
    K = TrajSE2OracleKernels()
    assert not hasattr(K, "trajse2_vjp") and PackedTrajectorySE2.fused_backward and hasattr(th.HipKernels, "trajse2_vjp")
    assert PackedTrajectorySE2._VJP_KERNEL == "trajse2_vjp"
    calls = {"n": 0}
    real = th.eb.Collision2D.weighted_jacobians_error

    def counted(self):
        calls["n"] += 1
        return real(self)
    monkeypatch.setattr(th.eb.Collision2D, "weighted_jacobians_error", counted)
    g = load_golden(fixture)
    _, opt, leaves, sol, _ = _lm(th, g, K, backward_mode="implicit")
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedTrajectorySE2" and calls["n"] >= 5
    check_implicit_gradients(g, leaves, sol, g["var_order"].tolist())
