"""CPU-side (-m "not gpu") checks of the homography family's fused backward (csrc/homog_vjp_kernels.hip: thx_homog_vjp): its argument
checks through ctypes, and the gate that keeps a kernel set without the kernel on the torch route.  GPU twin:
tests/test_gpu_homog_vjp.py."""
import ctypes

import pytest

from tests.helpers import load_golden
from tests.homog_common import FIXTURES
from tests.test_cabi_and_host import lib_path  # noqa: F401  (the session fixture that builds)
from tests.test_homog_host import _lm, check_implicit_gradients

ORDER = ("terms", "n_terms", "n_align", "x", "ldx", "n", "u", "ldu", "m", "j_total", "scratch", "chunks", "rec", "plan", "grad_out", "B",
         "dtype", "stream")
PLAN = (2, 3, 2, 42, 3, 0, 4096, 4096, 4096, 600)   # (tensors, pairs, maps, max_cells, max_chans, pad, three tables, out_elems)


def test_bad_arguments_are_refused_before_any_launch(lib_path):  # noqa: F811
    from theseus_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    plan = _lib.HomogGradPlan(*PLAN)
    ok = dict(terms=p, n_terms=3, n_align=2, x=p, ldx=16, n=16, u=p, ldu=16, m=10, j_total=80, scratch=p, chunks=5, rec=p,
              plan=ctypes.pointer(plan), grad_out=p, B=2, dtype=0, stream=None)

    def refused(needle, **kw):
        a = dict(ok, **kw)
        rc = lib.thx_homog_vjp(*[a[k] for k in ORDER])
        return rc == -1 and needle in lib.thx_last_error() and b"thx_homog_vjp" in lib.thx_last_error()
    for name in ("terms", "x", "u", "scratch", "rec", "plan", "grad_out"):
        assert refused(b"null pointer", **{name: None}), name
    for name in ("terms", "x", "u", "scratch", "rec", "grad_out"):
        assert refused(b"aligned", **{name: ctypes.c_void_p(4098)}), name
    assert refused(b"aligned", u=ctypes.c_void_p(4100), dtype=1)   # fp64 needs 8 bytes
    assert refused(b"dtype", dtype=7) and refused(b"dtype", dtype=-1)
    assert refused(b"n_terms", n_terms=0) and refused(b"batch", B=0) and refused(b"batch", B=-3)
    assert refused(b"ldx < n", ldx=15) and refused(b"ldu < n", ldu=15) and refused(b"n < 8", n=7)
    assert refused(b"n_align", n_align=4) and refused(b"chunks < 1", chunks=0) and refused(b"j_total", j_total=7)
    assert refused(b"grid limit", n_terms=2 ** 31 - 1, n_align=1, B=2 ** 31 - 1, plan=ctypes.pointer(_lib.HomogGradPlan(
        2, 3, 1, 42, 3, 0, 4096, 4096, 4096, 600)))
    for field, value, needle in (("tensors", None, b"null pointer in the plan"), ("map_off", None, b"null pointer in the plan"),
                                 ("pairs", 4098, b"aligned"), ("out_elems", 0, b"size in the plan"), ("n_maps", 1, b"do not fit"),
                                 ("max_cells", 2 ** 20, b"32-bit sort keys")):   # (a 1024 x 1024 map: too large for the key width)
        bad = _lib.HomogGradPlan(*PLAN)
        setattr(bad, field, value)
        assert refused(needle, plan=ctypes.pointer(bad)), field


@pytest.mark.parametrize("fixture", FIXTURES)
def test_a_kernel_set_without_the_kernel_stays_on_the_torch_route(fixture, monkeypatch):
    """HomogOracleKernels has no homog_vjp: the differentiated assemble(graph=True) evaluates the torch classes (counted here) and
    reproduces the fixture's gradients.  The gate is hasattr, never a fallback after a failure."""
    import theseus_amd as th
    from tests.homog_oracle_kernels import HomogOracleKernels
    K = HomogOracleKernels()
    assert not hasattr(K, "homog_vjp") and th.PackedHomography.fused_backward
    calls = {"n": 0}
    real = th.eb.HomographyAlignment.weighted_jacobians_error

    def counted(self):
        calls["n"] += 1
        return real(self)
    monkeypatch.setattr(th.eb.HomographyAlignment, "weighted_jacobians_error", counted)
    g = load_golden(fixture)
    _, opt, leaves, sol, _ = _lm(th, g, K, backward_mode="implicit")
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedHomography" and calls["n"] >= 1
    check_implicit_gradients(g, leaves, sol)


def test_the_gate_sees_requires_grad_set_after_the_table_was_built():
    """a shared feature map gets requires_grad_() with no Variable update in between: the plan is rebuilt before the gate reads it"""
    import theseus_amd as th
    from tests.homog_common import build
    from tests.homog_oracle_kernels import HomogOracleKernels
    K = HomogOracleKernels()
    K.homog_vjp = None   # (the gate asks hasattr; nothing is launched here)
    obj, _, _ = build(th, load_golden("homog_f64_shared"))
    packed = th.HipLinearization(obj, kernels=K).packed
    packed.sync()
    assert packed._grad_plan.servable and not packed._fused_backward_route()   # (nothing asks yet)
    obj.get_variable("w_align").tensor.requires_grad_(True)
    assert packed._fused_backward_route()
    obj.get_variable("feat_src").tensor.requires_grad_(True)
    assert not packed._fused_backward_route() and not packed._grad_plan.servable
