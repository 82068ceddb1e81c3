"""CPU-side (-m "not gpu") checks of homography alignment (theseus_amd/embodied.py: HomographyAlignment, theseus_amd/homography.py,
csrc/homog_kernels.hip): the torch class against the REAL reference's fixtures (tests/golden/homog_f64_*.npz,
tools/gen_homog_golden.py) and against autograd, the C ABI of the two new exports, their argument checks (through ctypes and in a
stand-alone program under the host sanitizers), which packed family ``packed_for`` selects, and LM / implicit gradients on the torch
stand-in of the kernels.  GPU twin: tests/test_gpu_homog.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.helpers import load_golden
from tests.homog_common import FIXTURES, LM_DAMPING, LM_KW, MARGIN, build, kernel_problem, min_margin, outside_fractions
from tests.test_cabi_and_host import declared_symbols, lib_path  # noqa: F401  (lib_path: the session fixture that builds)
from tests.test_traj2_host import assert_blocks_close, check_iterates

NAMES = ("thx_homog_eval", "thx_homog_error")


@pytest.mark.parametrize("fixture", FIXTURES)
def test_torch_class_reproduces_the_reference_blocks(fixture):
    """A few dozen flops per element and a sum over 84 elements, inputs of order 1: 1e-12 of the block's largest magnitude is four
    orders above fp64 rounding and far below any formula error."""
    import theseus_amd as th
    g = load_golden(fixture)
    obj, _, costs = build(th, g)
    assert costs == g["cost_order"].tolist() and list(obj.optim_vars) == g["var_order"].tolist()
    for name, c in obj.cost_functions.items():
        jac, err = c.weighted_jacobians_error()
        assert_blocks_close(err.numpy(), g[f"we_{name}"], 1e-12, f"{name} error")
        assert_blocks_close(c.weighted_error().numpy(), g[f"we_{name}"], 1e-12, f"{name} weighted_error")
        assert_blocks_close(jac[0].expand(3, -1, -1).numpy(), g[f"wj_{name}_0"], 1e-12, f"{name} block")
    assert_blocks_close(obj.error().numpy(), g["error"], 1e-12, "error vector")
    assert_blocks_close(obj.error_metric().numpy(), g["error_metric"], 1e-12, "error metric")
    assert min_margin(obj.cost_functions["align"]) >= MARGIN


def _autograd_block(cost):
    h0 = cost.H8.tensor

    def fn(h):
        cost.H8._tensor = h
        return cost.error()
    try:
        full = torch.autograd.functional.jacobian(fn, h0.clone())   # (B, 1, B, 8)
    finally:
        cost.H8._tensor = h0
    return torch.stack([full[b, :, b] for b in range(h0.shape[0])])


def _outside_problem():
    """13 x 19, the source points three times as far from the centre as the destination pixels"""
    return kernel_problem(3, 3, 13, 19, seed=4, scale=3.0)


@pytest.mark.parametrize("case", list(FIXTURES) + ["outside"])
def test_analytic_jacobian_equals_autograd_of_the_error(case):
    """fp64; floor() has no gradient and the mask is computed without one, so autograd differentiates exactly what jacobians()
    holds constant: 1e-10 of the block's largest entry"""
    import theseus_amd as th
    obj, _, _ = build(th, _outside_problem() if case == "outside" else load_golden(case))
    cost = obj.cost_functions["align"]
    if case == "outside":
        assert all(0.3 <= f <= 0.4 for f in outside_fractions(cost)), outside_fractions(cost)
    jac, err = cost.jacobians()
    want = _autograd_block(cost)
    assert float(want.abs().max()) > 0
    assert_blocks_close(jac[0].numpy(), want.numpy(), 1e-10, "block")
    assert_blocks_close(err.numpy(), cost.error().numpy(), 1e-15, "error")


def test_jacobians_stay_differentiable_in_both_feature_maps():
    import theseus_amd as th
    obj, leaves, _ = build(th, load_golden(FIXTURES[1]), grad=True)
    jac, err = obj.cost_functions["align"].weighted_jacobians_error()
    (jac[0].sum() + err.sum()).backward()
    assert all(float(v.grad.abs().max()) > 0 for v in leaves.values())


def _lm(th, g, kernels, device="cpu", **okw):
    obj, leaves, _ = build(th, g, device=device, grad=bool(okw.get("backward_mode")))
    opt = th.LevenbergMarquardt(obj, linearization_kwargs=dict(kernels=kernels) if kernels is not None else {}, **LM_KW)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)   # (info.state_history is kept in the default dtype, as the reference keeps it)
    try:
        sol, info = th.TheseusLayer(opt).forward(None, optimizer_kwargs=dict(damping=LM_DAMPING, **okw))
    finally:
        torch.set_default_dtype(old)
    return obj, opt, leaves, sol, info


def check_implicit_gradients(g, leaves, sol):
    """the generic path's tolerance for implicit LM gradients (simple_example_common.py: 1e-6 of the gradient's largest entry)"""
    final = sol["H8"]
    np.testing.assert_allclose(final.detach().cpu().numpy(), g["implicit_final"], rtol=1e-8, atol=1e-10)
    (final ** 2).sum().backward()
    for k, leaf in leaves.items():
        want = g[f"grad_{k}"]
        assert np.abs(want).max() > 0
        np.testing.assert_allclose(leaf.grad.cpu().numpy(), want, rtol=0, atol=1e-6 * np.abs(want).max(), err_msg=k)


@pytest.mark.parametrize("fixture", FIXTURES)
def test_torch_class_reproduces_the_reference_linearization(fixture):
    """AtA, Atb and the error metric from the torch class's blocks (the generic path: these kernels have no homog_eval)"""
    import theseus_amd as th
    from tests.oracle_kernels import OracleKernels
    g = load_golden(fixture)
    obj, _, _ = build(th, g)
    lin = th.HipLinearization(obj, kernels=OracleKernels())
    assert type(lin.packed).__name__ == "PackedEuclidean"
    lin.linearize()
    assert_blocks_close(torch.tril(lin.AtA).numpy(), np.tril(g["AtA"]), 1e-12, "AtA")
    assert_blocks_close(lin.Atb.squeeze(2).numpy(), g["Atb"], 1e-12, "Atb")
    assert_blocks_close(obj.error_metric().numpy(), g["error_metric"], 1e-12, "error metric")


@pytest.mark.parametrize("mode,kw", [("unroll", {}), ("truncated", dict(backward_num_iterations=2))])
def test_unrolled_gradients_on_the_fused_family_equal_the_generic_path(mode, kw):
    """The differentiated iterations are PackedEuclidean's torch evaluation on both families; the iterations before them (TRUNCATED)
    are fused on one and torch on the other, equal to a few ulp: gradients to 1e-9 of their largest entry."""
    import theseus_amd as th
    from tests.homog_oracle_kernels import HomogOracleKernels
    from tests.oracle_kernels import OracleKernels
    g = load_golden(FIXTURES[1])
    grads = {}
    for name, K in (("fused", HomogOracleKernels()), ("generic", OracleKernels())):
        _, opt, leaves, sol, _ = _lm(th, g, K, backward_mode=mode, **kw)
        assert type(opt.linear_solver.linearization.packed).__name__ == {"fused": "PackedHomography", "generic": "PackedEuclidean"}[name]
        (sol["H8"] ** 2).sum().backward()
        grads[name] = {k: v.grad.numpy() for k, v in leaves.items()}
    for k, want in grads["generic"].items():
        assert np.abs(want).max() > 0
        np.testing.assert_allclose(grads["fused"][k], want, rtol=0, atol=1e-9 * np.abs(want).max(), err_msg=k)


@pytest.mark.parametrize("fixture", FIXTURES)
def test_packed_homography_on_the_stand_in_kernels(fixture):
    """The packer's term table, decoded by the torch stand-in of the two kernels: linearization, LM iterates, implicit gradients."""
    import theseus_amd as th
    from tests.homog_oracle_kernels import HomogOracleKernels
    g = load_golden(fixture)
    K = HomogOracleKernels()
    obj, _, _ = build(th, g)
    lin = th.HipLinearization(obj, kernels=K)
    assert type(lin.packed).__name__ == "PackedHomography"
    lin.linearize()
    assert K.calls["homog_eval"] == 1
    assert_blocks_close(torch.tril(lin.AtA).numpy(), np.tril(g["AtA"]), 1e-12, "AtA")
    assert_blocks_close(lin.Atb.squeeze(2).numpy(), g["Atb"], 1e-12, "Atb")
    assert_blocks_close(obj.error_metric().numpy(), g["error_metric"], 1e-12, "error metric")
    assert K.calls["homog_error"] == 1
    with torch.no_grad():
        _, opt, _, _, info = _lm(th, g, K, track_err_history=True, track_state_history=True)
    assert K.calls["homog_eval"] >= 6
    check_iterates(g, info, g["var_order"].tolist())
    _, _, leaves, sol, _ = _lm(th, g, K, backward_mode="implicit")
    check_implicit_gradients(g, leaves, sol)


def test_replaced_and_edited_feature_maps_are_seen_on_the_stand_in_kernels():
    """a new tensor per outer step rebuilds the table; values changed in place need no rebuild"""
    import theseus_amd as th
    from tests.homog_oracle_kernels import HomogOracleKernels
    g = load_golden(FIXTURES[1])
    obj, _, _ = build(th, g)
    lin = th.HipLinearization(obj, kernels=HomogOracleKernels())
    lin.linearize()
    packed, before = lin.packed, lin.Atb.clone()
    new = torch.from_numpy(g["feat_src"]) * 0.7 + 0.1
    obj.update({"feat_src": new})
    lin.linearize()
    table = packed._table
    assert float((lin.Atb - before).abs().max()) > 1e-4
    jac, err = obj.cost_functions["align"].weighted_jacobians_error()
    assert_blocks_close(packed._Jv[0][0].numpy(), jac[0].numpy(), 1e-12, "block after the replacement")
    before = lin.Atb.clone()
    with torch.no_grad():
        new.mul_(1.3)
    lin.linearize()
    assert packed._table is table and float((lin.Atb - before).abs().max()) > 1e-4
    jac, err = obj.cost_functions["align"].weighted_jacobians_error()
    assert_blocks_close(packed._Jv[0][0].numpy(), jac[0].numpy(), 1e-12, "block after the edit in place")


def test_packed_for_selects_the_family():
    import theseus_amd as th
    from tests.homog_oracle_kernels import HomogOracleKernels
    from theseus_amd.packed import packed_for
    g = load_golden(FIXTURES[0])
    obj, _, _ = build(th, g)
    K = HomogOracleKernels()
    assert type(packed_for(obj, K)).__name__ == "PackedHomography" and th.PackedHomography is type(packed_for(obj, K))
    # Difference costs alone stay on the generic path
    only = th.Objective(dtype=torch.float64)
    only.add(obj.cost_functions["prior"])
    assert type(packed_for(only, K)).__name__ == "PackedEuclidean"
    with pytest.raises(th.UnsupportedObjective, match="at least one"):
        th.PackedHomography(only, K)
    # ... and so does an objective with any other cost
    v = obj.optim_vars["H8"]
    obj.add(th.AutoDiffCostFunction([v], lambda optim_vars, aux_vars: optim_vars[0].tensor[:, :2] ** 2, 2, name="extra"))
    assert type(packed_for(obj, K)).__name__ == "PackedEuclidean"


def test_wrong_weights_and_shapes_are_refused_by_name():
    import theseus_amd as th
    from tests.homog_oracle_kernels import HomogOracleKernels
    dt = torch.float64
    h = th.Vector(tensor=torch.tensor([[1.0, 0, 0, 0, 1, 0, 0, 0]], dtype=dt), name="h")
    a, b = torch.zeros(1, 2, 6, 7, dtype=dt), torch.zeros(1, 2, 6, 8, dtype=dt)
    with pytest.raises(ValueError, match="bad_shapes.*feat_src"):
        th.eb.HomographyAlignment(h, a, b, name="bad_shapes")
    with pytest.raises(ValueError, match="bad_weight.*1-dimensional"):
        th.eb.HomographyAlignment(h, a, a.clone(), th.DiagonalCostWeight(torch.ones(1, 2, dtype=dt)), name="bad_weight")
    with pytest.raises(ValueError, match="dof 8"):
        th.eb.HomographyAlignment(th.Vector(7, dtype=dt), a, a.clone())
    assert th.eb.HomographyAlignment(h, a, a.clone(), th.DiagonalCostWeight(torch.ones(1, 1, dtype=dt))).dim() == 1
    # feature maps replaced after construction: the packer refuses them, naming the cost
    obj, _, _ = build(th, load_golden(FIXTURES[0]))
    lin = th.HipLinearization(obj, kernels=HomogOracleKernels())
    lin.linearize()
    obj.get_variable("feat_dst").tensor = torch.zeros(1, 2, 6, 8, dtype=dt)   # (Objective.update itself refuses another shape)
    with pytest.raises(ValueError, match="align.*feat_dst"):
        lin.linearize()
    # a Diagonal weight of the wrong width on the prior
    obj = th.Objective(dtype=dt)
    obj.add(th.eb.HomographyAlignment(h, a, a.clone(), name="al"))
    obj.add(th.Difference(h, th.Vector(tensor=torch.zeros(1, 8, dtype=dt), name="t"), th.DiagonalCostWeight(torch.ones(1, 3, dtype=dt)),
                          name="narrow_prior"))
    with pytest.raises(ValueError, match="narrow_prior.*8-dimensional"):
        th.HipLinearization(obj, kernels=HomogOracleKernels()).linearize()


def test_header_library_and_ctypes_table_agree(lib_path):  # noqa: F811
    from theseus_amd import _lib
    text = open(os.path.join(ROOT, "include", "theseus_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, nargs in zip(NAMES, (16, 12)):
        assert name in declared_symbols() and name in _lib.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(lib_path), name)
        assert len(_lib._SIGNATURES[name]) == nargs
        proto = re.search(name + r"\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
        assert len(proto.split(",")) == nargs
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert _lib.load().thx_abi_version() == 30 == _lib.ABI_VERSION
    for macro, value in (("THX_HOMOG_ALIGN", _lib.HOMOG_ALIGN), ("THX_HOMOG_PRIOR", _lib.HOMOG_PRIOR),
                         ("THX_HOMOG_CHUNK", _lib.THX_HOMOG_CHUNK), ("THX_HOMOG_SUMS", _lib.THX_HOMOG_SUMS)):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", header).group(1)) == value
    from theseus_amd.homography import HOMOG_TERM
    assert HOMOG_TERM.itemsize == 128 and "homog_kernels.hip" in __import__("theseus_amd.build", fromlist=["SOURCES"]).SOURCES


def test_bad_arguments_are_refused_before_any_launch(lib_path):  # noqa: F811
    from theseus_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    ok = dict(terms=p, n_terms=3, n_align=2, x=p, ldx=16, n=16, scratch=p, chunks=5, J=p, j_total=80, e=p, lde=10, m=10, err=p, B=2,
              dtype=0, stream=None)
    orders = {"thx_homog_eval": ("terms", "n_terms", "n_align", "x", "ldx", "n", "scratch", "chunks", "J", "j_total", "e", "lde", "m",
                                 "B", "dtype", "stream"),
              "thx_homog_error": ("terms", "n_terms", "n_align", "x", "ldx", "n", "scratch", "chunks", "err", "B", "dtype", "stream")}
    for fname, order in orders.items():
        f = getattr(lib, fname)

        def refused(needle, **kw):
            a = dict(ok, **kw)
            rc = f(*[a[k] for k in order])
            return rc == -1 and needle in lib.thx_last_error() and fname.encode() in lib.thx_last_error()
        for name in order:
            if isinstance(ok[name], ctypes.c_void_p):
                assert refused(b"null pointer", **{name: None}), (fname, name)
                assert refused(b"aligned", **{name: ctypes.c_void_p(4098)}), (fname, name)
        assert refused(b"dtype", dtype=7) and refused(b"dtype", dtype=-1)
        assert refused(b"n_terms", n_terms=0) and refused(b"batch", B=0) and refused(b"batch", B=-3)
        assert refused(b"ldx < n", ldx=15) and refused(b"n < 8", n=7)
        assert refused(b"n_align", n_align=0) and refused(b"n_align", n_align=4) and refused(b"chunks < 1", chunks=0)
        assert refused(b"aligned", x=ctypes.c_void_p(4100), dtype=1)   # fp64 needs 8 bytes
        assert refused(b"aligned", scratch=ctypes.c_void_p(4100))      # the scratch is fp64 in either dtype
        assert refused(b"grid limit exceeded (n_align * B * chunks)", chunks=2 ** 30)
        assert refused(b"grid limit exceeded (n_align * B * chunks)", n_align=3, B=2 ** 30, chunks=1)
    f = lib.thx_homog_eval
    assert f(p, 3, 2, p, 16, 16, p, 5, p, 80, p, 9, 10, 2, 0, None) == -1 and b"lde < m" in lib.thx_last_error()
    assert f(p, 3, 2, p, 16, 16, p, 5, p, 7, p, 10, 10, 2, 0, None) == -1 and b"j_total" in lib.thx_last_error()
    assert (f(p, 2 ** 31 - 1, 1, p, 16, 16, p, 1, p, 80, p, 10, 10, 2 ** 31 - 1, 0, None) == -1
            and b"grid limit exceeded (n_terms * B)" in lib.thx_last_error())


def test_argument_checks_under_the_host_sanitizers(tmp_path):
    """A stand-alone program (tests/hostmath/homog_args.cpp) linked with csrc/homog_kernels.hip alone, host code built with
    AddressSanitizer + UndefinedBehaviorSanitizer: every bad call is refused, nothing is launched, the sanitizers stay quiet."""
    from theseus_amd import build as b
    exe = str(tmp_path / "homog_args")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wno-unused-value", "-Wno-pass-failed",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), "-I" + b.CSRC, os.path.join(ROOT, "tests", "hostmath", "homog_args.cpp"),
                    os.path.join(b.CSRC, "homog_kernels.hip"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "ALL REFUSED" in run.stdout, run.stdout + run.stderr


def run_implicit_with_nothing_to_differentiate(th, g, kernels, monkeypatch, device="cpu"):
    """``backward_mode="implicit"`` under no_grad; every torch evaluation of a cost function is refused -> (optimizer, final H8)"""
    def refuse(*a, **kw):
        raise AssertionError("a cost function was evaluated by torch although nothing is differentiated")
    for cls in (th.eb.HomographyAlignment, th.Difference):
        for method in ("error", "jacobians"):
            monkeypatch.setattr(cls, method, refuse)
    obj, _, _ = build(th, g, device=device)
    opt = th.LevenbergMarquardt(obj, linearization_kwargs=dict(kernels=kernels) if kernels is not None else {}, **LM_KW)
    with torch.no_grad():
        sol, _ = th.TheseusLayer(opt).forward(None, optimizer_kwargs=dict(damping=LM_DAMPING, backward_mode="implicit"))
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedHomography"
    return opt, sol["H8"]


def test_implicit_mode_under_no_grad_stays_fused(monkeypatch):
    import theseus_amd as th
    from tests.homog_oracle_kernels import HomogOracleKernels
    g = load_golden(FIXTURES[1])
    K = HomogOracleKernels()
    _, final = run_implicit_with_nothing_to_differentiate(th, g, K, monkeypatch)
    assert K.calls["homog_eval"] >= 2 and not final.requires_grad
    np.testing.assert_allclose(final.numpy(), g["implicit_final"], rtol=1e-8, atol=1e-10)
