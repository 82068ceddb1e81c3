"""CPU-side (-m "not gpu") checks of 2D motion planning (theseus_amd/embodied.py, csrc/traj_kernels.hip): the torch classes and the
generic path against the REAL reference's fixtures (tests/golden/traj2_f64_*.npz, tools/gen_traj2_golden.py), the C ABI of the two
new exports, their argument checks (through ctypes and in a stand-alone program under the host sanitizers), and which packed family
``packed_for`` selects.  GPU twin: tests/test_gpu_traj2.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.helpers import load_golden
from tests.test_cabi_and_host import declared_symbols, lib_path  # noqa: F401  (lib_path: the session fixture that builds)
from tests.traj2_common import ALL_CASES, FIXTURES, LM_DAMPING, LM_KW, build, classify, slice_aux, state_of

NAMES = ("thx_traj2_eval", "thx_traj2_error")


def assert_blocks_close(got, want, rel, what):
    """every block to ``rel`` of ITS largest magnitude"""
    scale = float(np.abs(want).max())
    err = float(np.abs(np.asarray(got) - want).max())
    assert err <= rel * max(scale, np.finfo(np.float64).tiny), f"{what}: {err:.3e} > {rel:.0e} * {scale:.3e}"


@pytest.mark.parametrize("fixture", FIXTURES)
def test_torch_classes_reproduce_the_reference_blocks(fixture):
    """Each value is a few dozen flops on inputs of order 1 (weights up to ~800): 1e-12 of the block's largest magnitude is four
    orders above fp64 rounding and far below any formula error."""
    import theseus_amd as th
    g = load_golden(fixture)
    obj, _, costs = build(th, g)
    assert costs == g["cost_order"].tolist() and list(obj.optim_vars) == g["var_order"].tolist()
    for name, c in obj.cost_functions.items():
        jac, err = c.weighted_jacobians_error()
        assert_blocks_close(err.numpy(), g[f"we_{name}"], 1e-12, f"{name} error")
        assert_blocks_close(c.weighted_error().numpy(), g[f"we_{name}"], 1e-12, f"{name} weighted_error")
        for s, j in enumerate(jac):
            assert_blocks_close(j.expand(3, -1, -1).numpy(), g[f"wj_{name}_{s}"], 1e-12, f"{name} block {s}")
    assert_blocks_close(obj.error().numpy(), g["error"], 1e-12, "error vector")


def test_fixtures_cover_the_cases_of_the_sdf():
    covered = set()
    for fixture in FIXTURES:
        covered |= classify(load_golden(fixture))
    assert covered == ALL_CASES


def test_gp_cost_weight_matches_the_reference():
    """The fixture's gp_0 blocks for pose2 / vel2 are U [I; 0] and U [0; I]: together the reference's weight matrix.  (Its gradient
    w.r.t. Qc_inv: test_generic_path_implicit_gradients_reproduce_the_reference.)"""
    import theseus_amd as th
    for fixture in FIXTURES:
        g = load_golden(fixture)
        w = th.eb.GPCostWeight(th.Variable(torch.from_numpy(g["Qc_inv"])), th.Variable(torch.from_numpy(g["dt"])))
        want = np.concatenate([g["wj_gp_0_2"], g["wj_gp_0_3"]], axis=2)
        assert_blocks_close(w.cost_weight_matrix().expand(3, -1, -1).numpy(), want, 1e-12, "U")
    with pytest.raises(ValueError, match="GPCostWeight"):
        one = th.Vector(2, dtype=torch.float64)
        th.eb.GPMotionModel(one, one.copy(), one.copy(), one.copy(), 0.5, th.ScaleCostWeight(1.0))


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


def check_iterates(g, info, names):
    """tests/test_gpu_generic.py's tolerance for the LM iterates of its reference fixture in fp64 (simple_example_common.py:
    rtol 1e-8, atol 1e-10; the error history at rtol 1e-6)"""
    got = torch.cat([info.state_history[k] for k in names], dim=1).permute(2, 0, 1).double().numpy()
    np.testing.assert_allclose(got, g["lm_iterates"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(info.err_history.numpy(), g["lm_err_history"], rtol=1e-6)


def check_implicit_gradients(g, leaves, sol, names):
    """the generic path's tolerance for implicit LM gradients (simple_example_common.py: 1e-6 of the gradient's largest entry)"""
    final = state_of(sol, names)
    np.testing.assert_allclose(final.detach().cpu().numpy(), g["implicit_final"], rtol=1e-8, atol=1e-10)
    (final ** 2).sum().backward()
    for k, leaf in leaves.items():
        want = g[f"grad_{k}"]
        np.testing.assert_allclose(leaf.grad.cpu().numpy(), want, rtol=0, atol=1e-6 * np.abs(want).max(), err_msg=k)


@pytest.mark.parametrize("fixture", FIXTURES)
def test_generic_path_lm_reproduces_the_reference_iterates(fixture):
    import theseus_amd as th
    from tests.oracle_kernels import OracleKernels
    g = load_golden(fixture)
    with torch.no_grad():
        obj, opt, _, sol, info = _lm(th, g, OracleKernels(), track_err_history=True, track_state_history=True)
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedEuclidean"   # (these kernels have no traj2_eval)
    check_iterates(g, info, g["var_order"].tolist())


@pytest.mark.parametrize("fixture", FIXTURES)
def test_generic_path_implicit_gradients_reproduce_the_reference(fixture):
    """sdf_data, cost_eps, Qc_inv (through GPCostWeight's Cholesky) and the start / goal targets"""
    import theseus_amd as th
    from tests.oracle_kernels import OracleKernels
    g = load_golden(fixture)
    _, _, leaves, sol, _ = _lm(th, g, OracleKernels(), backward_mode="implicit")
    check_implicit_gradients(g, leaves, sol, g["var_order"].tolist())


@pytest.mark.parametrize("fixture", FIXTURES)
def test_packed_trajectory_on_the_stand_in_kernels(fixture):
    """The packer's term table, decoded by the numpy stand-in of the two kernels: linearization, LM iterates, implicit gradients."""
    import theseus_amd as th
    from tests.traj2_oracle_kernels import Traj2OracleKernels
    g = load_golden(fixture)
    K = Traj2OracleKernels()
    obj, _, _ = build(th, g)
    lin = th.HipLinearization(obj, kernels=K)
    assert type(lin.packed).__name__ == "PackedTrajectory2D"
    lin.linearize()
    assert K.calls["traj2_eval"] == 1
    assert_blocks_close(torch.tril(lin.AtA).numpy(), np.tril(g["AtA"]), 1e-12, "AtA")
    assert_blocks_close(lin.Atb.squeeze(2).numpy(), g["Atb"], 1e-12, "Atb")
    assert_blocks_close(obj.error_metric().numpy(), g["error_metric"], 1e-12, "error metric")
    assert K.calls["traj2_error"] == 1
    with torch.no_grad():
        _, opt, _, _, info = _lm(th, g, K, track_err_history=True, track_state_history=True)
    check_iterates(g, info, g["var_order"].tolist())
    _, _, leaves, sol, _ = _lm(th, g, K, backward_mode="implicit")
    check_implicit_gradients(g, leaves, sol, g["var_order"].tolist())


@pytest.mark.parametrize("mode,kw", [("unroll", {}), ("truncated", dict(backward_num_iterations=2))])
def test_unrolled_gradients_on_the_fused_family_equal_the_generic_path(mode, kw):
    """The differentiated iterations are the parent's torch evaluation on both families; the iterations before them (TRUNCATED) are
    fused on one and torch on the other, equal to a few ulp: gradients to 1e-9 of their largest entry."""
    import theseus_amd as th
    from tests.oracle_kernels import OracleKernels
    from tests.traj2_oracle_kernels import Traj2OracleKernels
    g = load_golden(FIXTURES[1])
    grads = {}
    for name, K in (("fused", Traj2OracleKernels()), ("generic", OracleKernels())):
        _, opt, leaves, sol, _ = _lm(th, g, K, backward_mode=mode, **kw)
        assert type(opt.linear_solver.linearization.packed).__name__ == {"fused": "PackedTrajectory2D", "generic": "PackedEuclidean"}[name]
        (state_of(sol, g["var_order"].tolist()) ** 2).sum().backward()
        grads[name] = {k: v.grad.numpy() for k, v in leaves.items()}
    for k, want in grads["generic"].items():
        assert np.abs(want).max() > 0
        np.testing.assert_allclose(grads["fused"][k], want, rtol=0, atol=1e-9 * np.abs(want).max(), err_msg=k)


def test_packed_for_selects_the_family():
    import theseus_amd as th
    from tests.traj2_oracle_kernels import Traj2OracleKernels
    from theseus_amd.packed import packed_for
    g = load_golden(FIXTURES[0])
    obj, _, _ = build(th, g)
    assert type(packed_for(obj, Traj2OracleKernels())).__name__ == "PackedTrajectory2D"
    v = obj.optim_vars["pose_3"]
    obj.add(th.AutoDiffCostFunction([v], lambda optim_vars, aux_vars: optim_vars[0].tensor ** 2, 2, name="extra"))
    assert type(packed_for(obj, Traj2OracleKernels())).__name__ == "PackedEuclidean"


def test_out_of_scope_arguments_are_refused():
    import theseus_amd as th
    dt = torch.float64
    sdf, origin = torch.zeros(1, 4, 5, dtype=dt), torch.zeros(1, 2, dtype=dt)
    with pytest.raises(ValueError, match="SE2"):
        th.eb.Collision2D(th.SE2(dtype=dt), origin, sdf, 0.25, 0.1, th.ScaleCostWeight(1.0))
    with pytest.raises(NotImplementedError, match="occupancy_map"):
        th.eb.SignedDistanceField2D(origin, 0.25, occupancy_map=torch.zeros(1, 4, 5, dtype=dt))


def test_header_library_and_ctypes_table_agree(lib_path):  # noqa: F811
    from theseus_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "theseus_hip.h")).read(), flags=re.S)
    for name, nargs in zip(NAMES, (13, 9)):
        assert name in declared_symbols() and name in _lib.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(lib_path), name)
        assert len(_lib._SIGNATURES[name]) == nargs
        proto = re.search(name + r"\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
        assert len(proto.split(",")) == nargs
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert _lib.load().thx_abi_version() == 30 == _lib.ABI_VERSION
    from theseus_amd.embodied import TRAJ2_TERM
    assert TRAJ2_TERM.itemsize == 128 and "traj_kernels.hip" in __import__("theseus_amd.build", fromlist=["SOURCES"]).SOURCES


def test_bad_arguments_are_refused_before_any_launch(lib_path):  # noqa: F811
    from theseus_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    ok = dict(terms=p, n_terms=3, x=p, ldx=28, n=28, J=p, j_total=40, e=p, lde=12, m=12, err=p, B=2, dtype=0, stream=None)
    orders = {"thx_traj2_eval": ("terms", "n_terms", "x", "ldx", "n", "J", "j_total", "e", "lde", "m", "B", "dtype", "stream"),
              "thx_traj2_error": ("terms", "n_terms", "x", "ldx", "n", "err", "B", "dtype", "stream")}
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
        assert refused(b"ldx < n", ldx=27) and refused(b"n < 2", n=1)
        assert refused(b"aligned", x=ctypes.c_void_p(4100), dtype=1)   # fp64 needs 8 bytes
    f = lib.thx_traj2_eval
    assert f(p, 3, p, 28, 28, p, 40, p, 11, 12, 2, 0, None) == -1 and b"lde < m" in lib.thx_last_error()
    assert f(p, 3, p, 28, 28, p, 0, p, 12, 12, 2, 0, None) == -1 and b"j_total" in lib.thx_last_error()
    assert f(p, 2 ** 31 - 1, p, 28, 28, p, 40, p, 12, 12, 2 ** 31 - 1, 0, None) == -1 and b"grid limit" in lib.thx_last_error()


def test_argument_checks_under_the_host_sanitizers(tmp_path):
    """A stand-alone program (tests/hostmath/traj2_args.cpp) linked with csrc/traj_kernels.hip alone, host code built with
    AddressSanitizer + UndefinedBehaviorSanitizer: every bad call is refused, nothing is launched, the sanitizers stay quiet."""
    from theseus_amd import build as b
    exe = str(tmp_path / "traj2_args")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wno-unused-value", "-Wno-pass-failed",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), "-I" + b.CSRC, os.path.join(ROOT, "tests", "hostmath", "traj2_args.cpp"),
                    os.path.join(b.CSRC, "traj_kernels.hip"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "ALL REFUSED" in run.stdout, run.stdout + run.stderr


def assert_blocks_equal_the_torch_classes(packed, rel):
    """the fused evaluation's blocks and errors <-> the torch classes at the same state, each to ``rel`` of its largest magnitude"""
    Jv, ev = packed._eval()
    for c, cost in enumerate(packed.costs):
        jac, err = cost.weighted_jacobians_error()
        for k, (got, want) in enumerate([(ev[c], err)] + list(zip(Jv[c], jac))):
            assert_blocks_close(got.numpy(), want.expand_as(got).numpy(), rel, f"{cost.name} {'error' if k == 0 else f'block {k - 1}'}")


def test_sliced_auxiliaries_are_read_in_place():
    """Slices of larger batched tensors (dense per problem, non-contiguous as a whole) go into the term table with their own batch
    stride: no private copy, so the table is built once and an in-place edit of the parent tensor is seen.  An auxiliary whose
    per-problem values are NOT dense still gets its private copy, and the table is then looked at again at every call."""
    import theseus_amd as th
    from tests.traj2_oracle_kernels import Traj2OracleKernels
    g = load_golden(FIXTURES[1])
    obj, _, _ = build(th, g)
    parents = slice_aux(obj, g)
    lin = th.HipLinearization(obj, kernels=Traj2OracleKernels())
    lin.linearize()
    packed = lin.packed
    assert type(packed).__name__ == "PackedTrajectory2D"
    table, key = packed._table, packed._aux_key
    assert key is not None
    assert_blocks_equal_the_torch_classes(packed, 1e-12)
    assert_blocks_close(lin.Atb.squeeze(2).numpy(), g["Atb"], 1e-12, "Atb")   # (the same values as the fixture's own tensors)
    obj.error_metric()
    packed.sync(deep=True)
    assert packed._table is table
    with torch.no_grad():
        parents["cost_eps"][:, 1] += 0.3
        parents["sdf_data"][:, 0] *= 0.8
        parents["start"][:, 2:4] -= 0.05
    before = lin.Atb.clone()
    lin.linearize()
    assert packed._table is table and float((lin.Atb - before).abs().max()) > 1e-3
    assert_blocks_equal_the_torch_classes(packed, 1e-12)
    # every second column of a (B, 4) tensor: one problem's two values are not adjacent
    wide = torch.full((3, 4), -7.0, dtype=torch.float64)
    wide[:, ::2] = torch.from_numpy(g["goal"]) + 0.1
    obj.get_variable("goal").tensor = wide[:, ::2]
    assert not wide[:, ::2][0].is_contiguous()
    lin.linearize()
    assert packed._aux_key is None and packed._table is not table
    assert_blocks_equal_the_torch_classes(packed, 1e-12)
    with torch.no_grad():
        wide[:, ::2] += 0.2
    before = lin.Atb.clone()
    lin.linearize()   # (the copy is made again)
    assert float((lin.Atb - before).abs().max()) > 1e-3
    assert_blocks_equal_the_torch_classes(packed, 1e-12)


def run_implicit_with_nothing_to_differentiate(th, g, kernels, how, monkeypatch, device="cpu"):
    """``backward_mode="implicit"`` under no_grad (``how`` = "no_grad") or with no leaf requiring grad ("no_leaf"); every torch
    evaluation of a cost function is refused -> (optimizer, the final state (B, n))"""
    def refuse(*a, **kw):
        raise AssertionError("a cost function was evaluated by torch although nothing is differentiated")
    for cls in (th.eb.Collision2D, th.eb.DoubleIntegrator, th.Difference):
        for method in ("error", "jacobians"):
            monkeypatch.setattr(cls, method, refuse)
    obj, _, _ = build(th, g, device=device)
    opt = th.LevenbergMarquardt(obj, linearization_kwargs=dict(kernels=kernels) if kernels is not None else {}, **LM_KW)
    with torch.set_grad_enabled(how == "no_leaf"):
        sol, _ = th.TheseusLayer(opt).forward(None, optimizer_kwargs=dict(damping=LM_DAMPING, backward_mode="implicit"))
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedTrajectory2D"
    return opt, state_of(sol, g["var_order"].tolist())


@pytest.mark.parametrize("how", ["no_grad", "no_leaf"])
def test_implicit_mode_with_nothing_to_differentiate_stays_fused(how, monkeypatch):
    """The implicit last step linearizes with ``graph=True``; with nothing to differentiate it is one more thx_traj2_eval, and the
    result is the reference's state after its implicit run (check_implicit_gradients' tolerance for that state)."""
    import theseus_amd as th
    from tests.traj2_oracle_kernels import Traj2OracleKernels
    g = load_golden(FIXTURES[1])
    K = Traj2OracleKernels()
    _, final = run_implicit_with_nothing_to_differentiate(th, g, K, how, monkeypatch)
    assert K.calls["traj2_eval"] >= 2 and not final.requires_grad
    np.testing.assert_allclose(final.numpy(), g["implicit_final"], rtol=1e-8, atol=1e-10)
