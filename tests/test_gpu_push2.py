"""-m gpu: planar pushing on SE2 on the fused kernels (csrc/push_kernels.hip: thx_push2_eval, thx_push2_error; theseus_amd/pushing.py:
PackedPlanarPushing) against the torch classes and against the REAL reference's fixtures (tests/golden/push2_f64_*.npz).  CPU twin:
tests/test_push2_host.py.

Bounds.  fp64: every block and error within 1e-12 of its largest magnitude of the torch classes in fp64 (tests/test_gpu_traj2.py's).
fp32: a kernel's block may be at most F32_FACTOR = 4 x as far from the fp64 value as the REFERENCE's own fp32 evaluation of the
same fp32-rounded inputs is (recorded per block in the fixtures: f32d_*), with a floor of 16 * 2^-23 of the block's largest
magnitude for blocks the reference happens to get exactly.  Away from the fixtures (the random problems) the torch classes, which
reproduce the reference to 1e-12, stand in for it: the same rule with their fp32 evaluation."""
import numpy as np
import pytest
import torch

from tests.helpers import load_golden
from tests.push2_common import F32_FACTOR, F32_FLOOR, FIXTURES, build, random_problem, window_pairs
from tests.test_push2_host import _lm, check_implicit_gradients, check_iterates
from tests.test_traj2_host import assert_blocks_close

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _packed(th, obj):
    lin = th.HipLinearization(obj)
    assert type(lin.packed).__name__ == "PackedPlanarPushing" and type(lin.K).__name__ == "HipKernels"
    return lin, lin.packed


def _torch_blocks(th, f, dtype, **kw):
    """{cost: [error, block 0, ...]} of the torch classes on the CPU in ``dtype`` (fp32: of the fp32-rounded inputs), as float64"""
    obj, _, _ = build(th, f, dtype=dtype, **kw)
    B = f["obj0"].shape[0]
    out = {}
    for name, c in obj.cost_functions.items():
        jac, err = c.weighted_jacobians_error()
        out[name] = [err.expand(B, -1).double().numpy()] + [j.expand(B, -1, -1).double().numpy() for j in jac]
    return out


def compare(packed, want, bound, label):
    """thx_push2_eval's blocks and errors, thx_push2_error's metric against ``want`` ({cost: [error, blocks...]} in fp64);
    ``bound(cost, k, scale)`` = the largest admissible absolute difference of entry k.  Prints the worst ratio to the bound."""
    Jv, ev = packed._eval()
    metric = packed.error_metric().double().cpu().numpy()
    worst, total, slack, worst_at = 0.0, 0.0, 0.0, None
    for c, cost in enumerate(packed.costs):
        got = [ev[c]] + list(Jv[c])
        total = total + (want[cost.name][0] ** 2).sum(1)
        for k, (g, w) in enumerate(zip(got, want[cost.name])):
            scale = float(np.abs(w).max())
            diff = float(np.abs(g.double().cpu().numpy() - w).max())
            lim = bound(cost.name, k, scale)
            if k == 0:   # what errors within their bounds can move 0.5 * sum(e^2) by
                slack = slack + (np.abs(w) * lim + 0.5 * lim * lim).sum(1)
            if diff > worst * lim:
                worst, worst_at = (diff / lim if lim else np.inf), (cost.name, k, diff, lim)
            assert diff <= lim, f"{label}: {cost.name} {'error' if k == 0 else f'block {k - 1}'}: {diff:.3e} > {lim:.3e} (scale {scale:.3e})"
    print(f"{label}: worst difference / bound = {worst:.3f} at {worst_at}")
    return metric, 0.5 * total, slack


def f64_bound(name, k, scale):
    return 1e-12 * scale


@pytest.mark.parametrize("fixture", FIXTURES)
def test_fp64_kernels_match_the_torch_classes_at_the_fixture_inputs(fixture):
    import theseus_amd as th
    g = load_golden(fixture)
    obj, _, _ = build(th, g, device=DEV)
    _, packed = _packed(th, obj)
    metric, want, _ = compare(packed, _torch_blocks(th, g, torch.float64), f64_bound, fixture)
    np.testing.assert_allclose(metric, want, rtol=1e-12)
    assert float((packed.error_vector().cpu() - torch.from_numpy(g["error"])).abs().max()) <= 1e-12 * np.abs(g["error"]).max()


@pytest.mark.parametrize("fixture", FIXTURES)
def test_fp32_kernels_stay_within_four_times_the_references_own_fp32_distance(fixture):
    """Against the fp64 FIXTURE (the reference's blocks), every block of every cost; measured worst ratios: DESIGN.md 4.11."""
    import theseus_amd as th
    g = load_golden(fixture)
    obj, _, _ = build(th, g, device=DEV, dtype=torch.float32)
    _, packed = _packed(th, obj)
    want = {n: [g[f"we_{n}"]] + [g[f"wj_{n}_{s}"] for s in range(len(c.optim_vars()))] for n, c in obj.cost_functions.items()}

    def bound(name, k, scale):
        ref = float(g[f"f32d_we_{name}"] if k == 0 else g[f"f32d_wj_{name}_{k - 1}"])
        return max(F32_FACTOR * ref, F32_FLOOR * scale)
    metric, _, slack = compare(packed, want, bound, fixture + " fp32")
    # the metric: what errors within their bounds can move it by, plus the rounding of the fp32 result
    assert (np.abs(metric - g["error_metric"]) <= slack + 2.0 ** -23 * g["error_metric"]).all()


def _compare_random(th, f, T, dtype):
    obj, _, _ = build(th, f, device=DEV, dtype=dtype, T=T)
    _, packed = _packed(th, obj)
    exact = _torch_blocks(th, f, torch.float64, T=T) if dtype == torch.float64 else None
    if dtype == torch.float64:
        metric, want, _ = compare(packed, exact, f64_bound, f"random T={T} fp64")
        np.testing.assert_allclose(metric, want, rtol=1e-12)
    else:
        f32 = {k: np.asarray(v, np.float32).astype(np.float64) for k, v in f.items()}
        exact, own = _torch_blocks(th, f32, torch.float64, T=T), _torch_blocks(th, f32, torch.float32, T=T)

        def bound(name, k, scale):
            return max(F32_FACTOR * float(np.abs(own[name][k] - exact[name][k]).max()), F32_FLOOR * scale)
        metric, want, slack = compare(packed, exact, bound, f"random T={T} fp32")
        assert (np.abs(metric - want) <= slack + 2.0 ** -23 * want).all()
    return packed


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_kernels_match_the_torch_classes_on_a_random_problem(dtype):
    """B = 70 (no multiple of the wave size), T = 12: 1 + 11 + 17 + 12 + 12 = 53 terms, kind boundaries inside waves, a tenth of
    the effectors outside the grid"""
    import theseus_amd as th
    packed = _compare_random(th, random_problem(70, 12, seed=5), 12, dtype)
    assert len(packed.costs) == 53 and packed.n == 72 and packed.batch == 70


def test_more_than_256_terms():
    """T = 96, B = 5: 1 + 95 + 185 + 96 + 96 = 473 terms -- thx_push2_error's stride loop and more than one workgroup row of
    thx_push2_eval (473 * 5 threads); error metric and blocks only"""
    import theseus_amd as th
    packed = _compare_random(th, random_problem(5, 96, seed=9), 96, torch.float64)
    assert len(packed.costs) == 1 + 95 + len(window_pairs(96)) + 96 + 96 > 256


@pytest.mark.parametrize("fixture", FIXTURES)
def test_fused_assemble_matches_the_reference(fixture):
    import theseus_amd as th
    g = load_golden(fixture)
    obj, _, _ = build(th, g, device=DEV)
    lin, _ = _packed(th, obj)
    lin.linearize()
    assert_blocks_close(torch.tril(lin.AtA).cpu().numpy(), np.tril(g["AtA"]), 1e-12, "AtA")
    assert_blocks_close(lin.Atb.squeeze(2).cpu().numpy(), g["Atb"], 1e-12, "Atb")
    assert_blocks_close(obj.error_metric().cpu().numpy(), g["error_metric"], 1e-12, "error metric")


@pytest.mark.parametrize("fixture", FIXTURES)
def test_fused_lm_reproduces_the_reference_iterates(fixture):
    import theseus_amd as th
    g = load_golden(fixture)
    with torch.no_grad():
        _, opt, _, _, info = _lm(th, g, None, device=DEV, track_err_history=True, track_state_history=True)
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedPlanarPushing"
    check_iterates(g, info, g["var_order"].tolist())


@pytest.mark.parametrize("fixture", FIXTURES)
def test_implicit_gradients_reproduce_the_reference(fixture):
    import theseus_amd as th
    g = load_golden(fixture)
    _, opt, leaves, sol, _ = _lm(th, g, None, device=DEV, backward_mode="implicit")
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedPlanarPushing"
    check_implicit_gradients(g, leaves, sol, g["var_order"].tolist())


def test_the_fused_path_is_really_taken(monkeypatch):
    """No cost function is evaluated by torch in a no_grad LM run: one thx_push2_eval per linearization, thx_push2_error for every
    error metric."""
    import theseus_amd as th
    g = load_golden(FIXTURES[0])
    K = th.HipKernels()
    calls = {"push2_eval": 0, "push2_error": 0, "block_assemble_strided": 0}
    for name in calls:
        def counted(*a, _f=getattr(K, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(K, name, counted)

    def refuse(*a, **kw):
        raise AssertionError("a cost function was evaluated by torch on the fused path")
    for cls in (th.eb.QuasiStaticPushingPlanar, th.eb.MovingFrameBetween, th.eb.EffectorObjectContactPlanar, th.Difference):
        for method in ("error", "jacobians"):
            monkeypatch.setattr(cls, method, refuse)
    linearizations, metrics = {"n": 0}, {"n": 0}
    real = th.HipLinearization._assemble

    def counting_assemble(self):
        linearizations["n"] += 1
        return real(self)
    monkeypatch.setattr(th.HipLinearization, "_assemble", counting_assemble)
    real_metric = th.PackedPlanarPushing.error_metric

    def counting_metric(self, *a, **kw):
        metrics["n"] += 1
        return real_metric(self, *a, **kw)
    monkeypatch.setattr(th.PackedPlanarPushing, "error_metric", counting_metric)
    with torch.no_grad():
        _, opt, _, _, info = _lm(th, g, K, device=DEV, track_err_history=True, track_state_history=True)
    assert opt.linear_solver.linearization.K is K
    assert linearizations["n"] >= 5 and calls["push2_eval"] == linearizations["n"] == calls["block_assemble_strided"]
    assert metrics["n"] >= 6 and calls["push2_error"] == metrics["n"]   # the initial error + one per iteration
    check_iterates(g, info, g["var_order"].tolist())


def test_replaced_aux_values_are_seen_by_the_next_call():
    import theseus_amd as th
    g = load_golden(FIXTURES[0])
    obj, _, _ = build(th, g, device=DEV)
    lin, packed = _packed(th, obj)
    lin.linearize()
    H0, e0, table0 = lin.AtA.clone(), obj.error_metric().clone(), packed._table

    def expected():
        h = dict(g)
        h["eff_radius"], h["sdf_data"] = obj.get_variable("eff_radius").tensor.cpu().numpy(), obj.get_variable("sdf_data").tensor.cpu().numpy()
        return _torch_blocks(th, h, torch.float64)
    new_radius = torch.tensor([[0.3]], dtype=torch.float64, device=DEV)
    new_sdf = torch.from_numpy(g["sdf_data"]).to(DEV) * 0.8 - 0.05
    obj.update({"eff_radius": new_radius, "sdf_data": new_sdf})
    lin.linearize()
    assert packed._table is not table0
    assert float((lin.AtA - H0).abs().max()) > 1e-3 and float((obj.error_metric() - e0).abs().max()) > 1e-3
    metric, want, _ = compare(packed, expected(), f64_bound, "replaced")
    np.testing.assert_allclose(metric, want, rtol=1e-12)
    # in-place edits of an auxiliary tensor need no rebuild: the table points at the tensor itself
    table1 = packed._table
    new_radius.fill_(0.02)
    metric, want, _ = compare(packed, expected(), f64_bound, "edited in place")
    np.testing.assert_allclose(metric, want, rtol=1e-12)
    assert packed._table is table1


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_two_evaluations_of_one_state_are_bitwise_equal(dtype):
    import theseus_amd as th
    obj, _, _ = build(th, random_problem(70, 12, seed=7), device=DEV, dtype=dtype, T=12)
    _, packed = _packed(th, obj)
    packed._eval()
    J1, e1, m1 = packed._J.clone(), packed._e.clone(), packed.error_metric().clone()
    packed._J.fill_(float("nan"))
    packed._e.fill_(float("nan"))
    packed._eval()
    assert torch.equal(J1, packed._J) and torch.equal(e1, packed._e) and torch.equal(m1, packed.error_metric())
    assert bool(torch.isfinite(J1).all()) and bool(torch.isfinite(e1).all())   # every element of the buffers is written
