"""-m gpu: the SE2 motion planner on the fused kernels (csrc/trajse2_kernels.hip: thx_trajse2_eval, thx_trajse2_error,
thx_trajse2_retract; theseus_amd/planning_se2.py: PackedTrajectorySE2) against the torch classes and against the REAL reference's
fixtures (tests/golden/trajse2_f64_*.npz).  CPU twin: tests/test_trajse2_host.py.

Bounds: tests/test_gpu_push2.py's.  fp64: every block and error within 1e-12 of its largest magnitude of the torch classes in fp64.
fp32: a kernel's block may be at most F32_FACTOR = 4 x as far from the fp64 value as the REFERENCE's own fp32 evaluation of the same
fp32-rounded inputs is (recorded per block in the fixtures: f32d_*), with a floor of F32_FLOOR = 16 * 2^-23 of the block's largest
magnitude.  Away from the fixtures (the random problem) the torch classes, which reproduce the reference to 1e-12, stand in for it.
Measured worst ratios: DESIGN.md 4.14."""
import numpy as np
import pytest
import torch

from tests.helpers import load_golden
from tests.push2_common import F32_FACTOR, F32_FLOOR
from tests.test_gpu_push2 import compare, f64_bound
from tests.test_push2_host import check_implicit_gradients, check_iterates
from tests.test_traj2_host import assert_blocks_close
from tests.test_trajse2_host import _lm
from tests.trajse2_common import FIXTURES, build, random_problem

pytestmark = pytest.mark.gpu
DEV = "cuda"
RANDOM_B = RANDOM_N = 70   # past one wave of problems, no multiple of 64; 4 + 4 * 70 + 1 = 285 terms > 256: the error kernel's
                           # stride loop and the edge of the 256-thread workgroups of the evaluation both run


def _packed(th, obj):
    lin = th.HipLinearization(obj)
    assert type(lin.packed).__name__ == "PackedTrajectorySE2" and type(lin.K).__name__ == "HipKernels"
    return lin, lin.packed


def _torch_blocks(th, f, dtype, **kw):
    """{cost: [error, block 0, ...]} of the torch classes on the CPU in ``dtype`` (fp32: of the fp32-rounded inputs), as float64"""
    obj, _, _ = build(th, f, dtype=dtype, **kw)
    B = f["pose0"].shape[0]
    out = {}
    for name, c in obj.cost_functions.items():
        jac, err = c.weighted_jacobians_error()
        out[name] = [err.expand(B, -1).double().numpy()] + [j.expand(B, -1, -1).double().numpy() for j in jac]
    return out


@pytest.fixture(scope="module")
def random_reference():
    """the random problem and the torch classes' blocks of it, computed once: fp64 of the fp64 inputs, fp64 and fp32 of the
    fp32-rounded inputs"""
    import theseus_amd as th
    f = random_problem(RANDOM_B, RANDOM_N, seed=11)
    f32 = {k: np.asarray(v, np.float32).astype(np.float64) for k, v in f.items()}
    kw = dict(N=RANDOM_N)
    return f, _torch_blocks(th, f, torch.float64, **kw), _torch_blocks(th, f32, torch.float64, **kw), _torch_blocks(th, f32, torch.float32, **kw)


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
    """Against the fp64 FIXTURE (the reference's blocks), every block of every cost"""
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


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_kernels_match_the_torch_classes_on_a_random_problem(dtype, random_reference):
    """B = 70, N = 70: 285 terms, n = 426, kind boundaries inside waves, a tenth of the poses outside the grid, per-problem
    grids / cost_eps / dt / Qc_inv / weights"""
    import theseus_amd as th
    f, exact64, exact32, own32 = random_reference
    obj, _, _ = build(th, f, device=DEV, dtype=dtype, N=RANDOM_N)
    _, packed = _packed(th, obj)
    packed.sync()
    assert len(packed.costs) == 285 > 256 and packed.n == 426 and packed.batch == 70
    if dtype == torch.float64:
        metric, want, _ = compare(packed, exact64, f64_bound, "random B=70 N=70 fp64")
        np.testing.assert_allclose(metric, want, rtol=1e-12)
    else:
        def bound(name, k, scale):
            return max(F32_FACTOR * float(np.abs(own32[name][k] - exact32[name][k]).max()), F32_FLOOR * scale)
        metric, want, slack = compare(packed, exact32, bound, "random B=70 N=70 fp32")
        assert (np.abs(metric - want) <= slack + 2.0 ** -23 * want).all()
    # every element of the buffers is written, and two evaluations of one state give the same bits
    J1, e1, m1 = packed._J.clone(), packed._e.clone(), packed.error_metric().clone()
    packed._J.fill_(float("nan"))
    packed._e.fill_(float("nan"))
    packed._eval()
    assert torch.equal(J1, packed._J) and torch.equal(e1, packed._e) and torch.equal(m1, packed.error_metric())
    assert bool(torch.isfinite(J1).all()) and bool(torch.isfinite(e1).all())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_retract_matches_the_torch_retract(dtype):
    """thx_trajse2_retract against se2_torch.retract / a plain add in fp64 on the same (fp32-rounded) inputs: V = 9 mixed records,
    B = 70, a delta with a row stride wider than 3 V, a mask.  fp64: 1e-14 of the largest value.  fp32: the kernel rounds
    step * delta and the result once each and evaluates in fp64 in between -- 2 roundings of 2^-24 relative on values of at most
    the largest result, plus the Taylor branch of exp below the fp32 threshold 3e-2 (theta^4 / 120 < 7e-9): 8 * 2^-24 of the
    largest value bounds all of it."""
    import theseus_amd as th
    from theseus_amd import se2_torch as S
    K = th.HipKernels()
    gen = torch.Generator().manual_seed(5)
    V, B, ldd = 9, 70, 32
    kind = torch.tensor([0, 1, 0, 0, 1, 1, 0, 1, 0], dtype=torch.uint8)
    ang = torch.randn(V, B, generator=gen, dtype=torch.float64)
    x = torch.cat([torch.randn(V, B, 2, generator=gen, dtype=torch.float64), ang.cos().unsqueeze(2), ang.sin().unsqueeze(2)], dim=2).to(dtype)
    x[kind == 1, :, 3] = 7.0   # (a pad element that is NOT zero must not survive a move)
    delta = (0.3 * torch.randn(B, ldd, generator=gen, dtype=torch.float64)).to(dtype)
    delta[0, 2], delta[1, 8], delta[2, 20] = 0.0, 1e-9, 0.1   # (an angle of exactly 0, below and just above the thresholds)
    mask = (torch.rand(B, generator=gen) < 0.3).to(torch.uint8)
    out = torch.full_like(x, float("nan")).to(DEV)
    K.trajse2_retract(x.to(DEV), kind.to(DEV), delta.to(DEV), 0.25, mask.to(DEV), out)
    got = out.cpu()
    step = torch.tensor(0.25, dtype=dtype)
    keep = mask.bool()
    for k in range(V):
        d = (delta[:, 3 * k:3 * k + 3] * step).double()
        xk = x[k].double()
        want = S.retract(xk, d) if kind[k] == 0 else torch.cat([xk[:, :3] + d, torch.zeros(B, 1, dtype=torch.float64)], dim=1)
        tol = (1e-14 if dtype == torch.float64 else 8 * 2.0 ** -24) * float(want.abs().max())
        assert float((got[k][~keep].double() - want[~keep]).abs().max()) <= tol, k
        assert torch.equal(got[k][keep], x[k][keep])   # masked problems copy their records
        if kind[k]:
            assert bool((got[k][~keep, 3] == 0).all())
    out2 = torch.empty_like(out)
    K.trajse2_retract(x.to(DEV), kind.to(DEV), delta.to(DEV), 0.25, None, out2)   # (no mask at all)
    assert torch.equal(out2.cpu()[:, ~keep], got[:, ~keep]) and bool(torch.isfinite(out2).all())


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
        _, opt, _, sol, info = _lm(th, g, None, device=DEV, track_err_history=True, track_state_history=True)
    assert type(opt.linear_solver).__name__ == "HipCholeskySolver"
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedTrajectorySE2"
    check_iterates(g, info, g["var_order"].tolist())
    assert sol["pose_1"].shape == (3, 4) and sol["vel_1"].shape == (3, 3)
    state = opt.linear_solver.linearization.packed.state
    assert bool((state[[k for k, n in enumerate(g["var_order"].tolist()) if n.startswith("vel")], :, 3] == 0).all())   # the pad stays 0


@pytest.mark.parametrize("fixture", FIXTURES)
def test_implicit_gradients_reproduce_the_reference(fixture):
    import theseus_amd as th
    g = load_golden(fixture)
    _, opt, leaves, sol, _ = _lm(th, g, None, device=DEV, backward_mode="implicit")
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedTrajectorySE2"
    check_implicit_gradients(g, leaves, sol, g["var_order"].tolist())


def test_unroll_with_gradients_is_refused_by_name():
    import theseus_amd as th
    g = load_golden(FIXTURES[0])
    with pytest.raises(NotImplementedError, match="backward_mode='unroll'.*SE2 motion planning"):
        _lm(th, g, None, device=DEV, backward_mode="unroll")


def test_the_fused_path_is_really_taken(monkeypatch):
    """No cost function is evaluated by torch in a no_grad LM run: one thx_trajse2_eval per linearization, thx_trajse2_error for
    every error metric, thx_trajse2_retract for every step."""
    import theseus_amd as th
    g = load_golden(FIXTURES[0])
    K = th.HipKernels()
    calls = {"trajse2_eval": 0, "trajse2_error": 0, "trajse2_retract": 0, "block_assemble_strided": 0}
    for name in calls:
        def counted(*a, _f=getattr(K, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(K, name, counted)

    def refuse(*a, **kw):
        raise AssertionError("a cost function was evaluated by torch on the fused path")
    for cls in (th.eb.Collision2D, th.eb.GPMotionModel, th.eb.Nonholonomic, th.eb.HingeCost, th.eb.XYDifference, th.Difference):
        for method in ("error", "jacobians"):
            monkeypatch.setattr(cls, method, refuse)
    linearizations = {"n": 0}
    real = th.HipLinearization._assemble

    def counting_assemble(self):
        linearizations["n"] += 1
        return real(self)
    monkeypatch.setattr(th.HipLinearization, "_assemble", counting_assemble)
    with torch.no_grad():
        _, opt, _, _, info = _lm(th, g, K, device=DEV, track_err_history=True, track_state_history=True)
    assert opt.linear_solver.linearization.K is K
    assert linearizations["n"] >= 5 and calls["trajse2_eval"] == linearizations["n"] == calls["block_assemble_strided"]
    assert calls["trajse2_error"] >= 6 and calls["trajse2_retract"] >= 5   # the initial error + one per iteration; one step each
    check_iterates(g, info, g["var_order"].tolist())


def test_edited_and_replaced_aux_values_are_seen_by_the_next_call():
    import theseus_amd as th
    g = load_golden(FIXTURES[0])
    obj, _, _ = build(th, g, device=DEV)
    lin, packed = _packed(th, obj)
    lin.linearize()
    H0, e0, table0, state0 = lin.AtA.clone(), obj.error_metric().clone(), packed._table, packed.state

    def expected():
        h = dict(g)
        h["sdf_data"], h["goal"] = obj.get_variable("sdf_data").tensor.cpu().numpy(), obj.get_variable("goal").tensor.cpu().numpy()
        return _torch_blocks(th, h, torch.float64)
    # an in-place edit of sdf_data needs neither a re-pack of the state nor a rebuild of the table: the table points at the tensor
    with torch.no_grad():
        obj.get_variable("sdf_data").tensor.mul_(0.8).sub_(0.05)
    lin.linearize()
    assert packed._table is table0 and packed.state is state0
    assert float((lin.AtA - H0).abs().max()) > 1e-3 and float((obj.error_metric() - e0).abs().max()) > 1e-3
    metric, want, _ = compare(packed, expected(), f64_bound, "sdf_data edited in place")
    np.testing.assert_allclose(metric, want, rtol=1e-12)
    # a replaced goal rebuilds the table
    e1 = obj.error_metric().clone()
    obj.update({"goal": torch.tensor([[0.3, -0.2]], dtype=torch.float64, device=DEV)})
    lin.linearize()
    assert packed._table is not table0 and float((obj.error_metric() - e1).abs().max()) > 1e-3
    metric, want, _ = compare(packed, expected(), f64_bound, "goal replaced")
    np.testing.assert_allclose(metric, want, rtol=1e-12)
