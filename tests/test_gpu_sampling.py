"""-m gpu: posterior samples and marginal covariances on the cached Cholesky factor -- HipCholeskySolver.sample_deltas /
marginal_covariance and TheseusLayer.compute_samples (theseus/theseus_layer.py:99-135) against the reference's formula evaluated
in fp64 on the CPU from the device's own hessian_approx() and delta:
    delta_samples = delta[..., None] + solve_triangular(cholesky(AtA / T)^T, y, upper=True)
and against the oracle's retraction (oracle/pose_graph.py) of the current variables by every sample."""
import pytest
import torch

from oracle import lie as olie
from oracle import pose_graph as opg

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
EDGES = [(0, 1), (1, 2), (2, 3), (3, 4), (0, 2), (1, 3), (2, 4), (0, 4)]
P = 5
PRIOR_WEIGHT = 1.0   # cond(AtA) of both graphs at the linearization the tests use: see test_fixture_is_well_conditioned


def relerr(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return float((got - want).abs().max() / want.abs().max())


def reference_delta_samples(AtA, delta, y, temperature):
    """theseus_layer.py:113-123 in fp64 on the CPU; y (n, k) or (B, n, k)."""
    A = AtA.double().cpu() / temperature
    sqrt_AtA = torch.linalg.cholesky(A).permute(0, 2, 1)
    y = y.double().cpu()
    if y.dim() == 2:
        y = y.unsqueeze(0).expand(A.shape[0], -1, -1)
    return torch.linalg.solve_triangular(sqrt_AtA, y, upper=True) + delta.double().cpu().unsqueeze(-1)


# ---- generic objective: a quadratic fit, one Vector of three coefficients -------------------------------------------------------
def quadratic_fit(th, dtype, device="cuda", kernels=None):
    B, N = 4, 8
    gen = torch.Generator().manual_seed(21)
    xs = torch.linspace(-1, 1, N, dtype=torch.float64).repeat(B, 1) + 0.05 * torch.randn(B, N, dtype=torch.float64, generator=gen)
    coef = torch.randn(B, 3, dtype=torch.float64, generator=gen)
    ys = coef[:, :1] + coef[:, 1:2] * xs + coef[:, 2:] * xs ** 2 + 0.01 * torch.randn(B, N, dtype=torch.float64, generator=gen)
    x = th.Variable(xs.to(dtype).to(device), name="x")
    y = th.Variable(ys.to(dtype).to(device), name="y")
    c = th.Vector(tensor=torch.zeros(B, 3, dtype=dtype, device=device), name="c")

    def residual(optim_vars, aux_vars):
        cc, (xx, yy) = optim_vars[0].tensor, aux_vars
        return yy.tensor - (cc[:, :1] + cc[:, 1:2] * xx.tensor + cc[:, 2:] * xx.tensor ** 2)
    obj = th.Objective(dtype=dtype)
    obj.add(th.AutoDiffCostFunction([c], residual, N, aux_vars=[x, y],
                                    cost_weight=th.ScaleCostWeight(torch.ones(1, 1, dtype=dtype, device=device))))
    opt = th.GaussNewton(obj, max_iterations=3, linearization_kwargs=dict(kernels=kernels) if kernels is not None else None)
    return th.TheseusLayer(opt), opt.linear_solver, c


@pytest.mark.parametrize("dtype,bar", [(F64, 1e-10), (F32, 1e-4)], ids=["f64", "f32"])
def test_compute_samples_on_a_generic_objective(dtype, bar):
    import theseus_amd as th
    layer, solver, c = quadratic_fit(th, dtype)
    layer.forward(None)
    assert type(solver).__name__ == "HipCholeskySolver" and type(solver.linearization.packed).__name__ == "PackedEuclidean"
    n, k, T = 3, 7, 0.5
    y = torch.randn(n, k, dtype=torch.float64, generator=torch.Generator().manual_seed(4)).to(dtype).cuda()
    before = c.tensor.clone()
    version = solver.factor_version
    samples = layer.compute_samples(solver, n_samples=k, temperature=T, noise=y)
    assert solver.factor_version == version + 1 and solver.linearization._AtA_cache is None   # one factorisation, no dense AtA
    assert tuple(samples.shape) == (4, n, k) and samples.dtype == dtype and not samples.requires_grad
    assert torch.equal(c.tensor, before)
    AtA, delta = solver.linearization.hessian_approx(), solver.solve()
    want = reference_delta_samples(AtA, delta, y, T) + before.double().cpu().unsqueeze(-1)
    err = relerr(samples, want)
    print("generic", dtype, "compute_samples error", err)
    assert err < bar, err
    # per-problem noise (B, n, k), as a dict
    yb = torch.randn(4, n, k, dtype=torch.float64, generator=torch.Generator().manual_seed(5)).to(dtype).cuda()
    d = layer.compute_samples(solver, k, T, noise=yb, return_dict=True)
    assert list(d) == ["c"] and tuple(d["c"].shape) == (4, k, n)
    want = reference_delta_samples(AtA, delta, yb, T) + before.double().cpu().unsqueeze(-1)
    err = relerr(d["c"].transpose(1, 2), want)
    print("generic", dtype, "per-problem noise error", err)
    assert err < bar, err
    # a seeded generator gives what passing its draw gives
    drawn = torch.randn(n, k, generator=torch.Generator(device="cuda").manual_seed(3), device="cuda", dtype=dtype)
    a = layer.compute_samples(solver, k, T, generator=torch.Generator(device="cuda").manual_seed(3))
    b = layer.compute_samples(solver, k, T, noise=drawn)
    assert torch.equal(a, b)
    assert torch.equal(c.tensor, before)


# ---- pose graphs: 5 poses, 8 edges, 1 prior ---------------------------------------------------------------------------------------
def pose_graph(th, group, dtype, B=3, device="cuda", kernels=None):
    gen = torch.Generator().manual_seed(7 if group == "SE3" else 8)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, generator=gen)  # noqa: E731
    if group == "SE3":
        G, exp, dof = th.SE3, olie.se3_exp, 6
    else:
        from oracle import lie_se2
        G, exp, dof = th.SE2, lie_se2.se2_exp, 3
    Gc = opg.GROUPS[group]
    truth = exp(0.6 * rnd(B * P, dof)).view(B, P, *exp(rnd(1, dof)).shape[1:])
    start = Gc.retract(truth, 0.05 * rnd(B, P, dof))
    obj = th.Objective(dtype=dtype)
    dev = lambda t: t.to(dtype).to(device)  # noqa: E731
    poses = [G(tensor=dev(start[:, k]), name=f"pose_{k}") for k in range(P)]
    for e, (i, j) in enumerate(EDGES):
        meas = Gc.retract(Gc.compose(Gc.inverse(truth[:, i]), truth[:, j]).unsqueeze(1), 0.02 * rnd(B, 1, dof))[:, 0]
        w = th.DiagonalCostWeight(th.Variable(dev(0.8 + 0.4 * torch.rand(1, dof, dtype=torch.float64, generator=gen)), name=f"w_{e}"))
        obj.add(th.Between(poses[i], poses[j], G(tensor=dev(meas), name=f"meas_{e}"), w, name=f"between_{e}"))
    pw = th.ScaleCostWeight(th.Variable(dev(torch.full((1, 1), PRIOR_WEIGHT, dtype=torch.float64)), name="pw"))
    obj.add(th.Difference(poses[0], G(tensor=dev(truth[:, 0]), name="prior_target"), pw, name="prior"))
    opt = th.LevenbergMarquardt(obj, max_iterations=3, linearization_kwargs=dict(kernels=kernels) if kernels is not None else None)
    return th.TheseusLayer(opt), opt.linear_solver, poses


_GRAPHS = {}


def solved_graph(group, dtype):
    """(layer, solver, poses) after layer.forward, once per module."""
    if (group, dtype) not in _GRAPHS:
        import theseus_amd as th
        layer, solver, poses = pose_graph(th, group, dtype)
        layer.forward(None)
        _GRAPHS[(group, dtype)] = (layer, solver, poses)
    return _GRAPHS[(group, dtype)]


@pytest.mark.parametrize("group", ["SE3", "SE2"])
def test_fixture_is_well_conditioned(group):
    """The fp32 bar of the covariance test measures the kernel only if cond(AtA) stays below 1e4."""
    _, solver, _ = solved_graph(group, F64)
    cond = torch.linalg.cond(solver.linearization.hessian_approx().double().cpu())
    print(group, "cond(AtA)", cond.tolist())
    assert float(cond.max()) < 1e4


@pytest.mark.parametrize("group", ["SE3", "SE2"])
def test_compute_samples_on_a_pose_graph(group):
    layer, solver, poses = solved_graph(group, F64)
    assert type(solver).__name__ == "HipCholeskySolver"
    B, k, T, dof = 3, 33, 2.0, 6 if group == "SE3" else 3
    n = P * dof
    y = torch.randn(n, k, dtype=torch.float64, generator=torch.Generator().manual_seed(6)).cuda()
    before = [p.tensor.clone() for p in poses]
    # the samples come from the ONE factorisation of solve(), and the dense AtA is never built
    lin = solver.linearization
    lin._AtA_cache = None
    if lin._compact:
        lin._H = None
    version = solver.factor_version
    out = layer.compute_samples(solver, k, T, noise=y, return_dict=True)
    assert solver.factor_version == version + 1
    assert lin._AtA_cache is None and (not lin._compact or lin._H is None)
    assert list(out) == [f"pose_{i}" for i in range(P)]
    assert all(torch.equal(p.tensor, b) for p, b in zip(poses, before))
    deltas = solver.sample_deltas(k, T, noise=y)
    assert tuple(deltas.shape) == (B, n, k)
    AtA, delta = solver.linearization.hessian_approx(), solver.solve()
    err = relerr(deltas, reference_delta_samples(AtA, delta, y, T))
    print(group, "sample_deltas error", err)
    assert err < 1e-10, err
    current = torch.stack([b.cpu() for b in before], dim=1)                       # (B, P, *record)
    want = torch.stack([opg.retract(current, deltas[:, :, s].cpu().contiguous()) for s in range(k)], dim=2)   # (B, P, k, *record)
    for i in range(P):
        got = out[f"pose_{i}"]
        assert tuple(got.shape) == (B, k, *before[i].shape[1:])
        err = relerr(got, want[:, i])
        assert err < 1e-10, (i, err)
    with pytest.raises(ValueError, match="return_dict=True"):
        layer.compute_samples(solver, k, T, noise=y)


@pytest.mark.parametrize("dtype,bar", [(F64, 1e-9), (F32, 1e-3)], ids=["f64", "f32"])
def test_marginal_covariance(dtype, bar):
    _, solver, _ = solved_graph("SE3", dtype)
    version = solver.factor_version
    C = solver.marginal_covariance(["pose_3", "pose_0"])
    assert solver.factor_version == version + 1
    assert tuple(C.shape) == (3, 12, 12) and C.dtype == dtype
    assert torch.equal(C, C.transpose(1, 2))
    full = torch.linalg.inv(solver.linearization.hessian_approx().double().cpu())
    idx = torch.tensor(list(range(18, 24)) + list(range(0, 6)))
    want = full[:, idx][:, :, idx]
    errs = [relerr(C[b], want[b]) for b in range(3)]
    print("marginal covariance", dtype, errs)
    assert max(errs) < bar, errs
    # solve_multi_with_factor on the factor marginal_covariance just left (undamped): H^-1 applied to a block of vectors
    rhs = torch.randn(3, 9, 30, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).to(dtype).cuda()
    x = solver.solve_multi_with_factor(rhs)
    assert x.data_ptr() != rhs.data_ptr()
    err = relerr(x, rhs.double().cpu() @ full)
    assert err < bar, err
