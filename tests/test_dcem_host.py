"""-m "not gpu": DCEM's torch twin (theseus_amd/dcem.py: dcem_update_torch) against the REAL reference's fixtures
(tests/golden/dcem_f64_soft.npz, dcem_f64_modes.npz, written by tools/gen_dcem_golden.py), and the argument errors of the optimizer.
The kernels' side: tests/test_gpu_dcem.py.

The twin runs the reference's own torch operations in the reference's order, on the reference's device and dtype here (CPU, fp64):
it has to give the reference's bits (``torch.equal``).  Its autograd gradients differ from the reference's only by where the error
metric is summed: 1e-10 of the gradient's largest entry."""
import numpy as np
import pytest
import torch

from tests import dcem_common as dc


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def error_metric(A, t, X):
    """0.5 |A (x - t) + 0.1 sum(sin x)|^2 at X (..., B, n): the fixture objective's error metric on plain tensors"""
    e = (A @ (X - t).unsqueeze(-1)).squeeze(-1) + 0.1 * torch.sin(X).sum(dim=-1, keepdim=True)
    return (e ** 2).sum(dim=-1) / 2


def test_twin_reproduces_every_recorded_iteration_bit_for_bit():
    from theseus_amd.dcem import dcem_update_torch
    g = dc.load("dcem_f64_soft")
    mu, sigma = _t(g["x0"]), torch.ones(dc.B, dc.N_DOF, dtype=torch.float64)
    for it in range(dc.N_ITER):
        X = dc.samples(mu, sigma, _t(g["noise"][it]))
        fX = _t(g["fX"][it]).t().contiguous()
        # (the recorded errors are the objective's at these samples: the noise replays the reference's draws)
        assert torch.allclose(error_metric(_t(g["A"]), _t(g["t"]), X), fX, rtol=1e-13, atol=0)
        m, s, w, nu, bracket, flags = dcem_update_torch(fX, X, dc.N_ELITE, 1.0, True, 1e-3, 100, dc.BRANCH)
        assert torch.equal(w, _t(g["w"][it])) and torch.equal(m, _t(g["mu"][it])) and torch.equal(s, _t(g["sigma"][it])), it
        assert not flags.any() and bool(((bracket[:, 1] - bracket[:, 0]) <= 1e-3).all())
        assert bool(((bracket[:, 0] <= nu) & (nu <= bracket[:, 1])).all())
        mu, sigma = m, s


@pytest.mark.parametrize("mode", list(dc.MODES))
def test_twin_reproduces_every_recorded_mode_bit_for_bit(mode):
    from theseus_amd.dcem import dcem_update_torch
    g = dc.load("dcem_f64_modes")
    extra, S = dc.MODES[mode]
    kw = dict(n_elite=dc.N_ELITE, temp=1.0, normalize=True)
    kw.update({k: v for k, v in extra.items() if k in kw})
    X = dc.samples(_t(g["x0"]), torch.ones(dc.B, dc.N_DOF, dtype=torch.float64), _t(g[f"{mode}_noise"][0]))
    assert X.shape[0] == S
    m, s, w, _, _, flags = dcem_update_torch(_t(g[f"{mode}_fX"]).t().contiguous(), X, lml_eps=1e-3, branch=dc.BRANCH, **kw)
    assert torch.equal(w, _t(g[f"{mode}_w"])) and torch.equal(m, _t(g[f"{mode}_mu"])) and torch.equal(s, _t(g[f"{mode}_sigma"]))
    assert not flags.any()
    if mode == "hard":
        assert sorted(w.unique().tolist()) == [0.0, 1.0] and bool((w.sum(dim=1) == dc.N_ELITE).all())
    if mode == "all_elite":
        assert bool((w == 1.0 - 1e-5).all())


def test_twin_autograd_reproduces_the_recorded_unroll_gradients():
    """the six chained updates on the twin, errors by plain torch: d sum(solution^2) / d t and / d initial x"""
    from theseus_amd.dcem import dcem_update_torch
    g = dc.load("dcem_f64_soft")
    A, t, x0 = _t(g["A"]), _t(g["t"]).requires_grad_(), _t(g["x0"]).requires_grad_()
    mu, sigma = x0, torch.ones(dc.B, dc.N_DOF, dtype=torch.float64)
    for it in range(dc.N_ITER):
        X = dc.samples(mu, sigma, _t(g["noise"][it]))
        mu, sigma = dcem_update_torch(error_metric(A, t, X), X, dc.N_ELITE, 1.0, True, 1e-3, 100, dc.BRANCH)[:2]
    assert torch.allclose(mu.detach(), _t(g["mu"][-1]), rtol=0, atol=1e-14)
    (mu ** 2).sum().backward()
    for leaf, want in ((t, g["grad_t"]), (x0, g["grad_x0"])):
        assert np.abs(want).max() > 1e-3
        np.testing.assert_allclose(leaf.grad.numpy(), want, rtol=0, atol=1e-10 * np.abs(want).max())


def test_twin_takes_ties_by_the_lower_sample_index_and_flags_an_unfinished_search():
    from theseus_amd import _lib
    from theseus_amd.dcem import dcem_update_torch
    fX = torch.tensor([[3.0], [1.0], [1.0], [1.0], [0.5]], dtype=torch.float64)   # (S = 5, B = 1)
    X = torch.arange(5, dtype=torch.float64).view(5, 1, 1)
    w = dcem_update_torch(fX, X, 2, None)[2]
    assert w.tolist() == [[0.0, 1.0, 0.0, 0.0, 1.0]]
    flags = dcem_update_torch(fX, X, 2, 1.0, lml_n_iter=1, branch=3)[5]
    assert int(flags[0]) & _lib.DCEM_FLAG_NOT_CONVERGED


def _optimizer(**kw):
    import theseus_amd as th
    obj, leaves = dc.build(th, dc.problem())
    return th, obj, th.DCEM(obj, **dict(dc.DCEM_KW, **kw))


def test_constructor_mirrors_the_reference_and_stores_the_bounds():
    th, obj, opt = _optimizer(lb=-1.0, ub=2.0)
    assert (opt.lb, opt.ub, opt.lml_branch, opt.n_samples, opt.n_elite, opt.temp, opt.lml_eps) == (-1.0, 2.0, 100, 40, 5, 1.0, 1e-3)
    assert type(opt.packed).__name__ == "PackedEuclidean" and not hasattr(opt, "linear_solver")
    assert th.DCEM(obj, lml_branch=10).lml_branch == 10
    layer = th.TheseusLayer(opt)
    assert layer.optimizer is opt and layer.objective is obj


def test_non_euclidean_variables_are_refused_naming_dcem():
    import theseus_amd as th
    pose = th.SE3(tensor=torch.eye(3, 4, dtype=torch.float64).repeat(2, 1, 1), name="pose")
    target = th.SE3(tensor=torch.eye(3, 4, dtype=torch.float64).repeat(2, 1, 1), name="target")
    obj = th.Objective(dtype=torch.float64)
    weight = th.ScaleCostWeight(th.Variable(torch.ones(1, 1, dtype=torch.float64), name="w"))
    obj.add(th.Difference(pose, target, weight, name="prior"))
    with pytest.raises(th.UnsupportedObjective, match="DCEM"):
        th.DCEM(obj)


def test_argument_errors():
    th, obj, opt = _optimizer()
    with pytest.raises(ValueError, match="n_elite"):
        th.DCEM(obj, n_elite=0)
    with pytest.raises(ValueError, match="n_sample"):
        th.DCEM(obj, n_sample=5000)
    with pytest.raises(ValueError, match="lml_branch"):
        th.DCEM(obj, lml_branch=1)
    for mode in ("implicit", "truncated"):
        with pytest.raises(NotImplementedError, match="DCEM currently only supports 'unroll' backward mode."):
            opt.optimize(backward_mode=mode)
    before = [v.tensor for v in obj.optim_vars.values()]
    with pytest.raises(ValueError, match="noise"):
        opt.optimize(noise=torch.zeros(dc.N_ITER, dc.N_SAMPLE, dc.B, dc.N_DOF + 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="noise"):
        opt.optimize(noise=torch.zeros(dc.N_ITER, dc.N_SAMPLE, dc.B, dc.N_DOF, dtype=torch.float32))
    # the refused calls left the variables on valid tensors with the start values
    assert not opt.packed._vars_stale
    for v, t in zip(obj.optim_vars.values(), before):
        assert torch.equal(v.tensor, t)


def test_the_exports_check_their_arguments_before_any_launch():
    import ctypes
    from theseus_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)

    def update(S=8, B=2, n=3, n_elite=2, branch=10, dtype=1, fX=one, flags=one):
        return lib.thx_dcem_update(fX, one, S, B, n, n_elite, 1.0, 1, 1e-3, 100, branch, one, one, one, one, one, flags, dtype, None)

    def vjp(S=8, B=2, n=3, n_elite=2, dtype=1, w=one):
        return lib.thx_dcem_update_vjp(one, one, one, one, w, one, one, S, B, n, n_elite, 1.0, 1, one, one, dtype, None)
    for call in (update, vjp):
        for kw, message in ((dict(S=0), b"S < 1"), (dict(S=_lib.THX_DCEM_MAX_S + 1), b"THX_DCEM_MAX_S"), (dict(n=0), b"n < 1"),
                            (dict(n_elite=0), b"n_elite < 1"), (dict(B=0), b"empty batch"), (dict(dtype=5), b"dtype")):
            assert call(**kw) != 0 and message in lib.thx_last_error(), (call.__name__, kw, lib.thx_last_error())
    assert update(branch=1) != 0 and b"branch < 2" in lib.thx_last_error()
    assert update(fX=None) != 0 and b"null pointer" in lib.thx_last_error()
    assert vjp(w=None) != 0 and b"null pointer" in lib.thx_last_error()
    assert update(fX=ctypes.c_void_p(12)) != 0 and b"aligned" in lib.thx_last_error()
    assert update(flags=ctypes.c_void_p(18)) != 0 and b"aligned" in lib.thx_last_error()
    assert vjp(w=ctypes.c_void_p(20), dtype=1) != 0 and b"aligned" in lib.thx_last_error()


def test_there_is_no_cpu_fallback():
    th, obj, opt = _optimizer()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.optimize()
    assert not opt.packed._vars_stale
