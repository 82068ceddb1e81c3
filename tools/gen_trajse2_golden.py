"""Generate the SE2 motion-planning fixtures by RUNNING THE REAL REFERENCE (test infrastructure; needs the reference importable, CPU
only).

    python -m tools.gen_trajse2_golden

The reference's own MotionPlannerObjective(pose_type=th.SE2, nonholonomic_w=10, positive_vel_w=5) (theseus/utils/examples/
motion_planning/motion_planner.py) plus the extra HingeCost of tests/trajse2_common.py (finite limits, DiagonalCostWeight), fp64.
Writes under tests/golden/:
  trajse2_f64_shared.npz    grid, origin, cost_eps, dt, Qc_inv, weights, start, goal with batch 1
  trajse2_f64_batched.npz   the same with per-problem values
Each records the inputs, every cost's weighted Jacobian blocks and error at the initial state (wj_<cost>_<slot>, we_<cost>), AtA /
Atb of DenseLinearization, the error metric, the iterates of 5 LM iterations (step_size 0.25, damping 0.1, CholeskyDenseSolver),
the implicit-mode gradients of sum(solution^2) w.r.t. sdf_data, collision_w, cost_eps, Qc_inv, start, goal and the two scalar
weights, and -- per block -- how far the reference's OWN fp32 evaluation of the fp32-rounded inputs is from its fp64 one (f32d_*).
The initial states are placed by hand so that, between the two fixtures, they cover: a pose inside the grid, outside on each side,
exactly on a grid row / column, on the last row / column, distance above and below cost_eps, a GP pair with relative rotation
exactly 0, below the near-zero threshold and at +-(pi - 0.01 ... 0.02), forward velocities below / inside / exactly at the hinge's
bound and a component of the extra hinge above its upper bound (asserted below, together with the margins that keep every
non-exact case on its side of its kink in fp32).
"""
import importlib.util
import os

import numpy as np
import torch

from oracle.gen_golden import OUT, import_reference
from tests.trajse2_common import ALL_CASES, LEAVES, LM_DAMPING, LM_KW, N, add_extra_hinge, classify, pose, pose_cells, rect_sdf, state_of

R, C, CELL, B = 12, 16, 0.25, 3
TOTAL_TIME = 2.5
THRESHOLDS = (1e-6, 1e-3, 3e-2, 1e-1)   # se2 near_zero / d_near_zero of fp64 and of fp32 (theseus/global_params.py)
XH = dict(xh_down=np.array([[-1.0, -0.5, -0.8]]), xh_up=np.array([[1.5, 0.5, 0.8]]), xh_thr=np.array([[0.1, 0.1, 0.1]]))


def planner_objective_class(th):
    """MotionPlannerObjective, loaded from its file (the examples package imports optional dependencies)"""
    path = os.path.join(os.path.dirname(th.__file__), "utils", "examples", "motion_planning", "motion_planner.py")
    spec = importlib.util.spec_from_file_location("reference_motion_planner", path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.MotionPlannerObjective


def make_problem(batched: bool):
    rng = np.random.default_rng(41 + batched)
    origins = np.array([[-2.0, -1.5], [-1.75, -1.25], [-2.25, -1.5]]) if batched else np.array([[-2.0, -1.5]])
    halves = [(0.75, 0.5), (0.6, 0.45), (0.85, 0.4)]
    sdf = np.stack([rect_sdf(origins[k], CELL, R, C, halves[k]) for k in range(len(origins))])
    org = lambda b: origins[b if batched else 0]  # noqa: E731
    pi = np.pi
    # per problem and step: (col, row) cell coordinates of the translation in the problem's grid, angle | None = exactly the
    # identity rotation; grid-line coordinates are integers: origin + integer * 0.25 is exact in fp32 and fp64
    plan = [
        [((2.3, 3.4), None), ((-2.0, 6.52), None), ((17.2, 6.8), 5e-7), ((8.44, -1.6), 0.2), ((9.6, 12.4), 0.5), ((3.88, 6.84), 0.3)],
        [((5.2, 2.2), 0.7), ((3.48, 4.0), 0.7 + pi - 0.01), ((5.0, 9.08), 0.7 + pi - 0.01 - (pi - 0.02)), ((9.6, 11.0), 0.9),
         ((15.0, 7.2), 1.03), ((12.3, 3.3), 1.2)],
        [((1.3, 1.7), -0.4), ((8.5, 6.3), -0.27), ((4.3, 5.7), -0.1), ((6.6, 9.3), 0.15), ((13.7, 10.2), 0.4), ((14.4, 1.6), 0.6)]]
    pose0 = np.zeros((B, N + 1, 4))
    for b in range(B):
        for i, ((col, row), ang) in enumerate(plan[b]):
            q = org(b) + CELL * np.array([col, row])
            pose0[b, i] = [q[0], q[1], 1.0, 0.0] if ang is None else [q[0], q[1], np.cos(ang), np.sin(ang)]
    # forward velocities: below (< 1), exactly at (== 1) and inside (> 1) the bound down_limit + threshold = 0 + 1 of positive_vel_i;
    # vel_N is the extra hinge's: components above up - thr, inside and below down + thr
    vel0 = rng.normal(0, 0.3, (B, N + 1, 3))
    vel0[..., 0] = [[0.4, 1.0, 1.6, 0.25, 2.0, 1.45], [1.0, 0.7, 1.2, 0.9, 1.3, 0.6], [1.5, 0.3, 1.0, 1.1, 0.8, -0.95]]
    vel0[:, N, 1:] = [[0.1, -0.75], [0.45, 0.2], [-0.1, 0.75]]
    nb = B if batched else 1
    start = np.stack([pose(pose0[b, 0, 0] + 0.05, pose0[b, 0, 1] - 0.03, [0.0, 0.7, -0.4][b] + 0.23 + 0.11 * b) for b in range(nb)])
    goal = np.stack([pose0[b, N, :2] + [0.04, -0.06] for b in range(nb)])
    pick = (lambda a: np.asarray(a, np.float64)) if batched else (lambda a: np.asarray(a, np.float64)[:1])
    Qc = [[[2.0, 0.3, -0.2], [0.3, 1.5, 0.1], [-0.2, 0.1, 1.2]], [[1.0, -0.2, 0.1], [-0.2, 2.5, 0.4], [0.1, 0.4, 0.9]],
          [[3.0, 0.5, 0.3], [0.5, 0.8, -0.1], [0.3, -0.1, 1.6]]]
    return dict(pose0=pose0, vel0=vel0, start=start, goal=goal, sdf_origin=origins, cell_size=np.full((len(origins), 1), CELL),
                sdf_data=sdf, cost_eps=pick([[0.4], [0.3], [0.5]]), dt=pick([[0.5], [0.4], [0.625]]), Qc_inv=pick(Qc),
                collision_w=pick([[5.0], [3.0], [8.0]]), nonholonomic_w=pick([[10.0], [7.0], [12.0]]),
                positive_vel_w=pick([[5.0], [4.0], [6.5]]), xh_w=pick([[2.0, 1.5, 0.8], [1.0, 2.5, 0.6], [3.0, 0.7, 1.2]]), **XH)


def build_reference(th, MPO, f, dtype=torch.float64, grad=False):
    """The reference's own objective with the fixture's values -> (objective, {leaf name: tensor}, [cost names])"""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)   # (HingeCost builds its limit / threshold tensors in the default dtype)
    try:
        obj = MPO(R, 0.4, TOTAL_TIME, 5.0, np.eye(3).tolist(), N, pose_type=th.SE2, dtype=dtype, nonholonomic_w=10.0,
                  positive_vel_w=5.0)
        add_extra_hinge(th, obj, f, N, dtype=dtype)
    finally:
        torch.set_default_dtype(old)
    t = lambda key: torch.from_numpy(np.asarray(f[key])).to(dtype)  # noqa: E731
    leaves = {k: t(k).clone().requires_grad_(grad) for k in LEAVES}
    value = lambda key: leaves[key] if key in leaves else t(key)  # noqa: E731
    for key in ("start", "goal", "sdf_origin", "cell_size", "sdf_data", "cost_eps", "dt", "collision_w"):
        obj.aux_vars[key].tensor = value(key)
    cf = obj.cost_functions
    for i in range(1, N + 1):
        # (the planner builds its placeholder grid map_size x map_size and the SDF container keeps THAT size for its bounds tests
        #  and clamps: hand it the size of the 12 x 16 grid that was just assigned)
        cf[f"collision_{i}"].sdf._num_rows, cf[f"collision_{i}"].sdf._num_cols = R, C
    cf["gp_1"].weight.Qc_inv.tensor = value("Qc_inv")
    cf["nonholonomic_1"].weight.scale.tensor = value("nonholonomic_w")
    cf["positive_vel_1"].weight.scale.tensor = value("positive_vel_w")
    assert all(cf[f"gp_{i}"].weight is cf["gp_1"].weight and cf[f"nonholonomic_{i}"].weight is cf["nonholonomic_1"].weight
               and cf[f"positive_vel_{i}"].weight is cf["positive_vel_1"].weight for i in range(1, N + 1))
    for i in range(N + 1):
        obj.optim_vars[f"pose_{i}"].tensor = t("pose0")[:, i].clone()
        obj.optim_vars[f"vel_{i}"].tensor = t("vel0")[:, i].clone()
    obj.update()
    return obj, leaves, list(cf.keys())


def check_margins(f, obj):
    """Every translation that is not exactly on a grid line is at least 1e-3 cells away from one, every distance at least 1e-3
    away from cost_eps, every angle a Taylor switch looks at 1e-3 (relative) away from the four thresholds or exactly 0, every
    relative rotation 1e-3 away from +-pi, every hinge input exactly at its bound or 1e-3 away from it: converting the inputs to
    fp32 cannot move a case across a kink."""
    cases = set()
    for coord in pose_cells(f):
        fr = coord - np.floor(coord)
        assert ((fr == 0) | ((fr > 1e-3) & (fr < 1 - 1e-3))).all()

    def angles_ok(ang, name):
        for thr in THRESHOLDS:
            assert ((ang == 0) | (np.abs(np.abs(ang) - thr) > 1e-3 * thr)).all(), (name, ang)
    for name, c in obj.cost_functions.items():
        if name.startswith("collision"):
            d = c._compute_distances_and_jacobians()[0].numpy()
            gap = d - c.cost_eps.tensor.numpy()
            assert (np.abs(gap) > 1e-3).all(), (name, d.ravel(), gap.ravel())
            cases |= ({"d_above_eps"} if (gap > 0).any() else set()) | ({"d_below_eps"} if ((gap < 0) & (d != 0)).any() else set())
        elif name.startswith("gp"):
            ang = c.pose1.local(c.pose2).numpy()[:, 2]
            angles_ok(ang, name)
            assert (np.pi - np.abs(ang) > 1e-3).all()
            cases |= {k for k, m in (("rel_exactly_0", ang == 0), ("rel_below_near_zero", (ang != 0) & (np.abs(ang) < 1e-6)),
                                     ("near_plus_pi", (ang > np.pi - 0.021) & (ang < np.pi - 0.009)),
                                     ("near_minus_pi", (ang < -np.pi + 0.021) & (ang > -np.pi + 0.009))) if m.any()}
        elif name == "pose_0":
            angles_ok(c.error().numpy()[:, 2], name)
        elif name.startswith("positive_vel") or name == "extra_hinge":
            v, thr = c.vector.tensor.numpy(), c.threshold.tensor.numpy()
            down, up = c.down_limit.tensor.numpy() + thr, c.up_limit.tensor.numpy() - thr
            for bound in (down, up):
                assert ((v == bound) | ~(np.abs(v - bound) <= 1e-3)).all(), (name, v, bound)
            tag = "xh" if name == "extra_hinge" else "hinge"
            cases |= {k for k, m in ((f"{tag}_below", v < down), (f"{tag}_above", v > up), (f"{tag}_at_bound", v == down),
                                     (f"{tag}_inside", (v > down) & (v < up) & np.isfinite(down))) if m.any()}
    return cases


def generate(th, MPO, name, batched):
    f = make_problem(batched)
    out = dict(f)
    obj, _, costs = build_reference(th, MPO, f)
    names = list(obj.optim_vars.keys())
    out["var_order"], out["cost_order"] = np.array(names), np.array(costs)
    # the reference's own fp32 evaluation of the fp32-rounded inputs
    obj32, _, _ = build_reference(th, MPO, f, dtype=torch.float32)
    for cname, c in obj.cost_functions.items():
        jac, err = c.weighted_jacobians_error()
        jac32, err32 = obj32.cost_functions[cname].weighted_jacobians_error()
        assert err32.dtype == torch.float32
        out[f"we_{cname}"] = err.numpy()
        out[f"f32d_we_{cname}"] = np.abs(err32.double().numpy() - err.numpy()).max()
        for s, j in enumerate(jac):
            out[f"wj_{cname}_{s}"] = j.numpy()
            out[f"f32d_wj_{cname}_{s}"] = np.abs(jac32[s].double().numpy() - j.numpy()).max()
    lin = th.DenseLinearization(obj)
    lin.linearize()
    out.update(AtA=lin.AtA.numpy(), Atb=lin.Atb.squeeze(2).numpy(), error_metric=obj.error_metric().numpy(), error=obj.error().numpy())
    cases = check_margins(f, obj)
    # 5 LM iterations
    obj, _, _ = build_reference(th, MPO, f)
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.CholeskyDenseSolver, vectorize=False, **LM_KW)
    with torch.no_grad():
        sol, info = th.TheseusLayer(opt).forward(optimizer_kwargs=dict(damping=LM_DAMPING, track_err_history=True, track_state_history=True))
    out["lm_iterates"] = torch.cat([info.state_history[k] for k in names], dim=1).permute(2, 0, 1).numpy()   # (K + 1, B, 42)
    out["lm_err_history"] = info.err_history.numpy()
    # implicit backward
    obj, leaves, _ = build_reference(th, MPO, f, grad=True)
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.CholeskyDenseSolver, vectorize=False, **LM_KW)
    sol, info = th.TheseusLayer(opt).forward(optimizer_kwargs=dict(damping=LM_DAMPING, backward_mode="implicit"))
    final = state_of(sol, names)
    loss = (final ** 2).sum()
    loss.backward()
    out.update(implicit_final=final.detach().numpy(), implicit_loss=loss.item(), **{f"grad_{k}": v.grad.numpy() for k, v in leaves.items()})
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    worst = max(float(v) for k, v in out.items() if k.startswith("f32d_"))
    print(name, os.path.getsize(path), "bytes; err", out["lm_err_history"][:, 0], "->", out["lm_err_history"][:, -1], "loss", loss.item(),
          "worst fp32 distance", worst, {k: float(v.grad.abs().max()) for k, v in leaves.items()})
    return classify(f) | cases


def main():
    th, _ = import_reference()
    torch.set_default_dtype(torch.float64)   # (as the reference's example does: HingeCost creates default-dtype tensors)
    MPO = planner_objective_class(th)
    covered = generate(th, MPO, "trajse2_f64_shared", False) | generate(th, MPO, "trajse2_f64_batched", True)
    wanted = ALL_CASES | {"d_above_eps", "d_below_eps", "rel_exactly_0", "rel_below_near_zero", "near_plus_pi", "near_minus_pi",
                          "hinge_below", "hinge_inside", "hinge_at_bound", "xh_above"}
    assert not wanted - covered, f"the fixtures' initial states do not cover {wanted - covered}"
    print("covered:", sorted(covered))


if __name__ == "__main__":
    main()
