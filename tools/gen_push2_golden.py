"""Generate the planar-pushing fixtures by RUNNING THE REAL REFERENCE (test infrastructure; needs the reference importable, CPU
only).

    python -m tools.gen_push2_golden

th.eb.QuasiStaticPushingPlanar / MovingFrameBetween / EffectorObjectContactPlanar / th.Difference on SE2 (tests/push2_common.py
builds the objective on either API), fp64.  Writes under tests/golden/:
  push2_f64_shared.npz    grids, origins, c_square, eff_radius, weights, measurements, motion-capture targets with batch 1
  push2_f64_batched.npz   the same with per-problem values
Each records the inputs, every cost's weighted Jacobian blocks and error at the initial poses (wj_<cost>_<slot>, we_<cost>), AtA /
Atb of DenseLinearization, the error metric, the iterates of 5 LM iterations with CholeskyDenseSolver, the implicit-mode gradients
of sum(solution^2) w.r.t. the measurements, the five weights, sdf_data, c_square, eff_radius and the motion-capture targets, and --
per cost -- how far the reference's OWN fp32 evaluation of the fp32-rounded inputs is from its fp64 one (f32d_we_<cost>,
f32d_wj_<cost>_<slot>: the largest absolute difference of the block), which is what the fp32 kernels are measured against.
The initial poses are placed by hand so that, between the two fixtures, they cover: effector inside the grid, outside on each side,
exactly on a grid row / column, on the last row / column, distance above and below eff_radius, a moving-frame residual rotation of
exactly 0 and below the near-zero threshold (Taylor branch), a relative rotation near +pi and near -pi in a pushing term (asserted
below, together with the margins that keep every non-exact case on its side of its kink in fp32).
"""
import os

import numpy as np
import torch

from oracle.gen_golden import OUT, import_reference
from tests.push2_common import ALL_CASES, LM_DAMPING, LM_KW, T, build, classify, contact_cells, pose, rect_sdf, state_of, window_pairs

R, C, CELL, B = 12, 16, 0.25, 3
HALF = (0.75, 0.5)
THRESHOLDS = (1e-6, 1e-3, 3e-2, 1e-1)   # se2 near_zero / d_near_zero of fp64 and of fp32 (theseus/global_params.py)


def se2_mul(a, b):
    return np.array([a[0] + a[2] * b[0] - a[3] * b[1], a[1] + a[3] * b[0] + a[2] * b[1], a[2] * b[2] - a[3] * b[3], a[3] * b[2] + a[2] * b[3]])


def se2_inv(a):
    return np.array([-(a[2] * a[0] + a[3] * a[1]), -(-a[3] * a[0] + a[2] * a[1]), a[2], -a[3]])


def make_problem(batched: bool):
    rng = np.random.default_rng(23 + batched)
    origins = np.array([[-2.0, -1.5], [-1.75, -1.25], [-2.25, -1.5]]) if batched else np.array([[-2.0, -1.5]])
    halves = [HALF, (0.6, 0.45), (0.85, 0.4)]
    sdf = np.stack([rect_sdf(origins[k], CELL, R, C, halves[k]) for k in range(len(origins))])
    org = lambda b: origins[b if batched else 0]  # noqa: E731
    ident = np.array([1.0, 0.0])
    # per problem and step: (object translation, object angle | None = exactly the identity, contact point in (col, row) cell
    # coordinates of the object's grid, effector angle | None); translations of identity-rotation objects are multiples of 1/8 and
    # grid-line coordinates integers: origin + integer * 0.25 is exact in fp32 and fp64
    plan = [
        [((0.5, 0.25), None, (-2.0, 6.52), 0.3), ((0.625, 0.25), None, (17.2, 6.8), None), ((0.75, 0.375), None, (8.44, -1.6), 0.2),
         ((0.875, 0.375), None, (9.6, 12.4), None), ((1.0, 0.4), 0.3, (3.88, 6.84), -0.4), ((1.1, 0.45), 0.42, (5.6, 6.4), 0.1)],
        [((0.25, 0.25), None, (3.48, 4.0), 0.7), ((0.5, 0.25), None, (5.0, 9.08), None), ((0.5, 0.5), None, (9.6, 11.0), -0.2),
         ((0.75, 0.5), None, (15.0, 7.2), None), ((0.8, 0.55), -0.25, (12.3, 3.3), 0.5), ((0.9, 0.6), -0.4, (11.7, 2.6), 0.9)],
        [((-0.3, 0.1), 0.1, (4.3, 5.7), 1.0), ((-0.2, 0.15), 0.22, (4.45, 5.3), 1.1), ((-0.1, 0.2), 0.1, (4.7, 4.4), 1.3),
         ((0.0, 0.22), 0.1 + np.pi - 0.01, (11.7, 7.3), 1.2), ((0.1, 0.3), 0.1 + np.pi - 0.01 - (np.pi - 0.02), (5.3, 3.4), 1.0),
         ((0.2, 0.33), 0.25, (5.8, 3.1), 0.8)]]
    obj0, eff0 = np.zeros((B, T, 4)), np.zeros((B, T, 4))
    for b in range(B):
        for i, (t, ang, (col, row), eang) in enumerate(plan[b]):
            cs = ident if ang is None else np.array([np.cos(ang), np.sin(ang)])
            q = org(b) + CELL * np.array([col, row])
            obj0[b, i] = [t[0], t[1], cs[0], cs[1]]
            ecs = ident if eang is None else np.array([np.cos(eang), np.sin(eang)])
            eff0[b, i] = [t[0] + (cs[0] * q[0] - cs[1] * q[1]), t[1] + (cs[1] * q[0] + cs[0] * q[1]), ecs[0], ecs[1]]
    pairs = window_pairs(T)
    nb = B if batched else 1
    meas = np.zeros((nb, len(pairs), 4))
    for b in range(nb):
        for k, (a, i) in enumerate(pairs):
            # the relative effector pose in the moving object frame of problem b, perturbed
            p1f = se2_mul(se2_inv(obj0[b, a]), eff0[b, a])
            p2f = se2_mul(se2_inv(obj0[b, i]), eff0[b, i])
            meas[b, k] = se2_mul(se2_mul(se2_inv(p1f), p2f), pose(*rng.normal(0, [0.05, 0.05, 0.2])))
    # pair (1, 3): problems 0 and 1 have identity rotations at steps 1 and 3 -- a residual rotation of exactly 0 with an identity
    # measurement rotation (shared fixture, problems 0 and 1), and of 5e-7 < near_zero (batched fixture, problem 1)
    k13 = pairs.index((1, 3))
    meas[0, k13] = [0.31, -0.12, 1.0, 0.0]
    if batched:
        meas[1, k13] = [0.27, 0.08, np.cos(5e-7), np.sin(5e-7)]
    mocap = eff0.copy() if batched else eff0[:1].copy()
    for b in range(mocap.shape[0]):
        for i in range(T):
            mocap[b, i] = se2_mul(mocap[b, i], pose(*rng.normal(0, [0.04, 0.04, 0.25])))
    start = np.stack([se2_mul(obj0[b, 0], pose(0.05, -0.03, 0.23 + 0.11 * b)) for b in range(nb)])
    pick = (lambda a: np.asarray(a)) if batched else (lambda a: np.asarray(a)[:1])
    return dict(obj0=obj0, eff0=eff0, obj_start=start, mocap=mocap, meas=meas, sdf_origin=origins,
                cell_size=np.full((len(origins), 1), CELL), sdf_data=sdf, eff_radius=pick([[0.1], [0.05], [0.15]]),
                c_square=pick([[0.8125], [0.5625], [0.8825]]), w_start=pick([[4.0], [2.5], [6.0]]),
                w_qsp=pick([[2.0, 1.5, 0.8], [1.0, 2.5, 0.6], [3.0, 0.7, 1.2]]), w_mfb=pick([[1.5, 1.2, 0.9], [0.8, 2.0, 0.5], [2.2, 1.1, 0.7]]),
                w_contact=pick([[5.0], [3.0], [8.0]]), w_mc=pick([[3.0, 2.0, 1.0], [2.0, 3.5, 0.5], [4.0, 1.0, 1.5]]))


def check_margins(th, f, obj):
    """Every contact point that is not exactly on a grid line is at least 1e-3 cells away from one, every distance at least 1e-3
    away from eff_radius, every angle a Taylor switch looks at 1e-3 (relative) away from the four thresholds or exactly 0, every
    angle of a pushing term 1e-3 away from +-pi: converting the inputs to fp32 cannot move a case across a kink."""
    cases = set()
    for coord in contact_cells(f):
        fr = coord - np.floor(coord)
        assert ((fr == 0) | ((fr > 1e-3) & (fr < 1 - 1e-3))).all()
    for name, c in obj.cost_functions.items():
        if name.startswith("intersect"):
            d = c._compute_distances_and_jacobians()[0].numpy()
            gap = d - c.eff_radius.tensor.numpy()
            assert (np.abs(gap) > 1e-3).all(), (name, d.ravel(), gap.ravel())
            cases |= ({"d_above_radius"} if (gap > 0).any() else set()) | ({"d_below_radius"} if ((gap < 0) & (d != 0)).any() else set())
        elif name.startswith("qsp"):
            ang = c.obj1.between(c.obj2).theta().numpy()
            assert (np.pi - np.abs(ang) > 1e-3).all()
            cases |= ({"near_plus_pi"} if (ang > np.pi - 0.05).any() else set()) | ({"near_minus_pi"} if (ang < -np.pi + 0.05).any() else set())
        else:
            ang = np.abs(c.error().numpy()[:, 2])
            for thr in THRESHOLDS:
                assert ((ang == 0) | (np.abs(ang - thr) > 1e-3 * thr)).all(), (name, ang)
            if name.startswith("mf_between"):
                cases |= ({"residual_exactly_0"} if (ang == 0).any() else set()) | ({"residual_below_near_zero"} if ((ang > 0) & (ang < 1e-6)).any() else set())
    return cases


def generate(th, name, batched):
    f = make_problem(batched)
    out = dict(f)
    obj, _, costs = build(th, f)
    names = list(obj.optim_vars.keys())
    out["var_order"], out["cost_order"] = np.array(names), np.array(costs)
    obj.update()
    # the reference's own fp32 evaluation of the fp32-rounded inputs
    obj32, _, _ = build(th, f, dtype=torch.float32)
    obj32.update()
    for cname, c in obj.cost_functions.items():
        jac, err = c.weighted_jacobians_error()
        jac32, err32 = obj32.cost_functions[cname].weighted_jacobians_error()
        out[f"we_{cname}"] = err.numpy()
        out[f"f32d_we_{cname}"] = np.abs(err32.double().numpy() - err.numpy()).max()
        for s, j in enumerate(jac):
            out[f"wj_{cname}_{s}"] = j.numpy()
            out[f"f32d_wj_{cname}_{s}"] = np.abs(jac32[s].double().numpy() - j.numpy()).max()
    lin = th.DenseLinearization(obj)
    lin.linearize()
    out.update(AtA=lin.AtA.numpy(), Atb=lin.Atb.squeeze(2).numpy(), error_metric=obj.error_metric().numpy(), error=obj.error().numpy())
    cases = check_margins(th, f, obj)
    # 5 LM iterations
    obj, _, _ = build(th, f)
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.CholeskyDenseSolver, vectorize=False, **LM_KW)
    with torch.no_grad():
        sol, info = th.TheseusLayer(opt).forward(optimizer_kwargs=dict(damping=LM_DAMPING, track_err_history=True, track_state_history=True))
    out["lm_iterates"] = torch.cat([info.state_history[k] for k in names], dim=1).permute(2, 0, 1).numpy()   # (K + 1, B, 4 V)
    out["lm_err_history"] = info.err_history.numpy()
    # implicit backward
    obj, leaves, _ = build(th, f, grad=True)
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
    torch.set_default_dtype(torch.float64)
    covered = generate(th, "push2_f64_shared", False) | generate(th, "push2_f64_batched", True)
    wanted = ALL_CASES | {"d_above_radius", "d_below_radius", "near_plus_pi", "near_minus_pi", "residual_exactly_0",
                          "residual_below_near_zero"}
    assert not wanted - covered, f"the fixtures' initial poses do not cover {wanted - covered}"
    print("covered:", sorted(covered))


if __name__ == "__main__":
    main()
