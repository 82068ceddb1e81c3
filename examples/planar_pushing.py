"""Planar pushing pose estimation (the reference's examples/tactile_pose_estimation.py) on theseus_amd's own API and the fused kernels
(theseus_amd/pushing.py: PackedPlanarPushing -- thx_push2_eval + thx_block_assemble + the tiled Cholesky at n = 6 T).

The reference's tactile data set and measurement network are not part of this repository: the episode is SYNTHETIC -- a rectangle
(0.24 x 0.16) pushed by a point effector that starts on one of its edges and moves along a gentle arc, the object following the
quasi-static model exactly; the "tactile" measurements are the true relative effector poses in the moving object frame with noise,
the motion capture the true effector poses with noise.  The objective is the estimator's (theseus/utils/examples/
tactile_pose_estimation/pose_estimator.py) with its options: T = 25 steps,
moving-frame window min 10 / max 40 / step 5, unit weights except the ones given below, eff_radius 0, c_square from the
rectangle's shape, Levenberg-Marquardt with the dense Cholesky solver.

    python examples/planar_pushing.py [--batch 16] [--steps 25] [--iters 20] [--dtype f64]

prints the objective's error before and after and the object-pose error against the synthetic ground truth.  On one MI355X (batch
16, fp64, 20 iterations) the objective goes from 47.6 to 0.0382, the mean object position error from 1.20e-1 at the initial guess
(every object pose = the start pose) to 2.8e-3 (of a 0.24 x 0.16 rectangle) and the mean rotation error from 4.2e-2 to 6.3e-3 rad.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RECT = (0.24, 0.16)
WINDOW = (10, 40, 5)


def rect_sdf(origin, cell, rows, cols, half):
    xs, ys = origin[0] + cell * np.arange(cols), origin[1] + cell * np.arange(rows)
    X, Y = np.meshgrid(xs, ys)
    qx, qy = np.abs(X) - half[0], np.abs(Y) - half[1]
    return np.hypot(np.maximum(qx, 0), np.maximum(qy, 0)) + np.minimum(np.maximum(qx, qy), 0)


def se2(x, y, th):
    return np.stack([x, y, np.cos(th), np.sin(th)], axis=-1)


def mul(a, b):
    return np.stack([a[..., 0] + a[..., 2] * b[..., 0] - a[..., 3] * b[..., 1], a[..., 1] + a[..., 3] * b[..., 0] + a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 2] - a[..., 3] * b[..., 3], a[..., 3] * b[..., 2] + a[..., 2] * b[..., 3]], axis=-1)


def inv(a):
    return np.stack([-(a[..., 2] * a[..., 0] + a[..., 3] * a[..., 1]), -(-a[..., 3] * a[..., 0] + a[..., 2] * a[..., 1]), a[..., 2],
                     -a[..., 3]], axis=-1)


def window_pairs(T, window=WINDOW):
    lo, hi, step = window
    return [(i - off, i) for i in range(lo, T) for off in range(lo, min(i, hi), step)]


def qsp_residual(o1, o2, e1, e2, c_square):
    """D V - Vp of the quasi-static model (theseus_amd.eb.QuasiStaticPushingPlanar) on (B, 4) numpy poses"""
    c, s = o2[:, 2], o2[:, 3]
    un = lambda v: np.stack([c * v[:, 0] + s * v[:, 1], -s * v[:, 0] + c * v[:, 1]], axis=1)  # noqa: E731
    p, v, u = un(e2[:, :2] - o2[:, :2]), un(o2[:, :2] - o1[:, :2]), un(e2[:, :2] - e1[:, :2])
    om = np.arctan2(s * o1[:, 2] - c * o1[:, 3], c * o1[:, 2] + s * o1[:, 3])
    return np.stack([v[:, 0] - p[:, 1] * om - u[:, 0], v[:, 1] + p[:, 0] * om - u[:, 1],
                     -p[:, 1] * v[:, 0] + p[:, 0] * v[:, 1] - c_square * om], axis=1)


def push(o1, e1, e2, c_square):
    """The object pose after the effector moved from e1 to e2: the root of the quasi-static residual (Newton, batched)."""
    x = np.stack([o1[:, 0], o1[:, 1], np.arctan2(o1[:, 3], o1[:, 2])], axis=1)
    f = lambda z: qsp_residual(o1, se2(z[:, 0], z[:, 1], z[:, 2]), e1, e2, c_square)  # noqa: E731
    for _ in range(20):
        r = f(x)
        J = np.stack([(f(x + 1e-7 * np.eye(3)[k]) - r) / 1e-7 for k in range(3)], axis=2)
        x = x - np.linalg.solve(J, r[:, :, None])[:, :, 0]
    return se2(x[:, 0], x[:, 1], x[:, 2])


def synthetic_episode(B, T, seed=0, window=WINDOW):
    """Ground truth and noisy inputs of B pushing episodes: dict of numpy arrays.  The effector starts on the rectangle's left edge
    and moves along a gentle arc; the object follows the quasi-static model exactly (sticking contact)."""
    rng = np.random.default_rng(seed)
    c_square = RECT[0] ** 2 + RECT[1] ** 2
    obj = [se2(rng.uniform(-0.1, 0.1, B), rng.uniform(-0.1, 0.1, B), rng.uniform(-0.5, 0.5, B))]
    contact = se2(np.full(B, -RECT[0] / 2), rng.uniform(-0.06, 0.06, B), np.zeros(B))
    eff = [mul(obj[0], contact)]
    heading = np.arctan2(obj[0][:, 3], obj[0][:, 2]) + rng.uniform(-0.3, 0.3, B)
    bend, step = rng.uniform(-0.03, 0.03, B), rng.uniform(0.008, 0.012, B)
    for i in range(1, T):
        h = heading + bend * i
        e = eff[-1].copy()
        e[:, 0], e[:, 1] = e[:, 0] + step * np.cos(h), e[:, 1] + step * np.sin(h)
        obj.append(push(obj[-1], eff[-1], e, c_square))
        eff.append(e)
    obj, eff = np.stack(obj, axis=1), np.stack(eff, axis=1)
    noise = lambda sx, st, *shape: se2(rng.normal(0, sx, shape), rng.normal(0, sx, shape), rng.normal(0, st, shape))  # noqa: E731
    pairs = window_pairs(T, window)
    rel = lambda k: mul(inv(obj[:, k]), eff[:, k])  # noqa: E731
    meas = np.stack([mul(mul(inv(rel(a)), rel(b)), noise(1e-3, 5e-3, B)) for a, b in pairs], axis=1) if pairs else np.zeros((B, 0, 4))
    cell, rows, cols = 0.02, 25, 33
    origin = np.array([[-0.32, -0.24]])
    return dict(obj_gt=obj, eff_gt=eff, mocap=mul(eff, noise(1e-3, 1e-2, B, T)), meas=meas, obj_start=obj[:, 0].copy(),
                sdf_origin=origin, cell_size=np.array([[cell]]), sdf_data=rect_sdf(origin[0], cell, rows, cols, (RECT[0] / 2, RECT[1] / 2))[None])


def make_objective(th, T, B, dtype=torch.float64, device="cuda", window=WINDOW, seed=0):
    """-> (objective, episode): the estimator's objective, every object pose initialised at the start pose and every effector pose
    at its motion-capture reading."""
    ep = synthetic_episode(B, T, seed, window)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(device)  # noqa: E731
    objs = [th.SE2(tensor=t(ep["obj_start"]), name=f"obj_pose_{i}") for i in range(T)]
    effs = [th.SE2(tensor=t(ep["mocap"][:, i]), name=f"eff_pose_{i}") for i in range(T)]
    start = th.SE2(tensor=t(ep["obj_start"]), name="obj_start_pose")
    mocap = [th.SE2(tensor=t(ep["mocap"][:, i]), name=f"motion_capture_{i}") for i in range(T)]
    pairs = window_pairs(T, window)
    meas = [th.SE2(tensor=t(ep["meas"][:, k]), name=f"nn_measurement_{a}_{b}") for k, (a, b) in enumerate(pairs)]
    origin = th.Point2(tensor=t(ep["sdf_origin"]), name="sdf_origin")
    cell = th.Variable(t(ep["cell_size"]), name="sdf_cell_size")
    sdf = th.Variable(t(ep["sdf_data"]), name="sdf_data")
    radius = th.Variable(torch.zeros(1, 1, dtype=dtype, device=device), name="eff_radius")
    ones = lambda n, v=1.0: torch.full((1, n), v, dtype=dtype, device=device)  # noqa: E731
    qsp_w = th.DiagonalCostWeight(th.Variable(ones(3, 100.0), name="qsp_weight"))
    mf_w = th.DiagonalCostWeight(th.Variable(ones(3, 10.0), name="mf_between_weight"))
    hit_w = th.ScaleCostWeight(th.Variable(ones(1, 10.0), name="intersect_weight"))
    mc_w = th.DiagonalCostWeight(th.Variable(ones(3, 10.0), name="mc_weight"))
    c_square = RECT[0] ** 2 + RECT[1] ** 2
    obj = th.Objective(dtype=dtype)
    k = 0
    for i in range(T):
        if i == 0:
            obj.add(th.Difference(objs[0], start, mc_w, name="obj_priors_0"))
        if i < T - 1:
            obj.add(th.eb.QuasiStaticPushingPlanar(objs[i], objs[i + 1], effs[i], effs[i + 1], c_square, qsp_w, name=f"qsp_{i}"))
        while k < len(pairs) and pairs[k][1] == i:
            a = pairs[k][0]
            obj.add(th.eb.MovingFrameBetween(objs[a], objs[i], effs[a], effs[i], meas[k], mf_w, name=f"mf_between_{a}_{i}"))
            k += 1
        obj.add(th.eb.EffectorObjectContactPlanar(objs[i], effs[i], origin, sdf, cell, radius, hit_w, name=f"intersect_{i}"))
        obj.add(th.Difference(effs[i], mocap[i], mc_w, name=f"eff_priors_{i}"))
    return obj, ep


def pose_error(values, ep, T):
    """mean position / rotation error of the object poses against the ground truth"""
    est = torch.stack([values[f"obj_pose_{i}"].detach().double().cpu() for i in range(T)], dim=1).numpy()
    gt = ep["obj_gt"]
    d = np.arctan2(est[..., 3], est[..., 2]) - np.arctan2(gt[..., 3], gt[..., 2])
    return float(np.hypot(est[..., 0] - gt[..., 0], est[..., 1] - gt[..., 1]).mean()), float(np.abs(np.arctan2(np.sin(d), np.cos(d))).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f64")
    a = ap.parse_args()
    import theseus_amd as th
    dtype = torch.float32 if a.dtype == "f32" else torch.float64
    obj, ep = make_objective(th, a.steps, a.batch, dtype)
    opt = th.LevenbergMarquardt(obj, th.CholeskyDenseSolver, max_iterations=a.iters, step_size=1.0, abs_err_tolerance=0.0,
                                rel_err_tolerance=0.0)
    packed = opt.linear_solver.linearization.packed
    before = pose_error({k: v.tensor for k, v in obj.optim_vars.items()}, ep, a.steps)
    with torch.no_grad():
        values, info = th.TheseusLayer(opt).forward(None, optimizer_kwargs=dict(damping=0.1, track_err_history=True))
    after = pose_error(values, ep, a.steps)
    hist = info.err_history
    print(f"{type(packed).__name__}: {len(obj.cost_functions)} costs, n = {packed.n}, batch {a.batch}, {a.dtype}")
    print(f"error before {float(hist[:, 0].mean()):.6g}  after {float(hist[:, -1].mean()):.6g}  ({a.iters} LM iterations)")
    print(f"object pose error against the ground truth: position {before[0]:.3e} -> {after[0]:.3e}, rotation {before[1]:.3e} -> {after[1]:.3e} rad")


if __name__ == "__main__":
    main()
