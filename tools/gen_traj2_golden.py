"""Generate the 2D motion-planning fixtures by RUNNING THE REAL REFERENCE (test infrastructure; needs the reference importable,
CPU only).

    python -m tools.gen_traj2_golden

th.eb.Collision2D / th.eb.GPMotionModel / th.Difference on Point2 / Vector(2) (tests/traj2_common.py builds the objective on either
API), fp64.  Writes under tests/golden/:
  traj2_f64_shared.npz    sdf_origin / cell_size / sdf_data / cost_eps / Qc_inv with batch 1
  traj2_f64_batched.npz   the same with per-problem values (origins, grids, eps, Qc_inv, collision weights)
Each records the inputs, every cost's weighted Jacobian blocks and error at the initial trajectory (wj_<cost>_<slot>, we_<cost>),
AtA / Atb of DenseLinearization, the error metric, the iterates of 5 LM iterations with CholeskyDenseSolver, and -- implicit backward
mode -- the gradients of sum(solution^2) w.r.t. sdf_data, cost_eps, Qc_inv and the start / goal targets.
The initial points are placed by hand so that, between the two fixtures, they cover: an interior cell, out of bounds on each side,
exactly on a grid row / column, exactly on the last row / column, distance above and below cost_eps (asserted below).
"""
import os

import numpy as np
import torch

from oracle.gen_golden import OUT, import_reference
from tests.traj2_common import ALL_CASES, LM_DAMPING, LM_KW, N, build, classify, disc_sdf, state_of

R, C, CELL, B = 12, 16, 0.25, 3


def make_problem(batched: bool):
    rng = np.random.default_rng(11 + batched)
    origins = np.array([[-2.0, -1.5], [-1.75, -1.25], [-2.25, -1.5]]) if batched else np.array([[-2.0, -1.5]])
    discs = [[(-0.3, 0.0, 0.5), (0.9, -0.6, 0.35)], [(-0.6, 0.2, 0.4), (0.7, 0.1, 0.45)], [(0.0, -0.3, 0.55), (-1.2, 0.6, 0.3)]]
    sdf = np.stack([disc_sdf(origins[k], CELL, R, C, discs[k]) for k in range(len(origins))])
    ox, oy = origins[:, 0], origins[:, 1]
    xmax, ymax = ox + (C - 1) * CELL, oy + (R - 1) * CELL
    o = lambda k: k if batched else 0  # noqa: E731
    # hand-placed initial trajectories (x, y); grid-line coordinates are origin + integer * 0.25: exact in fp32 and fp64
    poses0 = np.array([
        [[ox[o(0)] - 0.5, 0.1], [-1.37, -0.52], [ox[o(0)] + 5 * CELL, 0.13], [0.11, oy[o(0)] + 4 * CELL], [0.4, ymax[o(0)]],
         [xmax[o(0)], 0.3], [xmax[o(0)] + 0.55, 0.2]],
        [[0.1, oy[o(1)] - 0.4], [-1.1, -0.9], [-0.93, 0.31], [-0.1, 0.43], [0.32, 0.52], [1.21, 0.77], [0.2, ymax[o(1)] + 0.35]],
        [[-1.6, -0.8], [-1.07, -0.61], [-0.58, -0.47], [-0.03, -0.21], [0.52, 0.07], [1.03, 0.36], [1.5, 0.6]]])
    vels0 = rng.normal(0.0, 0.4, (B, N + 1, 2))
    f = dict(sdf_origin=origins, cell_size=np.full((len(origins), 1), CELL), sdf_data=sdf,
             cost_eps=np.array([[0.4], [0.3], [0.45]]) if batched else np.array([[0.4]]), dt=np.array([[0.5]]),
             Qc_inv=(np.array([[[2.0, 0.3], [0.3, 1.5]]]) * np.array([1.0, 0.6, 1.7]).reshape(3, 1, 1)) if batched
             else np.array([[[2.0, 0.3], [0.3, 1.5]]]),
             w_collision=np.array([[5.0], [3.0], [8.0]]) if batched else np.array([[5.0]]), w_pose=np.array([[10.0]]),
             w_vel=np.array([[3.0, 5.0]]), start=poses0[:, 0] + np.array([0.07, -0.04]), goal=poses0[:, -1] + np.array([-0.05, 0.06]),
             poses0=poses0, vels0=vels0)
    return f


def check_margins(th, f):
    """Every initial point that is not exactly on a grid line is at least 1e-3 cells away from one, and every in-bounds distance
    at least 1e-3 away from cost_eps: converting the inputs to fp32 cannot move a point across a kink."""
    p, o = f["poses0"], f["sdf_origin"]
    for coord in ((p[..., 0] - o[:, None, 0]) / CELL, (p[..., 1] - o[:, None, 1]) / CELL):
        fr = coord - np.floor(coord)
        assert ((fr == 0) | ((fr > 1e-3) & (fr < 1 - 1e-3))).all()
    sdf = th.eb.SignedDistanceField2D(torch.from_numpy(o), torch.from_numpy(f["cell_size"]), torch.from_numpy(f["sdf_data"]))
    d, _ = sdf.signed_distance(torch.from_numpy(p).permute(0, 2, 1).contiguous())
    gap = (d.numpy() - f["cost_eps"])
    assert (np.abs(gap) > 1e-3).all()
    return {"d_above_eps"} if (gap > 0).any() else set(), {"d_below_eps"} if ((gap < 0) & (d.numpy() != 0)).any() else set()


def generate(th, name, batched):
    f = make_problem(batched)
    out = dict(f)
    obj, _, costs = build(th, f)
    names = list(obj.optim_vars.keys())
    out["var_order"], out["cost_order"] = np.array(names), np.array(costs)
    obj.update()
    for cname, c in obj.cost_functions.items():
        jac, err = c.weighted_jacobians_error()
        out[f"we_{cname}"] = err.numpy()
        for s, j in enumerate(jac):
            out[f"wj_{cname}_{s}"] = j.numpy()
    lin = th.DenseLinearization(obj)
    lin.linearize()
    out.update(AtA=lin.AtA.numpy(), Atb=lin.Atb.squeeze(2).numpy(), error_metric=obj.error_metric().numpy(), error=obj.error().numpy())
    # 5 LM iterations
    obj, _, _ = build(th, f)
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.CholeskyDenseSolver, vectorize=False, **LM_KW)
    with torch.no_grad():
        sol, info = th.TheseusLayer(opt).forward(optimizer_kwargs=dict(damping=LM_DAMPING, track_err_history=True, track_state_history=True))
    out["lm_iterates"] = torch.cat([info.state_history[k] for k in names], dim=1).permute(2, 0, 1).numpy()   # (K + 1, B, n)
    out["lm_err_history"] = info.err_history.numpy()
    # implicit backward
    obj, leaves, _ = build(th, f, grad=True)
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.CholeskyDenseSolver, vectorize=False, **LM_KW)
    sol, info = th.TheseusLayer(opt).forward(optimizer_kwargs=dict(damping=LM_DAMPING, backward_mode="implicit"))
    final = state_of(sol, names)
    loss = (final ** 2).sum()
    loss.backward()
    out.update(implicit_final=final.detach().numpy(), implicit_loss=loss.item(), **{f"grad_{k}": v.grad.numpy() for k, v in leaves.items()})
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    above, below = check_margins(th, f)
    print(name, "err", out["lm_err_history"][:, 0], "->", out["lm_err_history"][:, -1], "loss", loss.item(),
          {k: float(v.grad.abs().max()) for k, v in leaves.items()})
    return classify(f) | above | below


def main():
    th, _ = import_reference()
    torch.set_default_dtype(torch.float64)
    covered = generate(th, "traj2_f64_shared", False) | generate(th, "traj2_f64_batched", True)
    missing = (ALL_CASES | {"d_above_eps", "d_below_eps"}) - covered
    assert not missing, f"the fixtures' initial points do not cover {missing}"
    print("covered:", sorted(covered))


if __name__ == "__main__":
    main()
