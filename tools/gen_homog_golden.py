"""Generate the homography-alignment fixtures by RUNNING THE REAL REFERENCE (test infrastructure; needs the reference importable,
CPU only).

    python -m tools.gen_homog_golden

The objective of tests/homog_common.py on the reference: th.AutoDiffCostFunction (vmap) with the error function below -- the
example's homography_error_fn (examples/homography_estimation.py:140-168) on the reference's own
theseus.third_party.utils.grid_sample, with the mesh grid x = 2 j / (Ww - 1) - 1, the inverse by the cofactor formula and the plain
division by q_z (kornia, whose warp_grid the example calls, is not a dependency here) -- plus th.Difference on the 8-dof variable.
fp64, B = 3, C = 2, 6 x 7 feature maps.  Writes under tests/golden/:
  homog_f64_shared.npz    feature maps of batch 1, ScaleCostWeight on the prior
  homog_f64_batched.npz   per-problem feature maps, DiagonalCostWeight (8) on the prior
Each records the inputs, both costs' weighted Jacobian block and error at the initial homography (wj_<cost>_0, we_<cost>), AtA / Atb
of DenseLinearization, the error metric, the iterates of 5 LM iterations with CholeskyDenseSolver, and -- implicit backward mode --
the gradients of sum(solution^2) w.r.t. both feature maps.
Asserted: at every recorded iterate every source coordinate is at least 1e-3 pixel away from an integer, so converting the inputs
to fp32 cannot move a point across a cell boundary.
"""
import os

import numpy as np
import torch

from oracle.gen_golden import OUT, import_reference
from tests.homog_common import LM_DAMPING, LM_KW, MARGIN, build, drifts, h8_from_source_map, smooth_maps, source_map

B, C, HH, WW = 3, 2, 6, 7


def cofactor_inverse(h):
    """(B, 8) -> (B, 3, 3) = adj(H) / det(H), H = [h0 .. h7, 1]"""
    a, b, c, d, e, f, g, k = (h[:, n] for n in range(8))
    i = torch.ones_like(a)
    A = [e * i - f * k, c * k - b * i, b * f - c * e, f * g - d * i, a * i - c * g, c * d - a * f, d * k - e * g, b * g - a * k,
         a * e - b * d]
    det = (a * A[0] + b * A[3]) + c * A[6]
    return torch.stack([x / det for x in A], dim=1).reshape(-1, 3, 3)


def source_grid(h, Hh, Ww):
    """(B, 8) -> (B, Hh, Ww, 2) normalised source coordinates of every destination pixel"""
    G = cofactor_inverse(h)
    x = (2 * torch.arange(Ww, dtype=h.dtype) / (Ww - 1) - 1).repeat(Hh)
    y = (2 * torch.arange(Hh, dtype=h.dtype) / (Hh - 1) - 1).repeat_interleave(Ww)
    q = [(G[:, r, 0:1] * x + G[:, r, 1:2] * y) + G[:, r, 2:3] for r in range(3)]
    return torch.stack([q[0] / q[2], q[1] / q[2]], dim=-1).reshape(-1, Hh, Ww, 2)


def error_fn(optim_vars, aux_vars):
    from theseus.third_party.utils import grid_sample
    h = optim_vars[0].tensor.reshape(-1, 8)
    src, dst = aux_vars[0].tensor, aux_vars[1].tensor
    n = max(h.shape[0], src.shape[0], dst.shape[0])
    src, dst = src.expand(n, -1, -1, -1), dst.expand(n, -1, -1, -1)
    grid = source_grid(h, *src.shape[-2:]).expand(n, -1, -1, -1)
    loss = torch.nn.functional.mse_loss(grid_sample(src, grid), dst, reduction="none")
    mask = grid_sample(torch.ones_like(src), grid.detach()) > 0.9
    loss, mask = loss.reshape(n, -1), mask.reshape(n, -1)
    return (loss * mask).sum(dim=1, keepdim=True) / mask.sum(dim=1, keepdim=True)


def make_problem(batched: bool):
    seed = 21 + batched
    dr = drifts(B, 0.1 / (WW - 1), seed)
    G0 = np.stack([source_map(HH, WW, (0.5, 0.5), 1.0, dr[k]) for k in range(B)])
    Gt = np.stack([source_map(HH, WW, (0.38, 0.62), 1.0, -dr[k]) for k in range(B)])
    Bf = B if batched else 1
    h0 = h8_from_source_map(G0)
    return dict(H8_0=h0, H8_prior=h0 + np.random.default_rng(seed).normal(0, 0.01, h0.shape),
                feat_src=smooth_maps(Bf, C, HH, WW, seed + 1), feat_dst=smooth_maps(Bf, C, HH, WW, seed + 1, Gt[:Bf]),
                w_align=np.array([[4.0], [6.0], [5.0]]) if batched else np.array([[5.0]]),
                w_prior=np.linspace(0.7, 1.3, 8).reshape(1, 8) if batched else np.array([[1.0]]))


def check_margins(iterates):
    """(K + 1, B, 8) homographies: the smallest distance of any source coordinate from an integer, in pixels"""
    worst = 1.0
    for h in iterates:
        g = source_grid(torch.from_numpy(np.ascontiguousarray(h)), HH, WW)
        pix = torch.stack([((g[..., 0] + 1) / 2) * (WW - 1), ((g[..., 1] + 1) / 2) * (HH - 1)])
        worst = min(worst, float((pix - torch.round(pix)).abs().min()))
    assert worst >= MARGIN, f"a source coordinate lies {worst:.2e} pixel from an integer"
    return worst


def generate(th, name, batched):
    def align(H8, src, dst, weight, cname):
        return th.AutoDiffCostFunction([H8], error_fn, 1, cost_weight=weight, aux_vars=[src, dst], name=cname, autograd_mode="vmap")
    f = make_problem(batched)
    out = dict(f)
    obj, _, costs = build(th, f, align=align)
    names = list(obj.optim_vars.keys())
    out["var_order"], out["cost_order"] = np.array(names), np.array(costs)
    obj.update()
    for cname, c in obj.cost_functions.items():
        jac, err = c.weighted_jacobians_error()
        out[f"we_{cname}"] = err.detach().numpy()
        for s, j in enumerate(jac):
            out[f"wj_{cname}_{s}"] = j.detach().numpy()
    lin = th.DenseLinearization(obj)
    lin.linearize()
    out.update(AtA=lin.AtA.numpy(), Atb=lin.Atb.squeeze(2).numpy(), error_metric=obj.error_metric().numpy(), error=obj.error().numpy())
    # 5 LM iterations
    obj, _, _ = build(th, f, align=align)
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.CholeskyDenseSolver, vectorize=False, **LM_KW)
    with torch.no_grad():
        sol, info = th.TheseusLayer(opt).forward(optimizer_kwargs=dict(damping=LM_DAMPING, track_err_history=True, track_state_history=True))
    out["lm_iterates"] = torch.cat([info.state_history[k] for k in names], dim=1).permute(2, 0, 1).numpy()   # (K + 1, B, 8)
    out["lm_err_history"] = info.err_history.numpy()
    # implicit backward
    obj, leaves, _ = build(th, f, grad=True, align=align)
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.CholeskyDenseSolver, vectorize=False, **LM_KW)
    sol, info = th.TheseusLayer(opt).forward(optimizer_kwargs=dict(damping=LM_DAMPING, backward_mode="implicit"))
    final = torch.cat([sol[k] for k in names], dim=1)
    loss = (final ** 2).sum()
    loss.backward()
    out.update(implicit_final=final.detach().numpy(), implicit_loss=loss.item(), **{f"grad_{k}": v.grad.numpy() for k, v in leaves.items()})
    margin = check_margins(list(out["lm_iterates"]) + [out["implicit_final"]])
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(name, "err", out["lm_err_history"][:, 0], "->", out["lm_err_history"][:, -1], "loss", loss.item(), "margin", margin,
          {k: float(v.grad.abs().max()) for k, v in leaves.items()})


def main():
    th, _ = import_reference()
    torch.set_default_dtype(torch.float64)
    generate(th, "homog_f64_shared", False)
    generate(th, "homog_f64_batched", True)


if __name__ == "__main__":
    main()
