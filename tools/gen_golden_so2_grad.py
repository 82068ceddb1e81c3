"""Generate the SO2 gradient fixtures by RUNNING THE REAL REFERENCE (test infrastructure; needs the reference importable, CPU only).

    python -m tools.gen_golden_so2_grad

The SO2 twins of oracle/gen_golden.py:gen_so3_implicit and gen_pg23_unrolled: th.TheseusLayer over th.LevenbergMarquardt /
th.GaussNewton on a planar rotation graph (th.Between + th.Difference on th.SO2; so2.py has no custom backward, so the reference's
gradients are plain autograd through its closed forms).  loss = <coef, final poses>.  Writes under tests/golden/:
  pgso2_f64_implicit.npz         backward_mode="implicit"; gradients w.r.t. measurements, DiagonalCostWeights, prior targets, prior
                                 ScaleCostWeights
  pgso2_f64_robust_implicit.npz  the same problem with WelschLoss on every Between cost and HuberLoss on the priors, each role with
                                 its own learnable log_loss_radius
  pgso2_f64_unrolled.npz         the same problem differentiated THROUGH the iterations: gn_unroll, lm_trunc, lm_ellips_unroll (the
                                 kwargs of gen_pg23_unrolled), plus the gradient w.r.t. the initial poses under UNROLL
Absolute angles are drawn over the whole circle, so records with cos < 0 and compositions that wrap around +-pi occur.
"""
import os

import numpy as np
import torch

from oracle.gen_golden import OUT, import_reference
from tests.so2_grad_common import build

P, E, B, ITERS = 7, 12, 4, 6
IMPLICIT_KW = dict(max_iterations=ITERS, step_size=1.0, damping=1e-3, gauss_newton=False)
UNROLLED_CASES = (("gn_unroll", "GaussNewton", "unroll", 3, {}),
                  ("lm_trunc", "LevenbergMarquardt", "truncated", 5, dict(damping=0.02, backward_num_iterations=2)),
                  ("lm_ellips_unroll", "LevenbergMarquardt", "unroll", 4,
                   dict(damping=0.05, adaptive_damping=True, ellipsoidal_damping=True)))
LOG_RADIUS = dict(between=0.0, prior=-12.0)   # Welsch on the Between costs, Huber on the priors


def make_problem(th):
    dtype, G = torch.float64, th.SO2
    gen = torch.Generator().manual_seed(67)
    rng = np.random.default_rng(67)
    edges = [(i, i + 1) for i in range(P - 1)]
    while len(edges) < E:
        i, j = sorted(rng.choice(P, 2, replace=False).tolist())
        edges.append((j, i) if rng.random() < 0.3 else (i, j))
    edges = torch.tensor(edges, dtype=torch.long)
    ex = lambda t: G.exp_map(t).tensor  # noqa: E731
    comp = lambda a, b: G(tensor=a).compose(G(tensor=b)).tensor  # noqa: E731
    inv = lambda a: G(tensor=a).inverse().tensor  # noqa: E731
    rnd = lambda n, rs: ex(rs * (2 * torch.rand(n, 1, dtype=dtype, generator=gen) - 1))  # noqa: E731
    gt = rnd(B * P, np.pi).view(B, P, 2)   # absolute angles over the whole circle
    gi, gj = gt[:, edges[:, 0]].reshape(-1, 2), gt[:, edges[:, 1]].reshape(-1, 2)
    meas = comp(comp(inv(gi), gj), rnd(B * E, 0.05)).view(B, E, 2)
    poses0 = comp(gt.reshape(-1, 2), rnd(B * P, 0.3)).view(B, P, 2)
    prior_idx = torch.tensor([0, P // 2], dtype=torch.long)
    prior_target = comp(gt[:, prior_idx].reshape(-1, 2), rnd(B * 2, 0.02)).view(B, 2, 2)
    w_between = (0.5 + torch.rand(B, E, 1, dtype=dtype, generator=gen)) * 10
    w_prior = torch.tensor([[[1e-1], [2.0]]], dtype=dtype)
    coef = torch.randn(B, P, 2, dtype=dtype, generator=torch.Generator().manual_seed(5))
    return dict(group=np.array("SO2"), P=P, edges=edges.numpy(), meas=meas.numpy(), w_between=w_between.numpy(),
                prior_idx=prior_idx.numpy(), prior_target=prior_target.numpy(), w_prior=w_prior.numpy(), poses0=poses0.numpy(),
                coef=coef.numpy())


def final_poses(sol, n):
    return torch.stack([sol[f"pose_{k}"] for k in range(n)], 1)


def gen_implicit(th, f, name, robust):
    if robust:
        f = dict(f, log_radius_between=np.array(LOG_RADIUS["between"]), log_radius_prior=np.array(LOG_RADIUS["prior"]))
    obj, leaves = build(th, f, robust=robust)
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.CholeskyDenseSolver, vectorize=True, max_iterations=ITERS, step_size=1.0,
                                abs_err_tolerance=0.0, rel_err_tolerance=0.0)
    sol, _ = th.TheseusLayer(opt).forward(optimizer_kwargs=dict(backward_mode="implicit", damping=IMPLICIT_KW["damping"]))
    final = final_poses(sol, int(f["P"]))
    loss = (torch.from_numpy(f["coef"]) * final).sum()
    loss.backward()
    out = dict(f, final=final.detach().numpy(), loss=loss.item(), opt_kwargs=np.array(repr(IMPLICIT_KW)),
               **{f"grad_{k}": v.grad.numpy() for k, v in leaves.items()})
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(name, "loss", loss.item(), {k: float(v.grad.abs().max()) for k, v in leaves.items()})


def gen_unrolled(th, f):
    out = dict(f)
    for tag, cls, mode, iters, okw in UNROLLED_CASES:
        obj, leaves = build(th, f, poses0_grad=True)
        opt = getattr(th, cls)(obj, linear_solver_cls=th.CholeskyDenseSolver, vectorize=True, max_iterations=iters, step_size=1.0,
                               abs_err_tolerance=0.0, rel_err_tolerance=0.0)
        sol, info = th.TheseusLayer(opt).forward(optimizer_kwargs=dict(backward_mode=mode, track_err_history=True, **okw))
        final = final_poses(sol, int(f["P"]))
        loss = (torch.from_numpy(f["coef"]) * final).sum()
        loss.backward()
        out.update({f"{tag}_final": final.detach().numpy(), f"{tag}_loss": loss.item(), f"{tag}_err_history": info.err_history.numpy(),
                    f"{tag}_kwargs": np.array(repr(dict(okw, max_iterations=iters, mode=mode, gauss_newton=cls == "GaussNewton")))})
        for k, v in leaves.items():
            if v.grad is not None:   # (TRUNCATED: the head of the loop runs without gradients, nothing reaches the initial poses)
                out[f"{tag}_grad_{k}"] = v.grad.numpy()
        print("pgso2_f64_unrolled", tag, "loss", loss.item(), "|grad_meas|", leaves["meas"].grad.abs().max().item(),
              "poses0" if leaves["poses0"].grad is not None else "")
    np.savez_compressed(os.path.join(OUT, "pgso2_f64_unrolled.npz"), **out)


def main():
    th, _ = import_reference()
    torch.set_default_dtype(torch.float64)
    f = make_problem(th)
    gen_implicit(th, f, "pgso2_f64_implicit", robust=False)
    gen_implicit(th, f, "pgso2_f64_robust_implicit", robust=True)
    gen_unrolled(th, f)


if __name__ == "__main__":
    main()
