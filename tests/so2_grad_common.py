"""Gradients of SO2 pose graphs (th.Between + th.Difference on th.SO2) through th.TheseusLayer -- backward_mode "implicit", "unroll"
and "truncated" -- against what the REAL reference recorded (tests/golden/pgso2_f64_{implicit,robust_implicit,unrolled}.npz,
tools/gen_golden_so2_grad.py).  ``th`` is theseus_amd (its own loop) or the reference's theseus (its loop with the plugin): both take
the same objective.  Shared by the CPU tests (stand-in kernels), the GPU tests (HIP kernels) and the fixture generator."""
import ast

import numpy as np
import torch

TOL_FINAL_IMPLICIT = 1e-7          # tests/implicit_common.py:check_against_reference
TOL_FINAL_UNROLLED = 1e-9          # tests/unrolled_common.py:run_pg_unrolled (2e-8 with robust costs)
REL_GRAD, REL_GRAD_POSES0 = 2e-6, 1e-5


def build(th, g, device="cpu", robust=False, poses0_grad=False, dtype=None):
    """The objective of fixture ``g`` with requires_grad leaves (measurements, between weights, prior targets, prior scales [, the
    two log_loss_radius, the initial poses]).  robust: WelschLoss on every Between cost, HuberLoss on the priors, one radius per
    role.  Returns (objective, leaves)."""
    dtype = dtype or torch.float64
    t = lambda a: torch.as_tensor(np.asarray(a)).to(device=device, dtype=dtype)  # noqa: E731
    G = th.SO2
    leaves = dict(meas=t(g["meas"]).requires_grad_(True), w_between=t(g["w_between"]).requires_grad_(True),
                  prior_target=t(g["prior_target"]).requires_grad_(True), w_prior=t(g["w_prior"]).requires_grad_(True))
    p0 = t(g["poses0"])
    if poses0_grad:
        p0 = leaves["poses0"] = p0.requires_grad_(True)
    wrap_b = wrap_p = lambda cf, nm: cf  # noqa: E731
    if robust:
        leaves["log_radius_between"] = t(np.full((1, 1), float(g["log_radius_between"]))).requires_grad_(True)
        leaves["log_radius_prior"] = t(np.full((1, 1), float(g["log_radius_prior"]))).requires_grad_(True)
        rb = th.Vector(tensor=leaves["log_radius_between"], name="log_radius_between")
        rp = th.Vector(tensor=leaves["log_radius_prior"], name="log_radius_prior")
        wrap_b = lambda cf, nm: th.RobustCostFunction(cf, th.WelschLoss, rb, name=nm)  # noqa: E731
        wrap_p = lambda cf, nm: th.RobustCostFunction(cf, th.HuberLoss, rp, name=nm)  # noqa: E731
    obj = th.Objective(dtype=dtype)
    pv = [G(tensor=p0[:, k] if poses0_grad else p0[:, k].clone(), name=f"pose_{k}") for k in range(int(g["P"]))]
    for k in range(g["edges"].shape[0]):
        i, j = np.asarray(g["edges"])[k].tolist()
        obj.add(wrap_b(th.Between(pv[i], pv[j], G(tensor=leaves["meas"][:, k], name=f"meas_{k}"),
                                  th.DiagonalCostWeight(th.Variable(leaves["w_between"][:, k], name=f"w_{k}")), name=f"between_{k}"),
                       f"robust_between_{k}"))
    for k in range(g["prior_idx"].shape[0]):
        obj.add(wrap_p(th.Difference(pv[int(g["prior_idx"][k])], G(tensor=leaves["prior_target"][:, k], name=f"tgt_{k}"),
                                     th.ScaleCostWeight(th.Variable(leaves["w_prior"][:, k], name=f"pw_{k}")), name=f"prior_{k}"),
                       f"robust_prior_{k}"))
    return obj, leaves


def run(th, g, device="cpu", tag=None, robust=False, dtype=None, optimizer_kwargs=None, to_device=False):
    """One TheseusLayer forward + backward of loss = <coef, final poses>.  tag None: the implicit fixture's run (opt_kwargs); else the
    unrolled fixture's run ``tag``.  optimizer_kwargs: extra constructor arguments (kernels, the plugin's classes).  to_device: move
    the layer (the reference's objects are built on the CPU and moved).  Returns (final poses, loss, {leaf: grad}, info)."""
    if tag is None:
        kw = ast.literal_eval(str(g["opt_kwargs"]))
        mode, step = "implicit", kw.pop("step_size")
    else:
        kw = ast.literal_eval(str(g[f"{tag}_kwargs"]))
        mode, step = kw.pop("mode"), 1.0
    iters, gn = kw.pop("max_iterations"), kw.pop("gauss_newton")
    obj, leaves = build(th, g, "cpu" if to_device else device, robust=robust, dtype=dtype,
                        poses0_grad=tag is not None and f"{tag}_grad_poses0" in g)
    cls = th.GaussNewton if gn else th.LevenbergMarquardt
    opt = cls(obj, max_iterations=iters, step_size=step, abs_err_tolerance=0.0, rel_err_tolerance=0.0, **(optimizer_kwargs or {}))
    layer = th.TheseusLayer(opt)
    if to_device:
        layer.to(device)
    sol, info = layer.forward(None, optimizer_kwargs=dict(backward_mode=mode, track_err_history=True, **kw))
    final = torch.stack([sol[f"pose_{k}"] for k in range(int(g["P"]))], 1)
    loss = (torch.as_tensor(np.asarray(g["coef"])).to(final) * final).sum()
    loss.backward()
    grads = {k: v.grad.detach().cpu() for k, v in leaves.items() if v.grad is not None}
    return final.detach().cpu(), float(loss.detach()), grads, info


def check_implicit(g, final, loss, grads, rel=REL_GRAD):
    """tests/implicit_common.py:check_against_reference, plus the two log_loss_radius gradients of the robust fixture."""
    from tests.implicit_common import check_against_reference
    check_against_reference(g, final.double(), loss, {k: v.double() for k, v in grads.items()}, rel=rel)
    for key in ("log_radius_between", "log_radius_prior"):
        if f"grad_{key}" in g:
            want = g[f"grad_{key}"]
            np.testing.assert_allclose(grads[key].double().numpy(), want, rtol=0, atol=rel * np.abs(want).max(), err_msg=key)


def check_unrolled(g, tag, final, loss, grads, info):
    """The bars of tests/unrolled_common.py:run_pg_unrolled."""
    np.testing.assert_allclose(final.numpy(), g[f"{tag}_final"], rtol=0, atol=TOL_FINAL_UNROLLED)
    np.testing.assert_allclose(info.err_history.cpu().numpy(), g[f"{tag}_err_history"], rtol=1e-6)
    assert abs(loss - float(g[f"{tag}_loss"])) < 10 * TOL_FINAL_UNROLLED
    for key in ("meas", "w_between", "prior_target", "w_prior"):
        want = g[f"{tag}_grad_{key}"]
        np.testing.assert_allclose(grads[key].numpy(), want, rtol=0, atol=REL_GRAD * np.abs(want).max(), err_msg=key)
    if f"{tag}_grad_poses0" in g:
        want = g[f"{tag}_grad_poses0"]
        np.testing.assert_allclose(grads["poses0"].numpy(), want, rtol=0, atol=REL_GRAD_POSES0 * np.abs(want).max(), err_msg="poses0")
    else:
        assert "poses0" not in grads
