"""Generate the DCEM fixtures by RUNNING THE REAL REFERENCE (test infrastructure; needs the reference importable, CPU only).

    python -m tools.gen_dcem_golden

The objective of tests/dcem_common.py on the reference, ``th.DCEM`` under ``torch.set_default_dtype(torch.double)`` (the reference
allocates sigma and the hard-mode weights in the default dtype).  The noise: the reference draws ``torch.empty(S, B, n).normal_()``
once per iteration (Normal.rsample) and nothing else consumes the global generator, so seeding, drawing the iterations' noise,
seeding again and running the optimizer gives a run whose samples are mu + noise[it] * sigma -- asserted below by replaying the run
with ``theseus_amd.dcem_update_torch`` on the recorded errors.  Writes under tests/golden/:
  dcem_f64_soft.npz    A, t, x0, noise (6, 40, 3, 4); per iteration fX (B, S) as the reference stacks it, w, mu, sigma; err_history,
                       status (names), converged_iter; and -- backward_mode="unroll" through th.TheseusLayer -- the gradients of
                       sum(solution^2) w.r.t. t and w.r.t. the initial x.
  dcem_f64_modes.npz   one recorded iteration for each mode of tests/dcem_common.py MODES: <mode>_noise, _fX, _w, _mu, _sigma.  The
                       reference exposes the weights only where it calls LML; for "hard" and "softmax" _w is the torch twin's, taken
                       from the run whose mu and sigma are asserted equal to the reference's.
Asserted: the reference printed no LML warning; in every bracketing round every grid value is at least 1e-6 away from zero (another
summation order cannot move a count); in hard mode the n_elite-th and the next smallest fX are at least 1e-6 apart.
"""
import contextlib
import io
import os

import numpy as np
import torch

from oracle.gen_golden import OUT, import_reference
from tests import dcem_common as dc

SEED = 5


def draw_noise(iters, S):
    torch.manual_seed(SEED)
    return torch.stack([torch.empty(S, dc.B, dc.N_DOF).normal_() for _ in range(iters)])


def run_reference(th, f, kw, optimizer_kwargs=None, grad=False):
    """One seeded run of th.DCEM -> dict(fX, w [LML calls only], mu, sigma per iteration; info; solution; leaves; printed)."""
    import theseus.optimizer.nonlinear.dcem as dcem_mod
    from theseus.third_party.lml import LML
    rec = dict(fX=[], w=[], mu=[], sigma=[])

    class RecordingLML(LML):
        def forward(self, x):
            y = super().forward(x)
            rec["w"].append(y.detach().clone())
            return y

    obj, leaves = dc.build(th, f, grad=grad)
    opt = th.DCEM(obj, vectorize=False, **kw)
    error_metric = obj.error_metric
    calls = []

    def recording_error_metric(input_tensors=None, **kwargs):
        out = error_metric(input_tensors, **kwargs)
        if input_tensors is not None:
            calls.append(out.detach().clone())
        return out

    def callback(optimizer, info, mu, it):
        rec["fX"].append(torch.stack(calls, dim=1))
        calls.clear()
        rec["mu"].append(torch.cat([mu[v.name] for v in optimizer.ordering], dim=1).detach().clone())
        rec["sigma"].append(optimizer.sigma.detach().clone())

    obj.error_metric = recording_error_metric
    saved, dcem_mod.LML = dcem_mod.LML, RecordingLML
    printed = io.StringIO()
    try:
        torch.manual_seed(SEED)
        with contextlib.redirect_stdout(printed):
            layer = th.TheseusLayer(opt, vectorize=False)
            inputs = {"x": leaves["x0"]} if grad else None
            kwargs = dict(track_err_history=True, end_iter_callback=callback, **(optimizer_kwargs or {}))
            if grad:
                sol, info = layer.forward(inputs, optimizer_kwargs=kwargs)
            else:
                with torch.no_grad():
                    sol, info = layer.forward(inputs, optimizer_kwargs=kwargs)
    finally:
        dcem_mod.LML = saved
    assert "LML Warning" not in printed.getvalue(), printed.getvalue()
    return dict(rec=rec, info=info, sol=torch.cat([sol[v.name] for v in opt.ordering], dim=1), leaves=leaves, opt=opt)


def replay(noise, f, rec, kw):
    """The run again on theseus_amd's torch twin from the recorded errors -> (worst deviation of w / mu / sigma relative to the largest
    magnitude, smallest |grid value| of any LML round)."""
    from theseus_amd.dcem import dcem_update_torch
    mu, sigma = torch.from_numpy(f["x0"]), torch.ones(dc.B, dc.N_DOF)
    worst, margin = 0.0, float("inf")
    for it in range(len(rec["mu"])):
        X = dc.samples(mu, sigma, noise[it])
        out = dcem_update_torch(rec["fX"][it].t().contiguous(), X, kw.get("n_elite", dc.N_ELITE), kw.get("temp", 1.0),
                                kw.get("normalize", True), 1e-3, 100, dc.BRANCH, with_margin=True)
        pairs = [(out[0], rec["mu"][it]), (out[1], rec["sigma"][it])] + ([(out[2], rec["w"][it])] if rec["w"] else [])
        for a, b in pairs:
            worst = max(worst, float((a - b).abs().max() / b.abs().max()))
        margin = min(margin, float(out[6]))
        mu, sigma = rec["mu"][it], rec["sigma"][it]
    return worst, margin


def main():
    th, _ = import_reference()
    torch.set_default_dtype(torch.float64)
    f = dc.problem()
    # ---- the soft (LML) run ----
    noise = draw_noise(dc.N_ITER, dc.N_SAMPLE)
    run = run_reference(th, f, dc.DCEM_KW)
    rec, info = run["rec"], run["info"]
    assert len(rec["mu"]) == dc.N_ITER and len(rec["w"]) == dc.N_ITER
    worst, margin = replay(noise, f, rec, dc.DCEM_KW)
    assert worst <= 1e-14, f"the twin's replay of the reference's run deviates by {worst:.2e}"
    assert margin >= 1e-6, f"a grid value of an LML round lies {margin:.2e} from zero"
    out = dict(f, noise=noise.numpy(), fX=torch.stack(rec["fX"]).numpy(), w=torch.stack(rec["w"]).numpy(),
               mu=torch.stack(rec["mu"]).numpy(), sigma=torch.stack(rec["sigma"]).numpy(), err_history=info.err_history.numpy(),
               status=np.array([s.name for s in info.status]), converged_iter=info.converged_iter.numpy(),
               last_err=info.last_err.numpy())
    grad_run = run_reference(th, f, dc.DCEM_KW, dict(backward_mode="unroll"), grad=True)
    assert torch.equal(grad_run["sol"].detach(), rec["mu"][-1]), "the differentiated run took other samples"
    loss = (grad_run["sol"] ** 2).sum()
    loss.backward()
    out.update(loss=loss.item(), grad_t=grad_run["leaves"]["t"].grad.numpy(), grad_x0=grad_run["leaves"]["x0"].grad.numpy())
    np.savez_compressed(os.path.join(OUT, "dcem_f64_soft.npz"), **out)
    print("dcem_f64_soft: err", out["err_history"][:, 0], "->", out["err_history"][:, -1], "replay", worst, "margin", margin,
          "status", out["status"], "|grad_t|", np.abs(out["grad_t"]).max(), "|grad_x0|", np.abs(out["grad_x0"]).max())
    # ---- one iteration per mode ----
    modes = dict(A=f["A"], t=f["t"], x0=f["x0"])
    for name, (extra, S) in dc.MODES.items():
        kw = dict(dc.DCEM_KW, max_iterations=1, **extra)
        noise = draw_noise(1, S)
        rec = run_reference(th, f, kw)["rec"]
        fX = rec["fX"][0]
        if name == "hard":
            ordered = fX.sort(dim=1).values
            gap = float((ordered[:, kw["n_elite"]] - ordered[:, kw["n_elite"] - 1]).min())
            assert gap >= 1e-6, f"hard mode: the elite boundary is {gap:.2e} wide"
        worst, margin = replay(noise, f, rec, kw)
        assert worst <= 1e-14 and margin >= 1e-6, (name, worst, margin)
        from theseus_amd.dcem import dcem_update_torch
        w = rec["w"][0] if rec["w"] else dcem_update_torch(fX.t().contiguous(), dc.samples(torch.from_numpy(f["x0"]), 1.0, noise[0]),
                                                           kw["n_elite"], kw.get("temp", 1.0), branch=dc.BRANCH)[2]
        modes.update({f"{name}_noise": noise.numpy(), f"{name}_fX": fX.numpy(), f"{name}_w": w.numpy(),
                      f"{name}_mu": rec["mu"][0].numpy(), f"{name}_sigma": rec["sigma"][0].numpy()})
        print("dcem_f64_modes:", name, "replay", worst, "margin", margin, "sum w", w.sum(dim=1).numpy())
    np.savez_compressed(os.path.join(OUT, "dcem_f64_modes.npz"), **modes)


if __name__ == "__main__":
    main()
