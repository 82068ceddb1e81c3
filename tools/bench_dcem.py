"""ms per DCEM iteration, and ms of the update alone, with the update on the kernels (thx_dcem_update) and on the torch twin
(``dcem_update_torch``) on the same device, interleaved; and ms of the kernels' backward (thx_dcem_update_vjp) alone:

    python tools/bench_dcem.py --batch 64 1024 --dtype f32 [--samples 100] [--out profiles/dcem/bench_dcem_f32.jsonl]

Objectives: batched IK on the Panda (examples/inverse_kinematics.py, n = 7, samples evaluated by thx_kin_error) and the 2D motion
planner (examples/motion_planning_2d.py with 100 intervals, n = 404, thx_traj2_error).  S = 100 samples (``--samples``), 5 elites,
100 grid values per LML round.  The optimizer itself never calls the twin: for the "twin" iteration this tool swaps the autograd Function of
theseus_amd/dcem.py for one that calls the twin, everything else -- sampling, S + 1 error launches, bookkeeping -- is the same.
Times are a host clock around work that ends in a device synchronise; one JSON line per (objective, batch)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.inverse_kinematics import make_objective as panda_objective  # noqa: E402
from examples.motion_planning_2d import make_objective as planner_objective  # noqa: E402

N_ELITE, BRANCH = 5, 100


class TwinUpdate:
    """stands in for theseus_amd.dcem.DcemUpdate: the same call on the torch twin"""

    @staticmethod
    def apply(fX, X, K, n_elite, temp, normalize, lml_eps, lml_n_iter, branch, out):
        from theseus_amd.dcem import dcem_update_torch
        res = dcem_update_torch(fX, X, n_elite, temp, normalize, lml_eps, lml_n_iter, branch)
        if out is not None:
            out[0].copy_(res[0])
            out[1].copy_(res[1])
            return (out[0], out[1]) + res[2:]
        return res


def timed(fn, repeats):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / repeats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S = a.samples
    import theseus_amd as th
    from theseus_amd import dcem as dcem_mod
    dtype = torch.float32 if a.dtype == "f32" else torch.float64
    kernel_update = dcem_mod.DcemUpdate
    for name, make in (("panda_ik", lambda B: panda_objective(th, B, dtype, "cuda")[0]),
                       ("motion_planning_2d", lambda B: planner_objective(th, 100, B, dtype, "cuda"))):
        for B in a.batch:
            obj = make(B)
            opt = th.DCEM(obj, max_iterations=a.iters, n_sample=S, n_elite=N_ELITE, init_sigma=0.1, abs_err_tolerance=0.0,
                          rel_err_tolerance=0.0, lml_branch=BRANCH)
            start = {k: v.tensor.clone() for k, v in obj.optim_vars.items()}
            gen = torch.Generator(device="cuda")

            def iteration(update):
                dcem_mod.DcemUpdate = update
                try:
                    obj.update({k: v.clone() for k, v in start.items()})
                    gen.manual_seed(3)
                    with torch.no_grad():
                        opt.optimize(generator=gen)
                finally:
                    dcem_mod.DcemUpdate = kernel_update
            # the update alone, on the samples of a first iteration
            n = opt.packed.n
            opt.packed.sync()
            X = torch.randn(S, B, n, generator=gen.manual_seed(4), dtype=dtype, device="cuda") * 0.1 + opt.packed.state.unsqueeze(0)
            fX = torch.stack([opt.packed.error_metric(state=X[s]).clone() for s in range(S)])
            args = (fX, X, th.default_kernels(), N_ELITE, 1.0, True, 1e-3, 100, BRANCH, None)
            variants = {"kernel": kernel_update, "twin": TwinUpdate}
            with torch.no_grad():
                for u in variants.values():          # warm-up: every shape of the timed window
                    iteration(u)
                    u.apply(*args)
                it_ms, up_ms = {k: [] for k in variants}, {k: [] for k in variants}
                for _ in range(a.repeats):           # interleaved: the variants see the same clocks
                    for k, u in variants.items():
                        it_ms[k].append(timed(lambda: iteration(u), 1) / a.iters)
                        up_ms[k].append(timed(lambda: u.apply(*args), 20))
                got, want = kernel_update.apply(*args), TwinUpdate.apply(*args)
                # the kernel's backward alone (thx_dcem_update_vjp), on the forward's own outputs
                mu, sigma, w = got[:3]
                grads = (torch.randn_like(mu), torch.randn_like(sigma))
                grad_X, grad_fX = torch.empty_like(X), torch.empty_like(fX)
                vjp = lambda: th.default_kernels().dcem_update_vjp(*grads, X, fX, w, mu, sigma, N_ELITE, 1.0, True, grad_X, grad_fX)  # noqa: E731
                vjp()
                vjp_ms = statistics.median(timed(vjp, 20) for _ in range(a.repeats))
            dev = max(float((g - w).abs().max() / w.abs().max()) for g, w in zip(got[:3], want[:3]))
            med = lambda d: {k: statistics.median(v) for k, v in d.items()}  # noqa: E731
            it, up = med(it_ms), med(up_ms)
            rec = dict(objective=name, packed=type(opt.packed).__name__, n=n, batch=B, dtype=a.dtype, samples=S, n_elite=N_ELITE,
                       branch=BRANCH, iters=a.iters, repeats=a.repeats,
                       iteration_ms_kernel=it["kernel"], iteration_ms_twin=it["twin"], iteration_twin_over_kernel=it["twin"] / it["kernel"],
                       update_ms_kernel=up["kernel"], update_ms_twin=up["twin"], update_twin_over_kernel=up["twin"] / up["kernel"],
                       iteration_ms_kernel_min=min(it_ms["kernel"]), iteration_ms_twin_min=min(it_ms["twin"]),
                       update_ms_kernel_min=min(up_ms["kernel"]), update_ms_twin_min=min(up_ms["twin"]),
                       vjp_ms_kernel=vjp_ms, update_deviation_from_twin=dev, device=torch.cuda.get_device_name(0))
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
