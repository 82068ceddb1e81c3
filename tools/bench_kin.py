"""ms per LM iteration of batched inverse kinematics on the Panda (examples/inverse_kinematics.py: LinkPoseCost on the end effector,
targets fk(rand), start from zeros, LM with step_size 0.5) in three variants, interleaved on one device:
  fused     PackedKinematics: thx_kin_eval / thx_kin_error
  torch     the SAME packed class with the fused evaluation switched off (``packed.fused = False``): every cost evaluated by its
            torch class (analytic Jacobian on theseus_amd/se3_torch.py)
  autodiff  the pose cost as an AutoDiffCostFunction over UrdfRobotModel.forward_kinematics on the generic path (PackedEuclidean;
            vmap(jacrev) through the Python loop over the links at every linearization)

    python tools/bench_kin.py --batch 64 1024 --dtype f32 --iters 15 --repeats 5 [--limits] [--out profiles/kin/x.jsonl]

One JSON line per batch size: median / min ms per iteration of the three variants, the ratios to the fused one and the final
objectives."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.inverse_kinematics import make_objective  # noqa: E402

VARIANTS = {"fused": ("PackedKinematics", True, False), "torch": ("PackedKinematics", False, False),
            "autodiff": ("PackedEuclidean", True, True)}


def optimizer(th, B, dtype, variant, iters, limits):
    family, fused, autodiff = VARIANTS[variant]
    obj, _, _ = make_objective(th, B, dtype, "cuda", limits=limits, autodiff=autodiff)
    opt = th.LevenbergMarquardt(obj, max_iterations=iters, step_size=0.5, abs_err_tolerance=0.0, rel_err_tolerance=0.0)
    packed = opt.linear_solver.linearization.packed
    assert type(packed).__name__ == family
    if family == "PackedKinematics":
        packed.fused = fused
    start = {k: v.tensor.clone() for k, v in obj.optim_vars.items()}
    return obj, opt, start


def run(obj, opt, start):
    obj.update({k: v.clone() for k, v in start.items()})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        opt.optimize(damping=0.1)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limits", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import theseus_amd as th
    dtype = torch.float32 if a.dtype == "f32" else torch.float64
    for B in a.batch:
        paths = {k: optimizer(th, B, dtype, k, a.iters, a.limits) for k in VARIANTS}
        for _ in range(a.warmup):
            for p in paths.values():
                run(*p)
        ms = {k: [] for k in paths}
        for _ in range(a.repeats):          # interleaved: the variants see the same clocks
            for k, p in paths.items():
                ms[k].append(run(*p) / a.iters)
        final = {k: float(p[1].linear_solver.linearization.packed.error_metric().mean()) for k, p in paths.items()}
        med = {k: statistics.median(v) for k, v in ms.items()}
        rec = dict(robot="panda", dof=7, costs=len(paths["fused"][0].cost_functions), limits=a.limits, batch=B, dtype=a.dtype,
                   iters=a.iters, warmup=a.warmup, repeats=a.repeats,
                   **{f"{k}_ms_per_iter": med[k] for k in VARIANTS}, **{f"{k}_min": min(ms[k]) for k in VARIANTS},
                   torch_over_fused=med["torch"] / med["fused"], autodiff_over_fused=med["autodiff"] / med["fused"],
                   **{f"final_error_{k}": final[k] for k in VARIANTS}, device=torch.cuda.get_device_name(0))
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
