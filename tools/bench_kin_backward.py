"""ms per training step of inverse kinematics (examples/inverse_kinematics.py: the Panda with joint limits and a rest-pose prior):
15 LM iterations through TheseusLayer with backward_mode="implicit", then loss.backward() into every auxiliary tensor -- the pose
target, every weight, the hinge's limits and threshold, the prior's target -- on the fused backward (PackedKinematics.fused_backward =
True: thx_kin_vjp) and on the torch classes (False), the same objective on one device, runs interleaved.  Both sides share the fused
forward.

    python tools/bench_kin_backward.py --batch 64 1024 --dtype f32 --iters 15 --repeats 7 [--out profiles/kin_vjp/x.jsonl]

One JSON line per batch size: median and min - max of forward + backward per call (wall clock around both, synchronised) and of the
backward alone (events around loss.backward()), per side; "faster" only where the median lies below the other side's by more than
that side's min - max spread."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.inverse_kinematics import make_objective  # noqa: E402


def layer(th, B, dtype, fused_backward, iters):
    obj, _, _ = make_objective(th, B, dtype, "cuda", limits=True)
    leaves = {(c.name, k): v.tensor.requires_grad_(True) for c in obj.cost_functions.values() for k, v in enumerate(c.aux_vars())}
    opt = th.LevenbergMarquardt(obj, max_iterations=iters, step_size=0.5, abs_err_tolerance=0.0, rel_err_tolerance=0.0)
    packed = opt.linear_solver.linearization.packed
    assert type(packed).__name__ == "PackedKinematics"
    packed.fused_backward = fused_backward
    start = {k: v.tensor.detach().clone() for k, v in obj.optim_vars.items()}
    return th.TheseusLayer(opt), leaves, start


def step(layer_, leaves, start):
    """-> (ms forward + backward, ms backward alone)"""
    for leaf in leaves.values():
        leaf.grad = None
    before, after = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sol, _ = layer_.forward({k: v.clone() for k, v in start.items()}, optimizer_kwargs=dict(damping=0.1, backward_mode="implicit"))
    loss = (sol["theta"] ** 2).sum()
    before.record()
    loss.backward()
    after.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, before.elapsed_time(after)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import theseus_amd as th
    dtype = torch.float32 if a.dtype == "f32" else torch.float64
    for B in a.batch:
        sides = {"fused": layer(th, B, dtype, True, a.iters), "torch": layer(th, B, dtype, False, a.iters)}
        for _ in range(a.warmup):
            for s in sides.values():
                step(*s)
        ms = {k: [] for k in sides}
        for _ in range(a.repeats):          # interleaved: both sides see the same clocks
            for k, s in sides.items():
                ms[k].append(step(*s))
        rec = dict(batch=B, dtype=a.dtype, iters=a.iters, repeats=a.repeats, device=torch.cuda.get_device_name(0))
        for k, v in ms.items():
            for what, col in (("step", 0), ("backward", 1)):
                t = [x[col] for x in v]
                rec[f"{k}_{what}_ms"], rec[f"{k}_{what}_min"], rec[f"{k}_{what}_max"] = statistics.median(t), min(t), max(t)
        for what in ("step", "backward"):
            spread = rec[f"torch_{what}_max"] - rec[f"torch_{what}_min"]
            rec[f"{what}_faster"] = rec[f"fused_{what}_ms"] < rec[f"torch_{what}_ms"] - spread
        # the two sides computed the same thing: the largest gradient difference relative to the torch side's largest entry
        rec["grad_rel_diff"] = max(float((sides["fused"][1][k].grad - sides["torch"][1][k].grad).abs().max() /
                                         sides["torch"][1][k].grad.abs().max().clamp_min(1e-30)) for k in sides["torch"][1])
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
