"""ms per training step of homography estimation (examples/homography_estimation.py): LM iterations through TheseusLayer with
backward_mode="implicit", then loss.backward() into both feature maps -- on the fused backward (PackedHomography.fused_backward =
True: thx_homog_vjp) and on the torch classes (False), the same objective on one device, runs interleaved.

    python tools/bench_homog_backward.py --size 60 80 --channels 1 32 --batch 64 1024 --dtype f32 --iters 10 --repeats 7 [--out profiles/homog_vjp/x.jsonl]

One JSON line per (channels, batch): median and min - max of forward + backward per call (wall clock around both, synchronised) and
of the backward alone (events around loss.backward()), per side; "faster" only where the median lies below the other side's by more
than that side's min - max spread.  On a commit without the kernel both sides are the torch classes."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.homography_estimation import IDENTITY8, image_pairs, make_objective  # noqa: E402

LEAVES = ("feat1", "feat2")


def layer(th, B, C, Hh, Ww, dtype, fused_backward, iters):
    """feature maps: C affine copies of the image pair (what a first CNN layer would hand over); H8 starts half a pixel off the
    identity, where no source coordinate is an integer"""
    img1, img2, _ = image_pairs(B, Hh, Ww, dtype, "cuda")
    gain = torch.linspace(0.5, 1.5, C, dtype=dtype, device="cuda").view(1, C, 1, 1)
    obj = make_objective(th, (img1 * gain).contiguous(), (img2 * gain).contiguous(), dtype, "cuda")
    leaves = {k: obj.get_variable(k).tensor.requires_grad_(True) for k in LEAVES}
    opt = th.LevenbergMarquardt(obj, max_iterations=iters, step_size=0.1, abs_err_tolerance=0.0, rel_err_tolerance=0.0)
    packed = opt.linear_solver.linearization.packed
    assert type(packed).__name__ == "PackedHomography"
    packed.fused_backward = fused_backward
    start = torch.tensor([IDENTITY8], dtype=dtype, device="cuda").repeat(B, 1)
    start[:, 2] += 1.0 / (Ww - 1)
    start[:, 5] += 1.0 / (Hh - 1)
    return th.TheseusLayer(opt), leaves, {"H8_1_2": start}


def step(layer_, leaves, start):
    """-> (ms forward + backward, ms backward alone)"""
    for leaf in leaves.values():
        leaf.grad = None
    before, after = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sol, _ = layer_.forward({k: v.clone() for k, v in start.items()}, optimizer_kwargs=dict(backward_mode="implicit"))
    loss = (sol["H8_1_2"] ** 2).sum()
    before.record()
    loss.backward()
    after.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, before.elapsed_time(after)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[60, 80])
    ap.add_argument("--channels", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import theseus_amd as th
    dtype = torch.float32 if a.dtype == "f32" else torch.float64
    Hh, Ww = a.size
    for C in a.channels:
        for B in a.batch:
            sides = {"fused": layer(th, B, C, Hh, Ww, dtype, True, a.iters), "torch": layer(th, B, C, Hh, Ww, dtype, False, a.iters)}
            for _ in range(a.warmup):
                for s in sides.values():
                    step(*s)
            ms = {k: [] for k in sides}
            for _ in range(a.repeats):          # interleaved: both sides see the same clocks
                for k, s in sides.items():
                    ms[k].append(step(*s))
            rec = dict(size=[Hh, Ww], channels=C, batch=B, dtype=a.dtype, iters=a.iters, repeats=a.repeats,
                       device=torch.cuda.get_device_name(0), has_kernel=hasattr(th.HipKernels, "homog_vjp"))
            for k, v in ms.items():
                for what, col in (("step", 0), ("backward", 1)):
                    t = [x[col] for x in v]
                    rec[f"{k}_{what}_ms"], rec[f"{k}_{what}_min"], rec[f"{k}_{what}_max"] = statistics.median(t), min(t), max(t)
            for what in ("step", "backward"):
                spread = rec[f"torch_{what}_max"] - rec[f"torch_{what}_min"]
                rec[f"{what}_faster"] = rec[f"fused_{what}_ms"] < rec[f"torch_{what}_ms"] - spread
            # the two sides computed the same thing: the largest gradient difference relative to the torch side's largest entry
            rec["grad_rel_diff"] = max(float((sides["fused"][1][k].grad - sides["torch"][1][k].grad).abs().max() /
                                             sides["torch"][1][k].grad.abs().max().clamp_min(1e-30)) for k in LEAVES)
            # ... and per problem (the homographies are not kept off the pixel lattice: a source coordinate that rounds to the other
            # side of an integer in the torch twin moves that problem's gradient, and no other's): the median problem, and how
            # many problems differ by more than 1e-4 of their own largest entry
            per = torch.stack([(sides["fused"][1][k].grad - sides["torch"][1][k].grad).abs().flatten(1).amax(1) /
                               sides["torch"][1][k].grad.abs().flatten(1).amax(1).clamp_min(1e-30) for k in LEAVES]).amax(0)
            rec["grad_rel_diff_median_problem"], rec["problems_above_1e-4"] = float(per.median()), int((per > 1e-4).sum())
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            del sides
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
