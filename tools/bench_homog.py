"""ms per LM iteration of the homography-alignment objective of examples/homography_estimation.py (HomographyAlignment + a Difference
regulariser, H8 from the identity, step size 0.1) on three paths -- same feature maps, same kernels downstream, interleaved on one
device:
  fused     PackedHomography: thx_homog_eval / thx_homog_error
  torch     the same packed class with ``fused = False``: the torch class's analytic jacobians() at every iteration
  autodiff  an AutoDiffCostFunction (vmap(jacrev)) on the same error function, on the generic path (PackedEuclidean): what a user
            could write before this family existed

    python tools/bench_homog.py --batch 64 1024 --channels 1 32 --size 60 80 --dtype f32 --iters 10 --repeats 7 [--out profiles/homog/x.jsonl]

The feature maps are the synthetic image pairs of the example, repeated over the channels with a per-channel gain.  Times: a host
clock around ``optimize`` ending in a device synchronise, after warm-up runs of every path; medians and minima over the repeats.
One JSON line per (batch, channels): ms per iteration of each path, the ratios, the final objective of each path (they must agree)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.homography_estimation import IDENTITY8, REG_WEIGHT, image_pairs, make_objective  # noqa: E402


def feature_maps(B, C, Hh, Ww, dtype):
    img1, img2, _ = image_pairs(B, Hh, Ww, dtype, "cuda")
    gain = torch.linspace(0.5, 1.5, C, dtype=dtype, device="cuda").view(1, C, 1, 1)
    return (img1 * gain).contiguous(), (img2 * gain).contiguous()


def autodiff_objective(th, feat1, feat2, dtype):
    def align_error(optim_vars, aux_vars):
        return th.eb.HomographyAlignment(optim_vars[0], aux_vars[0], aux_vars[1]).error()
    eye = torch.tensor([IDENTITY8], dtype=dtype, device="cuda")
    H8 = th.Vector(tensor=eye.repeat(feat1.shape[0], 1), name="H8_1_2")
    obj = th.Objective(dtype=dtype)
    obj.add(th.AutoDiffCostFunction([H8], align_error, 1, aux_vars=[th.Variable(feat1, name="feat1"), th.Variable(feat2, name="feat2")],
                                    cost_weight=th.ScaleCostWeight(torch.ones(1, 1, dtype=dtype, device="cuda")), name="alignment"))
    reg = th.ScaleCostWeight(th.Variable(torch.full((1, 1), REG_WEIGHT, dtype=dtype, device="cuda"), name="reg_w"))
    obj.add(th.Difference(H8, th.Vector(tensor=eye.clone(), name="identity"), reg, name="reg_homography"))
    return obj


def optimizer(th, path, feat1, feat2, dtype, iters):
    obj = autodiff_objective(th, feat1, feat2, dtype) if path == "autodiff" else make_objective(th, feat1, feat2, dtype, "cuda")
    opt = th.LevenbergMarquardt(obj, max_iterations=iters, step_size=0.1, abs_err_tolerance=0.0, rel_err_tolerance=0.0)
    packed = opt.linear_solver.linearization.packed
    assert type(packed).__name__ == ("PackedEuclidean" if path == "autodiff" else "PackedHomography")
    if path == "torch":
        packed.fused = False
    start = {k: v.tensor.clone() for k, v in obj.optim_vars.items()}
    return obj, opt, start


def run(obj, opt, start):
    obj.update({k: v.clone() for k, v in start.items()})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        opt.optimize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--channels", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--size", type=int, nargs=2, default=[60, 80])
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--paths", nargs="+", default=["fused", "torch", "autodiff"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import theseus_amd as th
    if not torch.cuda.is_available():
        raise SystemExit("bench_homog: no HIP device; there is nothing to measure on a CPU")
    dtype = torch.float32 if a.dtype == "f32" else torch.float64
    Hh, Ww = a.size
    for B in a.batch:
        for C in a.channels:
            feat1, feat2 = feature_maps(B, C, Hh, Ww, dtype)
            paths = {p: optimizer(th, p, feat1, feat2, dtype, a.iters) for p in a.paths}
            for _ in range(a.warmup):
                for p in paths.values():
                    run(*p)
            ms = {k: [] for k in paths}
            for _ in range(a.repeats):          # interleaved: every path sees the same clocks
                for k, p in paths.items():
                    ms[k].append(run(*p) / a.iters)
            rec = dict(batch=B, channels=C, size=[Hh, Ww], dtype=a.dtype, iters=a.iters, repeats=a.repeats, step_size=0.1)
            for k, p in paths.items():
                rec[f"{k}_ms_per_iter"], rec[f"{k}_min"] = statistics.median(ms[k]), min(ms[k])
                rec[f"final_error_{k}"] = float(p[0].error_metric().mean())
            for k in paths:
                if k != "fused" and "fused" in paths:
                    rec[f"{k}_over_fused"] = rec[f"{k}_ms_per_iter"] / rec["fused_ms_per_iter"]
            rec["device"] = torch.cuda.get_device_name(0)
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            del paths, feat1, feat2
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
