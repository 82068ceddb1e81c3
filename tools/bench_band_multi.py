"""Blocks of right-hand sides and marginal covariances on the band factor (thx_pb_solve_multi, thx_pb_inverse_band) against the
routes that exist without them, on the 2D motion planner of examples/motion_planning_2d.py.  The protocol of tools/bench_band.py: one
device, all sides interleaved, 2 warm-ups, median of 7 repeats with min .. max, fp32.

    python tools/bench_band_multi.py --intervals 100 --batch 64 1024 [--out profiles/band_multi/x.jsonl]

One JSON line per batch size and case (ms per call, synchronised before and after):
  * solve_multi, k = 10 and 128 vectors: HipBandedCholeskySolver.solve_multi_with_factor / HipCholeskySolver.solve_multi_with_factor
    on the dense factor of the same objective / a loop of k thx_band_solve calls;
  * marginals: HipBandedCholeskySolver.marginal_covariances() (one thx_pb_inverse_band launch) / HipCholeskySolver.marginal_covariance
    called once per variable / n unit vectors through thx_pb_solve_multi, each after its own undamped factorisation.
``faster_than_*``: the first side's median lies below the other's by more than the other's own min .. max spread."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.motion_planning_2d import make_objective  # noqa: E402
from tools.bench_band import emit, faster, stats  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def compare(sides, warmup, repeats):
    for _ in range(warmup):
        for fn in sides.values():
            fn()
    t = {k: [] for k in sides}
    for _ in range(repeats):
        for k, fn in sides.items():
            t[k].append(timed(fn))
    return {k: stats(v) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--intervals", type=int, default=100)
    ap.add_argument("--batch", type=int, nargs="*", default=[64, 1024])
    ap.add_argument("--vectors", type=int, nargs="*", default=[10, 128])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import theseus_amd as th
    for B in a.batch:
        obj = make_objective(th, a.intervals, B, torch.float32, "cuda")
        banded, dense = th.HipBandedCholeskySolver(obj), th.HipCholeskySolver(obj)
        with torch.no_grad():
            obj.update()
            for s in (banded, dense):
                s.linearization.linearize()
                s.solve()
        n, kd, K = banded.linearization.n, banded.band_plan().kd, banded.K
        common = dict(intervals=a.intervals, n=n, kd=kd, batch=B, dtype="f32", warmup=a.warmup, repeats=a.repeats,
                      device=torch.cuda.get_device_name(0))
        for k in a.vectors:
            R = torch.randn(B, k, n, dtype=torch.float32, device="cuda")
            Rl = R.transpose(0, 1).contiguous()          # (k, B, n): one contiguous (B, n) block per single-vector call
            Xl = torch.empty_like(Rl)

            def loop():
                for s in range(k):
                    K.band_solve(banded.Lb, n, kd, banded._perm, Rl[s], Xl[s])
            t = compare({"pb_solve_multi": lambda: banded.solve_multi_with_factor(R), "dense_solve_multi": lambda: dense.solve_multi_with_factor(R),
                         "band_solve_loop": loop}, a.warmup, a.repeats)
            emit(dict(what="solve_multi", vectors=k, ms=t, faster_than_dense=faster(t["pb_solve_multi"], t["dense_solve_multi"]),
                      faster_than_loop=faster(t["pb_solve_multi"], t["band_solve_loop"]), **common), a.out)
        names = [v.name for v in banded.linearization.ordering]
        eye = torch.eye(n, dtype=torch.float32, device="cuda").expand(B, n, n).contiguous()

        def unit_vectors():
            banded._factorize_undamped()
            return banded.solve_multi_with_factor(eye)
        t = compare({"pb_inverse_band": banded.marginal_covariances, "dense_per_variable": lambda: [dense.marginal_covariance([v]) for v in names],
                     "pb_unit_vectors": unit_vectors}, a.warmup, a.repeats)
        emit(dict(what="marginals", variables=len(names), ms=t, faster_than_dense=faster(t["pb_inverse_band"], t["dense_per_variable"]),
                  faster_than_unit_vectors=faster(t["pb_inverse_band"], t["pb_unit_vectors"]), **common), a.out)
        del obj, banded, dense, eye
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
