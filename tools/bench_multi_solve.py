"""Micro-benchmark of thx_chol_solve_multi against a loop of nrhs calls of the single-vector thx_chol_solve on the same factor (HIP
events on torch's current stream; one warm-up call each, then interleaved rounds, the median reported).

usage: python tools/bench_multi_solve.py [--n 1536] [--batch 256] [--nrhs 1,8,32,64] [--dtype f32] [--which 0] [--rounds 7] [--out FILE]
Prints one JSON line per nrhs.  ``L_TB_per_s``: terabytes of L the call streams (every tile of the lower triangle, once per
substitution and group of 32 vectors) over the median time, beside the 8 TB/s HBM peak; ``mfma_fraction``: the flops of the
triangular products (2 n^2 per vector and substitution on the full tiles the kernel multiplies) over the matrix-core peak."""
import argparse
import json
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from theseus_amd.kernels import default_kernels, round_up

# MI355X: v_mfma_f32_32x32x2_f32 157.3 TFLOP/s, v_mfma_f64_16x16x4_f64 78.6 TFLOP/s; HBM3E 8 TB/s
PEAK = {"f32": 157.3e12, "f64": 78.6e12}
HBM = 8e12

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1536)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--nrhs", default="1,8,32,64")
ap.add_argument("--dtype", default="f32")
ap.add_argument("--which", type=int, default=0)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_multi_solve.py needs a HIP device"
assert args.which == 0, "the single-vector yardstick is thx_chol_solve: which = 0"
K = default_kernels()
n, ld, B = args.n, round_up(args.n, 32), args.batch
dt = {"f32": torch.float32, "f64": torch.float64}[args.dtype]
esize = 4 if dt == torch.float32 else 8


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


gen = torch.Generator(device="cuda").manual_seed(0)
H = torch.empty(B, ld, ld, dtype=dt, device="cuda")
H.uniform_(-1, 1, generator=gen)
H.diagonal(dim1=1, dim2=2).add_(float(n))      # strictly diagonally dominant: SPD from the lower triangle
L = torch.zeros_like(H)
nt = (n + 127) // 128
panels = torch.empty(B, nt, 128, 128, dtype=dt, device="cuda")
info = torch.empty(B, dtype=torch.int32, device="cuda")
K.chol_factor(H, n, None, False, 1e-8, L, panels, info)
torch.cuda.synchronize()
assert int(info.abs().sum()) == 0
del H

lines = []
for nrhs in (int(v) for v in args.nrhs.split(",")):
    rhs = torch.randn(B, nrhs, n, dtype=dt, device="cuda", generator=gen)
    x = torch.empty_like(rhs)
    cols = [rhs[:, s].contiguous() for s in range(nrhs)]
    xs = [torch.empty_like(c) for c in cols]

    def multi():
        K.chol_solve_multi(L, n, panels, rhs, x, which=0)

    def loop():
        for c, o in zip(cols, xs):
            K.chol_solve(L, n, panels, c, o)

    contenders = dict(multi=multi, loop=loop)
    for fn in contenders.values():     # warm-up
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in contenders}
    for _ in range(args.rounds):
        for k, fn in contenders.items():
            times[k].append(event_ms(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    agree = float((x - torch.stack(xs, dim=1)).abs().max() / x.abs().max())
    groups = (nrhs + 31) // 32
    tiles = nt * (nt + 1) // 2                                  # tiles of the lower triangle (diagonal ones through the panels)
    l_bytes = 2.0 * B * groups * tiles * 128 * 128 * esize      # forward + backward
    flops = 2.0 * B * groups * 32 * 2.0 * tiles * 128 * 128     # what the matrix cores execute (a partial group is padded to 32)
    line = dict(n=n, B=B, dtype=args.dtype, nrhs=nrhs, rounds=args.rounds,
                ms={k: [round(t, 3) for t in v] for k, v in times.items()}, ms_median={k: round(v, 3) for k, v in med.items()},
                loop_over_multi=round(med["loop"] / med["multi"], 2), multi_vs_loop_max_rel=agree,
                L_TB_per_s=round(l_bytes / (med["multi"] * 1e-3) / 1e12, 3), L_fraction_of_hbm_peak=round(l_bytes / (med["multi"] * 1e-3) / HBM, 4),
                mfma_fraction=round(flops / (med["multi"] * 1e-3) / PEAK[args.dtype], 4))
    print(json.dumps(line), flush=True)
    lines.append(line)
    del rhs, x, cols, xs
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
