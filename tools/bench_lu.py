"""Micro-benchmark of thx_lu_factor + thx_lu_solve on random SPD batches (HIP events on torch's current stream), beside
torch.linalg.lu_factor + lu_solve on the same device (what the reference's LUDenseSolver executes on a GPU) and the HIP
Cholesky on the same inputs (half the flops).  Three interleaved rounds per contender after one warm-up call each.

usage: python tools/bench_lu.py [--n 1536] [--batches 8,256,4096] [--dtypes f32,f64] [--rounds 3] [--out FILE]
Prints one JSON line per (batch, dtype)."""
import argparse
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from theseus_amd.kernels import default_kernels, round_up

# MI355X matrix-core peaks (TFLOP/s): v_mfma_f32_32x32x2_f32 157.3, v_mfma_f64_16x16x4_f64 78.6
PEAK = {"f32": 157.3e12, "f64": 78.6e12}

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1536)
ap.add_argument("--batches", default="8,256,4096")
ap.add_argument("--dtypes", default="f32,f64")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--no-torch", action="store_true", help="skip torch.linalg.lu_factor / lu_solve")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_lu.py needs a HIP device"
K = default_kernels()
n, ld = args.n, round_up(args.n, 32)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run(B, tag):
    dt = {"f32": torch.float32, "f64": torch.float64}[tag]
    gen = torch.Generator(device="cuda").manual_seed(0)
    H = torch.empty(B, ld, ld, dtype=dt, device="cuda")
    H.uniform_(-1, 1, generator=gen)
    H.diagonal(dim1=1, dim2=2).add_(float(n))      # strictly diagonally dominant: SPD from the lower triangle
    rhs = torch.randn(B, n, dtype=dt, device="cuda", generator=gen)
    lam = torch.full((B,), 1e-3, dtype=dt, device="cuda")
    out = torch.empty_like(H)                      # the LU frame and the Cholesky's L in turn (one buffer: memory at B = 4096)
    piv = torch.empty(B, n, dtype=torch.int32, device="cuda")
    info = torch.empty(B, dtype=torch.int32, device="cuda")
    panels = torch.empty(B, (n + 127) // 128, 128, 128, dtype=dt, device="cuda")
    x = torch.empty_like(rhs)
    res = {}

    def hip_lu():
        K.lu_factor(H, n, lam, False, 1e-8, out, piv, info)
        K.lu_solve(out, n, piv, rhs, x)

    def hip_lu_factor_only():
        K.lu_factor(H, n, lam, False, 1e-8, out, piv, info)

    def hip_chol():
        K.chol_factor(H, n, lam, False, 1e-8, out, panels, info)
        K.chol_solve(out, n, panels, rhs, x)

    def torch_lu():
        # the reference's path: AtA is a full symmetric matrix there; the copy that adds the damping is part of its solve too
        M = H[:, :n, :n] + 1e-3 * torch.eye(n, dtype=dt, device="cuda")
        LUt, pt = torch.linalg.lu_factor(M)
        res["x_torch"] = torch.linalg.lu_solve(LUt, pt, rhs.unsqueeze(2)).squeeze(2)

    contenders = {"hip_lu": hip_lu, "hip_lu_factor": hip_lu_factor_only, "hip_chol": hip_chol}
    if not args.no_torch:
        # (torch factorises the full matrix: give it the symmetric one the HIP solvers see)
        Hs = torch.tril(H[:, :n, :n])
        H[:, :n, :n] = Hs + torch.tril(Hs, -1).transpose(1, 2)
        del Hs
        contenders["torch_lu"] = torch_lu
    times = {k: [] for k in contenders}
    skipped = {}
    for k, fn in list(contenders.items()):        # warm-up
        try:
            fn()
            torch.cuda.synchronize()
        except torch.OutOfMemoryError as e:
            skipped[k] = "out of memory"
            del contenders[k], times[k]
            torch.cuda.empty_cache()
    for _ in range(args.rounds):
        for k, fn in contenders.items():
            times[k].append(event_ms(fn))
    hip_lu()
    torch.cuda.synchronize()
    assert int(info.abs().sum()) == 0
    Hd = torch.tril(H[:2, :n, :n]).double()
    Hd = Hd + torch.tril(Hd, -1).transpose(1, 2) + 1e-3 * torch.eye(n, dtype=torch.float64, device="cuda")
    resid = float(((Hd @ x[:2].double().unsqueeze(2)).squeeze(2) - rhs[:2].double()).abs().max())
    flops = B * 2.0 * n ** 3 / 3
    line = dict(n=n, B=B, dtype=tag, rounds=args.rounds, ms={k: [round(t, 3) for t in v] for k, v in times.items()},
                ms_min={k: round(min(v), 3) for k, v in times.items()}, skipped=skipped, solve_residual_hip_lu=resid,
                hip_lu_factor_tflops=round(flops / min(times["hip_lu_factor"]) / 1e9, 2),
                hip_lu_factor_fraction_of_mfma_peak=round(flops / (min(times["hip_lu_factor"]) * 1e-3) / PEAK[tag], 4))
    if "x_torch" in res:
        line["x_vs_torch_max_rel"] = float((x - res["x_torch"]).abs().max() / res["x_torch"].abs().max())
    return line


lines = []
for tag in args.dtypes.split(","):
    for B in (int(b) for b in args.batches.split(",")):
        line = run(B, tag)
        torch.cuda.empty_cache()
        print(json.dumps(line), flush=True)
        lines.append(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
