"""Time the three banded-Cholesky entry points one by one (events around 50 calls each): n = 404 and 4004 at kd = 7, n = 404 at
kd = 63, batch 64 and 1024, fp32 and fp64.  One line per case: us per call and ns per column.  python tools/microbench/band_kernels.py"""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from theseus_amd.kernels import default_kernels
K = default_kernels()
def timed(fn, reps=50):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3
for dt in (torch.float32, torch.float64):
    for n, kd, B in ((404, 7, 64), (404, 7, 1024), (404, 63, 64), (4004, 7, 64)):
        ld = (n + 31) // 32 * 32
        H = torch.zeros(B, ld, ld, dtype=dt, device="cuda")
        i = torch.arange(n, device="cuda")
        H[:, i, i] = 4.0
        for o in range(1, kd + 1):
            H[:, i[o:], i[:-o]] = -0.4 / kd
        perm = torch.arange(n, dtype=torch.int32, device="cuda")
        Lb = torch.empty(B, n, kd + 1, dtype=dt, device="cuda"); info = torch.empty(B, dtype=torch.int32, device="cuda")
        g = torch.randn(B, n, dtype=dt, device="cuda"); y = torch.empty_like(g); x = torch.empty_like(g)
        t = dict(factor=timed(lambda: K.band_factor(H, n, kd, perm, None, False, 1e-8, Lb, info)),
                 factor_fwd=timed(lambda: K.band_factor(H, n, kd, perm, None, False, 1e-8, Lb, info, rhs=g, y=y)),
                 backward=timed(lambda: K.band_solve_backward(Lb, n, kd, perm, y, x)),
                 solve=timed(lambda: K.band_solve(Lb, n, kd, perm, g, x)))
        assert int(info.ne(0).sum()) == 0
        print(str(dt), "n", n, "kd", kd, "B", B, " ".join(f"{k} {v:.1f} us ({v / n * 1e3:.0f} ns/col)" for k, v in t.items()), flush=True)
