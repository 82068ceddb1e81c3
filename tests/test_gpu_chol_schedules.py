"""-m gpu: every schedule of the dense factorisation against fp64 LAPACK, with the path each call takes asserted through thx_chol_plan
(include/theseus_hip.h) -- so that a later change of a default cannot turn a schedule test into a comparison of a path with itself.

  * the right-looking schedule in all three launch arrangements (thx_chol_schedule.right_looking_mode 0 / 1 / 2) x fp32 / fp64, at
    the frames the product allocates (ld = round_up(n, 32): partial last tiles), ld beyond whole tiles, 1 ... 40 problems, no /
    scalar / ellipsoidal damping, forward substitution fused, as its own kernel (vector rows not 16-byte multiples) or not asked for;
  * failure reporting: info is LAPACK's (torch.linalg.cholesky_ex of the damped fp64 matrix) for a non-positive pivot in block
    column 0, 1, a late one, the partial last tile, and a NaN off the diagonal -- and the other problems of the batch keep their bits;
  * stale and poisoned buffers: the LM reuses L across iterations and allocates the panels / vectors with torch.empty -- a factor
    must not depend on what they held;
  * the dynamic-LDS limits, which the library raises kernel by kernel where it launches: one process in which every limit has to
    grow from call to call (a child process, so that no earlier test has raised them)."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def _kernels(**fields):
    """A kernels object of its own, with these thx_chol_schedule fields (the others: the library defaults)."""
    from theseus_amd.kernels import HipKernels
    K = HipKernels()
    for k, v in fields.items():
        setattr(K.chol_schedule, k, v)
    return K


def _spd(B, n, dtype, seed, cond=1e3):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.randn(B, n, n + 8, dtype=F64, device="cuda", generator=gen)
    M = A @ A.transpose(1, 2) / (n + 8) + (1.0 / cond) * torch.eye(n, dtype=F64, device="cuda")
    return M.to(dtype)


def _frame(M, ld):
    B, n = M.shape[0], M.shape[1]
    H = torch.zeros(B, ld, ld, dtype=M.dtype, device="cuda")
    H[:, :n, :n] = torch.tril(M)
    return H


def _vec(B, n, ldv, dtype, fill=0.0):
    return torch.full((B, ldv), fill, dtype=dtype, device="cuda")[:, :n]


def _damped(M, lam, ellipsoidal, eps):
    """H + D in fp64, as the factorisation sees it (dense_solver.py:_apply_damping)."""
    Md = M.double()
    if lam is None:
        return Md
    dg = torch.diagonal(Md, dim1=1, dim2=2)
    D = lam.double().view(-1, 1) * dg + eps if ellipsoidal else lam.double().view(-1, 1).expand_as(dg)
    return Md + torch.diag_embed(D)


def _factor(K, H, n, rhs, lam, ellipsoidal, eps, fwd, bufs=None):
    """One factorisation + solve with the caller's buffers (bufs: L, panels, y, x, info) or fresh zeroed ones.
    fwd: "rhs" (thx_chol_factor_forward + thx_chol_solve_backward) or "none" (thx_chol_factor + thx_chol_solve)."""
    B, ld = H.shape[0], H.shape[-1]
    nt = (n + 127) // 128
    ldv = rhs.stride(0)
    if bufs is None:
        bufs = (torch.zeros_like(H), torch.zeros(B, nt, 128, 128, dtype=H.dtype, device="cuda"), _vec(B, n, ldv, H.dtype),
                _vec(B, n, ldv, H.dtype), torch.zeros(B, dtype=torch.int32, device="cuda"))
    L, panels, y, x, info = bufs
    if fwd == "none":
        K.chol_factor(H, n, lam, ellipsoidal, eps, L, panels, info)
        K.chol_solve(L, n, panels, rhs, x)
    else:
        K.chol_factor(H, n, lam, ellipsoidal, eps, L, panels, info, rhs=rhs, y=y)
        K.chol_solve_backward(L, n, panels, y, x)
    torch.cuda.synchronize()
    return bufs


def _assert_plan(K, n, ld, B, dtype, lam, fwd, ldv, **expect):
    p = K.chol_plan(n, ld, B, dtype, damping=lam is not None, rhs=fwd != "none", ldv=ldv)
    for k, v in expect.items():
        assert p[k] == v, (k, p)
    return p


def _panel_mask(n, nt, dtype):
    """The panel elements a factorisation writes: the ten lower 32 x 32 sub-blocks of every tile, rows / columns inside the matrix."""
    m = torch.zeros(nt, 128, 128, dtype=torch.bool, device="cuda")
    for t in range(nt):
        v = min(128, n - 128 * t)
        for u in range(4):
            for w in range(u + 1):
                m[t, 32 * u:min(32 * u + 32, v), 32 * w:min(32 * w + 32, v)] = True
    return m


# ---- right-looking schedule: modes x dtypes x product layouts ----------------------------------------------------------------------
# (n, ld, B, damping, forward substitution); each row runs modes 0, 1, 2 and the left-looking schedule on the same inputs.
#   384 / 384: three tiles, RL's minimum;  366 / 384 and 1530 / 1536: the product's frames with a partial last tile;  1536: full
#   tiles;  1290 / 1408: a second frame wider than round_up(n, 32);  384 / 416: ld beyond whole tiles.  "rhs": the forward
#   substitution asked for -- vectors are (B, n) contiguous (the product's g), so it rides on the schedule for n % 4 == 0 (384,
#   1536) and runs as its own kernel for rows that are not 16-byte multiples (366, 1530, 1290: FACTOR_NEEDS_FORWARD); "none":
#   factor, then thx_chol_solve.
RL_CASES = {
    F32: [(384, 384, 1, None, "rhs"), (366, 384, 29, "scalar", "rhs"), (1530, 1536, 8, "ellipsoidal", "none"),
          (1536, 1536, 40, "scalar", "rhs"), (1290, 1408, 3, "ellipsoidal", "rhs"), (384, 416, 8, None, "none")],
    F64: [(384, 384, 40, "ellipsoidal", "rhs"), (366, 384, 3, None, "none"), (1530, 1536, 29, "scalar", "rhs"),
          (1536, 1536, 1, "ellipsoidal", "rhs"), (1290, 1408, 8, None, "rhs"), (384, 416, 29, "scalar", "none")],
}


@pytest.mark.parametrize("case", range(6))
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_right_looking_modes_vs_lapack(dtype, case):
    n, ld, B, damping, fwd = RL_CASES[dtype][case]
    f32 = dtype == F32
    eps = 1e-6
    M = _spd(B, n, dtype, seed=7 * n + B)
    H = _frame(M, ld)
    ldv = n
    rhs = _vec(B, n, ldv, dtype)
    rhs.copy_(torch.randn(B, n, dtype=F64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(B)).to(dtype))
    lam = None if damping is None else torch.linspace(0.02, 0.3, B, dtype=F64, device="cuda").to(dtype)
    ell = damping == "ellipsoidal"
    out = {}
    for mode in (0, 1, 2, "ll"):
        K = _kernels(right_looking_max_batch=0 if mode == "ll" else 64, right_looking_mode=-1 if mode == "ll" else mode,
                     column_pairs=0)
        if mode == "ll":
            _assert_plan(K, n, ld, B, dtype, lam, fwd, ldv, right_looking=0, column_pairs=0, split_diag=0)
        else:
            _assert_plan(K, n, ld, B, dtype, lam, fwd, ldv, right_looking=1, right_looking_mode=mode, split_diag=0,
                         forward_fused=int(fwd != "none" and n % 4 == 0))
        Hc = H.clone()
        L, panels, y, x, info = _factor(K, H, n, rhs, lam, ell, eps, fwd)
        assert torch.equal(H, Hc)                                          # (H is read only)
        assert int(info.abs().sum()) == 0, (mode, info)
        assert float(torch.triu(L, 1).abs().max()) == 0.0, mode           # (the upper triangle of the frame stays zero)
        out[mode] = (L[:, :n, :n], x.clone())
    Hd = _damped(M, lam, ell, eps)
    tol_L, tol_x = (2e-5, 2e-3) if f32 else (1e-13, 1e-10)
    sample = sorted({0, B // 2, B - 1})
    Lref = torch.linalg.cholesky(Hd[sample].cpu())                         # (LAPACK, fp64, on the host)
    xref = torch.cholesky_solve(rhs[sample].double().cpu().unsqueeze(2), Lref).squeeze(2)
    scale, xscale = float(Lref.abs().max()), float(xref.abs().max())
    res = lambda x: float(((Hd @ x.double().unsqueeze(2)).squeeze(2) - rhs.double()).abs().max() / rhs.abs().max())  # noqa: E731
    Ll, xl = out["ll"]
    for mode in (0, 1, 2, "ll"):
        Lm, xm = out[mode]
        assert float((Lm[sample].double().cpu() - Lref).abs().max()) / scale < tol_L, mode
        assert float((xm[sample].double().cpu() - xref).abs().max()) / xscale < tol_x, mode
        assert float((Lm - Ll).abs().max()) / scale < tol_L, mode
        assert float((xm - xl).abs().max()) / xscale < tol_x, mode
        assert res(xm) < 2.0 * res(xl) + (1e-6 if f32 else 1e-14), mode
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert float((out[a][0] - out[b][0]).abs().max()) / scale < tol_L, (a, b)
        assert float((out[a][1] - out[b][1]).abs().max()) / xscale < tol_x, (a, b)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", ["pg_full_f32_lm", "pg_full_f64_lm"])
def test_right_looking_modes_from_blocks(name, mode):
    """thx_chol_factor_hblocks in each right-looking mode (mode 1: block column 1's diagonal tile and substitutions straight from
    the block list, the damping pass from 2 * TILE on): L, panels, y bit-identical to the dense frame in the same mode, and within
    the bounds of LAPACK."""
    from tests.test_gpu_block_hessian import _assembled
    K = _kernels(right_looking_max_batch=64, right_looking_mode=mode)
    s, hb, dhb, H, gv, Hc, g2, n, ld = _assembled(K, name)
    B, dtype = H.shape[0], H.dtype
    nt = (n + 127) // 128
    lam = torch.full((B,), 1e-3, dtype=dtype, device="cuda")
    for layout in (None, dhb.c):
        p = K.chol_plan(n, ld, B, dtype, damping=True, rhs=True, ldv=gv.stride(0), layout=layout)
        assert p["right_looking"] == 1 and p["right_looking_mode"] == mode, p
    out = []
    for compact in (False, True):
        L = torch.zeros_like(H)
        panels = torch.zeros(B, nt, 128, 128, dtype=dtype, device="cuda")
        info = torch.empty(B, dtype=torch.int32, device="cuda")
        y = torch.empty_like(gv)
        if compact:
            K.chol_factor_hblocks(dhb, Hc, n, lam, True, 1e-8, L, panels, info, rhs=gv, y=y)
        else:
            K.chol_factor(H, n, lam, True, 1e-8, L, panels, info, rhs=gv, y=y)
        out.append((torch.tril(L[:, :n, :n]), panels, y, info))
    (La, Pa, ya, ia), (Lb, Pb, yb, ib) = out
    assert int(ia.abs().sum()) == 0 and int(ib.abs().sum()) == 0
    assert torch.equal(La, Lb) and torch.equal(ya, yb)
    mask = _panel_mask(n, nt, dtype).expand_as(Pa)
    assert torch.equal(Pa[mask], Pb[mask])
    # against LAPACK (fp64, on the host) with the bounds of tests/test_gpu_kernels.py:_chol_vs_lapack -- the backward error of the
    # factorisation, which does not depend on the conditioning of a pose graph's Hessian; y through its residual in L
    Hd = _damped(torch.tril(H[:, :n, :n]) + torch.tril(H[:, :n, :n], -1).transpose(1, 2), lam, True, 1e-8).cpu()
    assert int(torch.linalg.cholesky_ex(Hd).info.abs().sum()) == 0
    eps = 1.2e-7 if dtype == F32 else 2.3e-16
    Lg = La.double().cpu()
    resid = float((Lg @ Lg.transpose(1, 2) - Hd).abs().max() / Hd.abs().max())
    assert resid < 60 * eps * max(1, n / 64), resid
    ry = (Lg @ ya.double().cpu().unsqueeze(2)).squeeze(2) - gv.double().cpu()
    assert float(ry.abs().max() / (Lg.abs().max() * ya.double().abs().max())) < 60 * eps * max(1, n / 64)


# ---- every schedule: failure reporting and stale buffers ---------------------------------------------------------------------------
# (name, dtype, thx_chol_schedule fields, expected plan)
SCHEDULES = [
    ("ll", F32, dict(right_looking_max_batch=0, column_pairs=0), dict(right_looking=0, column_pairs=0, split_diag=0)),
    ("ll_split", F32, dict(split_diag_min_batch=0, column_pairs=0), dict(right_looking=0, column_pairs=0, split_diag=1)),
    ("pairs", F32, dict(right_looking_max_batch=0, column_pairs=1, column_pairs_min_batch=0),
     dict(right_looking=0, column_pairs=1, split_diag=0)),
    ("rl0", F32, dict(right_looking_max_batch=64, right_looking_mode=0), dict(right_looking=1, right_looking_mode=0)),
    ("rl1", F32, dict(right_looking_max_batch=64, right_looking_mode=1), dict(right_looking=1, right_looking_mode=1)),
    ("rl2", F32, dict(right_looking_max_batch=64, right_looking_mode=2), dict(right_looking=1, right_looking_mode=2)),
    ("ll", F64, dict(right_looking_max_batch=0), dict(right_looking=0, split_diag=0, f64_half_cols=4)),
    ("ll_split", F64, dict(split_diag_min_batch=0), dict(right_looking=0, split_diag=1, f64_half_cols=4)),
    ("ll_wide", F64, dict(right_looking_max_batch=0, f64_half_max_ktiles=0), dict(right_looking=0, f64_half_cols=0, f64_wide_cols=4)),
    ("rl0", F64, dict(right_looking_max_batch=64, right_looking_mode=0), dict(right_looking=1, right_looking_mode=0)),
    ("rl1", F64, dict(right_looking_max_batch=64, right_looking_mode=1), dict(right_looking=1, right_looking_mode=1)),
    ("rl2", F64, dict(right_looking_max_batch=64, right_looking_mode=2), dict(right_looking=1, right_looking_mode=2)),
]
SCHED_IDS = [f"{name}-{'f32' if dt == F32 else 'f64'}" for name, dt, _, _ in SCHEDULES]
# n = 620 in the product's frame (ld = 640 = five whole tiles): rows 512 ... 619 are the partial last tile
N_FAIL, LD_FAIL, B_FAIL, BAD = 620, 640, 5, 2
# where problem BAD breaks: a non-positive pivot in block column 0, 1 (mode 1's path straight from H), 3, the partial last tile --
# or a NaN off the diagonal (row 250 in block column 1, column 40 in block column 0)
BREAKS = [("col0", 50, 50, -5.0), ("col1", 200, 200, -5.0), ("late", 400, 400, -5.0), ("partial", 600, 600, -5.0),
          ("nan", 250, 40, float("nan"))]


@pytest.mark.parametrize("sched", range(len(SCHEDULES)), ids=SCHED_IDS)
def test_failure_is_reported_as_lapack_does(sched):
    name, dtype, fields, expect = SCHEDULES[sched]
    n, ld, B = N_FAIL, LD_FAIL, B_FAIL
    K = _kernels(**fields)
    lam = torch.full((B,), 1e-2, dtype=dtype, device="cuda")
    rhs = _vec(B, n, n, dtype)
    rhs.copy_(torch.randn(B, n, dtype=F64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)).to(dtype))
    _assert_plan(K, n, ld, B, dtype, lam, "rhs", n, **expect)
    M = _spd(B, n, dtype, seed=11)
    L0, _, y0, x0, i0 = _factor(K, _frame(M, ld), n, rhs, lam, False, 1e-8, "rhs")
    assert int(i0.abs().sum()) == 0
    keep = [b for b in range(B) if b != BAD]
    for where, r, c, v in BREAKS:
        Mb = M.clone()
        Mb[BAD, r, c] = v
        L, _, y, x, info = _factor(K, _frame(Mb, ld), n, rhs, lam, False, 1e-8, "rhs")
        expect_info = torch.linalg.cholesky_ex(_damped(Mb, lam, False, 1e-8).cpu()).info
        assert info.cpu().tolist() == expect_info.tolist(), (where, info.tolist(), expect_info.tolist())
        assert int(expect_info[BAD]) == r + 1
        assert torch.equal(torch.tril(L[keep, :n, :n]), torch.tril(L0[keep, :n, :n])), where
        assert torch.equal(y[keep], y0[keep]) and torch.equal(x[keep], x0[keep]), where


@pytest.mark.parametrize("sched", range(len(SCHEDULES)), ids=SCHED_IDS)
def test_factor_does_not_depend_on_stale_buffers(sched):
    """The LM's buffer life cycle (linear_solver.py, ba.py, sparse.py): L zeroed once and reused by every iteration and trial step,
    panels and vectors from torch.empty.  Factor A, then -- without re-zeroing L, panels, y, x filled with NaN -- factor B into the
    same buffers: the lower triangle of L, the panels the factorisation writes, y and x must be bit-identical to B on fresh zeroed
    buffers."""
    name, dtype, fields, expect = SCHEDULES[sched]
    n, ld, B = N_FAIL, LD_FAIL, B_FAIL
    nt = (n + 127) // 128
    K = _kernels(**fields)
    _assert_plan(K, n, ld, B, dtype, torch.ones(1), "rhs", n, **expect)
    rhs = _vec(B, n, n, dtype)
    rhs.copy_(torch.randn(B, n, dtype=F64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4)).to(dtype))
    HA, HB = _frame(_spd(B, n, dtype, seed=21, cond=1e2), ld), _frame(_spd(B, n, dtype, seed=22), ld)
    lamA = torch.full((B,), 0.5, dtype=dtype, device="cuda")
    lamB = torch.linspace(1e-3, 1e-1, B, dtype=F64, device="cuda").to(dtype)
    fresh = _factor(K, HB, n, rhs, lamB, True, 1e-8, "rhs")
    bufs = _factor(K, HA, n, rhs, lamA, False, 1e-8, "rhs")
    L, panels, y, x, info = bufs
    panels.fill_(float("nan"))
    y.fill_(float("nan"))
    x.fill_(float("nan"))
    info.fill_(-7)
    stale = _factor(K, HB, n, rhs, lamB, True, 1e-8, "rhs", bufs=bufs)
    (Lf, Pf, yf, xf, inf_), (Ls, Ps, ys, xs, ins) = fresh, stale
    assert int(inf_.abs().sum()) == 0 and torch.equal(inf_, ins)
    assert torch.equal(torch.tril(Lf[:, :n, :n]), torch.tril(Ls[:, :n, :n]))
    mask = _panel_mask(n, nt, dtype).expand_as(Pf)
    assert torch.equal(Pf[mask], Ps[mask])
    assert torch.equal(yf, ys) and torch.equal(xf, xs)
    assert not torch.isnan(xs).any()


# ---- dynamic-LDS limits that must grow within one process --------------------------------------------------------------------------
# The library raises a kernel's dynamic-LDS limit next to its launch and remembers per kernel how far.  The diagonal phase's LDS
# grows with n when the forward substitution is fused (its y buffer), the solves' with n (the whole vector): n = 128, 384, 640 in
# this order make every later call need more than any call before it.  B = 2: left-looking at one tile, right-looking from three
# tiles on (the dense-frame chol_diag instance, block rows in the backward substitution); B = 160: left-looking, in column pairs
# in fp32, the one-workgroup solves; then 384 x 8, right-looking again after the larger left-looking calls.
GROW_STEPS = [(128, 2), (384, 2), (640, 2), (128, 160), (384, 160), (640, 160), (384, 8)]


def _growing_limits_child():
    from theseus_amd.kernels import HipKernels
    K = HipKernels()
    for dtype in (F64, F32):
        f32 = dtype == F32
        tol_L, tol_x = (2e-5, 2e-3) if f32 else (1e-13, 1e-10)      # (as test_right_looking_modes_vs_lapack)
        for n, B in GROW_STEPS:
            ld = n
            p = K.chol_plan(n, ld, B, dtype, damping=False, rhs=True, ldv=n)
            assert p["right_looking"] == int(n >= 384 and B <= 8), (n, B, p)
            assert p["column_pairs"] == int(f32 and B == 160), (n, B, p)
            M = _spd(B, n, dtype, seed=13 * n + B)
            H = _frame(M, ld)
            rhs = _vec(B, n, n, dtype)
            rhs.copy_(torch.randn(B, n, dtype=F64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(n + B)).to(dtype))
            L, panels, y, x, info = (torch.zeros_like(H), torch.zeros(B, (n + 127) // 128, 128, 128, dtype=dtype, device="cuda"),
                                     _vec(B, n, n, dtype), _vec(B, n, n, dtype), torch.zeros(B, dtype=torch.int32, device="cuda"))
            x2 = _vec(B, n, n, dtype)
            K.chol_factor(H, n, None, False, 0.0, L, panels, info, rhs=rhs, y=y)      # thx_chol_factor_forward
            K.chol_solve(L, n, panels, rhs, x)                                        # thx_chol_solve
            K.chol_solve_backward(L, n, panels, y, x2)                                # (y, through the backward substitution)
            torch.cuda.synchronize()
            assert int(info.abs().sum()) == 0, (n, B, info)
            sample = sorted({0, B // 2, B - 1})
            Lref = torch.linalg.cholesky(M[sample].double().cpu())                    # (LAPACK, fp64, on the host)
            xref = torch.cholesky_solve(rhs[sample].double().cpu().unsqueeze(2), Lref).squeeze(2)
            eL = float((torch.tril(L[sample, :n, :n]).double().cpu() - Lref).abs().max() / Lref.abs().max())
            ex = float((x[sample].double().cpu() - xref).abs().max() / xref.abs().max())
            ey = float((x2[sample].double().cpu() - xref).abs().max() / xref.abs().max())
            print(f"{'f32' if f32 else 'f64'} n={n} B={B}: L {eL:.3e} (< {tol_L}), x {ex:.3e}, x from y {ey:.3e} (< {tol_x})", flush=True)
            assert eL < tol_L and ex < tol_x and ey < tol_x, (n, B, eL, ex, ey)
    print("GROWING-LIMITS-OK")


def test_lds_limits_grow_within_a_process():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "tests.test_gpu_chol_schedules"], cwd=root, env=env, capture_output=True, text=True,
                         timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "GROWING-LIMITS-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


if __name__ == "__main__":
    _growing_limits_child()
