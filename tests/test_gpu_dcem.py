"""-m gpu: DCEM on the kernels (csrc/dcem_kernels.hip: thx_dcem_update, thx_dcem_update_vjp; theseus_amd/dcem.py) against the REAL
reference's fixtures (tests/golden/dcem_f64_*.npz) and against the torch twin ``dcem_update_torch``.  CPU twin of this file:
tests/test_dcem_host.py.

Bounds.
  fp64   REL = 1e-12 of the compared tensor's largest magnitude (the bar of the family tests, tests/test_gpu_traj2.py): the kernel and
         the twin take the same bracket decisions as long as no grid value of an LML round lies within 1e-9 of zero -- such a case
         is skipped, and the test fails if more than 2 % are.
  fp32   LML mode: a bracket decision may differ.  Both final brackets contain the root nu* of sum sigmoid(x + nu) = N and are at
         most lml_eps wide, so with the fp64 twin on the same (fp32) inputs as the truth:  |nu - nu_ref| <= lml_eps,
         |w_i - w_ref_i| <= lml_eps / 4 (the sigmoid's slope),  |mu_j - mu_ref_j| <= sum_i |X_ij| lml_eps / (4 N), each plus fp32
         rounding: of the scores (the standardisation is rounded to fp32 once: the root moves by as much, RND_X below) and of the
         sums (RND_SUM ulps of sum |terms|).  sigma: from v = sigma^2 = sum w d^2 / N:  |dv| <= sum_i d_ij^2 (lml_eps / 4) / N +
         2 |mu_j| |1 - W / N| |dmu_j| and |dsigma| = |dv| / (sigma + sigma_ref).
         softmax / hard mode: no bracket; per case and per output (mu, sigma, w), the kernel's largest deviation from the fp64 twin
         is at most twice the fp32 TWIN's own, plus half an fp32 ulp of the output's largest magnitude (eps32 / 2 relative): what
         rounding the output to fp32 costs at the least, so that a twin which happens to land on the rounded value (deviation 0,
         or a small fraction of an ulp when the output is ONE number) does not ask for more than fp32 can hold.  The worst
         deviations over all cases and the largest share of a single bound are printed.
  vjp    fp64, against the twin's autograd: 1e-10 of the gradient's largest entry -- fp64 rounding (1.1e-16) accumulated over at
         most S * n = 1.3e5 terms of either sign is 1.5e-11 in the worst case; the twin itself is no more exact than that.
No test here reads the reference tree."""
import itertools
import math

import numpy as np
import pytest
import torch

from tests import dcem_common as dc
from tests.helpers import load_golden
from tests.homog_common import build as homog_build, kernel_problem
from tests.kin_common import build as kin_build

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL = 1e-12
EPS32 = float(np.finfo(np.float32).eps)
LML_EPS = 1e-3
SKIP_MARGIN = 1e-9


def _t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def kernel_update(fX, X, n_elite, temp, normalize=True, lml_eps=LML_EPS, branch=100):
    import theseus_amd as th
    return th.DcemUpdate.apply(fX, X, th.default_kernels(), n_elite, temp, normalize, lml_eps, 100, branch, None)


def rel_dev(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


# ---- the update against the fixtures ---------------------------------------------------------------------------------------------
def test_update_reproduces_every_recorded_iteration_and_mode():
    g = dc.load("dcem_f64_soft")
    worst = 0.0
    mu, sigma = _t(g["x0"]), torch.ones(dc.B, dc.N_DOF, dtype=torch.float64, device=DEV)
    for it in range(dc.N_ITER):
        X = dc.samples(mu, sigma, _t(g["noise"][it]))
        m, s, w, nu, bracket, flags = kernel_update(_t(g["fX"][it]).t().contiguous(), X, dc.N_ELITE, 1.0, branch=dc.BRANCH)
        for got, key in ((w, "w"), (m, "mu"), (s, "sigma")):
            worst = max(worst, rel_dev(got, _t(g[key][it])))
        assert not flags.any() and bool(((bracket[:, 1] - bracket[:, 0]) <= LML_EPS).all())
        mu, sigma = _t(g["mu"][it]), _t(g["sigma"][it])
    print(f"soft fixture, 6 iterations: worst deviation {worst:.3e} of the largest magnitude (allowed {REL:.0e})")
    assert worst <= REL
    g = dc.load("dcem_f64_modes")
    for mode, (extra, S) in dc.MODES.items():
        X = dc.samples(_t(g["x0"]), 1.0, _t(g[f"{mode}_noise"][0]))
        m, s, w, _, _, flags = kernel_update(_t(g[f"{mode}_fX"]).t().contiguous(), X, extra.get("n_elite", dc.N_ELITE),
                                             extra.get("temp", 1.0), extra.get("normalize", True), branch=dc.BRANCH)
        dev = max(rel_dev(w, _t(g[f"{mode}_w"])), rel_dev(m, _t(g[f"{mode}_mu"])), rel_dev(s, _t(g[f"{mode}_sigma"])))
        print(f"mode {mode}: worst deviation {dev:.3e} (allowed {REL:.0e})")
        assert dev <= REL and not flags.any(), mode


# ---- the update against the twin on random inputs --------------------------------------------------------------------------------
def random_cases():
    """(B, S, n, n_elite, branch, temp, normalize): every (B, kind of S, n) with three of the 36 settings each, dealt round robin --
    every setting meets six shapes; and three cases wider than one chunk of columns"""
    settings = list(itertools.product((1, 2, 5), (10, 100), (1.0, 0.3, None), (True, False)))
    shapes = list(itertools.product((1, 3, 70), ("N+1", 40, 100, 257, 1024, "<=N"), (1, 4, 33, 130)))
    cases = []
    for c, (B, S, n) in enumerate(shapes):
        for j in range(3):
            N, branch, temp, normalize = settings[(3 * c + j) % len(settings)]
            s = N + 1 if S == "N+1" else (N if S == "<=N" else S)
            cases.append((B, s, n, N, branch, temp, normalize))
    # past 256 columns the kernels take the columns in chunks
    return cases + [(3, 40, 300, 5, 10, 1.0, True), (3, 40, 300, 2, 100, 0.3, False), (1, 40, 600, 5, 10, None, True)]


def nan_case(case):
    """one sample, standardised: its std is 0 / 0 on either side (torch.std of one element)"""
    return case[1] == 1 and case[6] and case[5] is not None


def random_inputs(case, gen, dtype):
    B, S, n = case[:3]
    fX = (torch.randn(S, B, generator=gen, dtype=torch.float64) * 2.0 + 3.0).abs().to(dtype)
    X = (torch.randn(S, B, n, generator=gen, dtype=torch.float64) * 1.5 + 0.25).to(dtype)
    return fX.to(DEV), X.to(DEV)


def test_update_matches_the_twin_on_random_inputs_f64():
    from theseus_amd.dcem import dcem_update_torch
    gen = torch.Generator().manual_seed(1234)
    cases, skipped, worst = random_cases(), 0, 0.0
    assert {c[3] for c in cases} == {1, 2, 5} and {c[4] for c in cases} == {10, 100} and {c[5] for c in cases} == {1.0, 0.3, None}
    for case in cases:
        B, S, n, N, branch, temp, normalize = case
        fX, X = random_inputs(case, gen, torch.float64)
        want = dcem_update_torch(fX, X, N, temp, normalize, LML_EPS, 100, branch, with_margin=True)
        if float(want[6]) < SKIP_MARGIN:
            skipped += 1
            continue
        got = kernel_update(fX, X, N, temp, normalize, branch=branch)
        again = kernel_update(fX, X, N, temp, normalize, branch=branch)
        if nan_case(case):
            assert all(bool(torch.isnan(t).all()) for t in got[:3] + want[:3]), case
            continue
        for a, b in zip(got, again):
            assert torch.equal(a, b), f"two calls differ: {case}"
        dev = max(rel_dev(got[k], want[k]) for k in (0, 1, 2))
        worst = max(worst, dev)
        assert dev <= REL, f"{case}: {dev:.3e}"
        assert torch.equal(got[5], want[5]) and not got[5].any(), case
        if temp is not None and N > 1 and S > N:
            assert float((got[3] - want[3]).abs().max()) <= REL * max(1.0, float(want[3].abs().max()))
            assert float((got[2].sum(dim=1) - N).abs().max()) <= S * LML_EPS / 8, case
    print(f"fp64, {len(cases)} cases, {skipped} skipped: worst deviation {worst:.3e} (allowed {REL:.0e})")
    assert skipped <= 0.02 * len(cases)


def test_a_round_without_a_negative_grid_value_sets_its_flag():
    """Two scores far above 2046 equal ones, three elites: at the lower end of the first bracket the sum is already
    2 + 2046 sigmoid(-7) = 3.86 > 3.  The kernel and the twin both restart 7 below, say so in the flag word, and still find the root
    sigmoid(nu) = 1 / 2046."""
    import theseus_amd as th
    from theseus_amd.dcem import dcem_update_torch
    S, B, n, N = 2048, 2, 3, 3
    fX = torch.zeros(S, B, dtype=torch.float64, device=DEV)
    fX[5], fX[900] = -100.0, -100.0
    X = torch.randn(S, B, n, generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(DEV)
    want = dcem_update_torch(fX, X, N, 1.0, False, LML_EPS, 100, 10, with_margin=True)
    got = kernel_update(fX, X, N, 1.0, False, branch=10)
    assert float(want[6]) >= SKIP_MARGIN
    assert got[5].tolist() == want[5].tolist() == [th._lib.DCEM_FLAG_ALL_NONNEG] * B
    assert max(rel_dev(got[k], want[k]) for k in (0, 1, 2, 3)) <= REL
    root = math.log(1 / 2046) - math.log(1 - 1 / 2046)
    assert float((got[3] - root).abs().max()) <= LML_EPS / 2 and float((got[2].sum(dim=1) - N).abs().max()) <= S * LML_EPS / 8


def test_update_matches_the_twin_on_random_inputs_f32():
    from theseus_amd.dcem import dcem_update_torch
    gen = torch.Generator().manual_seed(4321)
    RND_X, RND_SUM = 64 * EPS32, 8 * EPS32
    worst_ratio, worst_lml = 0.0, 0.0
    devs = {"mu": (0.0, 0.0), "sigma": (0.0, 0.0), "w": (0.0, 0.0)}   # softmax / hard mode: worst (kernel, fp32 twin) over the cases
    FLOOR, failures = EPS32 / 2, []
    for case in random_cases():
        B, S, n, N, branch, temp, normalize = case
        fX, X = random_inputs(case, gen, torch.float32)
        ref = dcem_update_torch(fX.double(), X.double(), N, temp, normalize, LML_EPS, 100, branch)
        got = kernel_update(fX, X, N, temp, normalize, branch=branch)
        assert all(t.dtype == torch.float32 for t in got[:5]) and not got[5].any(), case
        if nan_case(case):
            assert all(bool(torch.isnan(t).all()) for t in got[:3]), case
            continue
        mu, sigma, w, nu, bracket = (t.double() for t in got[:5])
        lml = temp is not None and N > 1 and S > N
        if not lml:
            twin = dcem_update_torch(fX, X, N, temp, normalize, LML_EPS, 100, branch)
            for k, name in ((0, "mu"), (1, "sigma"), (2, "w")):
                top = float(ref[k].abs().max())
                dev_twin = float((twin[k].double() - ref[k]).abs().max()) / top
                dev = float((got[k].double() - ref[k]).abs().max()) / top
                devs[name] = (max(devs[name][0], dev), max(devs[name][1], dev_twin))
                worst_ratio = max(worst_ratio, dev / (2 * dev_twin + FLOOR))
                if not dev <= 2 * dev_twin + FLOOR:
                    failures.append(f"{case} {name}: kernel {dev:.3e}, fp32 twin {dev_twin:.3e} of the largest magnitude")
            continue
        # the standardised scores in fp64: what both brackets are about
        f = fX.double().t()
        if normalize:
            f = (f - f.mean(dim=1, keepdim=True)) / (f.std(dim=1, keepdim=True) + 1e-6)
        x = -f * temp
        slack = RND_X * (1.0 + float(x.abs().max()))
        lo, hi = bracket[:, 0], bracket[:, 1]
        assert float((hi - lo).max()) <= LML_EPS * (1 + 4 * EPS32), case
        g_lo = torch.sigmoid(x + (lo - slack).unsqueeze(1)).sum(dim=1) - N
        g_hi = torch.sigmoid(x + (hi + slack).unsqueeze(1)).sum(dim=1) - N
        assert bool((g_lo <= 0).all()) and bool((g_hi >= 0).all()), f"{case}: the bracket lost the root"
        d_nu = LML_EPS + slack
        assert float((nu - ref[3]).abs().max()) <= d_nu, case
        d_w = d_nu / 4 + 4 * EPS32
        assert float((w - ref[2]).abs().max()) <= d_w, case
        worst_lml = max(worst_lml, float((w - ref[2]).abs().max()) / d_w)
        Xd = X.double().transpose(0, 1)                                         # (B, S, n)
        d_mu = Xd.abs().sum(dim=1) * d_w / N + RND_SUM * (ref[2].unsqueeze(2) * Xd).abs().sum(dim=1) / N
        assert bool(((mu - ref[0]).abs() <= d_mu).all()), case
        d2 = (Xd - ref[0].unsqueeze(1)) ** 2
        W = ref[2].sum(dim=1, keepdim=True)
        d_v = d2.sum(dim=1) * d_w / N + 2 * ref[0].abs() * (1 - W / N).abs() * d_mu + d_mu ** 2 \
            + RND_SUM * (ref[2].unsqueeze(2) * d2).sum(dim=1) / N
        d_sigma = d_v / (sigma + ref[1]).clamp_min(1e-30) + 2 * EPS32 * ref[1]
        assert bool(((sigma - ref[1]).abs() <= d_sigma).all()), case
        assert float((w.sum(dim=1) - N).abs().max()) <= S * LML_EPS / 8 + S * 4 * EPS32, case
    print(f"fp32, LML mode: worst |dw| / bound {worst_lml:.3f}")
    for name, (dev, dev_twin) in devs.items():
        print(f"fp32, softmax / hard mode, {name}: worst deviation from the fp64 twin, of the largest magnitude: kernel {dev:.3e}, "
              f"fp32 twin {dev_twin:.3e}, ratio {dev / dev_twin:.3f}")
    print(f"fp32, softmax / hard mode: the largest share of a single case's and output's bound 2 x twin + floor: {worst_ratio:.3f} (allowed 1)")
    assert not failures, "\n".join(failures)


def test_bad_arguments_return_the_error_code():
    import theseus_amd as th
    K = th.default_kernels()

    def call(S=8, n=3, n_elite=2, branch=10):
        B = 2
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=DEV)  # noqa: E731
        K.dcem_update(z(S, B), z(S, B, n), n_elite, 1.0, True, LML_EPS, 100, branch, z(B, n), z(B, n), z(B, S), z(B), z(B, 2),
                      torch.zeros(B, dtype=torch.int32, device=DEV))
    call()
    for kw, message in ((dict(S=th._lib.THX_DCEM_MAX_S + 1), "THX_DCEM_MAX_S"), (dict(n_elite=0), "n_elite < 1"),
                        (dict(branch=1), "branch < 2")):
        with pytest.raises(RuntimeError, match=message):
            call(**kw)
    call(S=th._lib.THX_DCEM_MAX_S, n=1, n_elite=3)   # the limit itself runs
    lib = K.lib
    one = th._lib.ctypes.c_void_p(16)
    rc = lib.thx_dcem_update_vjp(one, one, one, one, one, one, one, 0, 1, 1, 1, 1.0, 1, one, one, 1, None)
    assert rc != 0 and b"S < 1" in lib.thx_last_error()
    rc = lib.thx_dcem_update_vjp(one, one, one, one, None, one, one, 4, 1, 1, 1, 1.0, 1, one, one, 1, None)
    assert rc != 0 and b"null pointer" in lib.thx_last_error()
    rc = lib.thx_dcem_update(one, one, 4, 1, 0, 1, 1.0, 1, 1e-3, 100, 10, one, one, one, one, one, one, 1, None)
    assert rc != 0 and b"n < 1" in lib.thx_last_error()
    rc = lib.thx_dcem_update(one, one, 4, 1, 1, 1, 1.0, 1, 1e-3, 100, 10, one, one, one, one, one, one, 7, None)
    assert rc != 0 and b"dtype" in lib.thx_last_error()


# ---- the backward ----------------------------------------------------------------------------------------------------------------
def test_vjp_matches_the_twin_autograd():
    from theseus_amd.dcem import dcem_update_torch
    gen = torch.Generator().manual_seed(99)
    worst, skipped, cases = 0.0, 0, random_cases()
    excluded = {"sigma = 0": 0, "grad_fX of two standardised scores": 0}
    assert {c[6] for c in cases} == {True, False}
    for case in cases:
        B, S, n, N, branch, temp, normalize = case
        if S == 1 or (temp is None and N == 1):
            excluded["sigma = 0"] += 1   # (one sample, or one elite in hard mode: its derivative is infinite on either side)
            continue
        fX, X = random_inputs(case, gen, torch.float64)
        g_mu = torch.randn(B, n, generator=gen, dtype=torch.float64).to(DEV)
        g_sigma = torch.randn(B, n, generator=gen, dtype=torch.float64).to(DEV)
        grads = []
        margin = math.inf
        for fn in ("twin", "kernel"):
            a, b = fX.clone().requires_grad_(), X.clone().requires_grad_()
            if fn == "twin":
                out = dcem_update_torch(a, b, N, temp, normalize, LML_EPS, 100, branch, with_margin=True)
                margin = float(out[6].detach())
            else:
                out = kernel_update(a, b, N, temp, normalize, branch=branch)
            loss = (out[0] * g_mu).sum() + (out[1] * g_sigma).sum()
            grads.append(torch.autograd.grad(loss, [a, b], allow_unused=True))
        if margin < SKIP_MARGIN:
            skipped += 1
            continue
        for k, name in ((0, "grad_fX"), (1, "grad_X")):
            if k == 0 and S == 2 and normalize and temp is not None:
                excluded["grad_fX of two standardised scores"] += 1   # (+-1 / sqrt(2) whatever fX is: what is left is cancellation)
                continue
            want, got = grads[0][k], grads[1][k]
            want = torch.zeros_like(got) if want is None else want
            assert bool(torch.isfinite(want).all()), case
            top = float(want.abs().max())
            dev = float((got - want).abs().max())
            if top == 0:
                assert dev == 0, f"{case} {name}"
                continue
            worst = max(worst, dev / top)
            assert dev <= 1e-10 * top, f"{case} {name}: {dev / top:.3e}"
    print(f"vjp fp64, {len(cases)} cases, {skipped} skipped for a grid value near zero, excluded {excluded}: worst deviation "
          f"{worst:.3e} of the largest entry (allowed 1e-10)")
    assert skipped <= 0.02 * len(cases)


@pytest.mark.parametrize("mode", ["lml", "softmax", "hard", "raw"])
def test_gradcheck_one_problem_per_mode(mode):
    """The LML weights are differentiable only as far as nu is found: with lml_eps = 1e-12 the forward's nu is exact to 5e-13, which a
    central difference of step 1e-6 turns into 2.5e-7 at most -- hence atol 1e-5."""
    gen = torch.Generator().manual_seed(5)
    S, B, n = 9, 1, 3
    fX = (torch.rand(S, B, generator=gen, dtype=torch.float64) * 4 + 0.5).to(DEV).requires_grad_()
    X = torch.randn(S, B, n, generator=gen, dtype=torch.float64).to(DEV).requires_grad_()
    N, temp, normalize = {"lml": (3, 1.0, True), "softmax": (1, 0.7, True), "hard": (3, None, True), "raw": (2, 0.5, False)}[mode]

    def fn(a, b):
        return kernel_update(a, b, N, temp, normalize, lml_eps=1e-12, branch=10)[:2]
    assert torch.autograd.gradcheck(fn, (fX, X), eps=1e-6, atol=1e-5, rtol=1e-6, nondet_tol=0.0)


# ---- the whole optimizer ---------------------------------------------------------------------------------------------------------
def _fixture_run(grad=False, **optimizer_kwargs):
    import theseus_amd as th
    g = dc.load("dcem_f64_soft")
    obj, leaves = dc.build(th, g, device=DEV, grad=grad)
    opt = th.DCEM(obj, lml_branch=dc.BRANCH, **dc.DCEM_KW)
    layer = th.TheseusLayer(opt)
    kw = dict(noise=_t(g["noise"]), **optimizer_kwargs)
    if grad:
        sol, info = layer.forward({"x": leaves["x0"]}, optimizer_kwargs=kw)
    else:
        with torch.no_grad():
            sol, info = layer.forward(None, optimizer_kwargs=kw)
    return g, opt, leaves, sol, info


def test_optimizer_reproduces_the_recorded_run():
    from theseus_amd.dcem import dcem_update_torch
    from tests.test_dcem_host import error_metric
    g, opt, _, sol, info = _fixture_run(track_err_history=True)
    # the twin over the same run on this device: what six chained updates cost when nothing but the device changes
    A, t = _t(g["A"]), _t(g["t"])
    mu, sigma = _t(g["x0"]), torch.ones(dc.B, dc.N_DOF, dtype=torch.float64, device=DEV)
    errs = [error_metric(A, t, mu)]
    for it in range(dc.N_ITER):
        X = dc.samples(mu, sigma, _t(g["noise"][it]))
        mu, sigma = dcem_update_torch(error_metric(A, t, X), X, dc.N_ELITE, 1.0, True, LML_EPS, 100, dc.BRANCH)[:2]
        errs.append(error_metric(A, t, mu))
    twin = {"mu": mu, "sigma": sigma, "err_history": torch.stack(errs, dim=1)}
    got = {"mu": sol["x"], "sigma": opt.sigma, "err_history": info.err_history.to(DEV)}
    want = {"mu": _t(g["mu"][-1]), "sigma": _t(g["sigma"][-1]), "err_history": _t(g["err_history"])}
    dev_twin = max(rel_dev(twin[k], want[k]) for k in want)
    dev = max(rel_dev(got[k], want[k]) for k in want)
    allowed = max(10 * dev_twin, dc.N_ITER * REL)
    print(f"six iterations against the fixture: torch twin on this device {dev_twin:.3e}, kernel path {dev:.3e} "
          f"(allowed {allowed:.3e} = the larger of 10 x the twin's and {dc.N_ITER} x {REL:.0e})")
    assert dev <= allowed
    assert [s.name for s in info.status] == g["status"].tolist() and info.converged_iter.tolist() == g["converged_iter"].tolist()
    assert info.iters_done == dc.N_ITER and torch.equal(info.last_err.cpu(), info.err_history[:, -1])
    assert not opt.lml_flags.any()


def test_layer_gradients_reproduce_the_recorded_ones():
    """the bar of tests/test_gpu_kin.py for implicit gradients: 1e-6 of the gradient's largest entry"""
    g, opt, leaves, sol, info = _fixture_run(grad=True, backward_mode="unroll")
    np.testing.assert_allclose(sol["x"].detach().cpu().numpy(), g["mu"][-1], rtol=1e-8, atol=1e-10)
    (sol["x"] ** 2).sum().backward()
    for k, want in (("t", g["grad_t"]), ("x0", g["grad_x0"])):
        dev = np.abs(leaves[k].grad.cpu().numpy() - want).max() / np.abs(want).max()
        print(f"grad_{k}: {dev:.3e} of the largest entry (allowed 1e-6)")
        np.testing.assert_allclose(leaves[k].grad.cpu().numpy(), want, rtol=0, atol=1e-6 * np.abs(want).max(), err_msg=k)


# ---- fused families ----------------------------------------------------------------------------------------------------------------
def _family_objective(th, family, dtype):
    """-> (objective, the packed class's name, the kernels' error launch, the variable's name, DCEM's initial sigma)"""
    if family == "kin":
        obj, _, _, _ = kin_build(th, load_golden("kin_f64_tree"), device=DEV, dtype=dtype)
        return obj, "PackedKinematics", "kin_error", "theta", 0.05
    obj, _, _ = homog_build(th, kernel_problem(3, 2, 45, 46, seed=3), device=DEV, dtype=dtype)
    return obj, "PackedHomography", "homog_error", "H8", 1e-3


def _family_run(family, dtype, fused, monkeypatch=None, S=12, iters=3):
    import theseus_amd as th
    from theseus_amd.generic import PackedState
    obj, packed_name, launch, var, sigma = _family_objective(th, family, dtype)
    opt = th.DCEM(obj, max_iterations=iters, n_sample=S, n_elite=4, init_sigma=sigma, abs_err_tolerance=0.0, rel_err_tolerance=0.0,
                  lml_branch=10)
    packed = opt.packed
    assert type(packed).__name__ == packed_name
    packed.fused = fused
    counts = {"error_launch": 0, "torch_cost_error": 0}
    if monkeypatch is not None:
        real, real_cost_error = getattr(packed.K, launch), PackedState._cost_error

        def counting(*a, **k):
            counts["error_launch"] += 1
            return real(*a, **k)

        def cost_error(self, c):   # (where the torch path evaluates a cost, whatever the cost class overrides)
            counts["torch_cost_error"] += 1
            return real_cost_error(self, c)
        monkeypatch.setattr(packed.K, launch, counting)
        monkeypatch.setattr(PackedState, "_cost_error", cost_error)
    B, n = 3, packed.n
    noise = torch.randn(iters, S, B, n, generator=torch.Generator().manual_seed(8), dtype=torch.float64).to(dtype).to(DEV)
    with torch.no_grad():
        info = opt.optimize(noise=noise, track_err_history=True)
    return obj.optim_vars[var].tensor, opt, info, counts


@pytest.mark.parametrize("family", ["kin", "homog"])
def test_a_fused_family_is_evaluated_by_its_error_kernel(family, monkeypatch):
    S, iters = 12, 3
    x, opt, info, counts = _family_run(family, torch.float64, True, monkeypatch, S, iters)
    assert counts == {"error_launch": 1 + iters * (S + 1), "torch_cost_error": 0}
    monkeypatch.undo()
    x2, opt2, info2, counts2 = _family_run(family, torch.float64, False, monkeypatch, S, iters)   # (the counter does see the torch path)
    assert counts2 == {"error_launch": 0, "torch_cost_error": (1 + iters * (S + 1)) * len(opt2.packed.costs)}
    allowed = iters * REL   # the update's bar, grown by the iterations
    if family == "homog":
        # The two runs do not get the same errors: thx_homog_error and the torch class agree to REL of an error's size (the bar of
        # tests/test_gpu_homog.py), and standardising divides that difference by the SPREAD of a problem's errors, which for
        # samples 1e-3 around a homography is far below their size.  So the scores, and with them weights, mean and sigma, may
        # differ by REL times size / spread -- taken from the last iteration's errors, where the samples are closest together.
        fX = opt2._fX
        amplification = float((fX.abs().max(dim=0).values / fX.std(dim=0)).max())
        print(f"homog: an error's size over the spread of a problem's errors: {amplification:.1f}")
        allowed *= max(1.0, amplification)
    for name, a, b in (("solution", x, x2), ("sigma", opt.sigma, opt2.sigma), ("err_history", info.err_history, info2.err_history)):
        dev = rel_dev(a, b)
        print(f"{family}, fused against the torch classes, {name}: {dev:.3e} (allowed {allowed:.1e})")
        assert dev <= allowed, name
    assert bool(torch.isfinite(info.err_history).all()) and not opt.lml_flags.any()
    assert float((info.err_history[:, -1] - info.err_history[:, 0]).abs().min()) > 0   # (the run moved)


def test_a_fused_family_in_fp32():
    theta, opt, info, _ = _family_run("kin", torch.float32, True)
    assert theta.shape == (3, opt.packed.n) and theta.dtype == torch.float32 and opt.sigma.shape == theta.shape
    assert info.err_history.shape == (3, 4) and bool(torch.isfinite(info.err_history).all())
    assert [s.name for s in info.status] == ["MAX_ITERATIONS"] * 3 and info.converged_iter.tolist() == [-1] * 3
    assert torch.equal(info.last_err, opt.packed.error_metric())
    assert torch.equal(info.last_err.cpu(), info.err_history[:, -1])
    import theseus_amd as th
    fresh, _, _, _ = kin_build(th, load_golden("kin_f64_tree"), device=DEV, dtype=torch.float32)
    assert torch.equal(info.err_history[:, 0], th.DCEM(fresh).packed.error_metric().cpu())


# ---- loop semantics ----------------------------------------------------------------------------------------------------------------
def host_replay(h, abs_tol, rel_tol):
    """dcem.py:160-204 with nonlinear_optimizer.py:110-119,184-213 on a recorded (B, K + 1) error history -> (statuses, converged_iter,
    iterations done)"""
    B, K = h.shape[0], h.shape[1] - 1
    status, conv_iter, conv = ["START"] * B, [0] * B, [False] * B
    done = 0
    for it in range(K):
        done += 1
        err, last = h[:, it + 1], h[:, it]
        conv_iter = [c + (0 if v else 1) for c, v in zip(conv_iter, conv)]
        if np.abs(err).mean() < abs_tol:
            conv = [True] * B
        else:
            conv = [bool(abs(l - e) < abs_tol or abs((l - e) / l) < rel_tol) for e, l in zip(err, last)]
        status = ["CONVERGED" if v else s for s, v in zip(status, conv)]
        if all(conv):
            break
    status = ["MAX_ITERATIONS" if s == "START" else s for s in status]
    return status, [-1 if s == "MAX_ITERATIONS" else c for s, c in zip(status, conv_iter)], done


def test_converged_problems_keep_moving_and_statuses_follow_the_reference():
    import theseus_amd as th
    g = dc.load("dcem_f64_soft")
    # rel 0.115: problem 0 converges at iteration 4 of 6 (its change there is 0.1139; 0.1208 the iteration before), the others at
    # 2 and 3 -- never all three at once
    rel_tol = 0.115
    obj, _ = dc.build(th, g, device=DEV)
    opt = th.DCEM(obj, lml_branch=dc.BRANCH, **dict(dc.DCEM_KW, rel_err_tolerance=rel_tol))
    with torch.no_grad():
        info = opt.optimize(noise=_t(g["noise"]), track_err_history=True)
    h = info.err_history.numpy()
    np.testing.assert_allclose(h, g["err_history"], rtol=1e-9)      # converged problems were not frozen: the recorded run's errors
    status, conv_iter, done = host_replay(h, 0.0, rel_tol)
    assert status == ["CONVERGED"] * 3 and done == dc.N_ITER
    assert abs((h[0, 3] - h[0, 4]) / h[0, 3]) < rel_tol < abs((h[0, 2] - h[0, 3]) / h[0, 2])   # (problem 0: iteration 4)
    assert [s.name for s in info.status] == status and info.converged_iter.tolist() == conv_iter and info.iters_done == done
    assert h[0, 4] != h[0, 5] != h[0, 6]
    # everybody at once: the loop stops there and last_err stays the previous iteration's (dcem.py:193-195)
    opt = th.DCEM(obj, lml_branch=dc.BRANCH, **dict(dc.DCEM_KW, rel_err_tolerance=0.7))
    obj.update({"x": _t(g["x0"])})
    with torch.no_grad():
        info = opt.optimize(noise=_t(g["noise"]), track_err_history=True)
    status, conv_iter, done = host_replay(g["err_history"], 0.0, 0.7)
    assert done == 1 and info.iters_done == 1 and [s.name for s in info.status] == status == ["CONVERGED"] * 3
    assert info.converged_iter.tolist() == conv_iter
    assert torch.equal(info.last_err.cpu(), info.err_history[:, 0]) and bool(torch.isinf(info.err_history[:, 2:]).all())
    np.testing.assert_allclose(obj.optim_vars["x"].tensor.cpu().numpy(), g["mu"][0], rtol=1e-9, atol=1e-12)


def test_track_best_solution_returns_the_state_of_the_smallest_recorded_error():
    seen = []
    g, opt, _, sol, info = _fixture_run(track_err_history=True, track_best_solution=True, track_state_history=True,
                                        end_iter_callback=lambda o, i, mu, it: seen.append((it, mu["x"].clone(), i.last_err.clone())))
    h = info.err_history
    # the callback saw every iteration's mean (the variables viewed it) and error
    assert [it for it, _, _ in seen] == list(range(dc.N_ITER))
    for it, mu, err in seen:
        np.testing.assert_allclose(mu.cpu().numpy(), g["mu"][it], rtol=1e-9, atol=1e-12)
        assert torch.equal(err.cpu(), h[:, it + 1])
    assert bool((h[1, 1:] > h[1, 0]).any())   # (problem 1 gets worse before it gets better: the best is not simply the last)
    best = h.argmin(dim=1)
    states = info.state_history["x"]          # (B, n, K + 1)
    for b in range(dc.B):
        assert torch.equal(info.best_solution["x"][b].to(states.dtype), states[b, :, best[b]]), b
        assert int(info.best_iter[b]) == max(int(best[b]) - 1, 0)
    assert torch.equal(info.best_err.cpu(), h.min(dim=1).values)
    assert torch.equal(states[..., -1], sol["x"].cpu().to(states.dtype))


def test_a_cost_that_raises_mid_loop_leaves_the_variables_valid():
    import theseus_amd as th
    g = dc.load("dcem_f64_soft")
    calls = {"n": 0, "armed": False}

    def err_fn(optim_vars, aux_vars):
        calls["n"] += 1
        if calls["armed"] and calls["n"] > 1 + dc.N_SAMPLE + 7:      # inside the second iteration's samples
            raise RuntimeError("cost function stand-in")
        return dc.err_fn(optim_vars, aux_vars)
    x = th.Vector(tensor=_t(g["x0"]), name="x")
    obj = th.Objective(dtype=torch.float64)
    weight = th.ScaleCostWeight(th.Variable(torch.ones(1, 1, dtype=torch.float64, device=DEV), name="w_fit"))
    obj.add(th.AutoDiffCostFunction([x], err_fn, dc.DIM, cost_weight=weight,
                                    aux_vars=[th.Variable(_t(g["A"]), name="A"), th.Variable(_t(g["t"]), name="t")], name="fit"))
    opt = th.DCEM(obj, lml_branch=dc.BRANCH, **dc.DCEM_KW)
    layer = th.TheseusLayer(opt)
    with torch.no_grad():
        layer.forward(None, optimizer_kwargs=dict(noise=_t(g["noise"])))     # a state buffer handed out: the next call privatizes
        calls.update(n=0, armed=True)
        with pytest.raises(RuntimeError, match="stand-in"):
            layer.forward({"x": _t(g["x0"])}, optimizer_kwargs=dict(noise=_t(g["noise"])))
        calls["armed"] = False
        assert not opt.packed._vars_stale
        held = obj.optim_vars["x"].tensor
        np.testing.assert_allclose(held.cpu().numpy(), g["mu"][0], rtol=1e-9, atol=1e-12)   # the state the loop had reached
        # new inputs: the recorded run again, as a fresh optimizer sees it
        sol, info = layer.forward({"x": _t(g["x0"])}, optimizer_kwargs=dict(noise=_t(g["noise"]), track_err_history=True))
    np.testing.assert_allclose(info.err_history.numpy(), g["err_history"], rtol=1e-9)
    np.testing.assert_allclose(held.cpu().numpy(), g["mu"][0], rtol=1e-9, atol=1e-12)       # ... and nobody wrote into what was held
