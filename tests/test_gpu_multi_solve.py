"""-m gpu: thx_chol_solve_multi (csrc/multi_solve_kernels.hip) -- triangular solves with a block of right-hand sides on a dense
Cholesky factor frame.  The factor comes from K.chol_factor; the expected values are computed on the CPU in fp64 from the DEVICE's
own L (copied to the host, cast to double) with torch.linalg.solve_triangular: the substitution alone is under test, not the
factorisation's rounding.  Error measure: max|x - x_ref| / max|x_ref| per problem; bars: the project's own for a Cholesky solve on
these matrices (tests/test_gpu_kernels.py: 1e-4 in fp32, 1e-11 in fp64)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
BAR = {F32: 1e-4, F64: 1e-11}
B = 3


@pytest.fixture(scope="module")
def K():
    from theseus_amd.kernels import HipKernels
    return HipKernels()


def _random_spd(nb, n, dtype, seed, cond=1e3):
    """The matrices of tests/test_gpu_kernels.py (_random_spd): A A^T / (n + 8) + I / cond."""
    gen = torch.Generator().manual_seed(seed)
    A = torch.randn(nb, n, n + 8, dtype=torch.float64, generator=gen)
    M = A @ A.transpose(1, 2) / (n + 8) + (1.0 / cond) * torch.eye(n, dtype=torch.float64)
    return M.to(dtype)


def _factor(K, n, dtype, ld=None, seed=None):
    from theseus_amd.kernels import round_up
    ld = ld or round_up(n, 32)
    M = _random_spd(B, n, dtype, seed=1000 + n if seed is None else seed)
    H = torch.zeros(B, ld, ld, dtype=dtype)
    H[:, :n, :n] = torch.tril(M)
    H = H.cuda()
    L = torch.zeros_like(H)
    panels = torch.empty(B, (n + 127) // 128, 128, 128, dtype=dtype, device="cuda")
    info = torch.empty(B, dtype=torch.int32, device="cuda")
    K.chol_factor(H, n, None, False, 1e-8, L, panels, info)
    assert int(info.abs().sum()) == 0
    return L, panels


_FACTORS = {}


def _cached(K, n, dtype):
    """(L, panels, L as fp64 on the host) of the (n, dtype) matrices: factorised once per module."""
    if (n, dtype) not in _FACTORS:
        L, panels = _factor(K, n, dtype)
        _FACTORS[(n, dtype)] = (L, panels, torch.tril(L[:, :n, :n].double().cpu()))
    return _FACTORS[(n, dtype)]


def _rhs(n, nrhs, dtype, seed=5):
    return torch.randn(B, nrhs, n, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _reference(L64, rhs, which):
    """fp64 on the CPU, from the device's L: rhs (B, nrhs, n) rows are vectors."""
    R = rhs.double().cpu().transpose(1, 2)   # (B, n, nrhs)
    if which != 1:
        R = torch.linalg.solve_triangular(L64, R, upper=False)
    if which != 2:
        R = torch.linalg.solve_triangular(L64.transpose(1, 2), R, upper=True)
    return R.transpose(1, 2)


def _errors(x, ref):
    x = x.double().cpu()
    return [float((x[b] - ref[b]).abs().max() / ref[b].abs().max()) for b in range(x.shape[0])]


def _check(x, ref, dtype, what):
    assert torch.isfinite(x).all(), what
    errs = _errors(x, ref)
    print(what, "errors", errs)
    assert max(errs) < BAR[dtype], (what, errs)


SHAPES = [(n, nrhs, 0) for n in (20, 128, 200, 390) for nrhs in (1, 5, 32, 33, 70)] + \
         [(20, 5, 1), (128, 33, 1), (200, 5, 1), (390, 33, 1), (20, 33, 2), (128, 5, 2), (200, 33, 2), (390, 5, 2)]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,nrhs,which", SHAPES)
def test_shapes_against_fp64_substitution_with_the_devices_factor(K, dtype, n, nrhs, which):
    L, panels, L64 = _cached(K, n, dtype)
    rhs = _rhs(n, nrhs, dtype).cuda()
    keep = rhs.clone()
    x = torch.empty_like(rhs)
    K.chol_solve_multi(L, n, panels, rhs, x, which=which)
    assert torch.equal(rhs, keep)   # out of place: the right-hand sides are only read
    _check(x, _reference(L64, rhs, which), dtype, f"n={n} nrhs={nrhs} which={which}")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("nrhs", [5, 33])
def test_strides_gaps_and_frame_padding(K, dtype, nrhs):
    """n = 132 in a 160-wide frame; vectors ldv = n + 12 apart, problems nrhs * ldv + 40 apart; the gaps of x keep their sentinel;
    rows n..ld-1 of L are NaN after factorising and must not reach the result."""
    n, ld, ldv = 132, 160, 132 + 12
    bstride = nrhs * ldv + 40
    L, panels = _factor(K, n, dtype, ld=ld, seed=77)
    L64 = torch.tril(L[:, :n, :n].double().cpu())
    L[:, n:, :] = float("nan")
    rhs = _rhs(n, nrhs, dtype, seed=9)
    sentinel = -12345.0
    rbuf = torch.full((B * bstride,), sentinel, dtype=dtype, device="cuda")
    xbuf = torch.full((B * bstride,), sentinel, dtype=dtype, device="cuda")
    rv = rbuf.as_strided((B, nrhs, n), (bstride, ldv, 1))
    xv = xbuf.as_strided((B, nrhs, n), (bstride, ldv, 1))
    rv.copy_(rhs.cuda())
    K.chol_solve_multi(L, n, panels, rv, xv, which=0)
    _check(xv, _reference(L64, rhs, 0), dtype, f"strided nrhs={nrhs}")
    written = torch.zeros(B * bstride, dtype=torch.bool, device="cuda")
    written.as_strided((B, nrhs, n), (bstride, ldv, 1)).fill_(True)
    assert bool((xbuf[~written] == sentinel).all())


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_in_place_has_the_bits_of_out_of_place(K, dtype, which):
    n, nrhs = 390, 33
    L, panels, _ = _cached(K, n, dtype)
    rhs = _rhs(n, nrhs, dtype, seed=11).cuda()
    x = torch.empty_like(rhs)
    K.chol_solve_multi(L, n, panels, rhs, x, which=which)
    y = rhs.clone()
    K.chol_solve_multi(L, n, panels, y, y, which=which)
    assert torch.equal(x, y)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_a_column_does_not_depend_on_the_rest_of_the_call(K, dtype):
    n, nrhs = 390, 70
    L, panels, _ = _cached(K, n, dtype)
    rhs = _rhs(n, nrhs, dtype, seed=13).cuda()
    x = torch.empty_like(rhs)
    K.chol_solve_multi(L, n, panels, rhs, x)
    again = torch.empty_like(rhs)
    K.chol_solve_multi(L, n, panels, rhs, again)
    assert torch.equal(x, again)
    for s in (0, 69):
        one = rhs[:, s:s + 1].contiguous()
        alone = torch.empty_like(one)
        K.chol_solve_multi(L, n, panels, one, alone)
        assert torch.equal(alone[:, 0], x[:, s]), s


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("schedule", ["default", "left_looking"])
def test_both_factor_schedules(dtype, schedule):
    """n = 390, B = 3 in a 512-wide frame: the default schedule is right-looking at this batch (it needs a frame of whole tiles:
    in the 416-wide one the default is left-looking too); right_looking_max_batch = 0 gives the left-looking one."""
    from theseus_amd.kernels import HipKernels
    Ks = HipKernels()
    n, ld, nrhs = 390, 512, 33
    if schedule == "left_looking":
        Ks.chol_right_looking_max_batch(0)
    plan = Ks.chol_plan(n, ld, B, dtype, damping=False, rhs=False)
    assert plan["right_looking"] == (1 if schedule == "default" else 0), plan
    L, panels = _factor(Ks, n, dtype, ld=ld, seed=31)
    L64 = torch.tril(L[:, :n, :n].double().cpu())
    rhs = _rhs(n, nrhs, dtype, seed=17).cuda()
    x = torch.empty_like(rhs)
    Ks.chol_solve_multi(L, n, panels, rhs, x)
    _check(x, _reference(L64, rhs, 0), dtype, f"schedule={schedule}")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_against_the_single_vector_kernels(K, dtype):
    """A cross-check of `which` and of the transposition: both sit within the bar of the fp64 value, so they agree to twice it."""
    n, nrhs = 390, 5
    L, panels, L64 = _cached(K, n, dtype)
    rhs = _rhs(n, nrhs, dtype, seed=19).cuda()
    x = torch.empty_like(rhs)
    K.chol_solve_multi(L, n, panels, rhs, x, which=0)
    xb = torch.empty_like(rhs)
    K.chol_solve_multi(L, n, panels, rhs, xb, which=1)
    single, single_b = torch.empty_like(rhs), torch.empty_like(rhs)
    for s in range(nrhs):
        v = rhs[:, s].contiguous()
        o = torch.empty_like(v)
        K.chol_solve(L, n, panels, v, o)
        single[:, s] = o
        K.chol_solve_backward(L, n, panels, v, o)
        single_b[:, s] = o
    for got, want, which in ((x, single, 0), (xb, single_b, 1)):
        _check(want, _reference(L64, rhs, which), dtype, f"single-vector kernel which={which}")
        errs = _errors(got, want.double().cpu())
        print("multi against single, which =", which, errs)
        assert max(errs) < 2 * BAR[dtype], (which, errs)


def test_bad_shapes_are_refused_by_the_binding(K):
    n = 20
    L, panels, _ = _cached(K, n, F32)
    rhs = _rhs(n, 5, F32).cuda()
    with pytest.raises(ValueError):
        K.chol_solve_multi(L, n, panels, rhs[:, :, :19], torch.empty(B, 5, 19, device="cuda"))
    with pytest.raises(ValueError):
        K.chol_solve_multi(L, n, panels, rhs.double(), rhs.double())
    with pytest.raises(ValueError):
        K.chol_solve_multi(L, n, panels, rhs[:, 0], rhs[:, 0])
    with pytest.raises(RuntimeError, match="which"):
        K.chol_solve_multi(L, n, panels, rhs, torch.empty_like(rhs), which=3)
