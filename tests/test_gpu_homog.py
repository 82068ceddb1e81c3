"""-m gpu: homography alignment on the fused kernels (csrc/homog_kernels.hip: thx_homog_eval, thx_homog_error;
theseus_amd/homography.py: PackedHomography) against the torch class in the same dtype and against the REAL reference's fixtures
(tests/golden/homog_f64_*.npz).  CPU twin: tests/test_homog_host.py.

The bound of every comparison with the torch class: |got - want| <= REL[dtype] * (weight / sum m) * sum |per-element term|, the sum
of magnitudes taken from the fp64 torch class (tests/homog_common.py: term_magnitudes) -- a few dozen flops per element in the run's
dtype, accumulated in fp64.  The error's terms m d^2 are all non-negative, so for it the bound is relative; the error metric
0.5 sum e^2 then lies within (2 REL + REL^2) of itself.  Prior blocks: REL of the block's largest magnitude, as in
tests/test_gpu_traj2.py.

Not tested, on purpose: the identity homography on sizes such as 60 x 80, where Ww - 1 is no power of two -- every source coordinate
is then an integer up to the last bit of ix, and which one-sided derivative floor() selects depends on that bit."""
import numpy as np
import pytest
import torch

from tests.helpers import load_golden
from tests.homog_common import FIXTURES, MARGIN, build, kernel_problem, min_margin, outside_fractions, smooth_maps, term_magnitudes
from tests.test_gpu_traj2 import REL
from tests.test_homog_host import (_lm, assert_blocks_close, check_implicit_gradients, check_iterates,
                                   run_implicit_with_nothing_to_differentiate)
from theseus_amd._lib import THX_HOMOG_CHUNK
from theseus_amd.homography import HOMOG_TERM

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = {torch.float64: "f64", torch.float32: "f32"}
both_dtypes = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])


def _packed(th, obj):
    lin = th.HipLinearization(obj)
    assert type(lin.packed).__name__ == "PackedHomography" and type(lin.K).__name__ == "HipKernels"
    return lin, lin.packed


def compare(packed, mags, rel):
    """thx_homog_eval's blocks and errors, thx_homog_error's metric <-> the torch classes at the same state, same dtype; ``mags``:
    term_magnitudes of the fp64 twin of the alignment cost"""
    Jv, ev = packed._eval()
    Jv, ev = [[j.clone() for j in J] for J in Jv], [e.clone() for e in ev]
    metric = packed.error_metric()
    B = packed.batch
    total = torch.zeros(B, dtype=torch.float64, device=DEV)
    for c, cost in enumerate(packed.costs):
        jac, err = cost.weighted_jacobians_error()
        total += (err.double() ** 2).sum(1).expand(B)
        if type(cost).__name__ == "HomographyAlignment":
            e_mag, j_mag = mags
            de, dj = (ev[c] - err).abs().double(), (Jv[c][0] - jac[0]).abs().double()
            print(f"{cost.name}: error {float((de / e_mag).max()):.3e}, block {float((dj / j_mag).max()):.3e} of the bound's sums "
                  f"(allowed {rel:.0e})")
            assert bool((de <= rel * e_mag).all()), f"{cost.name} error: {de.flatten().tolist()} > {rel:.0e} * {e_mag.flatten().tolist()}"
            assert bool((dj <= rel * j_mag).all()), f"{cost.name} block: {(dj / j_mag).max():.3e} of the sum of magnitudes > {rel:.0e}"
        else:
            for got, want, what in ((ev[c], err, "error"), (Jv[c][0], jac[0], "block")):
                want = want.expand_as(got)
                assert float((got - want).abs().max()) <= rel * float(want.abs().max()), f"{cost.name} {what}"
    want = 0.5 * total
    diff = float(((metric.double() - want).abs() / want).max())
    print(f"error metric {diff:.3e} (allowed {2 * rel + rel * rel:.1e})")
    assert diff <= 2 * rel + rel * rel


def run_case(f, dtype, lattice=False, edit=None):
    """build ``f`` in fp64 (the bound's magnitudes, the precondition) and in ``dtype`` (the comparison) -> (objective, packed, mags)"""
    import theseus_amd as th
    obj64, _, _ = build(th, f, device=DEV)
    if edit is not None:
        edit(obj64, torch.float64)
    cost64 = obj64.cost_functions["align"]
    if dtype == torch.float32 and not lattice:
        assert min_margin(cost64) >= MARGIN, "a source coordinate lies within 1e-3 pixel of an integer: choose another homography"
    mags = term_magnitudes(cost64)
    obj, _, _ = build(th, f, device=DEV, dtype=dtype)
    if edit is not None:
        edit(obj, dtype)
    _, packed = _packed(th, obj)
    compare(packed, mags, REL[dtype])
    return obj, packed, mags


@both_dtypes
@pytest.mark.parametrize("fixture", FIXTURES)
def test_kernels_match_the_torch_class_at_the_fixture_inputs(fixture, dtype):
    run_case(load_golden(fixture), dtype)


# fewer pixels than a wave; a partial workgroup; just above one chunk; just above two chunks (the last chunk partial)
SHAPES = [(1, 5, 7), (3, 13, 19), (2, 32, 33), (2, 45, 46)]


@both_dtypes
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C,Hh,Ww", SHAPES, ids=[f"{h}x{w}x{c}" for c, h, w in SHAPES])
def test_kernels_match_the_torch_class(C, Hh, Ww, B, dtype):
    assert (32 * 33 - THX_HOMOG_CHUNK, 45 * 46 - 2 * THX_HOMOG_CHUNK) == (32, 22)
    run_case(kernel_problem(B, C, Hh, Ww, seed=7 + Hh), dtype)


@both_dtypes
@pytest.mark.parametrize("Hh,Ww", [(5, 9), (9, 17)])
def test_identity_homography_on_exact_lattice_points(Hh, Ww, dtype):
    """Hh - 1 and Ww - 1 are powers of two: every source coordinate is an exact integer in both dtypes (asserted), the weights are
    1, 0, 0, 0 and ds/dix is the one-sided difference towards the next column -- the example's starting point"""
    import theseus_amd as th
    f = kernel_problem(3, 2, Hh, Ww, seed=5)
    f["H8_0"] = np.tile(np.array([[1.0, 0, 0, 0, 1, 0, 0, 0]]), (3, 1))
    f["feat_dst"] = smooth_maps(3, 2, Hh, Ww, seed=99)
    obj, packed, _ = run_case(f, dtype, lattice=True)
    ix, iy = obj.cost_functions["align"].source_points()
    jj = torch.arange(Ww, dtype=dtype, device=DEV).repeat(Hh)
    ii = torch.arange(Hh, dtype=dtype, device=DEV).repeat_interleave(Ww)
    assert bool((ix == jj).all()) and bool((iy == ii).all())
    assert float(packed._Jv[0][0].abs().max()) > 0


@both_dtypes
def test_warps_that_leave_the_image_on_every_side(dtype):
    """the source points lie three times as far from the centre as the destination pixels: a third of them beyond each edge, where
    the corner indices are clamped while the weights are not"""
    obj, _, _ = run_case(kernel_problem(3, 3, 13, 19, seed=4, scale=3.0), dtype)
    assert all(0.3 <= fr <= 0.4 for fr in outside_fractions(obj.cost_functions["align"]))


def _slice_maps(obj, dtype):
    """feat_src / feat_dst become slices ``big[:, 1]`` / ``big[:, 0]`` of (B, 2, C, Hh, Ww) tensors whose other half holds values no
    cost should ever see"""
    for name, k in (("feat_src", 1), ("feat_dst", 0)):
        v = obj.get_variable(name)
        big = torch.full((v.shape[0], 2) + tuple(v.shape[1:]), -7.0, dtype=dtype, device=DEV)
        big[:, k] = v.tensor
        v.tensor = big[:, k]
        assert v.tensor[0].is_contiguous() and (v.shape[0] == 1 or not v.tensor.is_contiguous())


@both_dtypes
def test_kernels_read_shared_and_sliced_feature_maps_through_their_batch_stride(dtype):
    _, packed, _ = run_case(kernel_problem(3, 2, 13, 19, seed=8, shared=True), dtype)   # batch 1: stride 0
    table = packed._table.cpu().numpy().view(HOMOG_TERM)
    assert table[0]["aux_bstride"][0] == 0 == table[0]["aux_bstride"][1]
    _, packed, _ = run_case(kernel_problem(3, 2, 13, 19, seed=8), dtype, edit=_slice_maps)
    table = packed._table.cpu().numpy().view(HOMOG_TERM)
    assert table[0]["aux_bstride"][0] == 2 * 2 * 13 * 19 == table[0]["aux_bstride"][1] and packed._aux_key is not None


@both_dtypes
def test_two_calls_give_the_same_bits(dtype):
    import theseus_amd as th
    obj, _, _ = build(th, kernel_problem(3, 2, 45, 46, seed=3), device=DEV, dtype=dtype)
    _, packed = _packed(th, obj)
    runs = []
    for _ in range(2):
        packed._eval()
        runs.append((packed._J.clone(), packed._e.clone(), packed.error_metric().clone()))
        packed._J.fill_(7.0)
        packed._scratch.fill_(7.0)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert bool(torch.isfinite(runs[0][0]).all()) and float(runs[0][0].abs().max()) > 0


@pytest.mark.parametrize("fixture", FIXTURES)
def test_fused_assemble_matches_the_reference(fixture):
    import theseus_amd as th
    g = load_golden(fixture)
    obj, _, _ = build(th, g, device=DEV)
    lin, _ = _packed(th, obj)
    lin.linearize()
    assert_blocks_close(torch.tril(lin.AtA).cpu().numpy(), np.tril(g["AtA"]), 1e-12, "AtA")
    assert_blocks_close(lin.Atb.squeeze(2).cpu().numpy(), g["Atb"], 1e-12, "Atb")
    assert_blocks_close(obj.error_metric().cpu().numpy(), g["error_metric"], 1e-12, "error metric")


@pytest.mark.parametrize("fixture", FIXTURES)
def test_fused_lm_reproduces_the_reference_iterates(fixture):
    import theseus_amd as th
    g = load_golden(fixture)
    with torch.no_grad():
        _, opt, _, _, info = _lm(th, g, None, device=DEV, track_err_history=True, track_state_history=True)
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedHomography"
    check_iterates(g, info, g["var_order"].tolist())


@pytest.mark.parametrize("fixture", FIXTURES)
def test_implicit_gradients_reproduce_the_reference(fixture):
    """w.r.t. both feature maps, through the torch twin"""
    import theseus_amd as th
    g = load_golden(fixture)
    _, opt, leaves, sol, _ = _lm(th, g, None, device=DEV, backward_mode="implicit")
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedHomography"
    check_implicit_gradients(g, leaves, sol)


def test_implicit_mode_under_no_grad_stays_fused(monkeypatch):
    """the implicit last step with nothing to differentiate: thx_homog_eval + the gradient thx_block_assemble formed, no torch class"""
    import theseus_amd as th
    g = load_golden(FIXTURES[1])
    _, final = run_implicit_with_nothing_to_differentiate(th, g, None, monkeypatch, device=DEV)
    np.testing.assert_allclose(final.cpu().numpy(), g["implicit_final"], rtol=1e-8, atol=1e-10)


def test_the_fused_path_is_really_taken(monkeypatch):
    """No cost function is evaluated by torch in a no_grad LM run: one thx_homog_eval per linearization, thx_homog_error for every
    error metric."""
    import theseus_amd as th
    g = load_golden(FIXTURES[0])
    K = th.HipKernels()
    calls = {"homog_eval": 0, "homog_error": 0, "block_assemble_strided": 0}
    for name in calls:
        def counted(*a, _f=getattr(K, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(K, name, counted)

    def refuse(*a, **kw):
        raise AssertionError("a cost function was evaluated by torch on the fused path")
    for cls in (th.eb.HomographyAlignment, th.Difference):
        for method in ("error", "jacobians"):
            monkeypatch.setattr(cls, method, refuse)
    linearizations = {"n": 0}
    real = th.HipLinearization._assemble

    def counting_assemble(self):
        linearizations["n"] += 1
        return real(self)
    monkeypatch.setattr(th.HipLinearization, "_assemble", counting_assemble)
    with torch.no_grad():
        _, opt, _, _, info = _lm(th, g, K, device=DEV, track_err_history=True, track_state_history=True)
    assert opt.linear_solver.linearization.K is K
    assert linearizations["n"] >= 5 and calls["homog_eval"] == linearizations["n"] == calls["block_assemble_strided"]
    assert calls["homog_error"] >= 6   # the initial error + one per iteration
    check_iterates(g, info, g["var_order"].tolist())


def test_replaced_feature_maps_are_seen_by_the_next_call():
    """what a CNN outside does at every outer step: new tensors -> the table is rebuilt; values changed in place -> it is not"""
    import theseus_amd as th
    g = load_golden(FIXTURES[1])
    obj, _, _ = build(th, g, device=DEV)
    lin, packed = _packed(th, obj)
    lin.linearize()
    H0, e0 = lin.AtA.clone(), obj.error_metric().clone()
    new_src = torch.from_numpy(g["feat_src"]).to(DEV) * 0.7 + 0.1
    new_dst = torch.from_numpy(g["feat_dst"]).to(DEV) * 1.2 - 0.05
    obj.update({"feat_src": new_src, "feat_dst": new_dst})
    lin.linearize()
    assert float((lin.AtA - H0).abs().max()) > 1e-4 and float((obj.error_metric() - e0).abs().max()) > 1e-4
    cost = obj.cost_functions["align"]
    compare(packed, term_magnitudes(cost), 1e-12)
    table = packed._table
    new_src.mul_(1.3)
    new_dst.add_(0.02)
    compare(packed, term_magnitudes(cost), 1e-12)
    assert packed._table is table
