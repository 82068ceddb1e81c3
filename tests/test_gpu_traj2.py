"""-m gpu: 2D motion planning on the fused kernels (csrc/traj_kernels.hip: thx_traj2_eval, thx_traj2_error; theseus_amd/embodied.py:
PackedTrajectory2D) against the torch classes in the same dtype and against the REAL reference's fixtures
(tests/golden/traj2_f64_*.npz).  CPU twin: tests/test_traj2_host.py."""
import numpy as np
import pytest
import torch

from tests.helpers import load_golden
from tests.test_traj2_host import (_lm, assert_blocks_close, check_implicit_gradients, check_iterates,
                                   run_implicit_with_nothing_to_differentiate)
from tests.traj2_common import FIXTURES, build, random_problem, slice_aux

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL = {torch.float64: 1e-12, torch.float32: 1e-5}   # of each block's largest magnitude (a few dozen flops per value)


def _packed(th, obj):
    lin = th.HipLinearization(obj)
    assert type(lin.packed).__name__ == "PackedTrajectory2D" and type(lin.K).__name__ == "HipKernels"
    return lin, lin.packed


def compare_with_torch_classes(packed, rel):
    """thx_traj2_eval's blocks and errors, thx_traj2_error's metric <-> the torch classes at the same state, same dtype"""
    Jv, ev = packed._eval()
    metric = packed.error_metric()
    B = packed.batch
    worst, total = 0.0, torch.zeros(B, dtype=torch.float64, device=DEV)
    for c, cost in enumerate(packed.costs):
        jac, err = cost.weighted_jacobians_error()
        total += (err.double() ** 2).sum(1).expand(B)
        pairs = [(ev[c], err)] + list(zip(Jv[c], jac))
        for k, (got, want) in enumerate(pairs):
            want = want.expand_as(got)
            scale = float(want.abs().max())
            diff = float((got - want).abs().max())
            worst = max(worst, diff / scale if scale else diff)
            assert diff <= rel * scale, f"{cost.name} {'error' if k == 0 else f'block {k - 1}'}: {diff:.3e} > {rel:.0e} * {scale:.3e}"
    want = 0.5 * total
    diff = float(((metric.double() - want).abs() / want).max())
    print(f"worst block {worst:.3e}, error metric {diff:.3e} (bound {rel:.0e})")
    assert diff <= rel
    assert float((packed._e - packed.error_vector()).abs().max()) <= rel * float(packed._e.abs().max())   # (B, m), objective row order


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("fixture", FIXTURES)
def test_kernels_match_the_torch_classes_at_the_fixture_inputs(fixture, dtype):
    import theseus_amd as th
    obj, _, _ = build(th, load_golden(fixture), device=DEV, dtype=dtype)
    _, packed = _packed(th, obj)
    compare_with_torch_classes(packed, REL[dtype])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_kernels_match_the_torch_classes_on_a_larger_random_problem(dtype):
    """B = 70 (no multiple of the wave size), N = 40: 4 + 41 + 40 = 85 terms per problem, a tenth of the points out of bounds"""
    import theseus_amd as th
    obj, _, _ = build(th, random_problem(70, 40, seed=5), device=DEV, dtype=dtype, N=40)
    _, packed = _packed(th, obj)
    assert len(packed.costs) == 85 and packed.n == 164
    compare_with_torch_classes(packed, REL[dtype])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_kernels_read_sliced_auxiliaries_through_their_batch_stride(dtype):
    """B = 3, N = 4; cost_eps, the start target and sdf_data are views into larger tensors (tests/traj2_common.py: slice_aux): the
    kernels index them by a batch stride that is not their width -- 3, 5 and 2 R C elements.  CPU twin:
    tests/test_traj2_host.py::test_sliced_auxiliaries_are_read_in_place."""
    import theseus_amd as th
    g = load_golden(FIXTURES[1])
    obj, _, _ = build(th, g, device=DEV, dtype=dtype, N=4)
    parents = slice_aux(obj, g, device=DEV, dtype=dtype)
    _, packed = _packed(th, obj)
    compare_with_torch_classes(packed, REL[dtype])
    table = packed._table
    assert packed._aux_key is not None
    with torch.no_grad():
        parents["cost_eps"][:, 1] += 0.3
        parents["sdf_data"][:, 0] *= 0.8
    compare_with_torch_classes(packed, REL[dtype])
    assert packed._table is table


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
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedTrajectory2D"
    check_iterates(g, info, g["var_order"].tolist())


@pytest.mark.parametrize("fixture", FIXTURES)
def test_implicit_gradients_reproduce_the_reference(fixture):
    import theseus_amd as th
    g = load_golden(fixture)
    _, opt, leaves, sol, _ = _lm(th, g, None, device=DEV, backward_mode="implicit")
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedTrajectory2D"
    check_implicit_gradients(g, leaves, sol, g["var_order"].tolist())


def test_implicit_mode_under_no_grad_stays_fused(monkeypatch):
    """the implicit last step with nothing to differentiate: thx_traj2_eval + the gradient thx_block_assemble formed, no torch class"""
    import theseus_amd as th
    g = load_golden(FIXTURES[1])
    _, final = run_implicit_with_nothing_to_differentiate(th, g, None, "no_grad", monkeypatch, device=DEV)
    np.testing.assert_allclose(final.cpu().numpy(), g["implicit_final"], rtol=1e-8, atol=1e-10)


def test_the_fused_path_is_really_taken(monkeypatch):
    """No cost function is evaluated by torch in a no_grad LM run: one thx_traj2_eval per linearization, thx_traj2_error for every
    error metric."""
    import theseus_amd as th
    g = load_golden(FIXTURES[0])
    K = th.HipKernels()
    calls = {"traj2_eval": 0, "traj2_error": 0, "block_assemble_strided": 0}
    for name in calls:
        def counted(*a, _f=getattr(K, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(K, name, counted)

    def refuse(*a, **kw):
        raise AssertionError("a cost function was evaluated by torch on the fused path")
    for cls in (th.eb.Collision2D, th.eb.DoubleIntegrator, th.Difference):
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
    assert linearizations["n"] >= 5 and calls["traj2_eval"] == linearizations["n"] == calls["block_assemble_strided"]
    assert calls["traj2_error"] >= 6   # the initial error + one per iteration
    check_iterates(g, info, g["var_order"].tolist())


def test_replaced_aux_values_are_seen_by_the_next_call():
    import theseus_amd as th
    g = load_golden(FIXTURES[0])
    obj, _, _ = build(th, g, device=DEV)
    lin, packed = _packed(th, obj)
    lin.linearize()
    H0, g0, e0 = lin.AtA.clone(), lin.Atb.clone(), obj.error_metric().clone()
    new_eps = torch.tensor([[0.7]], dtype=torch.float64, device=DEV)
    new_sdf = torch.from_numpy(g["sdf_data"]).to(DEV) * 0.8 - 0.05
    obj.update({"cost_eps": new_eps, "sdf_data": new_sdf})
    lin.linearize()
    assert float((lin.AtA - H0).abs().max()) > 1e-3 and float((obj.error_metric() - e0).abs().max()) > 1e-3
    compare_with_torch_classes(packed, 1e-12)
    # ... and H, g are those of the torch classes' blocks (the generic path on the same objective)
    from theseus_amd.euclidean import PackedEuclidean
    generic = PackedEuclidean(obj, packed.K)
    generic.sync()
    H = torch.zeros_like(lin._H)
    gg = torch.zeros_like(lin.g)
    generic.assemble(H, gg)
    assert float((H - lin._H).abs().max()) <= 1e-12 * float(H.abs().max())
    assert float((gg - lin.g).abs().max()) <= 1e-12 * float(gg.abs().max())
    # in-place edits of an auxiliary tensor need no re-pack: the table points at the tensor itself
    new_eps.fill_(0.2)
    compare_with_torch_classes(packed, 1e-12)
