"""State ownership of every packer behind the optimizer loop (-m "not gpu", TEST stand-in kernels): the properties
tests/test_host_state.py pins for the pose-graph packer, on the pose-graph ("pg": PackedPoseGraph), bundle-adjustment ("ba":
PackedBA, with camera-camera Between costs, so ``cc_tensors`` is packed too) and generic ("generic": PackedEuclidean) packers --
the three users of theseus_amd/packer_base.py."""
import ast

import pytest
import torch

from tests.helpers import load_golden

KINDS = ["pg", "ba", "generic"]


class _Case:
    """One objective + LevenbergMarquardt + layer, the auxiliary tensors a test edits and how (``edit`` in place, ``undo`` returns
    the restored VALUES), and the optimizer kwargs of every forward()."""

    def __init__(self, kind, iters):
        import theseus_amd as th
        from tests.oracle_kernels import OracleKernels
        lm = dict(linearization_kwargs=dict(kernels=OracleKernels()), max_iterations=iters, abs_err_tolerance=0.0,
                  rel_err_tolerance=0.0)
        self.kind, self.okw = kind, dict(damping=1e-3)
        if kind == "pg":
            from tests.test_gpu_lm import build_objective
            self.obj, _ = build_objective(th, load_golden("pg_f64_lm"), device="cpu")
            self.aux = [c.weight.diagonal.tensor for c in self.obj.cost_functions.values() if hasattr(c.weight, "diagonal")]
            self.edit, self.undo = (lambda t: t.mul_(3.0)), (lambda t: t.detach() / 3.0)
            packer = "PackedPoseGraph"
        elif kind == "ba":
            from tests.ba_common import build_ba_objective
            g = load_golden("ba_f64_camcam_lm")
            self.obj, _, _ = build_ba_objective(th, g, device="cpu")
            kw = ast.literal_eval(str(g["opt_kwargs"]))
            self.okw = {k: v for k, v in kw.items() if k not in ("gauss_newton", "max_iterations", "step_size")}
            costs = [getattr(c, "cost_function", c) for c in self.obj.cost_functions.values()]   # (inside a RobustCostFunction)
            self.aux = [c.image_feature_point.tensor for c in costs if hasattr(c, "image_feature_point")]
            self.edit, self.undo = (lambda t: t.add_(5.0)), (lambda t: t.detach() - 5.0)
            packer = "PackedBA"
        else:
            self.obj = _two_cost_objective(th)
            self.aux = [v.tensor for c in self.obj.cost_functions.values() for v in c.aux_vars()]
            self.edit, self.undo = (lambda t: t.add_(1.0)), None   # (evaluated by torch on the live tensors: nothing to stamp)
            packer = "PackedEuclidean"
        assert self.aux
        self.opt = th.LevenbergMarquardt(self.obj, **lm)
        self.layer = th.TheseusLayer(self.opt)
        self.packed = self.opt.linear_solver.linearization.packed
        assert type(self.packed).__name__ == packer
        if kind == "ba":
            assert type(self.opt.linear_solver).__name__ == "HipSchurSolver" and self.packed.cc_costs
        self.start = {k: v.tensor.clone() for k, v in self.obj.optim_vars.items()}

    def forward(self, inputs=None, **kw):
        return self.layer.forward(inputs, optimizer_kwargs=dict(self.okw, **kw))


def _two_cost_objective(th):
    """The objective of tests/test_generic_host.py::test_generic_linearization_matches_torch_on_a_two_cost_objective, at a
    random start."""
    dt, B = torch.float64, 5
    gen = torch.Generator().manual_seed(3)
    u, w = th.Vector(2, name="u", dtype=dt), th.Vector(3, name="w", dtype=dt)
    d1 = th.Variable(torch.randn(B, 4, dtype=dt, generator=gen), name="d1")
    d2 = th.Variable(torch.randn(1, 3, dtype=dt, generator=gen), name="d2")

    def f1(optim_vars, aux_vars):    # (B, 4): mixes u and w
        uu, ww = optim_vars[0].tensor, optim_vars[1].tensor
        return torch.cat([uu * ww[:, :2], torch.sin(uu) + ww[:, 2:]], 1) - aux_vars[0].tensor

    def f2(optim_vars, aux_vars):    # (B, 3): w only
        return optim_vars[0].tensor ** 2 - aux_vars[0].tensor
    obj = th.Objective(dtype=dt)
    obj.add(th.AutoDiffCostFunction([u, w], f1, 4, aux_vars=[d1], cost_weight=th.ScaleCostWeight(torch.tensor(2.0, dtype=dt)), name="c1"))
    obj.add(th.AutoDiffCostFunction([w], f2, 3, aux_vars=[d2], cost_weight=th.DiagonalCostWeight(torch.tensor([[1.0, 0.5, 2.0]], dtype=dt)), name="c2"))
    obj.update({"u": torch.randn(B, 2, dtype=dt, generator=gen), "w": torch.randn(B, 3, dtype=dt, generator=gen)})
    return obj


@pytest.mark.parametrize("kind", KINDS)
def test_in_place_edit_and_restored_storage_of_auxiliary_tensors_are_seen(kind):
    """An auxiliary tensor edited IN PLACE (no Variable.update(): only its version counter moves) changes the next forward(); the
    values put back through ``t.data = ...`` (object and version counter stay, only the storage moves) give the first run's
    errors again."""
    c = _Case(kind, iters=1)
    _, info1 = c.forward(None, track_err_history=True)
    with torch.no_grad():
        for t in c.aux:
            c.edit(t)
    _, info2 = c.forward(c.start, track_err_history=True)
    e1, e2 = info1.err_history[:, 0], info2.err_history[:, 0]
    if kind == "pg":
        assert (e2 > 5.0 * e1).all(), (e1, e2)   # Between errors carry w^2 = 9x; the priors keep theirs
    assert (e2 != e1).all(), (e1, e2)
    if c.undo is None:
        return
    for t in c.aux:
        ver = t._version
        t.data = c.undo(t)
        assert t._version == ver
    _, info3 = c.forward(c.start, track_err_history=True)
    assert torch.allclose(info3.err_history[:, 0], e1, rtol=1e-12, atol=0), (e1, info3.err_history[:, 0])


@pytest.mark.parametrize("kind", KINDS)
def test_a_second_forward_does_not_overwrite_the_first_solution(kind):
    c = _Case(kind, iters=4)
    sol1, _ = c.forward(None)
    keep = {k: v.clone() for k, v in sol1.items()}
    sol2, _ = c.forward(None)                       # continues from sol1, no update() in between
    for k in keep:
        assert torch.equal(sol1[k], keep[k]), k     # sol1's tensors were not used as scratch
    assert any(not torch.equal(sol2[k], keep[k]) for k in keep)


@pytest.mark.parametrize("kind", KINDS)
def test_exception_inside_optimize_does_not_poison_the_next_forward(kind):
    c = _Case(kind, iters=3)
    c.forward(None)                                 # state buffer handed out -> the next optimize privatizes

    def raising_complete_step(*a, **k):
        raise RuntimeError("kernel error stand-in")
    orig = c.opt._complete_step
    c.opt._complete_step = raising_complete_step
    with pytest.raises(RuntimeError, match="stand-in"):
        c.forward(None)
    c.opt._complete_step = orig
    assert not c.packed._vars_stale
    _, info = c.forward(c.start, track_err_history=True)
    _, fresh = _Case(kind, iters=3).forward(None, track_err_history=True)
    assert torch.allclose(info.err_history, fresh.err_history, rtol=1e-12, atol=0)


def test_ba_repointings_per_forward_and_the_inputs_are_never_written():
    """The bundle-adjustment packer does not defer its first re-pointing (PackedPoseGraph does: tests/test_host_state.py): at most
    TWO per forward(inputs) -- to the packed copy of the inputs, and to the final state.  The caller's tensors keep their values."""
    c = _Case("ba", iters=3)
    c.forward(None)                                 # (first call: packs, builds the structure)
    calls = {"n": 0}
    orig = c.packed._repoint_variables

    def counted():
        calls["n"] += 1
        return orig()
    c.packed._repoint_variables = counted
    inputs = {k: v.clone() for k, v in c.start.items()}
    sol, _ = c.forward(inputs)
    assert 1 <= calls["n"] <= 2
    for k, v in inputs.items():
        assert torch.equal(v, c.start[k])           # never written into
        assert sol[k] is c.obj.optim_vars[k].tensor
    assert any(not torch.equal(sol[k], c.start[k]) for k in sol)   # (the loop moved)
