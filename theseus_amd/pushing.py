"""Planar pushing on SE2 (the pose estimator of the reference's examples/tactile_pose_estimation.py): the packed representation of an
objective whose optimisation variables are all SE2 and whose costs are QuasiStaticPushingPlanar, MovingFrameBetween,
EffectorObjectContactPlanar (theseus_amd/embodied.py) and Difference priors, each with a Scale / DiagonalCostWeight.

State: pose-major (V, B, 4), the SE2 record of csrc/lie_se2.cuh -- retraction is thx_se2_retract, the masked copies thx_copy_where,
the variables' tensors are the (B, 4) slices.  Tangent columns of variable k: 3k ... 3k + 2.

Non-differentiated path (under no_grad, or nothing tracked requires grad): ``assemble`` = thx_push2_eval into persistent block
buffers + thx_block_assemble on them, ``error_metric`` = thx_push2_error; no cost function is evaluated by torch.
``backward_mode="implicit"``: the last step evaluates the torch classes at the detached state with the graph, forms g by torch,
H from the detached blocks on the kernels, solves through the cached factor and retracts with the torch SE2 functions.
``"unroll"`` / ``"truncated"`` with something to differentiate are refused by the optimizer (no ``unrolled_step`` here).
"""
from typing import Optional

import torch

from . import _lib, se2_torch
from .generic import PackedState, _names
from .kernels import default_kernels, fast_approx_local_jacobians
from .term_table import TermKind, TermTable, term_dtype, weight_var

PUSH2_TERM = term_dtype("pose")


def _push2_kind(c):
    """THX_PUSH2_* of a cost function the fused kernels cover, else None."""
    names, w = _names(c), _names(c.weight)
    if not ("ScaleCostWeight" in w or "DiagonalCostWeight" in w):
        return None
    for cls, kind in (("QuasiStaticPushingPlanar", _lib.PUSH2_QSP), ("MovingFrameBetween", _lib.PUSH2_MFB),
                      ("EffectorObjectContactPlanar", _lib.PUSH2_CONTACT)):
        if cls in names:
            return kind
    if "Difference" in names and "SE2" in _names(c.var):
        return _lib.PUSH2_PRIOR
    return None


class PackedPlanarPushing(TermTable, PackedState):
    group = "SE2"
    family = "planar pushing (SE2)"

    _TERM, _TANGENT = PUSH2_TERM, 3
    _KINDS = {
        _lib.PUSH2_QSP: TermKind(lambda c: [(c.c_square, 1), (weight_var(c), None)], weight=1),
        _lib.PUSH2_MFB: TermKind(lambda c: [(c.measurement, 4), (weight_var(c), None)], weight=1),
        _lib.PUSH2_CONTACT: TermKind(lambda c: [(c.sdf_data, None), (c.sdf_origin, 2), (c.sdf_cell_size, 1), (c.eff_radius, 1),
                                                (weight_var(c), 1)], grid=0, wdim=1),
        _lib.PUSH2_PRIOR: TermKind(lambda c: [(c.target, 4), (weight_var(c), None)], weight=1),
    }
    _WEIGHT_WIDTHS = ((1, 3), "This cost needs a 3-dimensional DiagonalCostWeight.")

    def __init__(self, objective, kernels=None, order=None):
        from .packed import UnsupportedObjective
        if not hasattr(kernels or default_kernels(), "push2_eval"):
            raise UnsupportedObjective("these kernels have no fused planar-pushing evaluation")
        super().__init__(objective, kernels, order)

    def _check(self):
        from .packed import UnsupportedObjective
        self.kinds = [_push2_kind(c) for c in self.costs]
        if (not self.vars or any("SE2" not in _names(v) for v in self.vars) or not self.kinds
                or any(k is None for k in self.kinds)):
            raise UnsupportedObjective("HIP backend, fused planar pushing: every optimisation variable must be an SE2 and every cost a "
                                       "QuasiStaticPushingPlanar, MovingFrameBetween, EffectorObjectContactPlanar or Difference on SE2 "
                                       "with a Scale / DiagonalCostWeight.")
        if _lib.PUSH2_PRIOR in self.kinds and fast_approx_local_jacobians():
            raise UnsupportedObjective("HIP backend, fused planar pushing: fast_approx_local_jacobians=True is not fused into the "
                                       "kernels.")

    # ---- the (V, B, 4) layout ------------------------------------------------------------------------------------------------
    def _pack(self):
        obj = self.objective
        obj._resolve_batch_size()
        B = obj.batch_size
        with torch.no_grad():
            self._state = torch.stack([v.tensor if v.tensor.shape[0] == B else v.tensor.expand(B, -1) for v in self.vars],
                                      dim=0).contiguous()
        self._repoint_variables()

    def _var_view(self, state, k):
        return state[k]

    @property
    def batch(self):
        return self._state.shape[1]

    def keep_where(self, mask, out):
        self.K.copy_where(mask, self._state, out)

    def copy_where(self, mask, src, dst):
        self.K.copy_where(mask, src, dst)

    def solution_dict(self, state):
        return {v.name: state[k].cpu() for k, v in enumerate(self.vars)}

    def history_dict(self, hist, dtype):
        """(K + 1, V, B, 4) states -> name -> (B, 4, K + 1) on the host (nonlinear_optimizer.py:150-163)."""
        h = hist.to(dtype).cpu()
        return {v.name: h[:, k].movedim(0, -1).contiguous() for k, v in enumerate(self.vars)}

    def retract(self, delta: torch.Tensor, step: float, ignore_mask: Optional[torch.Tensor], out: torch.Tensor):
        """out = state exp(step * delta) (rows of ``ignore_mask`` keep the state): thx_se2_retract"""
        self.sync()
        self.K.retract(self._state, delta, step, self._mask_u8(ignore_mask), out)
        return out

    def _implicit_retract(self, X, delta):
        V, B = X.shape[:2]
        d = delta.view(B, V, 3).permute(1, 0, 2).reshape(V * B, 3)
        return se2_torch.retract(X.view(V * B, 4), d).view(V, B, 4)

    # ---- the fused evaluation (theseus_amd/term_table.py) ----------------------------------------------------------------------
    def _term_vars(self, c):
        return self.cost_vars[c]   # (pose indices)

    def _launch_eval(self, state):
        self.K.push2_eval(self._table, len(self.costs), state, self._J, self.j_total, self._e)

    def _launch_error(self, state, err):
        self.K.push2_error(self._table, len(self.costs), state, err)

    def _cost_error(self, c):   # (Difference.error() on SE2 is a kernel of its own, outside autograd: the torch Jacobians' error)
        return c.weighted_jacobians_error()[1]

    def error_vector(self, state=None):
        if self._differentiated() or not self.fused:
            return super().error_vector(state)
        self._eval(state)
        return self._e

    def assemble(self, H: torch.Tensor, g: torch.Tensor, graph: bool = False):
        """H (lower blocks) and g.  ``graph``: the blocks come from the torch classes, g is ALSO returned as a differentiable
        function of whatever they depend on (the implicit step); H stays outside autograd."""
        if fast_approx_local_jacobians() and _lib.PUSH2_PRIOR in self.kinds:
            raise NotImplementedError("HIP backend, fused planar pushing: fast_approx_local_jacobians=True is not fused into the kernels.")
        if graph:   # (always the torch classes, whether or not anything requires grad)
            return PackedState.assemble(self, H, g, True)
        return super().assemble(H, g)
