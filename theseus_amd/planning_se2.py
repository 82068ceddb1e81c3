"""The SE2 motion planner (the reference's MotionPlanner with pose_type=SE2, examples/se2_planning.py): the packed representation of
an objective whose optimisation variables are SE2 poses AND Vector(3) velocities and whose costs are the planner's seven kinds --
Collision2D on SE2, GPMotionModel (SE2, Vector, SE2, Vector) with a GPCostWeight, Nonholonomic on SE2, HingeCost on Vector(3),
Difference on SE2, Difference on Vector(3) and XYDifference (theseus_amd/embodied.py), all but the GP kind with a Scale /
DiagonalCostWeight.

State: ONE tensor (V, B, 4) in the objective's variable order.  An SE2 is its record of csrc/lie_se2.cuh, a velocity is
(v0, v1, v2, 0): its variable's tensor is the (B, 3) view ``state[k][:, :3]``; the pad element is written 0 by ``_pack`` and by the
retraction and never read by a kernel.  Tangent columns of variable k: 3k ... 3k + 2.  Retraction is thx_trajse2_retract (SE2 records
as thx_se2_retract, velocity records x + step * delta), the masked copies thx_copy_where.

Non-differentiated path (under no_grad, or nothing tracked requires grad): ``assemble`` = thx_trajse2_eval into persistent block
buffers + thx_block_assemble on them, ``error_metric`` = thx_trajse2_error; no cost function is evaluated by torch.
``backward_mode="implicit"``: PackedState.implicit_step on the torch classes, retracting with se2_torch.retract / a plain add.
``"unroll"`` / ``"truncated"`` with something to differentiate are refused by the optimizer (no ``unrolled_step`` here).
``fused = False``: the same class on the torch classes (tools/bench_trajse2.py's baseline).
"""
from typing import Optional

import numpy as np
import torch

from . import _lib, se2_torch
from .euclidean import _is_euclidean
from .generic import PackedState, _names
from .kernels import default_kernels, fast_approx_local_jacobians
from .term_table import TermKind, TermTable, term_dtype, weight_var

TRAJSE2_TERM = term_dtype("var")

_KINDS_MESSAGE = ("HIP backend, fused SE2 motion planning: every optimisation variable must be an SE2 or a Vector of dof 3 and every "
                  "cost one of seven kinds: Collision2D on SE2, GPMotionModel (SE2, Vector, SE2, Vector) with a GPCostWeight, "
                  "Nonholonomic on SE2, HingeCost on Vector(3), Difference on SE2, Difference on Vector(3) or XYDifference -- all but "
                  "the GPMotionModel with a Scale / DiagonalCostWeight.")


def _is_se2(v) -> bool:
    return "SE2" in _names(v)


def _is_vec3(v) -> bool:
    return _is_euclidean(v) and v.dof() == 3


def _trajse2_kind(c):
    """THX_TRAJSE2_* of a cost function the fused kernels cover, else None."""
    names, w = _names(c), _names(c.weight)
    if "GPMotionModel" in names:
        ok = "GPCostWeight" in w and _is_se2(c.pose1) and _is_se2(c.pose2) and _is_vec3(c.vel1) and _is_vec3(c.vel2)
        return _lib.TRAJSE2_GP if ok else None
    if not ("ScaleCostWeight" in w or "DiagonalCostWeight" in w):
        return None
    if "Collision2D" in names:
        return _lib.TRAJSE2_COLLISION if _is_se2(c.pose) else None
    if "Nonholonomic" in names:
        return _lib.TRAJSE2_NONHOLONOMIC if _is_se2(c.pose) and _is_vec3(c.vel) else None
    if "HingeCost" in names:
        return _lib.TRAJSE2_HINGE if _is_vec3(c.vector) else None
    if "XYDifference" in names:
        return _lib.TRAJSE2_PRIOR_XY
    if "Difference" in names:
        return _lib.TRAJSE2_PRIOR_SE2 if _is_se2(c.var) else (_lib.TRAJSE2_PRIOR_VEC if _is_vec3(c.var) else None)
    return None


class PackedTrajectorySE2(TermTable, PackedState):
    group = "SE2+R3"
    family = "SE2 motion planning"

    _TERM, _TANGENT = TRAJSE2_TERM, 3
    _KINDS = {
        _lib.TRAJSE2_COLLISION: TermKind(lambda c: [(c.sdf_data, None), (c.sdf_origin, 2), (c.sdf_cell_size, 1), (c.cost_eps, 1),
                                                    (weight_var(c), 1)], grid=0, wdim=1),
        _lib.TRAJSE2_GP: TermKind(lambda c: [(c.dt, 1), (c.weight.dt, 1), (c.weight.Qc_inv, 9)]),
        _lib.TRAJSE2_NONHOLONOMIC: TermKind(lambda c: [(weight_var(c), 1)], wdim=1),
        _lib.TRAJSE2_HINGE: TermKind(lambda c: [(c.down_limit, 3), (c.up_limit, 3), (c.threshold, 3), (weight_var(c), None)], weight=3),
        _lib.TRAJSE2_PRIOR_SE2: TermKind(lambda c: [(c.target, 4), (weight_var(c), None)], weight=1),
        _lib.TRAJSE2_PRIOR_VEC: TermKind(lambda c: [(c.target, 3), (weight_var(c), None)], weight=1),
        _lib.TRAJSE2_PRIOR_XY: TermKind(lambda c: [(c.target, 2), (weight_var(c), None)], weight=1),
    }
    _WEIGHT_WIDTHS = ((1, 2, 3), "This cost needs a DiagonalCostWeight of the cost's own dimension.")
    _DIMS = {_lib.TRAJSE2_COLLISION: 1, _lib.TRAJSE2_GP: 6, _lib.TRAJSE2_NONHOLONOMIC: 1, _lib.TRAJSE2_HINGE: 3,
             _lib.TRAJSE2_PRIOR_SE2: 3, _lib.TRAJSE2_PRIOR_VEC: 3, _lib.TRAJSE2_PRIOR_XY: 2}

    def __init__(self, objective, kernels=None, order=None):
        from .packed import UnsupportedObjective
        if not hasattr(kernels or default_kernels(), "trajse2_eval"):
            raise UnsupportedObjective("these kernels have no fused SE2 motion-planning evaluation")
        super().__init__(objective, kernels, order)

    def _check(self):
        from .packed import UnsupportedObjective
        self.kinds = [_trajse2_kind(c) for c in self.costs]
        if (not self.vars or any(not (_is_se2(v) or _is_vec3(v)) for v in self.vars) or not self.kinds
                or any(k is None for k in self.kinds)):
            raise UnsupportedObjective(_KINDS_MESSAGE)
        if not any(_is_se2(v) for v in self.vars):   # (all-Euclidean objectives keep going to PackedEuclidean)
            raise UnsupportedObjective("HIP backend, fused SE2 motion planning: no optimisation variable is an SE2.")
        if _lib.TRAJSE2_PRIOR_SE2 in self.kinds and fast_approx_local_jacobians():
            raise UnsupportedObjective("HIP backend, fused SE2 motion planning: fast_approx_local_jacobians=True is not fused into the "
                                       "kernels.")
        self.var_kind = np.array([0 if _is_se2(v) else 1 for v in self.vars], np.uint8)   # thx_trajse2_retract's: 0 SE2, 1 vector
        self._var_kind_dev = None

    def _sync_aux(self, deep: bool = False):
        """... and a Scale / Diagonal weight is as wide as 1 or as the cost: the dims of this family are 1, 2 and 3."""
        table = self._table
        super()._sync_aux(deep)
        if self._table is not table:
            for c, k in zip(self.costs, self.kinds):
                kind = self._KINDS[k]
                if kind.weight is not None and weight_var(c).tensor[0].numel() not in (1, self._DIMS[k]):
                    self._table = None
                    raise ValueError(f"This cost needs a {self._DIMS[k]}-dimensional DiagonalCostWeight.")

    # ---- the (V, B, 4) layout ------------------------------------------------------------------------------------------------
    def _pack(self):
        obj = self.objective
        obj._resolve_batch_size()
        B = obj.batch_size
        with torch.no_grad():
            first = self.vars[0].tensor
            state = torch.zeros(len(self.vars), B, 4, dtype=first.dtype, device=first.device)
            for k, v in enumerate(self.vars):
                state[k, :, :v.tensor.shape[1]] = v.tensor   # (a velocity leaves the pad element 0)
            self._state = state
        self._repoint_variables()

    def _var_view(self, state, k):
        return state[k] if self.var_kind[k] == 0 else state[k][:, :3]

    def _kinds_on(self, device):
        if self._var_kind_dev is None or self._var_kind_dev.device != device:
            self._var_kind_dev = torch.from_numpy(self.var_kind).to(device)
        return self._var_kind_dev

    @property
    def batch(self):
        return self._state.shape[1]

    def keep_where(self, mask, out):
        self.K.copy_where(mask, self._state, out)

    def copy_where(self, mask, src, dst):
        self.K.copy_where(mask, src, dst)

    def solution_dict(self, state):
        return {v.name: self._var_view(state, k).cpu() for k, v in enumerate(self.vars)}

    def history_dict(self, hist, dtype):
        """(K + 1, V, B, 4) states -> name -> (B, 4 | 3, K + 1) on the host (nonlinear_optimizer.py:150-163)."""
        h = hist.to(dtype).cpu()
        return {v.name: h[:, k, :, :4 - int(self.var_kind[k])].movedim(0, -1).contiguous() for k, v in enumerate(self.vars)}

    def retract(self, delta: torch.Tensor, step: float, ignore_mask: Optional[torch.Tensor], out: torch.Tensor):
        """out = state (+) step * delta (rows of ``ignore_mask`` keep the state): thx_trajse2_retract"""
        self.sync()
        self.K.trajse2_retract(self._state, self._kinds_on(self._state.device), delta, step, self._mask_u8(ignore_mask), out)
        return out

    def _implicit_retract(self, X, delta):
        V, B = X.shape[:2]
        d = delta.view(B, V, 3).permute(1, 0, 2)
        poses, vels = np.flatnonzero(self.var_kind == 0), np.flatnonzero(self.var_kind == 1)
        pi, vi = (torch.from_numpy(i).to(X.device) for i in (poses, vels))
        moved = se2_torch.retract(X[pi].reshape(-1, 4), d[pi].reshape(-1, 3)).view(len(poses), B, 4)
        added = torch.cat([X[vi][:, :, :3] + d[vi], torch.zeros_like(X[vi][:, :, 3:])], dim=2)   # (the pad element stays 0)
        back = torch.from_numpy(np.argsort(np.concatenate([poses, vels]))).to(X.device)
        return torch.cat([moved, added], dim=0)[back]

    # ---- the fused evaluation (theseus_amd/term_table.py) ----------------------------------------------------------------------
    def _term_vars(self, c):
        return self.cost_vars[c]   # (variable indices)

    def _launch_eval(self, state):
        self.K.trajse2_eval(self._table, len(self.costs), state, self._J, self.j_total, self._e)

    def _launch_error(self, state, err):
        self.K.trajse2_error(self._table, len(self.costs), state, err)

    def _cost_error(self, c):
        if "Difference" in _names(c) and _is_se2(c.var):   # (its error() is a kernel of its own, outside autograd)
            return c.weighted_jacobians_error()[1]
        return c.weighted_error()

    def error_vector(self, state=None):
        if self._differentiated() or not self.fused:
            return super().error_vector(state)
        self._eval(state)
        return self._e

    def assemble(self, H: torch.Tensor, g: torch.Tensor, graph: bool = False):
        """H (lower blocks) and g.  ``graph``: the blocks come from the torch classes, g is ALSO returned as a differentiable
        function of whatever they depend on (the implicit step); H stays outside autograd."""
        if fast_approx_local_jacobians() and _lib.TRAJSE2_PRIOR_SE2 in self.kinds:
            raise NotImplementedError("HIP backend, fused SE2 motion planning: fast_approx_local_jacobians=True is not fused into the "
                                      "kernels.")
        if graph:   # (always the torch classes, whether or not anything requires grad)
            return PackedState.assemble(self, H, g, True)
        return super().assemble(H, g)
