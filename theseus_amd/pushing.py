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
from typing import List, Optional

import numpy as np
import torch

from . import _lib, se2_torch
from .core import Objective, Variable
from .generic import BlockAssembler
from .kernels import default_kernels, fast_approx_local_jacobians, round_up

PUSH2_TERM = np.dtype([("kind", "<i4"), ("row0", "<i4"), ("pose", "<i4", (4,)), ("rows", "<i4"), ("cols", "<i4"), ("j_off", "<i8"),
                       ("aux", "<u8", (5,)), ("aux_bstride", "<i8", (5,)), ("wdim", "<i4"), ("pad", "<i4")])
assert PUSH2_TERM.itemsize == 128


def _names(obj):
    return {c.__name__ for c in type(obj).__mro__}


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


class PackedPlanarPushing:
    group = "SE2"
    family = "planar pushing (SE2)"
    own_implicit_step = True    # the optimizer's implicit last step is ``implicit_step`` below

    def __init__(self, objective: Objective, kernels=None, order=None):
        from .packed import UnsupportedObjective
        self.objective = objective
        self.K = kernels or default_kernels()
        if not hasattr(self.K, "push2_eval"):
            raise UnsupportedObjective("these kernels have no fused planar-pushing evaluation")
        self.order = tuple(order) if order is not None else tuple(objective.optim_vars.keys())
        if sorted(self.order) != sorted(objective.optim_vars.keys()):
            raise ValueError("the variable ordering must hold every optimisation variable of the objective exactly once")
        self.vars: List[Variable] = [objective.optim_vars[name] for name in self.order]
        self.costs = list(objective.cost_functions.values())
        self.kinds = [_push2_kind(c) for c in self.costs]
        if (not self.vars or any("SE2" not in _names(v) for v in self.vars) or not self.kinds
                or any(k is None for k in self.kinds)):
            raise UnsupportedObjective("HIP backend, fused planar pushing: every optimisation variable must be an SE2 and every cost a "
                                       "QuasiStaticPushingPlanar, MovingFrameBetween, EffectorObjectContactPlanar or Difference on SE2 "
                                       "with a Scale / DiagonalCostWeight.")
        if _lib.PUSH2_PRIOR in self.kinds and fast_approx_local_jacobians():
            raise UnsupportedObjective("HIP backend, fused planar pushing: fast_approx_local_jacobians=True is not fused into the "
                                       "kernels.")
        V = len(self.vars)
        self.cols = [(3 * k, 3) for k in range(V)]
        self.n, self.m = 3 * V, objective.dim()
        self.ld = round_up(self.n, 32)
        index = {v.name: k for k, v in enumerate(self.vars)}
        self.cost_vars = [[index[v.name] for v in c.optim_vars()] for c in self.costs]
        self.asm = BlockAssembler(self.cols, self.cost_vars, [c.dim() for c in self.costs])
        rows, r, joff, j = [], 0, [], 0
        for c, vs in zip(self.costs, self.cost_vars):
            rows.append(r)
            joff.append(j)
            r += c.dim()
            j += 3 * c.dim() * len(vs)
        self.rows, self.joff, self.j_total = rows, joff, j
        self.term_order = sorted(range(len(self.costs)), key=lambda c: self.kinds[c])   # (stable: by kind, then the objective's order)
        self.version = objective.current_version
        self.fused = True           # False: the same packed class on the torch classes (tools/bench_push2.py's baseline)
        self._state: Optional[torch.Tensor] = None
        self._views = None
        self._vars_stale = False
        self._state_exposed = False
        self._keep_graph_tensors = False
        self._defer_repoint = False
        self._blocks = None
        self._aux_refs = self._aux_key = self._table = None
        self._aux_stamp = -1
        self._J = self._e = self._Jv = self._ev = None
        self._asm_cache = {}

    # ---- state <-> variables -------------------------------------------------------------------------------------------------
    def _tracked(self):
        yield from self.vars
        seen = set()
        for c in self.costs:
            for a in c.aux_vars():
                if id(a) not in seen:
                    seen.add(id(a))
                    yield a

    def _pack(self):
        obj = self.objective
        obj._resolve_batch_size()
        B = obj.batch_size
        with torch.no_grad():
            self._state = torch.stack([v.tensor if v.tensor.shape[0] == B else v.tensor.expand(B, -1) for v in self.vars],
                                      dim=0).contiguous()
        self._repoint()

    def _repoint(self):
        with torch.set_grad_enabled(self._state.requires_grad):
            self._views = self._state.unbind(0)
        for v, t in zip(self.vars, self._views):
            v._tensor = t
        self._vars_stale = False
        self._state_exposed = True

    def sync(self, force: bool = False, deep: bool = False):
        """Re-pack when somebody replaced a variable's tensor, rebuild the term table when an auxiliary tensor was replaced."""
        if self._state is None or force:
            self._pack()
        elif not self._vars_stale:
            self.objective._resolve_batch_size()
            if any(v.tensor is not t for v, t in zip(self.vars, self._views)) or self._state.shape[1] != self.objective.batch_size:
                self._pack()
        self._sync_aux(deep or force)

    def privatize_state(self):
        if self._state_exposed:
            with torch.no_grad():
                self._state = self._state.detach().clone()
            self._state_exposed = False
            self._vars_stale = True

    def flush_variables(self):
        if self._vars_stale and self._state is not None:
            self._repoint()

    @property
    def state(self):
        return self._state

    @property
    def device(self):
        return self._state.device

    @property
    def batch(self):
        return self._state.shape[1]

    @property
    def optim_variables(self):
        return self.vars

    def alloc_state(self):
        return torch.empty_like(self._state)

    def clone_state(self):
        return self._state.clone()

    def swap_state(self, new, repoint: bool = False):
        old = self._state
        self._state = new
        if repoint:
            self._repoint()
        else:
            self._vars_stale = True
        return old

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
        m = None
        if ignore_mask is not None:
            m = ignore_mask if ignore_mask.dtype == torch.uint8 else ignore_mask.to(torch.uint8)
        self.K.retract(self._state, delta, step, m, out)
        return out

    # ---- the term table ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _weight_var(c):
        return c.weight.scale if "ScaleCostWeight" in _names(c.weight) else c.weight.diagonal

    def _term_aux(self, c, kind):
        """[(variable, elements per problem | None)] in the aux slot order of include/theseus_hip.h"""
        w = self._weight_var(c)
        if kind == _lib.PUSH2_QSP:
            return [(c.c_square, 1), (w, None)]
        if kind == _lib.PUSH2_MFB:
            return [(c.measurement, 4), (w, None)]
        if kind == _lib.PUSH2_CONTACT:
            return [(c.sdf_data, None), (c.sdf_origin, 2), (c.sdf_cell_size, 1), (c.eff_radius, 1), (w, 1)]
        return [(c.target, 4), (w, None)]

    def _sync_aux(self, deep: bool = False):
        if self._table is not None and not deep and self._aux_stamp == Variable._global_updates:
            return
        dev, dt, B = self._state.device, self._state.dtype, self._state.shape[1]
        aux = [self._term_aux(c, k) for c, k in zip(self.costs, self.kinds)]
        tensors = [[a.tensor for a, _ in ts] for ts in aux]
        key = tuple((id(t), t.data_ptr(), t.shape[0], t.stride(0)) for ts in tensors for t in ts) + (str(dev), B)
        self._aux_stamp = Variable._global_updates
        if self._table is not None and key == self._aux_key:
            return
        table = np.zeros(len(self.costs), PUSH2_TERM)
        refs = []
        for slot, c in enumerate(self.term_order):
            cost, kind, ts = self.costs[c], self.kinds[c], tensors[c]
            row = table[slot]
            row["kind"], row["row0"], row["j_off"] = kind, self.rows[c], self.joff[c]
            row["pose"] = self.cost_vars[c] + [-1] * (4 - len(self.cost_vars[c]))
            for k, (t, (_, width)) in enumerate(zip(ts, aux[c])):
                per = t[0].numel()
                if t.device != dev or t.dtype != dt:
                    raise RuntimeError(f"{cost.name}: an auxiliary tensor lives on {t.device} / {t.dtype}, the state on {dev} / {dt}; "
                                       "there is no CPU fallback")
                if t.shape[0] not in (1, B) or (width is not None and per != width):
                    raise ValueError(f"{cost.name}: auxiliary tensor of shape {tuple(t.shape)} does not fit batch {B}")
                td = t.detach()
                bstride = per
                if td[0].is_contiguous():
                    # one problem's values are dense: a (B, 4) slice of a batched tensor (a learned measurement) is read in place
                    # through its own batch stride
                    bstride = td.stride(0)
                elif not td.is_contiguous():
                    td = td.contiguous()
                    key = None   # (a private copy: look again at the next call)
                refs.append(td)
                row["aux"][k], row["aux_bstride"][k] = td.data_ptr(), bstride if t.shape[0] > 1 else 0
            if kind == _lib.PUSH2_CONTACT:
                if ts[0].ndim != 3:
                    raise ValueError(f"{cost.name}: sdf_data of shape {tuple(ts[0].shape)} is not a batch of grids")
                row["rows"], row["cols"], row["wdim"] = ts[0].shape[1], ts[0].shape[2], 1
            else:
                wdim = ts[1][0].numel()
                if wdim not in (1, 3):
                    raise ValueError("This cost needs a 3-dimensional DiagonalCostWeight.")
                row["wdim"] = wdim
        self._table = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(dev)
        self._aux_refs, self._aux_key = (tensors, refs), key
        if key is None:
            self._aux_stamp = -1

    def _buffers(self):
        B, dev, dt = self.batch, self._state.device, self._state.dtype
        if self._J is None or self._e.shape[0] != B or self._e.device != dev or self._e.dtype != dt:
            self._J = torch.zeros(self.j_total * B, dtype=dt, device=dev)
            self._e = torch.zeros(B, self.m, dtype=dt, device=dev)
            self._Jv, self._ev = [], []
            for c, cost in enumerate(self.costs):
                d, o = cost.dim(), self.joff[c]
                self._Jv.append([self._J[(o + 3 * d * s) * B:(o + 3 * d * (s + 1)) * B].view(B, d, 3)
                                 for s in range(len(self.cost_vars[c]))])
                self._ev.append(self._e[:, self.rows[c]:self.rows[c] + d])
            self._asm_cache = {}

    def _differentiated(self) -> bool:
        return torch.is_grad_enabled() and any(v.tensor.requires_grad for v in self._tracked())

    def _eval(self, state=None):
        """thx_push2_eval at ``state`` (default: the current one) -> (Jacobian block views, error views) of the persistent buffers"""
        self.sync()
        self._buffers()
        self.K.push2_eval(self._table, len(self.costs), self._state if state is None else state, self._J, self.j_total, self._e)
        return self._Jv, self._ev

    # ---- evaluation by the torch classes (the differentiated path) -------------------------------------------------------------
    class _at:
        """Context: the variables' tensors are the (B, 4) slices of ``state`` while the cost functions are evaluated."""

        def __init__(self, packed, state):
            self.p, self.state = packed, state

        def __enter__(self):
            self.saved = [v.tensor for v in self.p.vars]
            for k, v in enumerate(self.p.vars):
                v._tensor = self.state[k]

        def __exit__(self, *a):
            for v, t in zip(self.p.vars, self.saved):
                v._tensor = t

    def _torch_blocks(self, state=None):
        self.sync()
        Js, es = [], []
        with self._at(self, self._state if state is None else state):
            for c in self.costs:
                jac, err = c.weighted_jacobians_error()
                Js.append([j.contiguous() for j in jac])
                es.append(err.contiguous())
        return Js, es

    def weighted_blocks(self):
        """[(Jacobian blocks (B|1, dim, 3) per optimisation variable of the cost), ...], [weighted error (B|1, dim), ...]"""
        if self._differentiated() or not self.fused:
            return self._torch_blocks()
        return self._eval()

    def error_vector(self, state=None):
        if self._differentiated() or not self.fused:
            self.sync()
            with self._at(self, self._state if state is None else state):
                B = self.batch
                return torch.cat([c.weighted_jacobians_error()[1].expand(B, -1) for c in self.costs], dim=1)
        self._eval(state)
        return self._e

    def error_metric(self, state=None, out: Optional[torch.Tensor] = None, poses=None):
        self.sync()
        x = state if state is not None else (poses if poses is not None else self._state)
        if not self.fused:
            with torch.no_grad():
                err = (self.error_vector(x.detach()) ** 2).sum(dim=1) / 2
            if out is not None:
                out.copy_(err)
                return out
            return err
        err = out if out is not None else torch.empty(x.shape[1], dtype=x.dtype, device=x.device)
        self.K.push2_error(self._table, len(self.costs), x.detach(), err)
        return err

    def assemble(self, H: torch.Tensor, g: torch.Tensor, graph: bool = False):
        """H (lower blocks) and g.  ``graph``: the blocks come from the torch classes, g is ALSO returned as a differentiable
        function of whatever they depend on (the implicit step); H stays outside autograd."""
        if fast_approx_local_jacobians() and _lib.PUSH2_PRIOR in self.kinds:
            raise NotImplementedError("HIP backend, fused planar pushing: fast_approx_local_jacobians=True is not fused into the kernels.")
        if not graph and self.fused:
            Jv, ev = self._eval()
            self.K.block_assemble_strided(self.asm, Jv, ev, H, g, self._asm_cache)
            self._blocks = (Jv, ev)
            return None
        Js, es = self._torch_blocks()
        B = self.batch
        Jd = [[j.detach().expand(B, -1, -1).contiguous() for j in J] for J in Js]
        ed = [e.detach().expand(B, -1).contiguous() for e in es]
        self.asm.assemble(self.K, Jd, ed, H, g)
        self._blocks = (Jd, ed)
        if not graph:
            return None
        parts = [None] * len(self.vars)
        for c, (J, e) in enumerate(zip(Js, es)):
            for s, k in enumerate(self.cost_vars[c]):
                term = -(J[s].transpose(1, 2) @ e.unsqueeze(2)).squeeze(2)
                parts[k] = term if parts[k] is None else parts[k] + term
        return torch.cat([(p.expand(B, -1) if p is not None else torch.zeros(B, 3, dtype=H.dtype, device=H.device)) for p in parts],
                         dim=1)

    def supports_block_hessian(self) -> bool:
        return False

    def jacobian_blocks(self):
        return self._blocks[0] if self._blocks is not None else self.weighted_blocks()[0]

    def jacobian_times(self, blocks, v: torch.Tensor) -> torch.Tensor:
        """A v (B, m) from the per-cost blocks (Dogleg / trust-region ratio: dense_linearization.py:73-74)."""
        out = torch.zeros(v.shape[0], self.m, dtype=v.dtype, device=v.device)
        for c, J in enumerate(blocks):
            r, d = self.rows[c], self.costs[c].dim()
            for s, k in enumerate(self.cost_vars[c]):
                out[:, r:r + d] += (J[s] @ v[:, 3 * k:3 * k + 3].unsqueeze(2)).squeeze(2)
        return out

    def dense_A_b(self):
        """Dense A (B, m, n), b (B, m) -- tests / foreign consumers only."""
        Js, es = self.weighted_blocks()
        B = self.batch
        A = torch.zeros(B, self.m, self.n, dtype=self._state.dtype, device=self._state.device)
        b = torch.zeros(B, self.m, dtype=self._state.dtype, device=self._state.device)
        for c, (J, e) in enumerate(zip(Js, es)):
            r, d = self.rows[c], self.costs[c].dim()
            for s, k in enumerate(self.cost_vars[c]):
                A[:, r:r + d, 3 * k:3 * k + 3] = J[s]
            b[:, r:r + d] = -e
        return A, b

    # ---- BackwardMode.IMPLICIT -------------------------------------------------------------------------------------------------
    def implicit_step(self, opt, step: float, kwargs):
        from .euclidean import _CachedFactorSolve
        lin = opt.linear_solver.linearization
        self.flush_variables()
        lin._ensure_buffers()
        g_graph = self.assemble(lin._H, lin.g, graph=True)
        lin._after_assemble()
        X = self._state.detach()
        V, B = X.shape[:2]
        delta = _CachedFactorSolve.apply(opt, kwargs, g_graph)
        d = (float(step) * delta).view(B, V, 3).permute(1, 0, 2).reshape(V * B, 3)
        return se2_torch.retract(X.view(V * B, 4), d).view(V, B, 4), delta
