"""The term table of the fused cost families (csrc/term_family.cuh; the families: theseus_amd/embodied.py PackedTrajectory2D on
csrc/traj_kernels.hip, theseus_amd/pushing.py PackedPlanarPushing on csrc/push_kernels.hip, theseus_amd/planning_se2.py PackedTrajectorySE2 on csrc/trajse2_kernels.hip,
theseus_amd/homography.py PackedHomography on csrc/homog_kernels.hip, theseus_amd/kinematics.py PackedKinematics on
csrc/kin_kernels.hip): one 128-byte record per cost function,
sorted by kind, holding where the cost's rows and Jacobian blocks go, which variables it reads and the device pointers of its
auxiliary tensors themselves (an SDF grid shared by every cost is one tensor, stored once).  ``TermTable`` is a mixin for a packed
class (``PackedState`` of theseus_amd/generic.py) whose NON-differentiated evaluation is such a kernel: ``assemble(graph=False)`` =
the family's *_eval into persistent block buffers + thx_block_assemble on them, ``error_metric`` = the family's *_error.  Everything
differentiated is the packed class's own torch path.

A family supplies data and two launches:
  _TERM           its record (``term_dtype``)
  _TANGENT        the tangent width of its variables (every block is (B, dim, _TANGENT)); PackedKinematics sets it per instance
  _KINDS          {kind: TermKind}
  _WEIGHT_WIDTHS  (allowed widths of a Scale / Diagonal weight, the message for any other)
  _term_vars(c)   what goes into the variable field of cost c's record
  _launch_eval(state), _launch_error(state, err)
and sets ``self.kinds`` (one per cost function, objective order) before or in the packed class's constructor.

Optional, the backward of the implicit step (``assemble(graph=True)`` with an auxiliary tensor that requires grad) in kernels too:
  _VJP_KERNEL     the name of the kernel set's method, _VJP_REC the doubles of its per-(term, problem) record
  _VJP_ENTRIES    {kind: the record entry of each aux slot}
  _launch_vjp(table, state, u, rec, plan, grad_out, grid_work)
A family whose gradients are not a handful of record entries per term and 2-D fp64 grids (PackedHomography: feature maps) overrides
``_build_grad_plan`` (-> anything with GradPlan's ``inputs``, ``offsets`` and ``asked()``), ``_vjp`` and, for a gate of its own,
``_fused_backward_route``.  A family without them, or a kernel set without the method, stays on the torch path for everything differentiated."""
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .core import Variable
from .generic import _names

# thx_traj2_grad_pair / thx_traj2_grad_tensor / thx_traj2_grad_grid of include/theseus_hip.h
GRAD_PAIR = np.dtype([("term", "<i4"), ("entry", "<i4")])
GRAD_TENSOR = np.dtype([("pair_begin", "<i4"), ("pair_end", "<i4"), ("count", "<i4"), ("shared", "<i4"), ("out_off", "<i8")])
GRAD_GRID = np.dtype([("term_begin", "<i4"), ("term_end", "<i4"), ("rows", "<i4"), ("cols", "<i4"), ("shared", "<i4"), ("pad", "<i4"),
                      ("out_off", "<i8"), ("work_off", "<i8")])
assert (GRAD_PAIR.itemsize, GRAD_TENSOR.itemsize, GRAD_GRID.itemsize) == (8, 24, 40)


def term_dtype(var_field: str) -> np.dtype:
    """thx_traj2_term / thx_push2_term / thx_trajse2_term / thx_homog_term / thx_kin_term of include/theseus_hip.h; ``var_field``: the family's name of the variable field"""
    dt = np.dtype([("kind", "<i4"), ("row0", "<i4"), (var_field, "<i4", (4,)), ("rows", "<i4"), ("cols", "<i4"), ("j_off", "<i8"),
                   ("aux", "<u8", (5,)), ("aux_bstride", "<i8", (5,)), ("wdim", "<i4"), ("pad", "<i4")])
    assert dt.itemsize == 128
    return dt


def weight_var(c):
    return c.weight.scale if "ScaleCostWeight" in _names(c.weight) else c.weight.diagonal


class TermKind(NamedTuple):
    aux: Callable                  # cost -> [(variable, elements per problem | None)] in the aux slot order of include/theseus_hip.h
    grid: Optional[int] = None     # the aux slot of a (B|1, rows, cols) grid: its shape goes into ``rows`` / ``cols``; of a
                                   # (B|1, channels, rows, cols) one: the channel count also goes into ``pad`` (thx_homog_term.chans)
    wdim: int = 0                  # the record's ``wdim`` ...
    weight: Optional[int] = None   # ... or the aux slot of a Scale / Diagonal weight whose width it is


class GradPlan(NamedTuple):
    """Which record entries of which terms feed the gradient of every DISTINCT auxiliary tensor that requires grad."""
    inputs: list      # the distinct auxiliary tensors, in table order
    offsets: list     # per input: where its gradient starts in the kernel's output, None where none is asked for
    struct: object    # _lib.Traj2GradPlan (counts + the device pointers of ``tables``)
    tables: tuple     # the uploaded tables (kept alive)

    def asked(self):
        return tuple(o is not None for o in self.offsets)


class _FusedGradient(torch.autograd.Function):
    """g as a function of the auxiliary tensors: forward hands over the gradient the kernels formed, backward is the family's VJP
    kernel at the state of the forward.  The state is cloned: the optimiser loop retracts its state buffer in place, so a later
    ``forward()`` on the same objective would otherwise move it under a pending ``backward()``."""

    @staticmethod
    def forward(ctx, packed, g, *inputs):
        ctx.packed, ctx.plan, ctx.table, ctx.refs = packed, packed._grad_plan, packed._table, packed._aux_refs
        ctx.state = packed._state.detach().clone()
        return g.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, u):
        return (None, None) + ctx.packed._vjp(ctx.plan, ctx.table, ctx.state, u.contiguous())


class TermTable:
    fused = True    # False: the same packed class on the torch classes (tools/bench_push2.py's baseline)
    fused_backward = True   # False: the implicit step's backward through the torch classes (tools/bench_traj2_backward.py's baseline)

    def __init__(self, objective, kernels=None, order=None):
        super().__init__(objective, kernels, order)
        kinds = self.kinds
        rows, r, joff, j = [], 0, [], 0
        for c, vs in zip(self.costs, self.cost_vars):
            rows.append(r)
            joff.append(j)
            r += c.dim()
            j += self._TANGENT * c.dim() * len(vs)
        self.rows, self.joff, self.j_total = rows, joff, j
        self.term_order = sorted(range(len(self.costs)), key=lambda c: kinds[c])   # (stable: by kind, then the objective's order)
        self._aux_refs = self._aux_key = self._table = self._grad_plan = None
        self._vjp_rec = self._vjp_work = None
        self._aux_stamp = -1
        self._J = self._e = self._Jv = self._ev = None
        self._asm_cache = {}

    def sync(self, force: bool = False, deep: bool = False):
        """... and rebuild the term table when an auxiliary tensor was replaced."""
        super().sync(force, deep)
        self._sync_aux(deep or force)

    def _sync_aux(self, deep: bool = False):
        if self._table is not None and not deep and self._aux_stamp == Variable._global_updates:
            return
        dev, dt, B = self._state.device, self._state.dtype, self.batch
        aux = [self._KINDS[k].aux(c) for c, k in zip(self.costs, self.kinds)]
        tensors = [[a.tensor for a, _ in ts] for ts in aux]
        # which tensor every slot holds, and where each DISTINCT tensor lives (most are shared by many costs)
        key = tuple(id(t) for ts in tensors for t in ts)
        distinct = {id(t): t for ts in tensors for t in ts}
        key += tuple((t.data_ptr(), t.shape[0], t.stride(0), t.requires_grad) for t in distinct.values()) + (str(dev), B)
        self._aux_stamp = Variable._global_updates
        if self._table is not None and key == self._aux_key:
            return
        table = np.zeros(len(self.costs), self._TERM)
        var_field = self._TERM.names[2]
        refs = []
        for slot, c in enumerate(self.term_order):
            cost, kind, ts = self.costs[c], self._KINDS[self.kinds[c]], tensors[c]
            row = table[slot]
            row["kind"], row["row0"], row["j_off"] = self.kinds[c], self.rows[c], self.joff[c]
            variables = self._term_vars(c)
            row[var_field] = variables + [-1] * (4 - len(variables))
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
                    # one problem's values are dense: a slice of a larger batched tensor is read in place through its own batch stride
                    bstride = td.stride(0)
                elif not td.is_contiguous():
                    td = td.contiguous()
                    key = None   # (a private copy: look again at the next call)
                refs.append(td)
                row["aux"][k], row["aux_bstride"][k] = td.data_ptr(), bstride if t.shape[0] > 1 else 0
            row["wdim"] = kind.wdim
            if kind.grid is not None:
                grid = ts[kind.grid]
                if grid.ndim not in (3, 4):
                    raise ValueError(f"{cost.name}: sdf_data of shape {tuple(grid.shape)} is not a batch of grids")
                row["rows"], row["cols"] = grid.shape[-2], grid.shape[-1]
                if grid.ndim == 4:
                    row["pad"] = grid.shape[1]
            if kind.weight is not None:
                allowed, message = self._WEIGHT_WIDTHS
                row["wdim"] = wdim = ts[kind.weight][0].numel()
                if wdim not in allowed:
                    raise ValueError(message)
        self._table = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(dev)
        self._aux_refs, self._aux_key = (tensors, refs), key
        self._grad_plan = self._build_grad_plan(tensors, dev) if hasattr(self, "_launch_vjp") else None
        if key is None:
            self._aux_stamp = -1

    def _build_grad_plan(self, tensors, dev) -> GradPlan:
        """Stage B of the family's VJP kernel (include/theseus_hip.h: thx_traj2_grad_plan), built with the term table: per distinct
        tensor that requires grad the (term slot, record entry) pairs that feed it, or for a grid the collision terms that read it."""
        B = self.batch
        feeds = {}   # id -> (tensor, [(slot, entry)], [slot of a term that reads it as its grid])
        for slot, c in enumerate(self.term_order):
            kind, entries = self._KINDS[self.kinds[c]], self._VJP_ENTRIES[self.kinds[c]]
            for k, t in enumerate(tensors[c]):
                _, pairs, grid_terms = feeds.setdefault(id(t), (t, [], []))
                if k == kind.grid:
                    grid_terms.append(slot)
                else:
                    pairs.append((slot, entries[k]))
        inputs, offsets = [t for t, _, _ in feeds.values()], []
        pairs_all, terms_all, rows_t, rows_g, out, work = [], [], [], [], 0, 0
        for t, pairs, grid_terms in feeds.values():
            if not t.requires_grad:
                offsets.append(None)
                continue
            if pairs and grid_terms:
                raise ValueError("an auxiliary tensor that requires grad is both a grid and a parameter of the objective")
            shared = int(t.shape[0] == 1)
            if grid_terms:
                cells = t.shape[-2] * t.shape[-1]
                rows_g.append((len(terms_all), len(terms_all) + len(grid_terms), t.shape[-2], t.shape[-1], shared, 0, out, work))
                terms_all += grid_terms
                work += cells * B
            else:
                rows_t.append((len(pairs_all), len(pairs_all) + len(pairs), t[0].numel(), shared, out))
                pairs_all += pairs
            offsets.append(out)
            out += t.numel()
        arrays = (np.array(rows_t, GRAD_TENSOR), np.array(pairs_all, GRAD_PAIR), np.array(rows_g, GRAD_GRID), np.array(terms_all, np.int32))
        tables = tuple(torch.from_numpy(np.frombuffer(a.tobytes() or bytes(8), np.uint8).copy()).to(dev) for a in arrays)
        struct = _lib.Traj2GradPlan(len(rows_t), len(pairs_all), len(rows_g), len(terms_all), max([r[2] * r[3] for r in rows_g] + [0]), 0,
                                    *[t.data_ptr() for t in tables], out, work)
        return GradPlan(inputs, offsets, struct, tables)

    def _fused_backward_route(self) -> bool:
        """the gate of the fused backward: a property of the family and the kernel set, never a fallback after a failure"""
        return (self.fused_backward and hasattr(self, "_launch_vjp") and hasattr(self.K, self._VJP_KERNEL)
                and not self._state.requires_grad and any(t.requires_grad for t in self._grad_plan.inputs))

    def _vjp(self, plan: GradPlan, table, state, u):
        """-> one gradient per input of the plan, in that input's shape (None where none is asked for)"""
        dev = state.device
        need = len(self.costs) * self._VJP_REC * u.shape[0]   # (u is (B, n) in every family)
        if self._vjp_rec is None or self._vjp_rec.numel() < need or self._vjp_rec.device != dev:
            self._vjp_rec = torch.empty(need, dtype=torch.float64, device=dev)
        need = plan.struct.work_elems
        if need and (self._vjp_work is None or self._vjp_work.numel() < need or self._vjp_work.device != dev):
            self._vjp_work = torch.empty(need, dtype=torch.float64, device=dev)
        out = torch.zeros(plan.struct.out_elems, dtype=state.dtype, device=dev)
        self._launch_vjp(table, state, u, self._vjp_rec, plan.struct, out, self._vjp_work if need else None)
        return tuple(None if o is None else out[o:o + t.numel()].view(t.shape) for t, o in zip(plan.inputs, plan.offsets))

    def _buffers(self):
        B, dev, dt, w = self.batch, self._state.device, self._state.dtype, self._TANGENT
        if self._J is None or self._e.shape[0] != B or self._e.device != dev or self._e.dtype != dt:
            self._J = torch.zeros(self.j_total * B, dtype=dt, device=dev)
            self._e = torch.zeros(B, self.m, dtype=dt, device=dev)
            self._Jv, self._ev = [], []
            for c, cost in enumerate(self.costs):
                d, o = cost.dim(), self.joff[c]
                self._Jv.append([self._J[(o + w * d * s) * B:(o + w * d * (s + 1)) * B].view(B, d, w)
                                 for s in range(len(self.cost_vars[c]))])
                self._ev.append(self._e[:, self.rows[c]:self.rows[c] + d])
            self._asm_cache = {}

    def _differentiated(self) -> bool:
        return torch.is_grad_enabled() and any(v.tensor.requires_grad for v in self._tracked())

    def _eval(self, state=None):
        """the family's *_eval at ``state`` (default: the current one) -> (Jacobian block views, error views) of the persistent buffers"""
        self.sync()
        self._buffers()
        self._launch_eval(self._state if state is None else state)
        return self._Jv, self._ev

    def weighted_blocks(self):
        if self._differentiated() or not self.fused:
            return super().weighted_blocks()
        return self._eval()

    def assemble(self, H: torch.Tensor, g: torch.Tensor, graph: bool = False):
        """``graph`` with nothing to differentiate (the implicit step under no_grad, or no leaf requires grad) is fused as well: the
        returned gradient is the one the kernels formed.  With something to differentiate it is fused where the family has a VJP
        kernel (``_fused_backward_route``): the returned gradient is then a function of the auxiliary tensors whose backward is that
        kernel; the optimisation variables get no gradient, as on the torch path of the implicit step."""
        if not self.fused:
            return super().assemble(H, g, graph)
        differentiated = graph and self._differentiated()
        if differentiated:
            self.sync()
            if not self._fused_backward_route():
                return super().assemble(H, g, graph)
        Jv, ev = self._eval()
        self.K.block_assemble_strided(self.asm, Jv, ev, H, g, self._asm_cache)
        self._blocks = (Jv, ev)
        if not differentiated:
            return g.clone() if graph else None
        if self._grad_plan.asked() != tuple(t.requires_grad for t in self._grad_plan.inputs):
            self._sync_aux(deep=True)   # (requires_grad_() on a tensor the table already holds)
        return _FusedGradient.apply(self, g, *self._grad_plan.inputs)

    def error_metric(self, state=None, out: Optional[torch.Tensor] = None, poses=None):
        self.sync()
        x = state if state is not None else (poses if poses is not None else self._state)
        if not self.fused:
            with torch.no_grad():
                return super().error_metric(x.detach(), out)
        err = out if out is not None else torch.empty(self.batch, dtype=x.dtype, device=x.device)
        self._launch_error(x.detach(), err)
        return err
