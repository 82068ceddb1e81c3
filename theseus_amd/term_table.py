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
and sets ``self.kinds`` (one per cost function, objective order) before or in the packed class's constructor."""
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch

from .core import Variable
from .generic import _names


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


class TermTable:
    fused = True    # False: the same packed class on the torch classes (tools/bench_push2.py's baseline)

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
        self._aux_refs = self._aux_key = self._table = None
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
        key += tuple((t.data_ptr(), t.shape[0], t.stride(0)) for t in {id(t): t for ts in tensors for t in ts}.values()) + (str(dev), B)
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
        if key is None:
            self._aux_stamp = -1

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
        returned gradient is the one the kernels formed."""
        if not self.fused or (graph and self._differentiated()):
            return super().assemble(H, g, graph)
        Jv, ev = self._eval()
        self.K.block_assemble_strided(self.asm, Jv, ev, H, g, self._asm_cache)
        self._blocks = (Jv, ev)
        return g.clone() if graph else None

    def error_metric(self, state=None, out: Optional[torch.Tensor] = None, poses=None):
        self.sync()
        x = state if state is not None else (poses if poses is not None else self._state)
        if not self.fused:
            with torch.no_grad():
                return super().error_metric(x.detach(), out)
        err = out if out is not None else torch.empty(self.batch, dtype=x.dtype, device=x.device)
        self._launch_error(x.detach(), err)
        return err
