"""Homography image alignment (the reference's examples/homography_estimation.py): the packed representation of an objective whose
costs are HomographyAlignment (theseus_amd/embodied.py) on 8-dof Euclidean variables and Difference priors on such variables, each
with a Scale / DiagonalCostWeight, at least one of them an alignment cost.

It is PackedEuclidean -- the (B, n) state, retraction by thx_vec_retract, implicit / unrolled / truncated backward through the torch
classes -- whose NON-differentiated evaluation is fused (theseus_amd/term_table.py): ``assemble`` = thx_homog_eval into persistent
block buffers + thx_block_assemble on them, ``error_metric`` = thx_homog_error.  Both kernels reduce over the C Hh Ww elements of
every problem through a fp64 scratch (alignment terms, B, chunks, THX_HOMOG_SUMS) that this class owns.

The feature maps are auxiliary variables: a CNN outside hands over new tensors at every outer step, which the term table picks up
(a replaced tensor rebuilds the 128-byte records, values changed in place need nothing).

The implicit step's backward is fused too: ``assemble(graph=True)`` with an auxiliary tensor that requires grad and a state that
does not returns g as a function of the auxiliary tensors whose backward is thx_homog_vjp (feature maps per problem, weights,
prior targets).  A shared (batch-1) feature map that requires grad, ``unroll`` / ``truncated``, a kernel set without ``homog_vjp``
and ``fused_backward = False`` keep the torch classes.
"""
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .euclidean import PackedEuclidean, _is_euclidean
from .generic import _names
from .term_table import GRAD_PAIR, GRAD_TENSOR, TermKind, TermTable, term_dtype, weight_var

HOMOG_TERM = term_dtype("col")


def _homog_kind(c):
    """THX_HOMOG_* of a cost function the fused kernels cover, else None."""
    names, w = _names(c), _names(c.weight)
    if not ("ScaleCostWeight" in w or "DiagonalCostWeight" in w):
        return None
    if "HomographyAlignment" in names:
        return _lib.HOMOG_ALIGN
    if "Difference" in names and _is_euclidean(c.var) and c.var.dof() == 8:
        return _lib.HOMOG_PRIOR
    return None


def _align_aux(c):
    c.check_shapes()   # (the tensors may have been replaced since the cost was built: the message names the cost)
    return [(c.feat_src, None), (c.feat_dst, None), (weight_var(c), 1)]


def _prior_aux(c):
    if weight_var(c).tensor[0].numel() not in (1, 8):
        raise ValueError(f"{c.name}: this cost needs an 8-dimensional DiagonalCostWeight.")
    return [(c.target, 8), (weight_var(c), None)]


class PackedHomography(TermTable, PackedEuclidean):
    family = "homography alignment"

    _TERM, _TANGENT = HOMOG_TERM, 8
    _KINDS = {
        _lib.HOMOG_ALIGN: TermKind(_align_aux, grid=0, wdim=1),
        _lib.HOMOG_PRIOR: TermKind(_prior_aux, weight=1),
    }
    _WEIGHT_WIDTHS = ((1, 8), "This cost needs an 8-dimensional DiagonalCostWeight.")

    def __init__(self, objective, kernels=None, order=None):
        from .kernels import default_kernels
        from .packed import UnsupportedObjective
        K = kernels or default_kernels()
        if not hasattr(K, "homog_eval"):
            raise UnsupportedObjective("these kernels have no fused homography-alignment evaluation")
        self.kinds = [_homog_kind(c) for c in objective.cost_functions.values()]
        if any(k is None for k in self.kinds) or _lib.HOMOG_ALIGN not in self.kinds:
            raise UnsupportedObjective("HIP backend, fused homography alignment: every cost must be a HomographyAlignment or a Difference "
                                       "on an 8-dof Euclidean variable, with a Scale / DiagonalCostWeight, and at least one of them a "
                                       "HomographyAlignment.")
        self.n_align = self.kinds.count(_lib.HOMOG_ALIGN)
        self._scratch = None
        super().__init__(objective, K, order)

    def _term_vars(self, c):
        return [self.cols[k][0] for k in self.cost_vars[c]]   # (state columns)

    def _chunks(self):
        """(fp64 scratch, chunks per problem) for the feature maps the table points at now"""
        chunks = 1
        for c, k in zip(self.costs, self.kinds):
            if k == _lib.HOMOG_ALIGN:
                Hh, Ww = c.feat_src.tensor.shape[2:]
                chunks = max(chunks, -(-(Hh * Ww) // _lib.THX_HOMOG_CHUNK))
        need = self.n_align * self.batch * chunks * _lib.THX_HOMOG_SUMS
        dev = self._state.device
        if self._scratch is None or self._scratch.numel() < need or self._scratch.device != dev:
            self._scratch = torch.zeros(need, dtype=torch.float64, device=dev)
        return self._scratch, chunks

    def _launch_eval(self, state):
        scratch, chunks = self._chunks()
        self.K.homog_eval(self._table, len(self.costs), self.n_align, state, self.n, scratch, chunks, self._J, self.j_total, self._e)

    def _launch_error(self, state, err):
        scratch, chunks = self._chunks()
        self.K.homog_error(self._table, len(self.costs), self.n_align, state, self.n, scratch, chunks, err)

    # ---- the implicit step's backward (thx_homog_vjp) ----
    # Served on the fused route: feature maps that require grad and whose batch dimension is the problem batch (slices of a larger
    # tensor through its batch stride included), every alignment cost's weight, the priors' targets and weights (batch-1 ones are
    # summed over the problems in index order in the kernel).  A batch-1 (shared) feature map that requires grad keeps the whole
    # backward on the torch classes: its sum over the problems would need a (B, C, Hh, Ww) work buffer.  So does a feature map
    # that requires grad and is read by more than one slot (the pixel pass gives every gradient buffer one owner).
    _VJP_KERNEL, _VJP_REC = "homog_vjp", _lib.THX_HOMOG_REC
    # where each aux slot's derivative sits in a term's record (include/theseus_hip.h); None: a feature map, written by the pixel pass
    _VJP_ENTRIES = {_lib.HOMOG_ALIGN: (None, None, 0), _lib.HOMOG_PRIOR: (0, 8)}

    def _build_grad_plan(self, tensors, dev) -> "HomogGradPlan":
        """thx_homog_grad_plan, built with the term table: per distinct small tensor that requires grad the (term slot, record
        entry) pairs that feed it; per alignment term where the gradients of its two feature maps start in the kernel's output."""
        B = self.batch
        feeds = {}   # id -> (tensor, [(slot, entry)], [(slot, 0 | 1) it is the feat_src | feat_dst of])
        for slot, c in enumerate(self.term_order):
            for k, (t, entry) in enumerate(zip(tensors[c], self._VJP_ENTRIES[self.kinds[c]])):
                _, pairs, maps = feeds.setdefault(id(t), (t, [], []))
                (maps if entry is None else pairs).append((slot, k if entry is None else entry))
        inputs, offsets, rows_t, pairs_all, out, servable = [t for t, _, _ in feeds.values()], [], [], [], 0, True
        map_off = np.full((self.n_align, 2), -1, np.int64)
        for t, pairs, maps in feeds.values():
            if not t.requires_grad:
                offsets.append(None)
                continue
            if maps:
                servable &= not pairs and len(maps) == 1 and t.shape[0] == B
                map_off[maps[0]] = out
            else:
                rows_t.append((len(pairs_all), len(pairs_all) + len(pairs), t[0].numel(), int(t.shape[0] == 1), out))
                pairs_all += pairs
            offsets.append(out)
            out += t.numel()
        shapes = [tensors[c][0].shape for c in self.term_order[:self.n_align]]
        arrays = (np.array(rows_t, GRAD_TENSOR), np.array(pairs_all, GRAD_PAIR), map_off)
        tables = tuple(torch.from_numpy(np.frombuffer(a.tobytes() or bytes(8), np.uint8).copy()).to(dev) for a in arrays)
        chunks = max(-(-(s[2] * s[3]) // _lib.THX_HOMOG_CHUNK) for s in shapes)
        struct = _lib.HomogGradPlan(len(rows_t), len(pairs_all), self.n_align if (map_off >= 0).any() else 0,
                                    max(s[2] * s[3] for s in shapes), max(s[1] for s in shapes), 0, *[t.data_ptr() for t in tables], out)
        return HomogGradPlan(inputs, offsets, struct, tables, servable, chunks)

    def _fused_backward_route(self) -> bool:
        """... and every feature map that requires grad is per problem and has one reader (above).  ``servable`` belongs to the
        tensors that asked when the plan was built: after requires_grad_() on a tensor the table already holds the plan is rebuilt
        first, so the gate never reads a stale answer."""
        if self._grad_plan.asked() != tuple(t.requires_grad for t in self._grad_plan.inputs):
            self._sync_aux(deep=True)
        return super()._fused_backward_route() and self._grad_plan.servable

    def _vjp(self, plan, table, state, u):
        dev, B = state.device, state.shape[0]
        need = len(self.costs) * self._VJP_REC * B
        if self._vjp_rec is None or self._vjp_rec.numel() < need or self._vjp_rec.device != dev:
            self._vjp_rec = torch.empty(need, dtype=torch.float64, device=dev)
        need = self.n_align * B * plan.chunks * _lib.THX_HOMOG_SUMS
        if self._vjp_work is None or self._vjp_work.numel() < need or self._vjp_work.device != dev:
            self._vjp_work = torch.zeros(need, dtype=torch.float64, device=dev)   # (its own scratch: the forward's may be in use)
        out = torch.zeros(plan.struct.out_elems, dtype=state.dtype, device=dev)
        self._launch_vjp(table, state, u, self._vjp_rec, plan, out, self._vjp_work)
        return tuple(None if o is None else out[o:o + t.numel()].view(t.shape) for t, o in zip(plan.inputs, plan.offsets))

    def _launch_vjp(self, table, state, u, rec, plan, grad_out, scratch):
        self.K.homog_vjp(table, len(self.costs), self.n_align, state, self.n, u, self.m, self.j_total, scratch, plan.chunks, rec,
                         plan.struct, grad_out)


class HomogGradPlan(NamedTuple):
    """term_table.GradPlan for this family: ``struct`` is a _lib.HomogGradPlan; ``servable``: the fused route can serve every
    feature map that requires grad; ``chunks``: the sort chunks per problem of the largest map the table points at."""
    inputs: list
    offsets: list
    struct: object
    tables: tuple
    servable: bool
    chunks: int

    def asked(self):
        return tuple(o is not None for o in self.offsets)
