"""Homography image alignment (the reference's examples/homography_estimation.py): the packed representation of an objective whose
costs are HomographyAlignment (theseus_amd/embodied.py) on 8-dof Euclidean variables and Difference priors on such variables, each
with a Scale / DiagonalCostWeight, at least one of them an alignment cost.

It is PackedEuclidean -- the (B, n) state, retraction by thx_vec_retract, implicit / unrolled / truncated backward through the torch
classes -- whose NON-differentiated evaluation is fused (theseus_amd/term_table.py): ``assemble`` = thx_homog_eval into persistent
block buffers + thx_block_assemble on them, ``error_metric`` = thx_homog_error.  Both kernels reduce over the C Hh Ww elements of
every problem through a fp64 scratch (alignment terms, B, chunks, THX_HOMOG_SUMS) that this class owns.

The feature maps are auxiliary variables: a CNN outside hands over new tensors at every outer step, which the term table picks up
(a replaced tensor rebuilds the 128-byte records, values changed in place need nothing).
"""
import torch

from . import _lib
from .euclidean import PackedEuclidean, _is_euclidean
from .generic import _names
from .term_table import TermKind, TermTable, term_dtype, weight_var

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
