"""The band plan of ``HipBandedCholeskySolver`` (theseus_amd/linear_solver.py): the order of the linearization's columns in which
tril(AtA) has the smallest half-bandwidth, found once per structure on the host.

The pattern is the list of non-zero blocks of tril(H) the linearization assembles into -- never the numbers.  Variables are ordered
by reverse Cuthill-McKee on the graph whose edges are the off-diagonal blocks (``sparse.rcm_order``), the order is expanded to scalar
columns, and the natural order is kept when it is no wider: a chain objective that adds its far end's priors early (the motion
planners: pose_N, vel_N sit at columns 4..7) is banded only after the reordering.  Everything a caller hands to the solver or gets
back stays in the linearization's order; ``perm`` lives inside the solver (``thx_band_factor`` gathers through it)."""
from typing import List, Tuple

import numpy as np
import torch

from . import _lib
from .packed import UnsupportedObjective


class BandPlan:
    """perm (n) int32: ``perm[k]`` = the linearization column at banded position k; kd: scalar half-bandwidth of the permuted
    pattern (largest row - col over the elements of its non-zero blocks); n: number of columns."""

    def __init__(self, perm: np.ndarray, kd: int, n: int):
        perm = np.ascontiguousarray(perm, dtype=np.int32)
        if perm.shape != (n,) or not np.array_equal(np.sort(perm), np.arange(n, dtype=np.int32)):
            raise ValueError("BandPlan: perm is not a permutation of the linearization's columns")
        self.perm, self.kd, self.n = perm, int(kd), int(n)
        self._dev = {}

    def device_perm(self, device) -> torch.Tensor:
        key = str(device)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self.perm.copy()).to(device)
        return self._dev[key]

    def __iter__(self):   # (perm, kd, n)
        return iter((self.perm, self.kd, self.n))

    def __repr__(self):
        return f"BandPlan(n={self.n}, kd={self.kd})"


def scalar_block_pattern(linearization) -> List[Tuple[int, int, int, int]]:
    """[(row0, col0, rows, cols)] of the non-zero blocks of tril(H), in the linearization's own column order."""
    if getattr(linearization, "full_matrix", None) is not None:
        raise NotImplementedError("HipBandedCholeskySolver: a system handed over as plain tensors has no block pattern to find a "
                                  "band in; use HipCholeskySolver (or HipLUSolver) for it.")
    packed = getattr(linearization, "packed", None)
    asm = getattr(packed, "asm", None)
    if asm is None:   # (the plugin's generic path keeps its block assembler on the linearization, compiled at the first linearize())
        asm = getattr(linearization, "asm", None)
    if asm is not None and hasattr(asm, "lower_block_pattern"):
        return [tuple(int(v) for v in blk) for blk in asm.lower_block_pattern()]
    structure = getattr(packed, "structure", None)
    if structure is not None and hasattr(structure, "hessian_blocks"):
        hb = structure.hessian_blocks()
        d = int(hb.bd)
        return [(d * int(p), d * int(q), d, d) for p, q in np.asarray(hb.blocks).tolist()]
    raise UnsupportedObjective(f"HipBandedCholeskySolver: {type(packed).__name__} exposes no block pattern of its Hessian "
                               "(a block assembler or a pose-graph structure); use HipCholeskySolver.")


def _half_bandwidth(blocks, pos) -> int:
    """Scalar half-bandwidth when column c sits at position pos[c] (every variable's columns stay together and in order)."""
    kd = 0
    for r0, c0, da, db in blocks:
        pr, pc = int(pos[r0]), int(pos[c0])
        kd = max(kd, pr + da - 1 - pc, pc + db - 1 - pr)
    return kd


def band_plan(linearization, ordering: str = "auto") -> BandPlan:
    """The BandPlan of a linearization.  ``ordering``: "auto" -- reverse Cuthill-McKee on the variable graph unless the
    linearization's own order is no wider; "natural" -- the linearization's own order.  Raises ``UnsupportedObjective`` when the
    half-bandwidth exceeds ``THX_BAND_MAX_KD``."""
    if ordering not in ("auto", "natural"):
        raise ValueError(f"ordering must be 'auto' or 'natural', got {ordering!r}")
    blocks = scalar_block_pattern(linearization)
    starts = [int(c) for c in linearization.var_start_cols]
    dims = [int(d) for d in linearization.var_dims]
    n = sum(dims)
    var_of = {c: k for k, c in enumerate(starts)}
    natural = np.arange(n, dtype=np.int64)
    kd_nat = _half_bandwidth(blocks, natural)
    perm, kd = natural, kd_nat
    if ordering == "auto" and kd_nat > 0:
        try:
            edges = sorted({(var_of[r0], var_of[c0]) for r0, c0, _, _ in blocks if r0 != c0})
        except KeyError:
            raise UnsupportedObjective("HipBandedCholeskySolver: the Hessian's blocks do not start at variable boundaries") from None
        from .sparse import rcm_order
        order = rcm_order(len(starts), edges)
        cand = np.concatenate([np.arange(starts[v], starts[v] + dims[v], dtype=np.int64) for v in order])
        pos = np.empty(n, dtype=np.int64)
        pos[cand] = np.arange(n)
        kd_rcm = _half_bandwidth(blocks, pos)
        if kd_rcm < kd_nat:
            perm, kd = cand, kd_rcm
    if kd > _lib.THX_BAND_MAX_KD:
        raise UnsupportedObjective(f"HipBandedCholeskySolver: the objective's half-bandwidth is kd = {kd} (n = {n}), above the limit "
                                   f"of {_lib.THX_BAND_MAX_KD} of the banded solver; use HipCholeskySolver.")
    return BandPlan(perm, kd, n)
