"""`LinearSolver` plugin surface + the HIP dense Cholesky and pivoted-LU solvers.

ABC contract: theseus/optimizer/linear/linear_solver.py:15-37.  ``HipCholeskySolver`` replaces
``CholeskyDenseSolver`` (theseus/optimizer/linear/dense_solver.py:20-161): damping semantics of
``DenseSolver._apply_damping`` (:38-64, out of place), ``torch.linalg.cholesky`` +
``torch.cholesky_solve`` (:159-161) become one batched tiled HIP factorisation + two triangular
solves; a non positive-definite system raises ``RuntimeError`` like ``torch.linalg.cholesky`` does.
``HipLUSolver`` replaces ``LUDenseSolver`` (dense_solver.py:125-141) for systems that are not numerically positive
definite: ``torch.linalg.lu_factor`` + ``lu_solve`` become thx_lu_factor + thx_lu_solve*.
"""
import abc
import math
import warnings
from typing import Any, Dict, Optional, Sequence, Type, Union

import torch

from .core import Objective
from .linearization import HipLinearization, Linearization
from . import _lib


class LinearSolver(abc.ABC):
    def __init__(self, objective: Objective, linearization_cls: Optional[Type[Linearization]] = None,
                 linearization_kwargs: Optional[Dict[str, Any]] = None, **kwargs):
        linearization_kwargs = linearization_kwargs or {}
        self.linearization: Linearization = linearization_cls(objective, **linearization_kwargs)

    def reset(self, **kwargs):
        pass

    @abc.abstractmethod
    def solve(self, damping: Optional[Union[float, torch.Tensor]] = None, **kwargs) -> torch.Tensor:
        pass


class _FactorSnapshot(tuple):
    """(L, panels) of ``factor_snapshot`` with the order the factor was made in (``ordered``: HipCholeskyCore._factor_ord)."""
    ordered = None


class HipCholeskyCore:
    """Back-end half of the solver (buffers, factor, solves), shared by theseus_amd's mirror class below and
    the adapter for the real ``theseus`` (theseus_amd/plugin.py)."""

    # "auto": a block-compact linearization is factorised in the order of thx_hblock_order -- the columns of H, L, g and x inside
    # the solver follow the permutation, everything a caller hands in or gets back stays in the linearization's order;
    # "natural": the linearization's own order
    ordering = "auto"

    def _core_init(self):
        self.K = self.linearization.K
        self._L = self._panels = self.info = self._y = None
        self._lam = None
        self.factor_version = 0  # bumped by every factorisation (the implicit backward checks its factor is current)
        self._factor_ord = None  # (layout, maps) of compiler.OrderedHessianBlocks the CURRENT factor was made in, None: natural order
        self._Hp = self._gp = self._xp = None
        self._natural_frame = None
        self._force_natural = False

    # ---- the factor frame as callers see it ---------------------------------------------------------------------------------------
    @property
    def L(self):
        """The factor frame in the LINEARIZATION's order (tests / inspection; the solver itself works on ``_L``).  After a
        factorisation in the solver's own order that is a second factorisation of the same system -- the linearization as it
        stands, the damping of the last ``factorize`` -- in the natural order, made on first use and kept until the next one."""
        return self._L if self._factor_ord is None else self._natural_factor()[0]

    @L.setter
    def L(self, value):
        self._L = value

    @property
    def panels(self):
        return self._panels if self._factor_ord is None else self._natural_factor()[1]

    @panels.setter
    def panels(self, value):
        self._panels = value

    def _natural_factor(self):
        if self._natural_frame is None or self._natural_frame[0] != self.factor_version:
            lin = self.linearization
            L, panels = torch.zeros_like(self._L), torch.empty_like(self._panels)
            has_lam, ellipsoidal, eps = self._factored_with
            if getattr(lin, "_compact", False):
                self.K.chol_factor_hblocks(lin.hblocks, lin.Hc, lin.n, self._lam if has_lam else None, ellipsoidal, eps, L, panels,
                                           torch.zeros_like(self.info))
            else:
                self.K.chol_factor(lin.H, lin.n, self._lam if has_lam else None, ellipsoidal, eps, L, panels, torch.zeros_like(self.info))
            self._natural_frame = (self.factor_version, L, panels)
        return self._natural_frame[1:]

    def _ordered(self):
        """(DeviceHessianBlocks, device maps) of the layout the next factorisation runs in, None: the linearization's order."""
        lin = self.linearization
        if self.ordering == "natural" or self._force_natural:
            return None
        if self.ordering != "auto":
            raise ValueError(f"ordering must be 'auto' or 'natural', got {self.ordering!r}")
        # a block-compact linearization -- or one that could be and was asked to keep the dense frame (block_hessian=False): the
        # same order, so that both storages compute the same bits
        packed = getattr(lin, "packed", None)
        if getattr(lin, "_compact", False) and lin.hblocks is not None:
            host, dev = lin.hblocks.host, lin.Hc.device
        elif (not getattr(lin, "_compact", False) and getattr(packed, "supports_block_hessian", lambda: False)()
              and getattr(lin, "full_matrix", None) is None and lin.H is not None):
            host, dev = packed.structure.hessian_blocks(), lin.H.device
        else:
            return None
        from .compiler import ordered_hessian_blocks
        oh = ordered_hessian_blocks(host)
        return None if oh is None else oh.on(dev)

    def _ensure_buffers(self):
        lin = self.linearization
        g = lin.g     # (B, n): shape / dtype / device of the system (lin.H may be block-compact: never touched here)
        shape = (g.shape[0], lin.ld, lin.ld)
        if self._L is None or tuple(self._L.shape) != shape or self._L.device != g.device or self._L.dtype != g.dtype:
            B = g.shape[0]
            nt = (lin.n + _lib.THX_TILE - 1) // _lib.THX_TILE
            self._L = torch.zeros(shape, dtype=g.dtype, device=g.device)
            self._panels = torch.empty(B, nt, _lib.THX_TILE, _lib.THX_TILE, dtype=g.dtype, device=g.device)
            self._Hp = self._gp = self._xp = self._natural_frame = None
            self._y = torch.empty(B, lin.n, dtype=g.dtype, device=g.device)
            self.info = torch.zeros(B, dtype=torch.int32, device=g.device)
            self._lam = torch.empty(B, dtype=g.dtype, device=g.device)
            self._unfused_forward = False   # (decided per system size: see _solve)

    def _linearized(self) -> bool:
        lin = self.linearization
        return lin.linearized if hasattr(lin, "linearized") else lin.H is not None

    def _factor_call(self, lam, ellipsoidal_damping, damping_eps, rhs, y, pattern=None):
        """One factorisation launch sequence: H from the block list when the linearization keeps it compact."""
        lin = self.linearization
        self._factor_ord = self._natural_frame = None
        ordered = self._ordered() if pattern is None else None
        if ordered is not None:
            # the solver's own order: the block list moves into the permuted layout's block order (a block whose variables swap
            # sides of the diagonal transposed), g is gathered; ``y`` comes out in the permuted order and stays there -- the
            # backward substitution recognises it (_substitute)
            layout, maps = ordered
            compact = getattr(lin, "_compact", False)
            shape = (lin.Hc.shape[0], layout.host.bstride) if compact else tuple(lin.H.shape)
            if self._Hp is None or tuple(self._Hp.shape) != shape:
                self._Hp = torch.zeros(shape, dtype=self._L.dtype, device=self._L.device)
                self._gp, self._xp = torch.empty_like(self._y), torch.empty_like(self._y)
            if rhs is not None:
                self.K.vec_gather(rhs.contiguous(), self._gp, maps["to_perm"])
            rhs_p = self._gp if rhs is not None else None
            if compact:
                self.K.hblocks_permute(lin.Hc, self._Hp, maps["block_map"], layout.host.bd)
                self.K.chol_factor_hblocks(layout, self._Hp, lin.n, lam, ellipsoidal_damping, damping_eps, self._L, self._panels,
                                           self.info, rhs=rhs_p, y=y)
            else:   # (the dense frame of a matrix that has a block layout: block_hessian=False)
                self.K.frame_permute(lin.H, self._Hp, maps["to_perm"], lin.n)
                self.K.chol_factor(self._Hp, lin.n, lam, ellipsoidal_damping, damping_eps, self._L, self._panels, self.info,
                                   rhs=rhs_p, y=y)
            self._factor_ord = ordered
        elif getattr(lin, "_compact", False):
            self.K.chol_factor_hblocks(lin.hblocks, lin.Hc, lin.n, lam, ellipsoidal_damping, damping_eps, self._L, self._panels,
                                       self.info, pattern=pattern, rhs=rhs, y=y)
        elif pattern is not None:
            self.K.chol_factor_sparse(lin.H, lin.n, lam, ellipsoidal_damping, damping_eps, self._L, self._panels, self.info,
                                      pattern, rhs=rhs, y=y)
        else:
            self.K.chol_factor(lin.H, lin.n, lam, ellipsoidal_damping, damping_eps, self._L, self._panels, self.info, rhs=rhs, y=y)

    def factorize(self, damping: Optional[Union[float, torch.Tensor]] = None, ellipsoidal_damping: bool = True,
                  damping_eps: float = 1e-8, rhs: Optional[torch.Tensor] = None):
        """L L^T = AtA (+ damping); keeps L and the solve panels for later solves (the implicit backward
        re-uses them).  With ``rhs`` the forward substitution L y = rhs is fused into the factorisation
        (no extra pass over L) and y is returned."""
        if not self._linearized():
            raise RuntimeError("linearize() must be called before solve().")
        self._ensure_buffers()
        lam = None
        if damping is not None:
            lam = self._lam
            if isinstance(damping, torch.Tensor):
                lam.copy_(damping.to(lam.dtype).expand(lam.shape[0]))
            else:
                lam.fill_(float(damping))
        y = self._y if rhs is not None else None
        self.factor_version += 1
        self._factored_with = (lam is not None, bool(ellipsoidal_damping), float(damping_eps))   # (what L L^T is the factor of)
        self._factor_call(lam, ellipsoidal_damping, damping_eps, rhs, y)
        return y

    def solve_with_factor(self, rhs: torch.Tensor) -> torch.Tensor:
        """(L L^T)^-1 rhs with the cached factor (forward + backward substitution kernels)."""
        rhs = rhs.contiguous()
        x = torch.empty_like(rhs)
        self._substitute(rhs, x, backward_only=False)
        return x

    def factor_snapshot(self):
        """A private copy of the CURRENT factor, for a solve after the solver has factorised again (the differentiated iterations
        of BackwardMode.UNROLL / TRUNCATED: every iteration's backward solves with that iteration's factor)."""
        snap = _FactorSnapshot((self._L.clone(), self._panels.clone()))
        snap.ordered = self._factor_ord
        return snap

    def solve_with_snapshot(self, snapshot, rhs: torch.Tensor) -> torch.Tensor:
        """(L L^T)^-1 rhs with a factor kept by ``factor_snapshot`` (dense frame: thx_chol_solve), in the order it was made in."""
        L, panels = snapshot
        rhs = rhs.contiguous()
        x = torch.empty_like(rhs)
        self._solve_frame(L, panels, getattr(snapshot, "ordered", None), rhs, x, backward_only=False)
        return x

    solve_envelope = True   # False: the dense-frame solves read every tile of L in full (the same bits; tests compare the two)

    def _envelope(self, ordered=None) -> Dict[str, torch.Tensor]:
        """``row_first=`` of the dense-frame solves when the factor is a block layout's: every schedule of thx_chol_factor_hblocks
        leaves exact zeros left of the first non-zero column of each row of H, and the solves read the row envelope only
        (``ordered``: the factor was made in that layout -- its table)."""
        lin = self.linearization
        if self.solve_envelope and getattr(lin, "_compact", False) and lin.hblocks is not None:
            return {"row_first": (lin.hblocks if ordered is None else ordered[0]).t["row_first"]}
        return {}

    def _solve_frame(self, L, panels, ordered, rhs, x, backward_only: bool):
        """The dense-frame solves on (L, panels) made in ``ordered`` (None: the linearization's order).  A factor of the solver's
        own order takes rhs gathered into it (thx_vec_gather) -- unless rhs is the y its factorisation left, which is there
        already -- and x is gathered back."""
        n = self.linearization.n
        solve = self.K.chol_solve_backward if backward_only else self.K.chol_solve
        if ordered is None:
            solve(L, n, panels, rhs, x, **self._envelope())
            return
        maps = ordered[1]
        if rhs is self._y:
            src = rhs
        else:
            self.K.vec_gather(rhs, self._gp, maps["to_perm"])
            src = self._gp
        solve(L, n, panels, src, self._xp, **self._envelope(ordered))
        self.K.vec_gather(self._xp, x, maps["from_perm"])

    def _substitute(self, rhs, x, backward_only: bool):
        """x = L^-T rhs (``backward_only``) or (L L^T)^-1 rhs with the current factor (dense frame: the row envelope of L when the
        linearization is block-compact, else every tile)."""
        self._solve_frame(self._L, self._panels, self._factor_ord, rhs, x, backward_only)

    # ---- blocks of right-hand sides on the cached factor (thx_chol_solve_multi): posterior samples, marginal covariances ----------
    def _factor_owner(self) -> "HipCholeskyCore":
        """The core that holds the factor ``solve()`` left (theseus_amd/plugin.py: a system handed over as tensors has its own)."""
        return self

    def _factorize_undamped(self) -> "HipCholeskyCore":
        """L L^T = AtA of the linearization as it stands; returns the core that holds it."""
        self.factorize(None)
        self.check_info()
        return self

    def solve_multi_with_factor(self, rhs: torch.Tensor, which: int = 0) -> torch.Tensor:
        """``rhs`` (B, k, n), one vector per row, against the CURRENT factor: which = 0: (L L^T)^-1 rhs, 1: L^-T rhs, 2: L^-1 rhs
        (the codes of thx_chol_solve_levels).  Every group of 32 vectors reads L once per substitution.  Returns a new tensor."""
        own = self._factor_owner()
        if own is None or own._L is None or own.factor_version == 0:
            raise RuntimeError("solve_multi_with_factor: nothing has been factorised yet (solve() or factorize() first).")
        n = own.linearization.n
        if rhs.dim() != 3 or rhs.shape[0] != own._L.shape[0] or rhs.shape[2] != n or rhs.shape[1] < 1:
            raise ValueError(f"solve_multi_with_factor: rhs must be (B = {own._L.shape[0]}, k >= 1, n = {n}), got {tuple(rhs.shape)}")
        x = rhs.detach().to(own._L.dtype)
        maps = own._factor_ord[1] if own._factor_ord is not None else None
        # (a factor of the solver's own order, P H P^T = L L^T: which = 0 is H^-1 whatever the order; L^-1 takes its vectors in the
        #  linearization's order and L^-T returns them in it -- L^-T (L^-1 rhs) is H^-1 rhs)
        if maps is not None and which != 1:
            x = x.index_select(2, maps["to_perm"].long())
        x = x.clone(memory_format=torch.contiguous_format)
        own.K.chol_solve_multi(own._L, n, own._panels, x, x, which=which)
        if maps is not None and which != 2:
            x = x.index_select(2, maps["from_perm"].long())
        return x

    @torch.no_grad()
    def sample_deltas(self, n_samples: int = 10, temperature: float = 1.0, noise: Optional[torch.Tensor] = None,
                      generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """The ``delta_samples`` of TheseusLayer.compute_samples (theseus/theseus_layer.py:110-123), (B, n, n_samples): draws from
        N(delta, (AtA / temperature)^-1) as  delta + sqrt(temperature) L^-T y  with delta = ``solve()`` (undamped, on the
        linearization as it stands) and L the factor that solve just left -- the reference factorises AtA / temperature a second
        time, densely.  ``noise``: y as (n, n_samples), shared by the batch as in the reference, or (B, n, n_samples); None: drawn
        with ``generator``.  The result is a permuted view of the kernel's (B, n_samples, n) output."""
        if not temperature > 0:
            raise ValueError(f"sample_deltas: temperature must be positive, got {temperature}")
        if int(n_samples) < 1:
            raise ValueError(f"sample_deltas: n_samples must be at least 1, got {n_samples}")
        # (the draw that a given ``noise`` stands for is defined through the factor of AtA in the linearization's order,
        #  theseus_layer.py:113-123: this solve factorises in that order)
        self._force_natural = True
        try:
            delta = self.solve()
        finally:
            self._force_natural = False
        own = self._factor_owner()
        B, n = delta.shape
        if noise is None:
            noise = torch.randn(n, int(n_samples), generator=generator, device=delta.device, dtype=delta.dtype)
        if noise.dim() == 2 and tuple(noise.shape) == (n, n_samples):
            y = noise.t().unsqueeze(0).expand(B, n_samples, n)
        elif noise.dim() == 3 and tuple(noise.shape) == (B, n, n_samples):
            y = noise.transpose(1, 2)
        else:
            raise ValueError(f"sample_deltas: noise must be ({n}, {n_samples}) or ({B}, {n}, {n_samples}), got {tuple(noise.shape)}")
        y = y.to(device=delta.device, dtype=delta.dtype).clone(memory_format=torch.contiguous_format)
        own.K.chol_solve_multi(own._L, n, own._panels, y, y, which=1)
        y.mul_(math.sqrt(float(temperature))).add_(delta.unsqueeze(1))
        return y.transpose(1, 2)

    @torch.no_grad()
    def marginal_covariance(self, var_names: Sequence[str]) -> torch.Tensor:
        """(B, d, d): the rows and columns of (AtA)^-1 at the columns of the named optimisation variables, in the order given --
        their joint marginal covariance in the tangent space at the linearization point.  Factorises undamped and solves against
        the d unit vectors of those columns (one thx_chol_solve_multi call)."""
        lin = self.linearization
        names = list(var_names)
        if len(set(names)) != len(names):
            raise ValueError(f"marginal_covariance: repeated variable names in {names}")
        cols = []
        for name in names:
            try:
                k = lin.ordering.index_of(name)
            except KeyError:
                raise ValueError(f"marginal_covariance: {name!r} is not an optimisation variable of the objective") from None
            cols.extend(range(lin.var_start_cols[k], lin.var_start_cols[k] + lin.var_dims[k]))
        if not cols:
            raise ValueError("marginal_covariance: no variables named")
        own = self._factorize_undamped()
        B, n, d = own._L.shape[0], own.linearization.n, len(cols)
        idx = torch.tensor(cols, dtype=torch.long, device=own._L.device)
        if own._factor_ord is not None:   # (the factor's own order: the same columns, where it keeps them)
            idx = own._factor_ord[1]["from_perm"].long()[idx]
        E = torch.zeros(B, d, n, dtype=own._L.dtype, device=own._L.device)
        E[:, torch.arange(d, device=idx.device), idx] = 1
        own.K.chol_solve_multi(own._L, n, own._panels, E, E, which=0)
        C = E[:, :, idx]
        return (C + C.transpose(1, 2)) / 2

    def check_info(self):
        bad = self.info.nonzero()
        if bad.numel():
            b = int(bad[0])
            raise RuntimeError(
                f"linalg.cholesky: (Batch element {b}): The factorization could not be completed because the "
                f"input is not positive-definite (the leading minor of order {int(self.info[b])} is not "
                "positive-definite).")

    def singular_mask(self) -> torch.Tensor:
        """(B,) bool -- ``check_singular=True`` (dense_solver.py:91-103): the reference runs ``torch.lu`` on the UNDAMPED
        ``AtA`` and drops the batch items whose factorisation hits an exactly zero pivot.  For ``AtA = A^T A`` that is the
        case of an all-zero column of ``A`` (a variable every cost of which has zero weight): a zero on the diagonal of
        ``AtA``.  Rank deficiency that leaves a non-zero rounding residue (a gauge freedom) passes the reference's LU test
        too, and is solved here as it is there."""
        return (self.linearization.diagonal() == 0).any(dim=1)

    def dropped_mask(self) -> Optional[torch.Tensor]:
        """(B,) bool of the batch items the LAST ``_solve`` dropped under ``check_singular=True`` (zero step, dense_solver.py:91-103),
        else None.  The differentiated nodes keep it: a dropped item's step does not depend on anything, its gradients are zero
        (the reference's masked assignment), and its -- possibly broken -- factor must not reach the backward."""
        return getattr(self, "_last_singular", None) if getattr(self, "_check_singular", False) else None

    def post_singular_warning(self):
        """The reference's warning for ``check_singular=True`` (dense_solver.py:97-102) -- one host look at a device flag: called
        where the host synchronises anyway."""
        seen = getattr(self, "_singular_seen", None)
        self._singular_seen = None
        if seen is not None and bool(seen):
            warnings.warn("Singular matrix found in batch, solution will be set to all 0 for all singular matrices.", RuntimeWarning)

    def _solve(self, damping, ellipsoidal_damping, damping_eps, check_info) -> torch.Tensor:
        if damping is not None and isinstance(damping, torch.Tensor) and damping.ndim > 1:
            raise ValueError("Damping must be a float or a 1-D tensor.")
        g = self.linearization.g
        y = None
        if not getattr(self, "_unfused_forward", False):
            try:
                y = self.factorize(damping, ellipsoidal_damping, damping_eps, rhs=g)
            except RuntimeError as e:
                # the fused forward substitution keeps y_0:j in LDS next to the diagonal tile: n <= ~28 k in fp32, ~9 k in fp64
                # (fused diagonal kernel; ~18 k with the split one).  Beyond that: factorise without it and run both triangular
                # solves afterwards (the list-driven solves of the tile-sparse solver have no size limit).  The C side refuses
                # before launching anything, so nothing has to be undone.
                if "fused forward substitution" not in str(e):
                    raise
                self._unfused_forward = True
        delta = torch.empty_like(g)
        if y is not None:
            self._substitute(y, delta, backward_only=True)
        else:
            self.factorize(damping, ellipsoidal_damping, damping_eps, rhs=None)
            self._substitute(g, delta, backward_only=False)
        if getattr(self, "_check_singular", False):
            # dense_solver.py:91-103: items whose UNDAMPED AtA hits an exactly zero LU pivot are dropped (zero step, no failure, a
            # RuntimeWarning).  Here: a zero on diag(AtA) -- an all-zero column of A, the case A^T A produces (singular_mask).  Any
            # OTHER breakdown of the factorisation keeps its info code: the item is a FAILED solve (RuntimeError / FAIL status), as
            # it is in the reference, whose LU passes a rank-deficient matrix with a rounding residue on to torch.linalg.cholesky.
            # (Corner left different: exactly dependent columns with an exactly zero LU pivot but a non-zero diagonal -- the
            # reference zeroes the step, this solver reports the failed factorisation.)
            # Device-side select, no host sync; the warning is raised where the host looks at the solve anyway (check_info=True)
            # or, for the sync-free loop, by post_singular_warning() after the loop's own synchronisation.
            singular = self.singular_mask()
            self._last_singular = singular
            delta.masked_fill_(singular.unsqueeze(1), 0.0)
            self.info.masked_fill_(singular, 0)   # a dropped item is not a failed solve
            seen = singular.any()
            self._singular_seen = seen if getattr(self, "_singular_seen", None) is None else (self._singular_seen | seen)
            if check_info:
                self.post_singular_warning()
        if check_info:
            self.check_info()
        return delta


class HipCholeskySolver(HipCholeskyCore, LinearSolver):
    def __init__(self, objective: Objective, linearization_cls: Optional[Type[Linearization]] = None,
                 linearization_kwargs: Optional[Dict[str, Any]] = None, check_singular: bool = False, ordering: str = "auto",
                 **kwargs):
        """``ordering``: "auto" (default) -- a block-compact linearization is factorised in the envelope-reducing order of
        thx_hblock_order, inside the solver only; "natural" -- in the linearization's order."""
        if ordering not in ("auto", "natural"):
            raise ValueError(f"ordering must be 'auto' or 'natural', got {ordering!r}")
        self.ordering = ordering
        linearization_cls = linearization_cls or HipLinearization
        if not (isinstance(linearization_cls, type) and issubclass(linearization_cls, HipLinearization)):
            raise RuntimeError("HipCholeskySolver only works with theseus_amd.HipLinearization, "
                               f"but {linearization_cls} was provided.")
        LinearSolver.__init__(self, objective, linearization_cls, linearization_kwargs)
        self._check_singular = check_singular
        self._core_init()

    # theseus/optimizer/linear/dense_solver.py:84-123
    def solve(self, damping: Optional[Union[float, torch.Tensor]] = None, ellipsoidal_damping: bool = True,
              damping_eps: float = 1e-8, check_info: bool = True, **kwargs) -> torch.Tensor:
        return self._solve(damping, ellipsoidal_damping, damping_eps, check_info)


def _dense_cholesky_only(name: str):
    def method(self, *args, **kwargs):
        raise NotImplementedError(f"{type(self).__name__}.{name}: blocks of right-hand sides, posterior samples and marginal "
                                  "covariances need the dense factor frame of HipCholeskySolver (thx_chol_solve_multi).")
    method.__name__ = name
    return method


class DenseCholeskyOnly:
    """Mixed in FIRST by the cores whose factor is not a dense Cholesky frame (pivoted LU, tile-packed / pattern / level factors,
    the Schur solver): the multi-right-hand-side surface of ``HipCholeskyCore`` raises instead of reading a frame they lack."""
    solve_multi_with_factor = _dense_cholesky_only("solve_multi_with_factor")
    sample_deltas = _dense_cholesky_only("sample_deltas")
    marginal_covariance = _dense_cholesky_only("marginal_covariance")


class HipLUCore(DenseCholeskyOnly, HipCholeskyCore):
    """Back-end half of the pivoted-LU solver: the surface of ``HipCholeskyCore`` that the loops and the autograd nodes call, on
    thx_lu_factor / thx_lu_solve* (include/theseus_hip.h).  P (AtA + damping) = L U; the factor is (``LU``, ``piv``).  The backward
    solves of the differentiated modes use the same factor: AtA + damping is symmetric."""

    def _core_init(self):
        self.K = self.linearization.K
        self.LU = self.piv = self.info = self._y = None
        self._lam = self._frame = None
        self.factor_version = 0

    def _ensure_buffers(self):
        lin = self.linearization
        g = lin.g
        B, n = g.shape[0], lin.n
        if n > _lib.THX_LU_MAX_N:
            raise RuntimeError(f"HipLUSolver: systems of up to {_lib.THX_LU_MAX_N} unknowns (got {n})")
        shape = (B, lin.ld, lin.ld)
        if self.LU is None or tuple(self.LU.shape) != shape or self.LU.device != g.device or self.LU.dtype != g.dtype \
                or self.piv.shape[1] != n:
            # (every buffer is written entirely by the kernels: no initial contents needed)
            self.LU = torch.empty(shape, dtype=g.dtype, device=g.device)
            self.piv = torch.empty(B, n, dtype=torch.int32, device=g.device)
            self._y = torch.empty(B, n, dtype=g.dtype, device=g.device)
            self.info = torch.zeros(B, dtype=torch.int32, device=g.device)
            self._lam = torch.empty(B, dtype=g.dtype, device=g.device)
            self._frame = None

    def _factor_call(self, lam, ellipsoidal_damping, damping_eps, rhs, y, pattern=None):
        lin = self.linearization
        full = getattr(lin, "full_matrix", None)   # a system handed over as plain tensors: any square matrix, used as it is
        if full is not None:
            self.K.lu_factor(full.contiguous(), lin.n, lam, ellipsoidal_damping, damping_eps, self.LU, self.piv, self.info,
                             symmetric_lower=False)
        elif getattr(lin, "_compact", False):
            # block-compact Hessian: one extra pass expands it into a dense frame (blocks are rewritten each time, the zeros
            # between them are written once)
            if self._frame is None:
                self._frame = torch.zeros_like(self.LU)
            self.K.hblocks_expand(lin.hblocks, lin.Hc, self._frame)
            self.K.lu_factor(self._frame, lin.n, lam, ellipsoidal_damping, damping_eps, self.LU, self.piv, self.info)
        else:
            self.K.lu_factor(lin.H, lin.n, lam, ellipsoidal_damping, damping_eps, self.LU, self.piv, self.info)
        if rhs is not None:
            self.K.lu_solve_forward(self.LU, lin.n, self.piv, rhs, y)

    def factor_snapshot(self):
        return self.LU.clone(), self.piv.clone()

    def solve_with_snapshot(self, snapshot, rhs: torch.Tensor) -> torch.Tensor:
        LU, piv = snapshot
        rhs = rhs.contiguous()
        x = torch.empty_like(rhs)
        self.K.lu_solve(LU, self.linearization.n, piv, rhs, x)
        return x

    def _substitute(self, rhs, x, backward_only: bool):
        """x = U^-1 rhs (``backward_only``: rhs is the y of ``factorize``) or (AtA + damping)^-1 rhs with the current factor."""
        if backward_only:
            self.K.lu_solve_backward(self.LU, self.linearization.n, rhs, x)
        else:
            self.K.lu_solve(self.LU, self.linearization.n, self.piv, rhs, x)

    def check_info(self):
        bad = self.info.nonzero()
        if bad.numel():
            b = int(bad[0])
            raise RuntimeError(f"linalg.solve: (Batch element {b}): The solver failed because the input matrix is singular.")


class HipLUSolver(HipLUCore, LinearSolver):
    def __init__(self, objective: Objective, linearization_cls: Optional[Type[Linearization]] = None,
                 linearization_kwargs: Optional[Dict[str, Any]] = None, check_singular: bool = False, ordering: str = "auto",
                 **kwargs):
        """``ordering``: accepted for the constructor it shares with HipCholeskySolver; the pivoted LU chooses its own pivots and
        factorises in the linearization's order."""
        linearization_cls = linearization_cls or HipLinearization
        if not (isinstance(linearization_cls, type) and issubclass(linearization_cls, HipLinearization)):
            raise RuntimeError("HipLUSolver only works with theseus_amd.HipLinearization, "
                               f"but {linearization_cls} was provided.")
        LinearSolver.__init__(self, objective, linearization_cls, linearization_kwargs)
        self._check_singular = check_singular
        self._core_init()

    # theseus/optimizer/linear/dense_solver.py:84-123,125-141
    def solve(self, damping: Optional[Union[float, torch.Tensor]] = None, ellipsoidal_damping: bool = True,
              damping_eps: float = 1e-8, check_info: bool = True, **kwargs) -> torch.Tensor:
        return self._solve(damping, ellipsoidal_damping, damping_eps, check_info)


class HipBandedCholeskyCore(DenseCholeskyOnly, HipCholeskyCore):
    """Back-end half of the banded Cholesky solver: the surface of ``HipCholeskyCore`` that the loops and the autograd nodes call,
    on thx_band_factor / thx_band_solve* (include/theseus_hip.h).  P (AtA + damping) P^T = L L^T with P the band plan's column
    order (theseus_amd/banded.py), found once per structure; the factor is ``Lb`` (B, n, kd + 1), L's band by columns.  The
    linearization's dense frame is read in place through P -- n (kd + 1) elements of it -- and everything a caller hands in or gets
    back stays in the linearization's order.  A failed item raises the RuntimeError of ``HipCholeskyCore.check_info``; the "leading
    minor of order k" it names counts columns in the BANDED order (``band_plan().perm[k - 1]`` is the linearization's column)."""

    def _core_init(self):
        self.K = self.linearization.K
        self.Lb = self.info = self._y = None
        self._lam = self._frame = None
        self._plan = self._perm = None
        self.factor_version = 0

    def band_plan(self):
        """The ``banded.BandPlan`` of the linearization's structure (made on first use, kept)."""
        if self._plan is None:
            from .banded import band_plan
            self._plan = band_plan(self.linearization, "natural" if self.ordering == "natural" else "auto")
        return self._plan

    def _ensure_buffers(self):
        lin = self.linearization
        g = lin.g
        plan = self.band_plan()
        B, n = g.shape[0], lin.n
        if plan.n != n:
            raise RuntimeError(f"HipBandedCholeskySolver: the band plan was made for {plan.n} columns, the linearization has {n}")
        shape = (B, n, plan.kd + 1)
        if self.Lb is None or tuple(self.Lb.shape) != shape or self.Lb.device != g.device or self.Lb.dtype != g.dtype:
            # (every buffer is written entirely by the kernels: no initial contents needed)
            self.Lb = torch.empty(shape, dtype=g.dtype, device=g.device)
            self._y = torch.empty(B, n, dtype=g.dtype, device=g.device)
            self.info = torch.zeros(B, dtype=torch.int32, device=g.device)
            self._lam = torch.empty(B, dtype=g.dtype, device=g.device)
            self._perm = plan.device_perm(g.device)
            self._frame = None

    def _factor_call(self, lam, ellipsoidal_damping, damping_eps, rhs, y, pattern=None):
        lin, plan = self.linearization, self._plan
        if getattr(lin, "_compact", False):
            # block-compact Hessian: one extra pass expands it into a dense frame (blocks are rewritten each time, the zeros
            # between them are written once)
            if self._frame is None:
                self._frame = torch.zeros(self.Lb.shape[0], lin.ld, lin.ld, dtype=self.Lb.dtype, device=self.Lb.device)
            self.K.hblocks_expand(lin.hblocks, lin.Hc, self._frame)
            H = self._frame
        else:
            H = lin.H
        self.K.band_factor(H, lin.n, plan.kd, self._perm, lam, ellipsoidal_damping, damping_eps, self.Lb, self.info,
                           rhs=rhs.contiguous() if rhs is not None else None, y=y)

    def factor_snapshot(self):
        return self.Lb.clone()

    def solve_with_snapshot(self, snapshot, rhs: torch.Tensor) -> torch.Tensor:
        rhs = rhs.contiguous()
        x = torch.empty_like(rhs)
        self.K.band_solve(snapshot, self.linearization.n, self._plan.kd, self._perm, rhs, x)
        return x

    def _substitute(self, rhs, x, backward_only: bool):
        """x = P^T L^-T rhs (``backward_only``: rhs is the y of ``factorize``, in banded order) or (AtA + damping)^-1 rhs with the
        current factor."""
        solve = self.K.band_solve_backward if backward_only else self.K.band_solve
        solve(self.Lb, self.linearization.n, self._plan.kd, self._perm, rhs, x)


class HipBandedCholeskySolver(HipBandedCholeskyCore, LinearSolver):
    def __init__(self, objective: Objective, linearization_cls: Optional[Type[Linearization]] = None,
                 linearization_kwargs: Optional[Dict[str, Any]] = None, check_singular: bool = False, ordering: str = "auto",
                 **kwargs):
        """Opt-in solver for objectives whose Hessian is banded in some order of the variables (trajectories, odometry chains):
        ``linear_solver_cls=HipBandedCholeskySolver``.  ``ordering``: "auto" (default) -- reverse Cuthill-McKee on the variable
        graph unless the linearization's own order is no wider; "natural" -- the linearization's own order.  The first solve raises
        ``UnsupportedObjective`` when the half-bandwidth exceeds ``THX_BAND_MAX_KD``."""
        if ordering not in ("auto", "natural"):
            raise ValueError(f"ordering must be 'auto' or 'natural', got {ordering!r}")
        self.ordering = ordering
        linearization_cls = linearization_cls or HipLinearization
        if not (isinstance(linearization_cls, type) and issubclass(linearization_cls, HipLinearization)):
            raise RuntimeError("HipBandedCholeskySolver only works with theseus_amd.HipLinearization, "
                               f"but {linearization_cls} was provided.")
        LinearSolver.__init__(self, objective, linearization_cls, linearization_kwargs)
        self._check_singular = check_singular
        self._core_init()

    def solve(self, damping: Optional[Union[float, torch.Tensor]] = None, ellipsoidal_damping: bool = True,
              damping_eps: float = 1e-8, check_info: bool = True, **kwargs) -> torch.Tensor:
        return self._solve(damping, ellipsoidal_damping, damping_eps, check_info)
