"""`LinearSolver` plugin surface + the HIP dense Cholesky, pivoted-LU and banded Cholesky solvers.

ABC contract: theseus/optimizer/linear/linear_solver.py:15-37.  ``HipCholeskySolver`` replaces
``CholeskyDenseSolver`` (theseus/optimizer/linear/dense_solver.py:20-161): damping semantics of
``DenseSolver._apply_damping`` (:38-64, out of place), ``torch.linalg.cholesky`` +
``torch.cholesky_solve`` (:159-161) become one batched tiled HIP factorisation + two triangular
solves; a non positive-definite system raises ``RuntimeError`` like ``torch.linalg.cholesky`` does.
``HipLUSolver`` replaces ``LUDenseSolver`` (dense_solver.py:125-141) for systems that are not numerically positive
definite: ``torch.linalg.lu_factor`` + ``lu_solve`` become thx_lu_factor + thx_lu_solve*.

One core, ``FactorCore``, owns what the loops and the autograd nodes call; the back ends (``HipCholeskyCore``, ``HipLUCore``,
``HipBandedCholeskyCore``; theseus_amd/sparse.py: ``HipSparseCholeskyCore``) are siblings that implement its hooks.
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


def check_damping(damping):
    if damping is not None and isinstance(damping, torch.Tensor) and damping.ndim > 1:
        raise ValueError("Damping must be a float or a 1-D tensor.")


def checked_linearization_cls(name: str, linearization_cls, required=HipLinearization, required_name="theseus_amd.HipLinearization"):
    """``linearization_cls`` of solver class ``name`` (None: ``required``), refused unless it is a subclass of ``required``."""
    linearization_cls = linearization_cls or required
    if not (isinstance(linearization_cls, type) and issubclass(linearization_cls, required)):
        raise RuntimeError(f"{name} only works with {required_name}, but {linearization_cls} was provided.")
    return linearization_cls


_NO_ORDERING = object()


def init_solver(solver, name: str, objective, linearization_cls, linearization_kwargs, check_singular, ordering=_NO_ORDERING, *,
                base=LinearSolver, required=HipLinearization, required_name="theseus_amd.HipLinearization"):
    """The constructor the solver classes share: the ``ordering`` check (where the solver has one), the linearization-class check,
    ``base.__init__`` (the ``LinearSolver`` of this package, or the reference's: theseus_amd/plugin.py) and the core's buffers."""
    if ordering is not _NO_ORDERING:
        if ordering not in ("auto", "natural"):
            raise ValueError(f"ordering must be 'auto' or 'natural', got {ordering!r}")
        solver.ordering = ordering
    base.__init__(solver, objective, checked_linearization_cls(name, linearization_cls, required, required_name), linearization_kwargs)
    solver._check_singular = check_singular
    solver._core_init()


class FactorCore:
    """Back-end half of a solver, shared by theseus_amd's mirror classes below and the adapters for the real ``theseus``
    (theseus_amd/plugin.py): everything the loops and the autograd nodes call that does not depend on how a factor is stored.
    A back end implements the hooks

      ``_core_init()``                             its attributes (extends this one's)
      ``_ensure_buffers()``                        (re)allocates factor, ``_y`` (B, n), ``info`` (B,) int32 and ``_lam`` (B,)
      ``_factor_call(lam, ellipsoidal, eps, rhs)`` the factorisation launches; with ``rhs`` the forward substitution too: returns
                                                   its y (a handle ``_substitute(backward_only=True)`` recognises), else None
      ``_substitute(rhs, x, backward_only)``       x = (factor)^-1 rhs, or the backward half on the y of ``_factor_call``
      ``factor_snapshot()`` / ``solve_with_snapshot(snapshot, rhs)``

    and, where its factor serves blocks of right-hand sides, ``_apply_multi`` (dense Cholesky: thx_chol_solve_multi, banded
    Cholesky: thx_pb_solve_multi, tile-sparse Cholesky: thx_chol_solve_multi_sparse, and the bundle-adjustment Schur core
    (theseus_amd/ba.py): thx_ba_reduce_multi / thx_ba_backsub_multi around those solves, both bound per instance when the kernel
    set has them; the others leave it None and the multi-right-hand-side surface raises)."""

    def _core_init(self):
        self.K = self.linearization.K
        self.info = self._y = self._lam = None
        self.factor_version = 0  # bumped by every factorisation (the implicit backward checks its factor is current)

    def _linearized(self) -> bool:
        lin = self.linearization
        return lin.linearized if hasattr(lin, "linearized") else lin.H is not None

    def _lam_of(self, damping: Optional[Union[float, torch.Tensor]]) -> Optional[torch.Tensor]:
        """None, or the solver's (B,) ``_lam`` filled with ``damping`` (a float, or a tensor that expands to the batch)."""
        if damping is None:
            return None
        lam = self._lam
        if isinstance(damping, torch.Tensor):
            lam.copy_(damping.to(lam.dtype).expand(lam.shape[0]))
        else:
            lam.fill_(float(damping))
        return lam

    def factorize(self, damping: Optional[Union[float, torch.Tensor]] = None, ellipsoidal_damping: bool = True,
                  damping_eps: float = 1e-8, rhs: Optional[torch.Tensor] = None):
        """Factorises AtA (+ damping) and keeps the factor for later solves (the implicit backward re-uses it).  With ``rhs`` the
        forward substitution is fused into the factorisation (no extra pass over the factor) and its y is returned."""
        if not self._linearized():
            raise RuntimeError("linearize() must be called before solve().")
        self._ensure_buffers()
        lam = self._lam_of(damping)
        self.factor_version += 1
        self._factored_with = (lam is not None, bool(ellipsoidal_damping), float(damping_eps))   # (what the factor is the factor of)
        return self._factor_call(lam, ellipsoidal_damping, damping_eps, rhs)

    def solve_with_factor(self, rhs: torch.Tensor) -> torch.Tensor:
        """(AtA + damping)^-1 rhs with the cached factor (forward + backward substitution kernels)."""
        rhs = rhs.contiguous()
        x = torch.empty_like(rhs)
        self._substitute(rhs, x, backward_only=False)
        return x

    # ---- blocks of right-hand sides on the cached factor: posterior samples, marginal covariances ------------------------------
    # hook ``_apply_multi(x, which, scratch=False)``: the factor applied to the (B, k, n) block ``x`` (the solver's dtype, any
    # strides), which = 0: (L L^T)^-1 x, 1: L^-T x, 2: L^-1 x (the codes of thx_chol_solve_levels); returns a tensor the caller
    # may keep and leaves ``x`` alone -- unless ``scratch``: then x is a contiguous block of the caller's own, its columns where
    # ``_factor_cols`` puts them, and may be overwritten.
    _apply_multi = None

    def _need_multi(self, name: str):
        if self._apply_multi is None:
            raise NotImplementedError(f"{type(self).__name__}.{name}: blocks of right-hand sides, posterior samples and marginal "
                                      "covariances need the dense factor frame of HipCholeskySolver (thx_chol_solve_multi).")

    def _factor_cols(self, idx: torch.Tensor) -> torch.Tensor:
        """Where ``_apply_multi(which=0, scratch=True)`` keeps the linearization's columns ``idx``."""
        return idx

    def _factor_owner(self) -> "FactorCore":
        """The core that holds the factor ``solve()`` left (theseus_amd/plugin.py: a system handed over as tensors has its own)."""
        return self

    def _factorize_undamped(self) -> "FactorCore":
        """The factor of AtA of the linearization as it stands; returns the core that holds it."""
        self.factorize(None)
        self.check_info()
        return self

    def _sampling_solve(self) -> torch.Tensor:
        """delta of ``sample_deltas``: the undamped ``solve()`` whose factor the draw is made with."""
        return self.solve()

    def solve_multi_with_factor(self, rhs: torch.Tensor, which: int = 0) -> torch.Tensor:
        """``rhs`` (B, k, n), one vector per row, against the CURRENT factor P (AtA + damping) P^T = L L^T (P: the order the solver
        factorised in): which = 0: (L L^T)^-1 rhs, in and out in the linearization's order; 2: L^-1 P rhs -- linearization's order
        in, the solver's own out; 1: P^T L^-T rhs -- the solver's order in, linearization's out (1 after 2 is 0).  Dense frame:
        every group of 32 vectors reads L once per substitution; band: one wave per 64 vectors.  Returns a new tensor."""
        self._need_multi("solve_multi_with_factor")
        own = self._factor_owner()
        if own is None or own.factor_version == 0:
            raise RuntimeError("solve_multi_with_factor: nothing has been factorised yet (solve() or factorize() first).")
        B, n = own._y.shape[0], own.linearization.n
        if rhs.dim() != 3 or rhs.shape[0] != B or rhs.shape[2] != n or rhs.shape[1] < 1:
            raise ValueError(f"solve_multi_with_factor: rhs must be (B = {B}, k >= 1, n = {n}), got {tuple(rhs.shape)}")
        return own._apply_multi(rhs.detach().to(own._y.dtype), which)

    @torch.no_grad()
    def sample_deltas(self, n_samples: int = 10, temperature: float = 1.0, noise: Optional[torch.Tensor] = None,
                      generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """The ``delta_samples`` of TheseusLayer.compute_samples (theseus/theseus_layer.py:110-123), (B, n, n_samples): draws from
        N(delta, (AtA / temperature)^-1) as  delta + sqrt(temperature) P^T L^-T y  with delta = ``solve()`` (undamped, on the
        linearization as it stands) and L the factor that solve just left -- the reference factorises AtA / temperature a second
        time, densely.  ``noise``: y as (n, n_samples), shared by the batch as in the reference, or (B, n, n_samples); None: drawn
        with ``generator``.  The result is a permuted view of the kernel's (B, n_samples, n) output.  The distribution is the same
        on every back end; the DRAW that a given ``noise`` stands for is the reference's on the dense solver (the factor of AtA in
        the linearization's order) and another square root of the same covariance on the band factor (its banded order)."""
        self._need_multi("sample_deltas")
        if not temperature > 0:
            raise ValueError(f"sample_deltas: temperature must be positive, got {temperature}")
        if int(n_samples) < 1:
            raise ValueError(f"sample_deltas: n_samples must be at least 1, got {n_samples}")
        delta = self._sampling_solve()
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
        out = own._apply_multi(y.to(device=delta.device, dtype=delta.dtype), 1)
        out.mul_(math.sqrt(float(temperature))).add_(delta.unsqueeze(1))
        return out.transpose(1, 2)

    @torch.no_grad()
    def marginal_covariance(self, var_names: Sequence[str]) -> torch.Tensor:
        """(B, d, d): the rows and columns of (AtA)^-1 at the columns of the named optimisation variables (any set of them), in the
        order given -- their joint marginal covariance in the tangent space at the linearization point.  Factorises undamped and
        solves against the d unit vectors of those columns (one multi-vector kernel call)."""
        self._need_multi("marginal_covariance")
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
        B, n, d = own._y.shape[0], own.linearization.n, len(cols)   # (n: of the linearization -- a Schur core's _y is the camera part)
        idx = own._factor_cols(torch.tensor(cols, dtype=torch.long, device=own._y.device))
        E = torch.zeros(B, d, n, dtype=own._y.dtype, device=own._y.device)
        E[:, torch.arange(d, device=idx.device), idx] = 1
        C = own._apply_multi(E, 0, scratch=True)[:, :, idx]
        return (C + C.transpose(1, 2)) / 2

    # ---- failures, check_singular, the solve ---------------------------------------------------------------------------------------
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
        check_damping(damping)
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


class _FactorSnapshot(tuple):
    """(L, panels) of ``factor_snapshot`` with the order the factor was made in (``ordered``: HipCholeskyCore._factor_ord)."""
    ordered = None


class DenseFrameCore(FactorCore):
    """The dense factor frame ``_L`` (B, ld, ld) with its solve panels, factorised in the linearization's order -- as a whole, or
    along a tile pattern (theseus_amd/sparse.py).  What ``HipCholeskyCore`` and ``HipSparseCholeskyCore`` share."""

    def _core_init(self):
        FactorCore._core_init(self)
        self._L = self._panels = None

    @property
    def L(self):
        return self._L

    @L.setter
    def L(self, value):
        self._L = value

    @property
    def panels(self):
        return self._panels

    @panels.setter
    def panels(self, value):
        self._panels = value

    def _ensure_buffers(self):
        lin = self.linearization
        g = lin.g     # (B, n): shape / dtype / device of the system (lin.H may be block-compact: never touched here)
        shape = (g.shape[0], lin.ld, lin.ld)
        if self._L is None or tuple(self._L.shape) != shape or self._L.device != g.device or self._L.dtype != g.dtype:
            B = g.shape[0]
            nt = (lin.n + _lib.THX_TILE - 1) // _lib.THX_TILE
            self._L = torch.zeros(shape, dtype=g.dtype, device=g.device)
            self._panels = torch.empty(B, nt, _lib.THX_TILE, _lib.THX_TILE, dtype=g.dtype, device=g.device)
            self._y = torch.empty(B, lin.n, dtype=g.dtype, device=g.device)
            self.info = torch.zeros(B, dtype=torch.int32, device=g.device)
            self._lam = torch.empty(B, dtype=g.dtype, device=g.device)
            self._unfused_forward = False   # (decided per system size: see _solve)

    def _factor_call(self, lam, ellipsoidal_damping, damping_eps, rhs, pattern=None):
        """One factorisation launch sequence: H from the block list when the linearization keeps it compact."""
        lin = self.linearization
        y = self._y if rhs is not None else None
        if getattr(lin, "_compact", False):
            self.K.chol_factor_hblocks(lin.hblocks, lin.Hc, lin.n, lam, ellipsoidal_damping, damping_eps, self._L, self._panels,
                                       self.info, pattern=pattern, rhs=rhs, y=y)
        elif pattern is not None:
            self.K.chol_factor_sparse(lin.H, lin.n, lam, ellipsoidal_damping, damping_eps, self._L, self._panels, self.info,
                                      pattern, rhs=rhs, y=y)
        else:
            self.K.chol_factor(lin.H, lin.n, lam, ellipsoidal_damping, damping_eps, self._L, self._panels, self.info, rhs=rhs, y=y)
        return y

    def factor_snapshot(self):
        """A private copy of the CURRENT factor, for a solve after the solver has factorised again (the differentiated iterations
        of BackwardMode.UNROLL / TRUNCATED: every iteration's backward solves with that iteration's factor)."""
        return _FactorSnapshot((self._L.clone(), self._panels.clone()))


class HipCholeskyCore(DenseFrameCore):
    """The dense tiled Cholesky: the whole frame, in the linearization's order or the solver's own (``ordering``), solved along the
    row envelope; its frame serves blocks of right-hand sides (thx_chol_solve_multi)."""

    # "auto": a block-compact linearization is factorised in the order of thx_hblock_order -- the columns of H, L, g and x inside
    # the solver follow the permutation, everything a caller hands in or gets back stays in the linearization's order;
    # "natural": the linearization's own order
    ordering = "auto"

    def _core_init(self):
        DenseFrameCore._core_init(self)
        self._factor_ord = None  # (layout, maps) of compiler.OrderedHessianBlocks the CURRENT factor was made in, None: natural order
        self._Hp = self._gp = self._xp = None
        self._natural_frame = None
        self._force_natural = False

    # ---- the factor frame as callers see it ---------------------------------------------------------------------------------------
    @DenseFrameCore.L.getter
    def L(self):
        """The factor frame in the LINEARIZATION's order (tests / inspection; the solver itself works on ``_L``).  After a
        factorisation in the solver's own order that is a second factorisation of the same system -- the linearization as it
        stands, the damping of the last ``factorize`` -- in the natural order, made on first use and kept until the next one."""
        return self._L if self._factor_ord is None else self._natural_factor()[0]

    @DenseFrameCore.panels.getter
    def panels(self):
        return self._panels if self._factor_ord is None else self._natural_factor()[1]

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
        frame = self._L
        DenseFrameCore._ensure_buffers(self)
        if self._L is not frame:
            self._Hp = self._gp = self._xp = self._natural_frame = None

    def _factor_call(self, lam, ellipsoidal_damping, damping_eps, rhs):
        lin = self.linearization
        self._factor_ord = self._natural_frame = None
        ordered = self._ordered()
        if ordered is None:
            return DenseFrameCore._factor_call(self, lam, ellipsoidal_damping, damping_eps, rhs)
        # the solver's own order: the block list moves into the permuted layout's block order (a block whose variables swap
        # sides of the diagonal transposed), g is gathered; ``y`` comes out in the permuted order and stays there -- the
        # backward substitution recognises it (_substitute)
        layout, maps = ordered
        y = self._y if rhs is not None else None
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
        return y

    def factor_snapshot(self):
        snap = DenseFrameCore.factor_snapshot(self)
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

    # ---- blocks of right-hand sides (thx_chol_solve_multi) -----------------------------------------------------------------------
    def _apply_multi(self, x, which, scratch=False):
        """In place on a copy of ``x`` (on ``x`` itself: ``scratch``)."""
        maps = self._factor_ord[1] if (self._factor_ord is not None and not scratch) else None
        # (a factor of the solver's own order, P H P^T = L L^T: which = 0 is H^-1 whatever the order; L^-1 takes its vectors in the
        #  linearization's order and L^-T returns them in it -- L^-T (L^-1 rhs) is H^-1 rhs)
        if maps is not None and which != 1:
            x = x.index_select(2, maps["to_perm"].long())
        if not scratch:
            x = x.clone(memory_format=torch.contiguous_format)
        self.K.chol_solve_multi(self._L, self.linearization.n, self._panels, x, x, which=which)
        if maps is not None and which != 2:
            x = x.index_select(2, maps["from_perm"].long())
        return x

    def _factor_cols(self, idx):
        # (the factor's own order: the same columns, where it keeps them)
        return idx if self._factor_ord is None else self._factor_ord[1]["from_perm"].long()[idx]

    def _sampling_solve(self):
        # (the draw that a given ``noise`` stands for is defined through the factor of AtA in the linearization's order,
        #  theseus_layer.py:113-123: this solve factorises in that order)
        self._force_natural = True
        try:
            return self.solve()
        finally:
            self._force_natural = False


class HipCholeskySolver(HipCholeskyCore, LinearSolver):
    def __init__(self, objective: Objective, linearization_cls: Optional[Type[Linearization]] = None,
                 linearization_kwargs: Optional[Dict[str, Any]] = None, check_singular: bool = False, ordering: str = "auto",
                 **kwargs):
        """``ordering``: "auto" (default) -- a block-compact linearization is factorised in the envelope-reducing order of
        thx_hblock_order, inside the solver only; "natural" -- in the linearization's order."""
        init_solver(self, "HipCholeskySolver", objective, linearization_cls, linearization_kwargs, check_singular, ordering)

    # theseus/optimizer/linear/dense_solver.py:84-123
    def solve(self, damping: Optional[Union[float, torch.Tensor]] = None, ellipsoidal_damping: bool = True,
              damping_eps: float = 1e-8, check_info: bool = True, **kwargs) -> torch.Tensor:
        return self._solve(damping, ellipsoidal_damping, damping_eps, check_info)


class HipLUCore(FactorCore):
    """Back-end half of the pivoted-LU solver, on thx_lu_factor / thx_lu_solve* (include/theseus_hip.h).  P (AtA + damping) = L U;
    the factor is (``LU``, ``piv``).  The backward solves of the differentiated modes use the same factor: AtA + damping is
    symmetric."""

    def _core_init(self):
        FactorCore._core_init(self)
        self.LU = self.piv = self._frame = None

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

    def _factor_call(self, lam, ellipsoidal_damping, damping_eps, rhs):
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
        if rhs is None:
            return None
        self.K.lu_solve_forward(self.LU, lin.n, self.piv, rhs, self._y)
        return self._y

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
        init_solver(self, "HipLUSolver", objective, linearization_cls, linearization_kwargs, check_singular)

    # theseus/optimizer/linear/dense_solver.py:84-123,125-141
    def solve(self, damping: Optional[Union[float, torch.Tensor]] = None, ellipsoidal_damping: bool = True,
              damping_eps: float = 1e-8, check_info: bool = True, **kwargs) -> torch.Tensor:
        return self._solve(damping, ellipsoidal_damping, damping_eps, check_info)


class HipBandedCholeskyCore(FactorCore):
    """Back-end half of the banded Cholesky solver, on thx_band_factor / thx_band_solve* (include/theseus_hip.h).
    P (AtA + damping) P^T = L L^T with P the band plan's column order (theseus_amd/banded.py), found once per structure; the factor
    is ``Lb`` (B, n, kd + 1), L's band by columns.  The linearization's dense frame is read in place through P -- n (kd + 1)
    elements of it -- and everything a caller hands in or gets back stays in the linearization's order.  A failed item raises the
    RuntimeError of ``FactorCore.check_info``; the "leading minor of order k" it names counts columns in the BANDED order
    (``band_plan().perm[k - 1]`` is the linearization's column)."""

    ordering = "auto"

    def _core_init(self):
        FactorCore._core_init(self)
        self.Lb = self._frame = None
        self._plan = self._perm = self._marg_index = None

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

    def _factor_call(self, lam, ellipsoidal_damping, damping_eps, rhs):
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
        y = self._y if rhs is not None else None
        self.K.band_factor(H, lin.n, plan.kd, self._perm, lam, ellipsoidal_damping, damping_eps, self.Lb, self.info,
                           rhs=rhs.contiguous() if rhs is not None else None, y=y)
        return y

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

    # ---- blocks of right-hand sides on the band factor (thx_pb_solve_multi, thx_pb_inverse_band) ------------------------------------
    def _need_multi(self, name: str):
        """The kernel set must carry the band factor's multi-vector kernels; one that does not (a kernel set handed in through
        ``linearization_kwargs`` that predates them) is an error here, never a detour through another path."""
        if not (hasattr(self.K, "band_solve_multi") and hasattr(self.K, "band_inverse")):
            raise NotImplementedError(f"{type(self).__name__}.{name}: the kernel set {type(self.K).__name__} has no band_solve_multi / "
                                      "band_inverse (thx_pb_solve_multi, thx_pb_inverse_band) for the band factor; HipCholeskySolver "
                                      "serves blocks of right-hand sides on its dense factor frame (thx_chol_solve_multi).")

    def _apply_multi(self, x, which, scratch=False):
        """Out of place; the kernel reads and writes the linearization's order through P itself."""
        x = x.to(self.Lb.device).contiguous()
        out = torch.empty_like(x)
        self.K.band_solve_multi(self.Lb, self.linearization.n, self._plan.kd, self._perm, x, out, which=which)
        return out

    @torch.no_grad()
    def marginal_covariances(self) -> Dict[str, torch.Tensor]:
        """{name: (B, d_k, d_k)}: EVERY optimisation variable's own marginal covariance -- the diagonal blocks of (AtA)^-1 -- from
        one undamped factorisation and ONE thx_pb_inverse_band launch (the band of the inverse by selected inversion, n kd^2 flops:
        the cost of the factorisation, where unit-vector solves cost n^2 kd).  A variable's columns are contiguous in the banded
        order, so its block lies inside the band when d_k - 1 <= kd; a wider variable raises."""
        self._need_multi("marginal_covariances")
        lin = self.linearization
        plan = self.band_plan()
        wide = [lin.ordering[k].name for k, d in enumerate(lin.var_dims) if d - 1 > plan.kd]
        if wide:
            raise RuntimeError(f"marginal_covariances: the blocks of {wide} are wider than the band (kd = {plan.kd}); use "
                               "marginal_covariance(names) for them.")
        self._factorize_undamped()
        n = lin.n
        Zb = torch.empty_like(self.Lb)
        self.K.band_inverse(self.Lb, n, plan.kd, Zb)
        if getattr(self, "_marg_index", None) is None or self._marg_index[0] is not plan or self._marg_index[1] != Zb.device:
            # per block size d: (variables, J, I) with block k of that size = Zb[:, J[k], I[k]] -- S(p0 + hi, p0 + lo), symmetric
            pos = torch.empty(n, dtype=torch.long)
            pos[torch.from_numpy(plan.perm).long()] = torch.arange(n)      # banded position of a linearization column
            groups = {}
            for k, (c0, d) in enumerate(zip(lin.var_start_cols, lin.var_dims)):
                p0 = int(pos[c0])
                if pos[c0:c0 + d].tolist() != list(range(p0, p0 + d)):
                    raise RuntimeError(f"marginal_covariances: the columns of {lin.ordering[k].name!r} are not contiguous in the band plan")
                groups.setdefault(int(d), []).append((lin.ordering[k].name, p0))
            index = []
            for d, members in groups.items():
                r = torch.arange(d)
                hi, lo = torch.maximum(r[:, None], r[None, :]), torch.minimum(r[:, None], r[None, :])
                p0 = torch.tensor([p for _, p in members]).view(-1, 1, 1)
                index.append(([name for name, _ in members], (p0 + lo).to(Zb.device), (hi - lo).expand(len(members), d, d).to(Zb.device)))
            self._marg_index = (plan, Zb.device, index)
        out = {}
        for names, J, I in self._marg_index[2]:        # one gather per block size
            out.update(zip(names, Zb[:, J, I].unbind(1)))
        return out


class HipBandedCholeskySolver(HipBandedCholeskyCore, LinearSolver):
    def __init__(self, objective: Objective, linearization_cls: Optional[Type[Linearization]] = None,
                 linearization_kwargs: Optional[Dict[str, Any]] = None, check_singular: bool = False, ordering: str = "auto",
                 **kwargs):
        """Opt-in solver for objectives whose Hessian is banded in some order of the variables (trajectories, odometry chains):
        ``linear_solver_cls=HipBandedCholeskySolver``.  ``ordering``: "auto" (default) -- reverse Cuthill-McKee on the variable
        graph unless the linearization's own order is no wider; "natural" -- the linearization's own order.  The first solve raises
        ``UnsupportedObjective`` when the half-bandwidth exceeds ``THX_BAND_MAX_KD``."""
        init_solver(self, "HipBandedCholeskySolver", objective, linearization_cls, linearization_kwargs, check_singular, ordering)

    def solve(self, damping: Optional[Union[float, torch.Tensor]] = None, ellipsoidal_damping: bool = True,
              damping_eps: float = 1e-8, check_info: bool = True, **kwargs) -> torch.Tensor:
        return self._solve(damping, ellipsoidal_damping, damping_eps, check_info)
