"""DCEM, the differentiable cross-entropy method (theseus/optimizer/nonlinear/dcem.py:26-248): a sampling optimizer.  Per iteration
it draws ``n_sample`` states X = mu + sigma * eps around the current one, evaluates the objective at each, turns the errors into
weights -- the LML projection onto "n_elite of them" (theseus/third_party/lml.py), a softmax for ``n_elite == 1``, hard top-k for
``temp=None`` -- and moves to the weighted mean; sigma becomes the weighted standard deviation.

What runs where:
  sampling      one torch ``addcmul`` into a sample-major (S, B, n) buffer: every X[s] is a contiguous (B, n) state;
  evaluation    ``packed.error_metric(state=X[s], out=fX[s])``: one fused ``*_error`` launch per sample for the term-table families
                (theseus_amd/term_table.py), the torch classes for generic objectives and whenever something is differentiated;
  update        ``thx_dcem_update`` (csrc/dcem_kernels.hip), one workgroup per problem, and ``thx_dcem_update_vjp`` behind it:
                ``DcemUpdate`` below, one autograd node, used under no_grad and with gradients alike;
  bookkeeping   histories, best solution, final info: the ``_RunTracker`` of theseus_amd/nonlinear.py (``record``, ``finish``), as in LM;
  no linear solver and no linearization are constructed.
``dcem_update_torch`` is the same function on plain torch, written from the formulas: the comparator of the tests (and of
tools/bench_dcem.py).  The optimizer never calls it.

Only objectives whose optimisation variables are all Euclidean are accepted (the packers of group "Euclidean": the generic one,
PackedTrajectory2D, PackedHomography, PackedKinematics): a sample is ``mu + sigma * eps`` on the variables' tensors, which is what
the reference does for every variable (``_mu_vec_to_dict`` slices ``var.tensor`` by ``dof()``) and is wrong for Lie groups there.
"""
import math
from typing import Callable, Optional, Union

import torch

from . import _lib
from .core import Objective
from .euclidean import _is_euclidean
from .generic import PackedState
from .linearization import VariableOrdering
from .nonlinear import BackwardMode, NonlinearLeastSquares, NonlinearOptimizerInfo, NonlinearOptimizerParams, _RunTracker
from .packed import UnsupportedObjective, packed_for

LML_N_ITER = 100   # rounds of the LML bracketing at most (lml.py:39)


def _is_hard(temp) -> bool:
    return temp is None or not (temp < math.inf)   # (dcem.py:117)


# ------------------------------------------------------------------------------------------------------------------------------
# the update on plain torch
# ------------------------------------------------------------------------------------------------------------------------------
class _LMLTorch(torch.autograd.Function):
    """y = sigmoid(x + nu) with sum(y) = N: the bracketing search of lml.py:88-129 on (B, S) scores, every problem on its own
    (a problem's bracket moves only while it is wider than eps, as there), and the backward of lml.py:169-171."""

    @staticmethod
    def forward(ctx, x, N, eps, n_iter, branch):
        B, S = x.shape
        flags = torch.zeros(B, dtype=torch.int32, device=x.device)
        if S <= N:
            y = (1.0 - 1e-5) * torch.ones_like(x)
            ctx.dead = True
            zero = torch.zeros(B, dtype=x.dtype, device=x.device)
            ctx.mark_non_differentiable(flags)
            return y, zero, torch.zeros(B, 2, dtype=x.dtype, device=x.device), flags, zero.new_full((), math.inf)
        x_sorted, _ = torch.sort(x, dim=1, descending=True)
        lo = -x_sorted[:, N - 1] - 7.0
        hi = -x_sorted[:, N] + 7.0
        ls = torch.linspace(0, 1, branch, dtype=x.dtype, device=x.device)
        margin = x.new_full((), math.inf)   # the smallest |grid value| met: how close a count came to depending on rounding
        for _ in range(n_iter):
            r = hi - lo
            live = r > eps
            if not bool(live.any()):
                break
            nus = r.unsqueeze(1) * ls + lo.unsqueeze(1)
            fs = torch.sigmoid(x.unsqueeze(1) + nus.unsqueeze(2)).sum(dim=2) - N
            margin = torch.minimum(margin, fs[live].abs().min())
            i_lower = (fs < 0).sum(dim=1) - 1
            none = i_lower < 0
            flags = flags | (none & live).int() * _lib.DCEM_FLAG_ALL_NONNEG
            i_lower = i_lower.clamp(0, branch - 2)
            new_lo = nus.gather(1, i_lower.unsqueeze(1)).squeeze(1) - 7.0 * none.to(x.dtype)
            new_hi = nus.gather(1, (i_lower + 1).unsqueeze(1)).squeeze(1)
            lo, hi = torch.where(live, new_lo, lo), torch.where(live, new_hi, hi)
        r = hi - lo
        flags = flags | (r > eps).int() * _lib.DCEM_FLAG_NOT_CONVERGED
        nu = lo + r / 2.0
        y = torch.sigmoid(x + nu.unsqueeze(1))
        ctx.dead = False
        ctx.save_for_backward(y)
        bracket = torch.stack([lo, hi], dim=1)
        ctx.mark_non_differentiable(nu, bracket, flags, margin)
        return y, nu, bracket, flags, margin

    @staticmethod
    def backward(ctx, g, *unused):
        if ctx.dead:
            return torch.zeros_like(g), None, None, None, None
        (y,) = ctx.saved_tensors
        hinv = 1.0 / (1.0 / y + 1.0 / (1.0 - y))
        dnu = (hinv * g).sum(dim=1) / hinv.sum(dim=1)
        return hinv * (g - dnu.unsqueeze(1)), None, None, None, None


def dcem_update_torch(fX: torch.Tensor, X: torch.Tensor, n_elite: int, temp: Optional[float] = 1.0, normalize: bool = True,
                      lml_eps: float = 1e-3, lml_n_iter: int = LML_N_ITER, branch: int = 100, with_margin: bool = False):
    """fX (S, B), X (S, B, n) -> mu, sigma (B, n), w (B, S), nu (B), bracket (B, 2), flags (B) int32 [, margin]: what
    ``thx_dcem_update`` computes (include/theseus_hip.h), in the reference's own order of torch operations (dcem.py:117-154), so
    that on the reference's device and dtype it gives the reference's bits.  Differentiable w.r.t. fX and X, the LML step by its
    implicit backward.  ``margin`` (``with_margin``): the smallest |grid value| of the LML rounds, inf in the other modes."""
    S, B = fX.shape
    N = int(n_elite)
    if N < 1:
        raise ValueError("dcem_update_torch: n_elite < 1")
    f = fX.t().contiguous()   # (B, S), as the reference stacks it
    zero = torch.zeros(B, dtype=fX.dtype, device=fX.device)
    nu, bracket = zero, torch.zeros(B, 2, dtype=fX.dtype, device=fX.device)
    flags = torch.zeros(B, dtype=torch.int32, device=fX.device)
    margin = zero.new_full((), math.inf)
    if not _is_hard(temp):
        if normalize:
            f = (f - f.mean(dim=1).unsqueeze(1)) / (f.std(dim=1).unsqueeze(1) + 1e-6)
        if N == 1:
            w = torch.softmax(-f * temp, dim=1)
        else:
            w, nu, bracket, flags, margin = _LMLTorch.apply(-f * temp, N, float(lml_eps), int(lml_n_iter), int(branch))
        eps = 0.0
    else:
        idx = f.argsort(dim=1, stable=True)[:, :N]
        w = torch.zeros(B, S, dtype=fX.dtype, device=fX.device).scatter_(1, idx, 1.0)
        eps = 1e-10
    w3 = w.unsqueeze(2)
    Xt = X.transpose(0, 1)
    mu = torch.sum(w3 * Xt, dim=1) / N
    sigma = ((w3 * (Xt - mu.unsqueeze(1)) ** 2).sum(dim=1) / N).sqrt() + eps
    out = (mu, sigma, w, nu, bracket, flags)
    return out + (margin,) if with_margin else out


# ------------------------------------------------------------------------------------------------------------------------------
# the update on the kernels
# ------------------------------------------------------------------------------------------------------------------------------
class DcemUpdate(torch.autograd.Function):
    """(fX (S, B), X (S, B, n)) -> (mu, sigma (B, n), w (B, S), nu (B), bracket (B, 2), flags (B) int32): thx_dcem_update, and
    thx_dcem_update_vjp as its backward (w, nu, bracket, flags are not differentiable).  ``out``: None, or (mu, sigma) buffers to
    write into -- for callers under no_grad that recycle theirs."""

    @staticmethod
    def forward(ctx, fX, X, K, n_elite, temp, normalize, lml_eps, lml_n_iter, branch, out):
        fX, X = fX.detach().contiguous(), X.detach().contiguous()
        S, B, n = X.shape
        mu, sigma = out if out is not None else (torch.empty(B, n, dtype=X.dtype, device=X.device) for _ in range(2))
        w = torch.empty(B, S, dtype=X.dtype, device=X.device)
        nu = torch.empty(B, dtype=X.dtype, device=X.device)
        bracket = torch.empty(B, 2, dtype=X.dtype, device=X.device)
        flags = torch.empty(B, dtype=torch.int32, device=X.device)
        K.dcem_update(fX, X, n_elite, temp, normalize, lml_eps, lml_n_iter, branch, mu, sigma, w, nu, bracket, flags)
        ctx.K, ctx.args = K, (n_elite, temp, normalize)
        ctx.save_for_backward(X, fX, w, mu, sigma)
        ctx.mark_non_differentiable(w, nu, bracket, flags)
        return mu, sigma, w, nu, bracket, flags

    @staticmethod
    def backward(ctx, grad_mu, grad_sigma, *unused):
        X, fX, w, mu, sigma = ctx.saved_tensors
        grad_mu = torch.zeros_like(mu) if grad_mu is None else grad_mu.contiguous()
        grad_sigma = torch.zeros_like(sigma) if grad_sigma is None else grad_sigma.contiguous()
        grad_X, grad_fX = torch.empty_like(X), torch.empty_like(fX)
        ctx.K.dcem_update_vjp(grad_mu, grad_sigma, X, fX, w, mu, sigma, *ctx.args, grad_X, grad_fX)
        return grad_fX, grad_X, None, None, None, None, None, None, None, None


# ------------------------------------------------------------------------------------------------------------------------------
# the optimizer
# ------------------------------------------------------------------------------------------------------------------------------
class DCEM:
    """``theseus.DCEM`` on the HIP back end.  The constructor mirrors the reference's (dcem.py:38-76) and adds ``lml_branch``: the grid
    values per round of the LML search -- the reference takes 10 on the CPU and 100 on a GPU (lml.py:62-67); None means 100.
    ``lb`` / ``ub`` are stored and NOT applied, exactly as in the reference (nothing there reads them).

    Tuning hints, from the reference: with fewer iterations take more samples; more samples shrink the variance more slowly and
    make it likelier that the optimum is among the elite; more elites converge more slowly -- 5 is enough for most problems."""

    def __init__(self, objective: Objective, vectorize: bool = False, max_iterations: int = 50, n_sample: int = 100,
                 n_elite: int = 5, temp: Optional[float] = 1.0, init_sigma: Union[float, torch.Tensor] = 1.0, lb: float = None,
                 ub: float = None, lml_verbose: bool = False, lml_eps: float = 1e-3, normalize: bool = True,
                 abs_err_tolerance: float = 1e-6, rel_err_tolerance: float = 1e-4, lml_branch: Optional[int] = None, **kwargs):
        if int(n_elite) < 1:
            raise ValueError(f"DCEM: n_elite must be at least 1, got {n_elite}")
        if int(n_sample) < 1:
            raise ValueError(f"DCEM: n_sample must be at least 1, got {n_sample}")
        if n_sample > _lib.THX_DCEM_MAX_S:
            raise ValueError(f"DCEM: n_sample = {n_sample} exceeds the {_lib.THX_DCEM_MAX_S} samples thx_dcem_update keeps in LDS")
        if lml_branch is not None and int(lml_branch) < 2:
            raise ValueError(f"DCEM: lml_branch must be at least 2, got {lml_branch}")
        self.objective = objective
        for v in objective.optim_vars.values():
            if not _is_euclidean(v):
                raise UnsupportedObjective(
                    f"DCEM samples mu + sigma * eps on the variables' tensors: every optimisation variable must be Euclidean "
                    f"(Vector / Point2 / Point3); got {type(v).__name__} ({v.name}).  There is no CPU/eager fallback.")
        self.ordering = VariableOrdering(objective)
        self.packed = packed_for(objective, None, [v.name for v in self.ordering])
        if getattr(self.packed, "group", None) != "Euclidean":
            raise UnsupportedObjective(f"DCEM needs a packed state of Euclidean variables; this objective packs as "
                                       f"{type(self.packed).__name__}.")
        self.params = NonlinearOptimizerParams(abs_err_tolerance, rel_err_tolerance, max_iterations, 1.0)
        self.n_samples, self.n_elite = int(n_sample), int(n_elite)
        self.lb, self.ub = lb, ub
        self.temp, self.normalize = temp, normalize
        self.lml_eps, self.lml_verbose = lml_eps, lml_verbose
        self.lml_branch = 100 if lml_branch is None else int(lml_branch)
        self.init_sigma = init_sigma
        self._tot_dof = self.packed.n
        self.sigma: Optional[torch.Tensor] = None
        self.lml_flags: Optional[torch.Tensor] = None   # (B) int32: the THX_DCEM_FLAG_* bits of every update of the last optimize(), or-ed
        self._objective_version = objective.current_version
        self._X = self._fX = None

    set_params = NonlinearLeastSquares.set_params   # (it touches ``self.params`` alone)

    def reset_sigma(self, init_sigma: Union[float, torch.Tensor]) -> None:
        p = self.packed
        self.sigma = torch.ones(p.batch, self._tot_dof, dtype=self.objective.dtype, device=p.device) * init_sigma

    optimize = NonlinearLeastSquares.optimize   # (the version check, then ``self._optimize_impl``)

    def _optimize_impl(self, **kwargs) -> NonlinearOptimizerInfo:
        """State ownership as in NonlinearLeastSquares._optimize_impl: the loop moves the state through private buffers and re-points
        the variables at its end -- or, if anything raises, before the exception leaves."""
        packed = self.packed
        try:
            return self._optimize_loop(**kwargs)
        except BaseException:
            with torch.no_grad():
                packed.flush_variables()
            raise
        finally:
            packed._keep_graph_tensors = False

    def _check_convergence(self, err, last_err):
        """nonlinear_optimizer.py:110-119, the mean test as a device-side select"""
        conv = NonlinearLeastSquares._check_convergence(self, err, last_err)   # (the per-problem tests, on ``self.params``)
        return conv | (err.abs().mean() < self.params.abs_err_tolerance)

    def _optimize_loop(self, track_best_solution: bool = False, track_err_history: bool = False, track_state_history: bool = False,
                       verbose: bool = False, backward_mode: Union[str, BackwardMode] = BackwardMode.UNROLL,
                       end_iter_callback: Optional[Callable] = None, init_sigma=None, generator: Optional[torch.Generator] = None,
                       noise: Optional[torch.Tensor] = None, **kwargs) -> NonlinearOptimizerInfo:
        backward_mode = BackwardMode.resolve(backward_mode)
        if backward_mode not in (BackwardMode.UNROLL, BackwardMode.DLM):
            raise NotImplementedError("DCEM currently only supports 'unroll' backward mode.")
        packed, p = self.packed, self.params
        S, n, N = self.n_samples, self._tot_dof, self.n_elite
        outer_grad = torch.is_grad_enabled()
        # what is differentiated starts at the caller's own tensors (kept before the first sync re-points the variables)
        init_tensors = None
        if outer_grad:
            ts = [v.tensor for v in packed.optim_variables]
            if any(t.requires_grad for t in ts):
                init_tensors = ts
        graph = outer_grad and (init_tensors is not None or any(v.tensor.requires_grad for v in packed.tracked_list()))
        packed._keep_graph_tensors = init_tensors is not None
        with torch.no_grad():
            packed.sync(deep=True)
            packed.privatize_state()
            B, dev, dt = packed.batch, packed.device, self.objective.dtype
            if not isinstance(packed.state, torch.Tensor) or tuple(packed.state.shape) != (B, n):
                raise UnsupportedObjective(f"DCEM needs the packed state to be one (batch, dof) = {(B, n)} tensor; "
                                           f"{type(packed).__name__} keeps {getattr(packed.state, 'shape', type(packed.state))}")
            if noise is not None and (tuple(noise.shape) != (p.max_iterations, S, B, n) or noise.dtype != dt or noise.device != dev):
                raise ValueError(f"DCEM: noise must be a {(p.max_iterations, S, B, n)} tensor of {dt} on {dev} "
                                 f"(max_iterations, n_sample, batch, dof); got {tuple(noise.shape)} of {noise.dtype} on {noise.device}")
            self.reset_sigma(self.init_sigma if init_sigma is None else init_sigma)
            if tuple(self.sigma.shape) != (B, n):
                raise ValueError(f"DCEM: init_sigma must broadcast to {(B, n)}")
            tracker = _RunTracker(packed, p, dt, track_best_solution, track_err_history, track_state_history)
            info = tracker.info
            last_err = info.last_err = info.last_err.clone()
            if verbose:
                print(f"DCEM optimizer. Iteration: 0. Error: {last_err.mean().item()}")
            if self._X is None or tuple(self._X.shape) != (S, B, n) or self._X.dtype != dt or self._X.device != dev:
                self._X = torch.empty(S, B, n, dtype=dt, device=dev)
                self._fX = torch.empty(S, B, dtype=dt, device=dev)
            spare, spare_sigma = packed.alloc_state(), torch.empty_like(self.sigma)
            err_new = torch.empty(B, dtype=dt, device=dev)
            need_conv = p.abs_err_tolerance > 0 or p.rel_err_tolerance > 0
            conv = torch.zeros(B, dtype=torch.bool, device=dev)        # the previous iteration's verdict (nobody is frozen by it)
            ever_conv = torch.zeros(B, dtype=torch.bool, device=dev)   # status CONVERGED sticks (dcem.py:189-191)
            conv_iter = torch.zeros(B, dtype=torch.long, device=dev)
            flags_all = torch.zeros(B, dtype=torch.int32, device=dev)
        mu = packed.state
        if graph:
            mu = packed.state.detach()
            if init_tensors is not None:
                mu = packed.state_with_graph(init_tensors)   # same values, the caller's autograd history
        sigma = self.sigma
        hard = _is_hard(self.temp)
        update = (packed.K, N, None if hard else float(self.temp), self.normalize, self.lml_eps, LML_N_ITER, self.lml_branch)
        it = 0
        while it < p.max_iterations:
            with torch.no_grad():
                eps = noise[it] if noise is not None else torch.randn((S, B, n), generator=generator, dtype=dt, device=dev)
            if graph:
                # differentiated: the samples and their errors by the torch classes, with the graph
                X = torch.addcmul(mu.unsqueeze(0), sigma.unsqueeze(0), eps)
                fX = torch.stack([PackedState.error_metric(packed, state=X[s]) for s in range(S)], dim=0)
                mu, sigma, _, _, _, flags = DcemUpdate.apply(fX, X, *update, None)
                packed.swap_state(mu)
            else:
                with torch.no_grad():
                    X, fX = self._X, self._fX
                    torch.addcmul(mu.unsqueeze(0), sigma.unsqueeze(0), eps, out=X)
                    for s in range(S):
                        packed.error_metric(state=X[s], out=fX[s])
                    mu, sigma, _, _, _, flags = DcemUpdate.apply(fX, X, *update, (spare, spare_sigma))
                    spare, spare_sigma = packed.swap_state(mu), self.sigma
            self.sigma = sigma
            with torch.no_grad():
                flags_all |= flags
                err = packed.error_metric(state=mu.detach(), out=err_new)
                # _update_info (nonlinear_optimizer.py:184-213), then the convergence test of dcem.py:188-195
                conv_iter += 1 - conv.long()
                tracker.record(it, mu.detach(), err)
                if verbose:
                    print(f"Nonlinear optimizer. Iteration: {it + 1}. Error: {err.mean().item()} ")
                it += 1
                info.iters_done = it
                if need_conv:
                    conv = self._check_convergence(err, last_err)
                    ever_conv |= conv
                    # the reference's host decision of every iteration; with both tolerances 0 nothing can converge and the loop
                    # never reads the device
                    if bool(conv.all()):
                        break   # (info.last_err stays the previous iteration's, as there)
                last_err = err.clone()
                info.last_err = last_err
                if end_iter_callback is not None:
                    packed.flush_variables()   # (the variables view the new mean: the reference hands the callback that dict)
                    end_iter_callback(self, info, {v.name: v.tensor for v in packed.optim_variables}, it - 1)
        with torch.no_grad():
            if graph:
                packed.swap_state(mu, repoint=True)   # the variables view the graph-carrying result
            packed.flush_variables()
            self.lml_flags = flags_all
            if self.lml_verbose and bool(flags_all.ne(0).any()):
                print("LML Warning: Did not converge, or an example has all positive iterates.")
            return tracker.finish(ever_conv, conv_iter)
