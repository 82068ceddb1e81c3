"""Generic objectives on theseus_amd's own API (BASELINE.json configs[0]: examples/simple_example.py -- an
``AutoDiffCostFunction`` on a ``Vector``): any cost function that can hand over its weighted Jacobian blocks and error
(``CostFunction.weighted_jacobians_error``, theseus/core/cost_function.py:107-122), optimisation variables Euclidean
(``Vector`` / ``Point2`` / ``Point3``: retraction = addition, theseus/geometry/vector.py:177-178).

What runs where: the cost functions are evaluated by torch (they are user code -- the reference does the same,
core/cost_function.py:203-393); ``H = A^T A`` and ``g = A^T b`` are formed from the blocks by ``thx_block_assemble`` without the
dense ``A`` of DenseLinearization (dense_linearization.py:29-62), the damped system is factorised / solved by the tiled
Cholesky, LM's accept test and the masked retraction are the same kernels the pose-graph path uses.  The state the LM loop
moves around is ONE (B, n) tensor; the variables' tensors are column views of it.

Implicit backward (nonlinear_least_squares.py:121-135,265-292): the grad-enabled last Gauss-Newton step keeps H outside
autograd; ``g`` is formed by torch from the differentiable blocks, the solve's backward is one solve with the cached factor.
``backward_mode="unroll"`` / ``"truncated"`` (:222-282): the differentiated iterations keep H IN the graph -- torch forms the
(small) normal equations from the blocks, the damped solve runs on the kernels as in every other iteration and is one autograd
node whose backward is a solve with a copy of that iteration's factor (``_UnrolledSolve``).
"""
from typing import Optional

import torch

from .generic import PackedState, _names


def _is_euclidean(v) -> bool:
    return "Vector" in _names(v)


class PackedEuclidean(PackedState):
    """The packed state of Euclidean variables: one (B, n) tensor, the variables' tensors are column views of it."""

    group = "Euclidean"

    def _check(self):
        from .packed import UnsupportedObjective
        for v in self.vars:
            if not _is_euclidean(v):
                raise UnsupportedObjective(
                    f"HIP backend, generic path: optimisation variables must be Euclidean (Vector / Point2 / Point3); got "
                    f"{type(v).__name__} ({v.name}).  There is no CPU/eager fallback.")
        for c in self.costs:
            if not hasattr(c, "jacobians"):
                raise UnsupportedObjective(f"HIP backend, generic path: {type(c).__name__} ({c.name}) does not implement "
                                           "jacobians().")

    def _pack(self):
        obj = self.objective
        obj._resolve_batch_size()
        B = obj.batch_size
        parts = [v.tensor if v.tensor.shape[0] == B else v.tensor.expand(B, -1) for v in self.vars]
        with torch.no_grad():
            self._state = torch.cat(parts, dim=1).contiguous()
        self._repoint_variables()

    def _var_view(self, state, k):
        c0, d = self.cols[k]
        return state[:, c0:c0 + d]

    @property
    def batch(self):
        return self._state.shape[0]

    @staticmethod
    def _rec(t):   # (B, n) -> the (N = 1, B, record) layout of thx_copy_where / thx_vec_retract
        return t.view(1, *t.shape)

    def keep_where(self, mask, out):
        self.K.copy_where(mask, self._rec(self._state), self._rec(out))

    def copy_where(self, mask, src, dst):
        self.K.copy_where(mask, self._rec(src), self._rec(dst))

    def solution_dict(self, state):
        return {v.name: state[:, c0:c0 + d].cpu() for v, (c0, d) in zip(self.vars, self.cols)}

    def history_dict(self, hist, dtype):
        """(K + 1, B, n) states -> name -> (B, dof, K + 1) on the host (nonlinear_optimizer.py:150-163)."""
        h = hist.to(dtype).cpu()
        return {v.name: h[:, :, c0:c0 + d].permute(1, 2, 0).contiguous() for v, (c0, d) in zip(self.vars, self.cols)}

    def retract(self, delta: torch.Tensor, step: float, ignore_mask: Optional[torch.Tensor], out: torch.Tensor):
        """out = state + step * delta (rows of ``ignore_mask`` keep the state): thx_vec_retract on the one (B, n) record."""
        self.sync()
        self.K.vec_retract(self._rec(self._state), delta, 0, step, self._mask_u8(ignore_mask), self._rec(out))
        return out

    # ---- BackwardMode.UNROLL / TRUNCATED: one iteration as a differentiable function of the state and of whatever the cost
    #      functions depend on (nonlinear_least_squares.py:100-215 with the Hessian IN the graph) -------------------------------
    def normal_equations(self, Js, es):
        """(H (B, n, n) symmetric, g (B, n)) from the weighted blocks, by torch: the differentiable twin of ``assemble``."""
        B = self.batch
        ref = es[0]
        H = torch.zeros(B, self.n, self.n, dtype=ref.dtype, device=ref.device)
        g = torch.zeros(B, self.n, dtype=ref.dtype, device=ref.device)
        for c, (J, e) in enumerate(zip(Js, es)):
            for sa, ka in enumerate(self.cost_vars[c]):
                ca, da = self.cols[ka]
                g[:, ca:ca + da] = g[:, ca:ca + da] - (J[sa].transpose(1, 2) @ e.unsqueeze(2)).squeeze(2)
                for sb, kb in enumerate(self.cost_vars[c]):
                    cb, db = self.cols[kb]
                    H[:, ca:ca + da, cb:cb + db] = H[:, ca:ca + da, cb:cb + db] + J[sa].transpose(1, 2) @ J[sb]
        return H, g

    def prepare_unroll(self):
        pass   # (the blocks are evaluated by torch at every differentiated iteration: nothing to re-pack)

    def where_state(self, mask: torch.Tensor, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        return torch.where(mask.view(-1, 1), a, b)

    def state_with_graph(self, tensors):
        """The state assembled from the optimisation variables' OWN tensors (in ``optim_variables`` order), autograd history kept:
        where BackwardMode.UNROLL starts, so that gradients reach the values the caller passed in."""
        B = self._state.shape[0]
        return torch.cat([t if t.shape[0] == B else t.expand(B, -1) for t in tensors], dim=1)

    def unrolled_step(self, opt, X: torch.Tensor, frozen: Optional[torch.Tensor], kwargs):
        """X -> (X + step * delta where not ``frozen``, delta): the blocks are evaluated at X with the graph, the kernels get
        their detached values (what ``compute_delta`` factorises and LM's accept test reads), the solve is the autograd node."""
        solver = opt.linear_solver
        lin = solver.linearization
        lin._ensure_buffers()
        Js, es = [], []
        with self._at(self, X):
            for c in self.costs:
                jac, err = c.weighted_jacobians_error()
                Js.append([j.contiguous() for j in jac])
                es.append(err.contiguous())
        Jd, ed = [[j.detach() for j in J] for J in Js], [e.detach() for e in es]
        self.asm.assemble(self.K, Jd, ed, lin._H, lin.g)
        self._blocks = (Jd, ed)
        lin._after_assemble()
        H, g = self.normal_equations(Js, es)
        delta = _UnrolledSolve.apply(opt, kwargs, H, g)
        X_new = X + float(opt.params.step_size) * delta
        if frozen is not None:
            X_new = torch.where(frozen.view(-1, 1), X, X_new)
        return X_new, delta

    def _implicit_retract(self, X, delta):
        return X + delta


class _UnrolledSolve(torch.autograd.Function):
    """delta = (H + D)^-1 g as a differentiable function of H and g (D: the optimizer's damping of this iteration, a function of
    diag(H) when ellipsoidal -- dense_solver.py:38-64).  Forward: the optimizer's own ``compute_delta`` on the kernels (the
    buffers hold the detached H, g).  Backward, with w = (H + D)^-1 grad_delta from a COPY of this iteration's factor (later
    iterations overwrite the solver's):  grad_g = w,  grad_H = -w delta^T - diag(lambda w * delta) [ellipsoidal]."""

    @staticmethod
    def forward(ctx, opt, kwargs, H, g):
        solver = opt.linear_solver
        delta = opt.compute_delta(**kwargs)
        if bool(solver.info.ne(0).any()):
            try:
                solver.check_info()
            except RuntimeError as run_err:
                raise RuntimeError(f"There was an error while running the linear optimizer. Original error message: {run_err}. "
                                   "Backward pass will not work. To obtain the best solution seen before the error, run with "
                                   "torch.no_grad()") from None
        damped, ellipsoidal, _ = solver._factored_with
        ctx.solver, ctx.n = solver, solver.linearization.n
        ctx.factor = solver.factor_snapshot()
        ctx.dropped = solver.dropped_mask() if hasattr(solver, "dropped_mask") else None   # check_singular: zero step, zero gradient
        ctx.lam = solver._lam.clone() if (damped and ellipsoidal) else None
        ctx.save_for_backward(delta)
        return delta

    @staticmethod
    def backward(ctx, grad_delta):
        (delta,) = ctx.saved_tensors
        if ctx.dropped is not None:
            grad_delta = grad_delta.masked_fill(ctx.dropped.unsqueeze(1), 0.0)
        w = ctx.solver.solve_with_snapshot(ctx.factor, grad_delta)
        if ctx.dropped is not None:
            w = w.masked_fill(ctx.dropped.unsqueeze(1), 0.0)
        grad_H = -(w.unsqueeze(2) * delta.unsqueeze(1))
        if ctx.lam is not None:
            grad_H = grad_H - torch.diag_embed(ctx.lam.view(-1, 1) * w * delta)
        return None, None, grad_H, w
