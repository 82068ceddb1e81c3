"""Generic block assembly for objectives the fused pose-graph kernels do not cover.

``BlockAssembler`` turns "a list of cost functions, each with its (weighted) Jacobian blocks and error" -- what
``CostFunction.weighted_jacobians_error`` returns in the reference (theseus/core/cost_function.py:107-122) -- into the
lower triangle of H = A^T A and g = A^T b through ``thx_block_assemble`` (csrc/block_kernels.hip), never forming the
dense A of ``DenseLinearization`` (theseus/optimizer/dense_linearization.py:29-62).  The block structure (which
variable pairs meet in a cost) is compiled once; only the pointer tables are refreshed per call.

``PackedState`` is the packed-state plumbing every class built on it shares (theseus_amd/euclidean.py: PackedEuclidean,
theseus_amd/pushing.py: PackedPlanarPushing); a fused evaluation is added by theseus_amd/term_table.py: TermTable.
"""
import warnings
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .kernels import round_up
from .packer_base import StateOwner

H_TARGET = np.dtype([("row0", "<i4"), ("col0", "<i4"), ("dof_a", "<i4"), ("dof_b", "<i4"), ("term_begin", "<i4"),
                     ("term_end", "<i4"), ("elem_begin", "<i4"), ("pad", "<i4")])
H_TERM = np.dtype([("Ja", "<u8"), ("Jb", "<u8"), ("bstride_a", "<i8"), ("bstride_b", "<i8"), ("dim", "<i4"),
                   ("dof_a", "<i4"), ("dof_b", "<i4"), ("pad", "<i4")])
G_TARGET = np.dtype([("col0", "<i4"), ("dof", "<i4"), ("term_begin", "<i4"), ("term_end", "<i4"), ("elem_begin", "<i4"),
                     ("pad", "<i4")])
G_TERM = np.dtype([("J", "<u8"), ("e", "<u8"), ("bstride_j", "<i8"), ("bstride_e", "<i8"), ("dim", "<i4"), ("dof", "<i4")])
assert (H_TARGET.itemsize, H_TERM.itemsize, G_TARGET.itemsize, G_TERM.itemsize) == (32, 48, 24, 40)


def _names(obj):
    return {c.__name__ for c in type(obj).__mro__}


class BlockAssembler:
    def __init__(self, var_cols: Sequence[Tuple[int, int]], cost_vars: Sequence[Sequence[int]], cost_dims: Sequence[int]):
        """var_cols[v] = (first column, dof) of variable v in the linearization's ordering; cost_vars[c] = indices of
        the optimisation variables of cost c (Jacobian list order); cost_dims[c] = rows of cost c."""
        self.var_cols = [tuple(map(int, vc)) for vc in var_cols]
        self.cost_vars = [list(map(int, cv)) for cv in cost_vars]
        self.cost_dims = [int(d) for d in cost_dims]
        self.n = sum(d for _, d in self.var_cols)
        pairs = {}   # (va, vb) with col(va) >= col(vb)  ->  [(cost, slot_a, slot_b)]
        grads = {}   # v -> [(cost, slot)]
        for c, vs in enumerate(self.cost_vars):
            for sa, va in enumerate(vs):
                grads.setdefault(va, []).append((c, sa))
                for sb, vb in enumerate(vs):
                    ca, cb = self.var_cols[va][0], self.var_cols[vb][0]
                    if ca > cb or (ca == cb and sa == sb):
                        pairs.setdefault((va, vb), []).append((c, sa, sb))
                    elif ca == cb and sa != sb:
                        raise ValueError("a cost function lists the same optimisation variable twice")
        self.h_keys = sorted(pairs, key=lambda k: (self.var_cols[k[0]][0], self.var_cols[k[1]][0]))
        self.h_terms_of = [pairs[k] for k in self.h_keys]
        self.g_keys = sorted(grads, key=lambda v: self.var_cols[v][0])
        self.g_terms_of = [grads[v] for v in self.g_keys]
        ht = np.zeros(len(self.h_keys), H_TARGET)
        elems, e2t, tb = 0, [], 0
        for t, (va, vb) in enumerate(self.h_keys):
            (ra, da), (cb_, db) = self.var_cols[va], self.var_cols[vb]
            nt = len(self.h_terms_of[t])
            ht[t] = (ra, cb_, da, db, tb, tb + nt, elems, 0)
            e2t += [t] * (da * db)
            elems += da * db
            tb += nt
        self.h_targets, self.h_e2t, self.n_h_elems, self.n_h_terms = ht, np.asarray(e2t, np.int32), elems, tb
        gt = np.zeros(len(self.g_keys), G_TARGET)
        elems, e2t, tb = 0, [], 0
        for t, v in enumerate(self.g_keys):
            c0, d = self.var_cols[v]
            nt = len(self.g_terms_of[t])
            gt[t] = (c0, d, tb, tb + nt, elems, 0)
            e2t += [t] * d
            elems += d
            tb += nt
        self.g_targets, self.g_e2t, self.n_g_elems, self.n_g_terms = gt, np.asarray(e2t, np.int32), elems, tb
        self._dev = {}

    def lower_block_pattern(self):
        """[(row0, col0, dof_a, dof_b)] of the non-zero blocks of tril(H)."""
        return [(int(t["row0"]), int(t["col0"]), int(t["dof_a"]), int(t["dof_b"])) for t in self.h_targets]

    def _static(self, device):
        key = str(device)
        if key not in self._dev:
            up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(device)  # noqa: E731
            self._dev[key] = (up(self.h_targets), up(self.h_e2t), up(self.g_targets), up(self.g_e2t))
        return self._dev[key]

    def term_tables(self, jacobians: List[List[torch.Tensor]], errors: List[torch.Tensor]):
        """Pointer tables for the current Jacobian / error tensors (contiguous (B|1, dim, dof) and (B|1, dim))."""
        ht = np.zeros(self.n_h_terms, H_TERM)
        k = 0
        for terms in self.h_terms_of:
            for (c, sa, sb) in terms:
                Ja, Jb = jacobians[c][sa], jacobians[c][sb]
                ht[k] = (Ja.data_ptr(), Jb.data_ptr(), Ja.stride(0) if Ja.shape[0] > 1 else 0,
                         Jb.stride(0) if Jb.shape[0] > 1 else 0, Ja.shape[1], Ja.shape[2], Jb.shape[2], 0)
                k += 1
        gt = np.zeros(self.n_g_terms, G_TERM)
        k = 0
        for terms in self.g_terms_of:
            for (c, sa) in terms:
                J, e = jacobians[c][sa], errors[c]
                gt[k] = (J.data_ptr(), e.data_ptr(), J.stride(0) if J.shape[0] > 1 else 0,
                         e.stride(0) if e.shape[0] > 1 else 0, J.shape[1], J.shape[2])
                k += 1
        return ht, gt

    def check(self, jacobians, errors):
        for c, (Js, e) in enumerate(zip(jacobians, errors)):
            if len(Js) != len(self.cost_vars[c]):
                raise ValueError(f"cost {c}: expected {len(self.cost_vars[c])} Jacobian blocks, got {len(Js)}")
            for s, J in enumerate(Js):
                dof = self.var_cols[self.cost_vars[c][s]][1]
                if J.ndim != 3 or J.shape[1] != self.cost_dims[c] or J.shape[2] != dof or not J.is_contiguous():
                    raise ValueError(f"cost {c} slot {s}: Jacobian must be contiguous (B, {self.cost_dims[c]}, {dof}), "
                                     f"got {tuple(J.shape)}")
            if e.ndim != 2 or e.shape[1] != self.cost_dims[c] or not e.is_contiguous():
                raise ValueError(f"cost {c}: error must be contiguous (B, {self.cost_dims[c]})")

    def assemble(self, K, jacobians, errors, H: torch.Tensor, g: torch.Tensor, hessian: bool = True, gradient: bool = True):
        """H[:, lower blocks] = sum J_a^T J_b ; g = -sum J^T e.  The tensors in ``jacobians`` / ``errors`` must stay
        alive until the launch has run (the caller's stream order guarantees that for ordinary use)."""
        self.check(jacobians, errors)
        K.block_assemble(self, jacobians, errors, H if hessian else None, g if gradient else None)


class PackedState(StateOwner):
    """The packed-state interface of the optimiser loop (theseus_amd/packed.py: PackedPoseGraph) for objectives whose cost functions
    hand over their weighted Jacobian blocks: the state the loop moves around is ONE tensor, the variables' tensors are views of it,
    the cost functions are evaluated by torch at such views and H, g come from the blocks through ``BlockAssembler``.  A subclass
    fixes the layout: ``_check`` (what it accepts), ``_pack``, ``_var_view``, ``batch``, ``retract``, ``keep_where`` / ``copy_where``,
    ``solution_dict`` / ``history_dict`` and ``_implicit_retract`` (theseus_amd/euclidean.py: (B, n); theseus_amd/pushing.py: (V, B, 4))."""

    def __init__(self, objective, kernels=None, order=None):
        super().__init__(objective, kernels)
        self.order = tuple(order) if order is not None else tuple(objective.optim_vars.keys())
        if sorted(self.order) != sorted(objective.optim_vars.keys()):
            raise ValueError("the variable ordering must hold every optimisation variable of the objective exactly once")
        self.vars = [objective.optim_vars[name] for name in self.order]
        self.costs = list(objective.cost_functions.values())
        self._check()
        self.cols, col = [], 0
        for v in self.vars:
            self.cols.append((col, v.dof()))
            col += v.dof()
        self.n, self.m = col, objective.dim()
        self.ld = round_up(self.n, 32)
        index = {v.name: k for k, v in enumerate(self.vars)}
        self.cost_vars = [[index[v.name] for v in c.optim_vars()] for c in self.costs]
        self.asm = BlockAssembler(self.cols, self.cost_vars, [c.dim() for c in self.costs])
        self.version = objective.current_version
        self._state: Optional[torch.Tensor] = None
        self._views = None          # what the variables' tensors are when they view the state
        self._blocks = None         # weighted blocks of the last assemble(): the launch reads these tensors

    # ---- state <-> variables -----------------------------------------------------------------------------------------
    def _tracked(self):
        yield from self.vars
        seen = set()
        for c in self.costs:
            aux = c.aux_vars() + c.weight.aux_vars()
            for a in aux:
                if id(a) not in seen:
                    seen.add(id(a))
                    yield a

    def tracked_list(self):
        return list(self._tracked())

    def _get_state(self):
        return self._state

    def _set_state(self, new):
        self._state = new

    def _repoint_variables(self):
        with torch.set_grad_enabled(self._state.requires_grad):
            self._views = [self._var_view(self._state, k) for k in range(len(self.vars))]
        for v, t in zip(self.vars, self._views):
            v._tensor = t
        self._vars_stale = False
        self._state_exposed = True

    def sync(self, force: bool = False, deep: bool = False):
        """Re-pack when somebody replaced a variable's tensor (``Objective.update``, ``Variable.update``) -- an identity test
        per variable: these objectives have a handful of variables."""
        if self._state is None or force:
            self._pack()
            return
        if self._vars_stale:
            return   # the loop owns the state; the variables are re-pointed at its end
        if any(v.tensor is not t for v, t in zip(self.vars, self._views)) or self.batch != self._batch_of_vars():
            self._pack()

    def _batch_of_vars(self):
        self.objective._resolve_batch_size()
        return self.objective.batch_size

    @property
    def optim_variables(self):
        return self.vars

    # ---- evaluation (torch: the cost functions are user code) ----------------------------------------------------------
    class _at:
        """Context: the variables' tensors view ``state`` while the cost functions are evaluated."""

        def __init__(self, packed, state):
            self.p, self.state = packed, state

        def __enter__(self):
            self.saved = [v.tensor for v in self.p.vars]
            for k, v in enumerate(self.p.vars):
                v._tensor = self.p._var_view(self.state, k)

        def __exit__(self, *a):
            for v, t in zip(self.p.vars, self.saved):
                v._tensor = t

    def _cost_error(self, c):
        return c.weighted_error()

    def error_vector(self, state=None):
        self.sync()
        with self._at(self, self._state if state is None else state):
            B = self.batch
            return torch.cat([self._cost_error(c).expand(B, -1) for c in self.costs], dim=1)

    def error_metric(self, state=None, out: Optional[torch.Tensor] = None, poses=None):
        err = (self.error_vector(state if state is not None else poses) ** 2).sum(dim=1) / 2
        if out is not None:
            out.copy_(err)
            return out
        return err

    def weighted_blocks(self):
        """[(Jacobian blocks (B|1, dim, dof) per optimisation variable of the cost), ...], [weighted error (B|1, dim), ...]"""
        self.sync()
        Js, es = [], []
        with self._at(self, self._state):
            for c in self.costs:
                jac, err = c.weighted_jacobians_error()
                Js.append([j.contiguous() for j in jac])
                es.append(err.contiguous())
        return Js, es

    def assemble(self, H: torch.Tensor, g: torch.Tensor, graph: bool = False):
        """H (lower blocks) and g from the weighted blocks; ``graph``: also return g as a differentiable function of whatever the
        blocks depend on (the implicit step), H stays outside autograd."""
        Js, es = PackedState.weighted_blocks(self)   # (the torch classes, also where a subclass has a fused evaluation)
        Jd = [[j.detach() for j in J] for J in Js]
        ed = [e.detach() for e in es]
        self.asm.assemble(self.K, Jd, ed, H, g)
        self._blocks = (Jd, ed)
        if not graph:
            return None
        B = self.batch
        parts = [None] * len(self.vars)
        for c, (J, e) in enumerate(zip(Js, es)):
            for s, k in enumerate(self.cost_vars[c]):
                term = -(J[s].transpose(1, 2) @ e.unsqueeze(2)).squeeze(2)
                parts[k] = term if parts[k] is None else parts[k] + term
        return torch.cat([(p.expand(B, -1) if p is not None else torch.zeros(B, d, dtype=H.dtype, device=H.device))
                          for p, (_, d) in zip(parts, self.cols)], dim=1)

    def supports_block_hessian(self) -> bool:
        return False

    def jacobian_blocks(self):
        return self._blocks[0] if self._blocks is not None else self.weighted_blocks()[0]

    def jacobian_times(self, blocks, v: torch.Tensor) -> torch.Tensor:
        """A v (B, m) from the per-cost blocks (Dogleg / trust-region ratio: dense_linearization.py:73-74)."""
        out = torch.zeros(v.shape[0], self.m, dtype=v.dtype, device=v.device)
        r = 0
        for c, J in enumerate(blocks):
            d = self.costs[c].dim()
            for s, k in enumerate(self.cost_vars[c]):
                c0, dof = self.cols[k]
                out[:, r:r + d] += (J[s] @ v[:, c0:c0 + dof].unsqueeze(2)).squeeze(2)
            r += d
        return out

    def dense_A_b(self):
        """Dense A (B, m, n), b (B, m) -- tests / foreign consumers only."""
        Js, es = self.weighted_blocks()
        B = self.batch
        A = torch.zeros(B, self.m, self.n, dtype=self._state.dtype, device=self._state.device)
        b = torch.zeros(B, self.m, dtype=self._state.dtype, device=self._state.device)
        r = 0
        for c, (J, e) in enumerate(zip(Js, es)):
            d = self.costs[c].dim()
            for s, k in enumerate(self.cost_vars[c]):
                c0, dof = self.cols[k]
                A[:, r:r + d, c0:c0 + dof] = J[s]
            b[:, r:r + d] = -e
            r += d
        return A, b

    # ---- BackwardMode.IMPLICIT ----------------------------------------------------------------------------------------------
    def implicit_step(self, opt, step: float, kwargs):
        lin = opt.linear_solver.linearization
        self.flush_variables()
        lin._ensure_buffers()
        g_graph = self.assemble(lin._H, lin.g, graph=True)
        lin._after_assemble()
        delta = _CachedFactorSolve.apply(opt, kwargs, g_graph)
        return self._implicit_retract(self._state.detach(), float(step) * delta), delta


class _CachedFactorSolve(torch.autograd.Function):
    """delta = H^-1 g with H outside autograd: forward = undamped factorisation (the reference falls back to the optimizer's
    damped step when it fails, nonlinear_least_squares.py:130-135) + the two substitutions; backward = one solve with the
    cached factor (the "backward linear solve" of the implicit mode)."""

    @staticmethod
    def forward(ctx, opt, kwargs, g):
        solver = opt.linear_solver
        lin = solver.linearization
        lin.g.copy_(g.detach())
        y = solver.factorize(None, rhs=lin.g)
        if bool(solver.info.ne(0).any()):
            if kwargs.get("__strict_implicit_final_gn__", False):
                solver.check_info()
            warnings.warn("implicit backward: the undamped Gauss-Newton system is not positive definite, "
                          "falling back to the optimizer's damped step", RuntimeWarning)
            delta = opt.compute_delta(**kwargs)
            solver.check_info()
        else:
            delta = torch.empty_like(lin.g)   # (NOT like y: the level schedule's y is its padded vector)
            solver._substitute(y, delta, backward_only=True)
        ctx.solver, ctx.factor_version = solver, solver.factor_version
        return delta

    @staticmethod
    def backward(ctx, grad_delta):
        solver = ctx.solver
        if solver.factor_version != ctx.factor_version:
            raise RuntimeError("implicit backward: the cached Cholesky factor of this forward pass was overwritten by "
                               "a later factorisation on the same optimizer; call backward() before the next forward().")
        return None, None, solver.solve_with_factor(grad_delta.contiguous())
