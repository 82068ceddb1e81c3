"""TheseusLayer mirror (theseus/theseus_layer.py:29-174): forward = Objective.update + optimize."""
from typing import Any, Dict, Optional, Tuple, Union

import torch

from .dcem import DCEM
from .nonlinear import NonlinearLeastSquares, NonlinearOptimizerInfo


class TheseusLayer(torch.nn.Module):
    def __init__(self, optimizer: Union[NonlinearLeastSquares, DCEM], vectorize: bool = True, **kwargs):
        super().__init__()
        self.objective = optimizer.objective
        self.optimizer = optimizer
        self._objectives_version = optimizer.objective.current_version

    def forward(self, input_tensors: Optional[Dict[str, torch.Tensor]] = None,
                optimizer_kwargs: Optional[Dict[str, Any]] = None) -> Tuple[Dict[str, torch.Tensor], NonlinearOptimizerInfo]:
        if self._objectives_version != self.objective.current_version:
            raise RuntimeError("The objective was modified after the layer's construction, which is "
                               "currently not supported.")
        optimizer_kwargs = optimizer_kwargs or {}
        self.objective.update(input_tensors)                      # theseus_layer.py:164-174
        info = self.optimizer.optimize(**optimizer_kwargs)
        vars_ = {name: var.tensor for name, var in self.objective.optim_vars.items()}
        return vars_, info

    @torch.no_grad()
    def compute_samples(self, linear_solver=None, n_samples: int = 10, temperature: float = 1.0, *,
                        noise: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None,
                        return_dict: bool = False):
        """theseus_layer.py:99-135 (the sampling step of LEO): ``n_samples`` draws of the optimisation variables from
        N(x*, (AtA / temperature)^-1), each the current variables retracted by one of ``linear_solver.sample_deltas(...)`` -- on
        the factor the solve leaves, without the reference's dense second factorisation.  The variables are not modified.
        ``return_dict=False``: the reference's (B, n_vars, n_samples) tensor, possible when every optimisation variable's tensor
        is as wide as its dof (Vector / Point2 / Point3); ``return_dict=True``: {name: (B, n_samples, *var.tensor.shape[1:])},
        for every objective HipCholeskySolver accepts.  ``noise`` / ``generator``: see ``sample_deltas``."""
        # When samples are not available, return None: the outer loop falls back to a perceptron loss (theseus_layer.py:105-108)
        if linear_solver is None:
            return None
        if not temperature > 0:
            raise ValueError(f"compute_samples: temperature must be positive, got {temperature}")
        if int(n_samples) < 1:
            raise ValueError(f"compute_samples: n_samples must be at least 1, got {n_samples}")
        packed = linear_solver.linearization.packed
        euclidean = getattr(packed, "group", None) == "Euclidean"
        if not euclidean and not return_dict:
            raise ValueError("compute_samples: the (B, n_vars, n_samples) tensor exists only when every optimisation variable's "
                             f"tensor is as wide as its dof; this objective optimises {packed.group} variables -- pass "
                             "return_dict=True.")
        samples = linear_solver.sample_deltas(n_samples, temperature, noise=noise, generator=generator)   # (B, n, k) view
        deltas = samples.transpose(1, 2)                                                                  # (B, k, n) contiguous
        B, k, n = deltas.shape
        packed.sync()
        K = packed.K
        # one retraction launch on B * k records: record (b, s) = the variables of problem b, retracted by sample s
        if euclidean:
            x = packed.state.unsqueeze(1).expand(B, k, n).reshape(1, B * k, n)
            out = torch.empty_like(x)
            K.vec_retract(x, deltas.view(B * k, n), 0, 1.0, None, out)
            out = out.view(B, k, n)
            if not return_dict:
                return out.transpose(1, 2)
            return {v.name: out[:, :, c0:c0 + d] for v, (c0, d) in zip(packed.vars, packed.cols)}
        poses = packed.tensors.poses                                                                      # (P, B, *record)
        P, rec = poses.shape[0], tuple(poses.shape[2:])
        x = poses.unsqueeze(2).expand(P, B, k, *rec).reshape(P, B * k, *rec)
        out = torch.empty_like(x)
        K.retract(x, deltas.view(B * k, n), 1.0, None, out)
        return dict(zip(packed.order, out.view(P, B, k, *rec).unbind(0)))

    def to(self, *args, **kwargs):
        super().to(*args, **kwargs)
        self.objective.to(*args, **kwargs)
        return self

    @property
    def device(self):
        return self.objective.device

    @property
    def dtype(self):
        return self.objective.dtype
