"""The objective of the DCEM fixtures (tests/golden/dcem_f64_soft.npz, dcem_f64_modes.npz, written by tools/gen_dcem_golden.py from
the REAL reference), built on either API: ``th`` is ``theseus_amd`` in the tests and ``theseus`` in the generator.

One ``Vector(4)`` x, one ``AutoDiffCostFunction`` of dim 5 with error  A (x - t) + 0.1 * sum(sin x)  for per-problem A (B, 5, 4) and
t (B, 4).  B = 3, start at zero, 40 samples, 5 elites, 6 iterations, both tolerances 0.

Also here: the one-line sampling step both sides share, and the modes of dcem_f64_modes.npz."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B, N_DOF, DIM = 3, 4, 5
N_SAMPLE, N_ELITE, N_ITER, BRANCH = 40, 5, 6, 10
DCEM_KW = dict(max_iterations=N_ITER, n_sample=N_SAMPLE, n_elite=N_ELITE, abs_err_tolerance=0.0, rel_err_tolerance=0.0)
# name -> (constructor keywords that differ from DCEM_KW, samples of the one recorded iteration)
MODES = {"hard": (dict(temp=None), N_SAMPLE), "softmax": (dict(n_elite=1), N_SAMPLE),
         "raw": (dict(normalize=False, temp=0.3), N_SAMPLE), "all_elite": (dict(n_sample=N_ELITE), N_ELITE)}


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def problem():
    rng = np.random.default_rng(21)
    return dict(A=rng.normal(0, 1, (B, DIM, N_DOF)), t=rng.uniform(-1.5, 1.5, (B, N_DOF)), x0=np.zeros((B, N_DOF)))


def err_fn(optim_vars, aux_vars):
    x, (A, t) = optim_vars[0].tensor, (v.tensor for v in aux_vars)
    return (A @ (x - t).unsqueeze(2)).squeeze(2) + 0.1 * torch.sin(x).sum(dim=1, keepdim=True)


def build(th, f, device="cpu", dtype=torch.float64, grad=False):
    """-> (objective, {"t": leaf, "x0": leaf}); ``grad``: the leaves require grad (x0 is what a caller passes for "x")."""
    def ten(key):
        return torch.from_numpy(np.asarray(f[key])).to(dtype).to(device)
    leaves = {"t": ten("t").clone().requires_grad_(grad), "x0": ten("x0").clone().requires_grad_(grad)}
    x = th.Vector(tensor=ten("x0").clone(), name="x")
    A = th.Variable(ten("A"), name="A")
    t = th.Variable(leaves["t"], name="t")
    obj = th.Objective(dtype=dtype)
    weight = th.ScaleCostWeight(th.Variable(torch.ones(1, 1, dtype=dtype, device=device), name="w_fit"))
    obj.add(th.AutoDiffCostFunction([x], err_fn, DIM, cost_weight=weight, aux_vars=[A, t], name="fit"))
    return obj, leaves


def samples(mu, sigma, eps):
    """X (S, B, n) of one iteration: Normal(mu, sigma).rsample((S,)) with the draw ``eps`` (dcem.py:104)"""
    return mu + eps * sigma
