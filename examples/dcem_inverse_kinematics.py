"""Batched inverse kinematics on the Panda from RANDOM starts: DCEM as the global stage, Levenberg-Marquardt as the local one.

    python examples/dcem_inverse_kinematics.py --batch 64 [--dtype f64] [--samples 100] [--dcem-iters 30]

The objective is the one of examples/inverse_kinematics.py (LinkPoseCost on the end effector, targets fk(rand)), but every problem
starts at joint angles drawn uniformly from [-2, 2] rad.  Three runs on the same starts and targets are printed next to each other:
LM alone, DCEM alone, and LM started at DCEM's best solution.  DCEM evaluates its samples
with the family's fused error kernel (thx_kin_error, one launch per sample) and updates with thx_dcem_update
(theseus_amd/dcem.py); no Jacobian is formed until LM takes over."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.inverse_kinematics import make_objective  # noqa: E402

SOLVED = 1e-6   # objective below which a problem counts as solved (a pose error of about a millimetre / milliradian)


def summary(name, err):
    print(f"{name:>12}: objective mean {float(err.mean()):.3e}, median {float(err.median()):.3e}, worst {float(err.max()):.3e}, "
          f"solved (< {SOLVED:.0e}) {int((err < SOLVED).sum())} of {err.numel()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--elite", type=int, default=5)
    ap.add_argument("--dcem-iters", type=int, default=30)
    ap.add_argument("--lm-iters", type=int, default=30)
    ap.add_argument("--sigma", type=float, default=1.0, help="DCEM's initial standard deviation (rad)")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import theseus_amd as th
    dtype = torch.float32 if a.dtype == "f32" else torch.float64
    obj, model, _ = make_objective(th, a.batch, dtype, "cuda", seed=a.seed)
    gen = torch.Generator().manual_seed(a.seed + 1)
    start = ((torch.rand(a.batch, model.robot.dof, generator=gen, dtype=torch.float64) * 4 - 2).to(dtype).to("cuda"))
    lm = th.LevenbergMarquardt(obj, max_iterations=a.lm_iters, step_size=0.5)
    dcem = th.DCEM(obj, max_iterations=a.dcem_iters, n_sample=a.samples, n_elite=a.elite, init_sigma=a.sigma,
                   abs_err_tolerance=0.0, rel_err_tolerance=0.0)
    print(f"{model.robot.name}: dof {model.robot.dof}, batch {a.batch}, {a.dtype}, packed as {type(dcem.packed).__name__}; "
          f"DCEM {a.dcem_iters} iterations of {a.samples} samples, {a.elite} elites; LM {a.lm_iters} iterations")
    with torch.no_grad():
        obj.update({"theta": start.clone()})
        summary("start", dcem.packed.error_metric())
        info = lm.optimize(damping=0.1)
        summary("LM alone", info.last_err)
        obj.update({"theta": start.clone()})
        info = dcem.optimize(generator=torch.Generator(device="cuda").manual_seed(a.seed + 2), track_best_solution=True)
        summary("DCEM", info.last_err)
        obj.update({"theta": info.best_solution["theta"].to("cuda")})
        info = lm.optimize(damping=0.1)
        summary("DCEM, then LM", info.last_err)


if __name__ == "__main__":
    main()
