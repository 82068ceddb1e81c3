"""Batched inverse kinematics on a URDF chain -- the third part of the reference's examples/inverse_kinematics.py on the fused path:
the Panda of tests/golden/panda_no_gripper.urdf, random reachable targets fk(rand), a start from zeros, Levenberg-Marquardt with 15
iterations and step_size = 0.5, every problem of the batch in one launch per linearization (theseus_amd/kinematics.py:
PackedKinematics on csrc/kin_kernels.hip).

    python examples/inverse_kinematics.py --batch 1024 [--limits] [--dtype f64] [--urdf robot.urdf --link tool]

The cost is LinkPoseCost = target.local(fk(theta)); the reference example writes pose.local(target), its negation, which has the same
squared error and the same Gauss-Newton step.  ``--limits`` adds joint limits (HingeCost; the limits are given here, they are not
read from the URDF) and a weak rest-pose prior (Difference)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PANDA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "panda_no_gripper.urdf")
EE_NAME = "panda_virtual_ee_link"
# the Panda's joint limits (rad)
PANDA_LOWER = (-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973)
PANDA_UPPER = (2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973)


def make_objective(th, B, dtype, device, urdf=PANDA, link=EE_NAME, limits=False, seed=0, autodiff=False):
    """-> (objective, model, target angles (B, dof)); ``autodiff``: the pose cost as an AutoDiffCostFunction over the model's forward
    kinematics (the generic path: what a user had to write before the fused family)"""
    model = th.eb.UrdfRobotModel(urdf, device=device, dtype=dtype, link_names=[link])
    dof = model.robot.dof
    gen = torch.Generator().manual_seed(seed)
    target_theta = torch.rand(B, dof, generator=gen, dtype=torch.float64).to(dtype).to(device)
    if limits and urdf == PANDA:   # (targets inside the limits)
        lo, hi = torch.tensor(PANDA_LOWER, dtype=dtype, device=device), torch.tensor(PANDA_UPPER, dtype=dtype, device=device)
        target_theta = lo + 0.1 + target_theta * (hi - lo - 0.2)
    with torch.no_grad():
        target = model.forward_kinematics(target_theta)[link]
    target.name = "target"
    theta = th.Vector(tensor=torch.zeros(B, dof, dtype=dtype, device=device), name="theta")
    weight = th.ScaleCostWeight(torch.ones(1, 1, dtype=dtype, device=device))
    obj = th.Objective(dtype=dtype)
    if autodiff:
        from theseus_amd import se3_torch

        def pose_error(optim_vars, aux_vars):
            return se3_torch.local(aux_vars[0].tensor, model.forward_kinematics(optim_vars[0].tensor)[link].tensor)
        obj.add(th.AutoDiffCostFunction([theta], pose_error, 6, cost_weight=weight, aux_vars=[target], name="ee_pose"))
    else:
        obj.add(th.eb.LinkPoseCost(theta, target, weight, model, link, name="ee_pose"))
    if limits:
        if urdf == PANDA:
            lo, hi = torch.tensor([PANDA_LOWER], dtype=dtype, device=device), torch.tensor([PANDA_UPPER], dtype=dtype, device=device)
        else:
            lo, hi = (torch.full((1, dof), v, dtype=dtype, device=device) for v in (-float("inf"), float("inf")))
        thr = torch.full((1, dof), 0.05, dtype=dtype, device=device)
        obj.add(th.eb.HingeCost(theta, lo, hi, thr, th.ScaleCostWeight(torch.full((1, 1), 10.0, dtype=dtype, device=device)),
                                name="joint_limits"))
        rest = th.Vector(tensor=(0.5 * (lo + hi)).nan_to_num(0.0, 0.0, 0.0), name="rest_pose")
        obj.add(th.Difference(theta, rest, th.ScaleCostWeight(torch.full((1, 1), 1e-2, dtype=dtype, device=device)), name="rest"))
    return obj, model, target_theta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--urdf", default=PANDA)
    ap.add_argument("--link", default=EE_NAME)
    ap.add_argument("--limits", action="store_true", help="add joint limits (HingeCost) and a rest-pose prior (Difference)")
    ap.add_argument("--iters", type=int, default=15)
    a = ap.parse_args()
    import theseus_amd as th
    dtype = torch.float32 if a.dtype == "f32" else torch.float64
    obj, model, _ = make_objective(th, a.batch, dtype, "cuda", a.urdf, a.link, a.limits)
    opt = th.LevenbergMarquardt(obj, max_iterations=a.iters, step_size=0.5)
    print(f"{model.robot.name}: dof {model.robot.dof}, batch {a.batch}, {a.dtype}, packed as "
          f"{type(opt.linear_solver.linearization.packed).__name__}")
    with torch.no_grad():
        sol, info = th.TheseusLayer(opt).forward(None, optimizer_kwargs=dict(damping=0.1, track_err_history=True))
        theta = sol["theta"].to("cuda")
        pose = model.forward_kinematics(theta)[a.link].tensor
        target = obj.get_variable("target").tensor
    err = info.err_history
    print(f"objective: mean {float(err[:, 0].mean()):.3e} -> {float(err[:, -1].mean()):.3e}, worst {float(err[:, -1].max()):.3e}")
    print(f"end-effector position error: mean {float((pose[:, :, 3] - target[:, :, 3]).norm(dim=1).mean()):.3e} m")
    if a.limits and a.urdf == PANDA:
        lo, hi = torch.tensor(PANDA_LOWER, dtype=dtype, device="cuda"), torch.tensor(PANDA_UPPER, dtype=dtype, device="cuda")
        print(f"joint-limit violations: {int(((theta < lo) | (theta > hi)).any(1).sum())} of {a.batch} problems")


if __name__ == "__main__":
    main()
