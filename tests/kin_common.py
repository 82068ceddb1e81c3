"""The inverse-kinematics objectives of the kin fixtures (tests/golden/kin_f64_panda.npz, kin_f64_tree.npz, written by
tools/gen_kin_golden.py from the REAL reference), built on either API: ``th`` is ``theseus_amd`` in the tests and ``theseus`` in the
generator (which passes its own ``link_cost``: an AutoDiffCostFunction over the reference's forward kinematics).

A problem is a dict (an npz, or ``chain_problem``'s):
  urdf                    file name under tests/golden  | chain_parents, chain_types, chain_origins, chain_axes  (Robot.from_joints)
  theta_0 (B, dof)        the start
  pose_link, w_pose, and  target_angles (B|1, dof): the pose target is fk(target_angles)  |  pose_target (B|1, 3, 4)
  pos_link, pos_target (B|1, 3), w_pos
  hinge_down, hinge_up, hinge_thr (1, dof), w_hinge
  prior_target (B|1, dof), w_prior
Costs in objective order: pose, pos, limits, prior (those whose keys are present); a weight of width 1 is a ScaleCostWeight, any
other a DiagonalCostWeight.  The leaves implicit gradients are taken for: target_angles (or pose_target), pos_target, prior_target.

Also here: random kinematic chains for the GPU tests."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("kin_f64_panda", "kin_f64_tree")
PANDA_URDF, TREE_URDF = "panda_no_gripper.urdf", "kin_tree.urdf"
EE_NAME = "panda_virtual_ee_link"
HOME_POSE = (-0.1394, -0.0205, -0.0520, -2.0691, 0.0506, 2.0029, -0.9168)   # (the reference test's start)
LM_KW = dict(max_iterations=5, step_size=0.5, abs_err_tolerance=0.0, rel_err_tolerance=0.0)
LM_DAMPING = 0.1
LEAVES = ("target_angles", "pose_target", "pos_target", "prior_target")


def has(f, key):
    return key in f and np.asarray(f[key]).size > 0


def make_model(th, f, dtype, device, link_names):
    """the UrdfRobotModel of a problem on theseus_amd"""
    if has(f, "urdf"):
        return th.eb.UrdfRobotModel(os.path.join(GOLDEN, str(f["urdf"])), device=device, dtype=dtype, link_names=link_names)
    robot = th.eb.Robot.from_joints(np.asarray(f["chain_parents"]).tolist(), [str(t) for t in np.asarray(f["chain_types"]).tolist()],
                                    f["chain_origins"], f["chain_axes"], dtype=dtype, device=device)
    return th.eb.UrdfRobotModel(None, link_names=link_names, robot=robot)


def _weight(th, t, name):
    v = th.Variable(t, name=name)
    return th.ScaleCostWeight(v) if t.shape[1] == 1 else th.DiagonalCostWeight(v)


def build(th, f, device="cpu", dtype=torch.float64, grad=False, model=None, link_cost=None, se3=None):
    """-> (objective, {leaf name: tensor}, [cost names in objective order], model); ``grad``: the leaves require grad."""
    def t(key):
        return torch.from_numpy(np.asarray(f[key])).to(dtype).to(device)
    links = [str(f[k]) for k in ("pose_link", "pos_link") if has(f, k)]
    model = model(f, dtype, device, links) if model is not None else make_model(th, f, dtype, device, links)
    se3 = se3 or (lambda tensor, name: th.SE3(tensor=tensor, name=name))
    if link_cost is None:
        def link_cost(kind, theta, target, weight, model, link, name):
            cls = th.eb.LinkPoseCost if kind == "pose" else th.eb.LinkPositionCost
            return cls(theta, target, weight, model, link, name=name)
    leaves = {}
    theta = th.Vector(tensor=t("theta_0").clone(), name="theta")
    obj = th.Objective(dtype=dtype)
    if has(f, "pose_link"):
        if has(f, "target_angles"):
            leaves["target_angles"] = t("target_angles").clone().requires_grad_(grad)
            target = model.forward_kinematics(leaves["target_angles"])[str(f["pose_link"])].tensor
        else:
            target = leaves["pose_target"] = t("pose_target").clone().requires_grad_(grad)
        obj.add(link_cost("pose", theta, se3(target, "pose_target"), _weight(th, t("w_pose"), "w_pose"), model, str(f["pose_link"]),
                          "pose"))
    if has(f, "pos_link"):
        leaves["pos_target"] = t("pos_target").clone().requires_grad_(grad)
        obj.add(link_cost("pos", theta, th.Point3(tensor=leaves["pos_target"], name="pos_target"), _weight(th, t("w_pos"), "w_pos"),
                          model, str(f["pos_link"]), "pos"))
    if has(f, "hinge_down"):
        obj.add(th.eb.HingeCost(theta, t("hinge_down"), t("hinge_up"), t("hinge_thr"), _weight(th, t("w_hinge"), "w_hinge"),
                                name="limits"))
    if has(f, "prior_target"):
        leaves["prior_target"] = t("prior_target").clone().requires_grad_(grad)
        obj.add(th.Difference(theta, th.Vector(tensor=leaves["prior_target"], name="prior_target"), _weight(th, t("w_prior"), "w_prior"),
                              name="prior"))
    return obj, leaves, list(obj.cost_functions.keys()), model


# ---- random chains ---------------------------------------------------------------------------------------------------------------
def random_rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def random_joints(types, parents, seed):
    """(origins (J, 3, 4), axes (J, 3)): random rotations, offsets of a few decimetres, random unit axes"""
    rng = np.random.default_rng(seed)
    J = len(types)
    origins = np.zeros((J, 3, 4))
    axes = np.zeros((J, 3))
    for i in range(J):
        origins[i, :, :3] = random_rotation(rng)
        origins[i, :, 3] = rng.uniform(-0.4, 0.4, 3)
        a = rng.normal(size=3)
        axes[i] = a / np.linalg.norm(a)
    return origins, axes


def chain_problem(th, types, parents, pose_link, pos_link, B, seed, shared_targets=False, hinge=True, prior=True, urdf=None,
                  away=(0.3, 0.9)):
    """A problem for the kernels alone (no reference run) on a random tree given by ``types`` / ``parents`` (Robot.from_joints) or on
    the robot of ``urdf`` (a file under tests/golden): the pose target is fk of angles ``away`` rad from the start in every
    joint; the tests assert through ``pose_angle`` that the pose error's rotation stays clear of both Taylor switches and of pi."""
    rng = np.random.default_rng(seed)
    if urdf is not None:
        f = dict(urdf=np.asarray(urdf))
        robot = th.eb.Robot.from_urdf_file(os.path.join(GOLDEN, urdf), dtype=torch.float64)
    else:
        origins, axes = random_joints(types, parents, seed)
        f = dict(chain_parents=np.asarray(parents), chain_types=np.asarray(types), chain_origins=origins, chain_axes=axes)
        robot = th.eb.Robot.from_joints(parents, types, origins, axes, dtype=torch.float64)
    dof = robot.dof
    f["theta_0"] = rng.uniform(-1.0, 1.0, (B, dof))
    Bt = 1 if shared_targets else B
    if pose_link is not None:
        f["pose_link"] = np.asarray(pose_link)
        away = rng.uniform(away[0], away[1], (Bt, dof)) * rng.choice([-1.0, 1.0], (Bt, dof))
        with torch.no_grad():
            T, _ = robot.link_fk(torch.from_numpy(f["theta_0"][:Bt] + away), pose_link, jacobian=False)
        f["pose_target"] = T.numpy()
        f["w_pose"] = np.linspace(0.5, 2.0, 6).reshape(1, 6)
    if pos_link is not None:
        f["pos_link"] = np.asarray(pos_link)
        f["pos_target"] = rng.uniform(-0.5, 0.5, (Bt, 3))
        f["w_pos"] = np.array([[1.5]])
    if hinge:
        f["hinge_down"] = np.full((1, dof), -0.5)
        f["hinge_up"] = np.full((1, dof), 0.6)
        f["hinge_up"][0, 0] = np.inf
        f["hinge_thr"] = np.full((1, dof), 0.05)
        f["w_hinge"] = np.linspace(1.0, 2.0, dof).reshape(1, dof)
        kinks = np.stack([f["hinge_down"] + f["hinge_thr"], f["hinge_up"] - f["hinge_thr"]])
        near = np.abs(f["theta_0"][None] - kinks[:, :, :]).min(0) < 1e-3   # (B, dof): move such a start off the kink
        f["theta_0"] = np.where(near, f["theta_0"] + 0.01, f["theta_0"])
    if prior:
        f["prior_target"] = rng.uniform(-0.3, 0.3, (Bt, dof))
        f["w_prior"] = np.array([[0.7]])
    return f


def pose_angle(cost):
    """the rotation angle of a LinkPoseCost's error, per problem (fp64)"""
    with torch.no_grad():
        return cost.error()[:, 3:].double().norm(dim=1)
