"""Generate the inverse-kinematics fixtures by RUNNING THE REAL REFERENCE (test infrastructure; needs the reference importable, CPU
only).

    python -m tools.gen_kin_golden

The objectives of tests/kin_common.py on the reference: the two link costs are th.AutoDiffCostFunction (autograd_mode="vmap") over
th.eb.UrdfRobotModel.forward_kinematics -- target.local(fk(theta)) and fk(theta).translation - target -- next to th.Difference and
th.eb.HingeCost.  The reference's vendored URDF parser calls Element.getchildren(), which Python's ElementTree no longer has: every
loaded torchkin.third_party.urdf_parser_py module gets ``xml_children`` replaced before anything is parsed.  fp64, B = 3.  Writes
under tests/golden/:
  kin_f64_panda.npz   the Panda (tests/golden/panda_no_gripper.urdf, a copy of the reference's data file): LinkPoseCost on the end
                      effector with a Scale weight, Difference prior with a Scale weight; target = fk(random angles), start =
                      HOME_POSE + noise.  Also the targets of the reference's own IK test (seed 1, float32 as there) for B = 1, 3.
  kin_f64_tree.npz    tests/golden/kin_tree.urdf: LinkPoseCost on tool_a with a Diagonal(6) weight, LinkPositionCost on tool_b with a
                      Diagonal(3) weight and a target of batch 1, HingeCost with some limits active at the start and one infinite,
                      Difference with a Diagonal(dof) weight.
Each records the inputs, the reference robot's table (joint order, types, parent / child link ids, origins, axes, every link's
ancestor_non_fixed_joint_ids), fk poses with body and spatial Jacobians of every link at the start, every cost's weighted Jacobian
block and error (wj_<cost>_0, we_<cost>), AtA / Atb of DenseLinearization, the error metric, the iterates of 5 LM iterations with
CholeskyDenseSolver, and -- implicit backward mode -- the gradients of sum(solution^2) w.r.t. the leaves of tests/kin_common.py
(the pose target's leaf is target_angles: the target stays on the manifold).
Asserted: the pose error's rotation angle lies in [0.2, 2.5] rad at every recorded iterate (away from both Taylor switches and from
pi), no hinge argument lies within 1e-3 of a kink, so an fp32 copy of the inputs takes the same branches, and every revolute joint
angle of every recorded state is at least 6e-3 rad: below 5e-3 the reference's rotation SO3.exp(angle * axis) takes a branch that is
off by angle^3 / 12, where theseus_amd's I + sin [a]x + (1 - cos) [a]x^2 is exact.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

from oracle.gen_golden import OUT, REF, import_reference
from tests.kin_common import EE_NAME, GOLDEN, HOME_POSE, LM_DAMPING, LM_KW, PANDA_URDF, TREE_URDF, build, has

B = 3


def patch_urdf_parser():
    import torchkin  # noqa: F401
    for name, mod in list(sys.modules.items()):
        if name.startswith("torchkin.third_party.urdf_parser_py") and hasattr(mod, "xml_children"):
            mod.xml_children = lambda n: [c for c in n if isinstance(c.tag, str)]


def reference_builders(th):
    paths = {}

    def urdf_path(model):
        return paths[id(model)]

    def model(f, dtype, device, links):
        m = th.eb.UrdfRobotModel(os.path.join(GOLDEN, str(f["urdf"])), device=device, dtype=dtype, link_names=links)
        paths[id(m)] = os.path.join(GOLDEN, str(f["urdf"]))
        return m

    def se3(tensor, name):
        return th.SE3(tensor=tensor, name=name, strict_checks=False)

    def link_cost(kind, theta, target, weight, model, link, name):
        # (one model per link: the reference's forward-kinematics backward does not batch under vmap with two selected links)
        model = th.eb.UrdfRobotModel(urdf_path(model), dtype=theta.dtype, link_names=[link])
        if kind == "pose":
            def fn(optim_vars, aux_vars):
                return aux_vars[0].local(model.forward_kinematics(optim_vars[0])[link])
            dim = 6
        else:
            def fn(optim_vars, aux_vars):
                return model.forward_kinematics(optim_vars[0])[link].tensor[:, :, 3] - aux_vars[0].tensor
            dim = 3
        return th.AutoDiffCostFunction([theta], fn, dim, cost_weight=weight, aux_vars=[target], name=name, autograd_mode="vmap")
    return dict(model=model, se3=se3, link_cost=link_cost)


def robot_table(robot):
    dof = robot.dof
    anc = -np.ones((robot.num_links, max(dof, 1)), dtype=np.int64)
    for link in robot.links:
        ids = link.ancestor_non_fixed_joint_ids
        anc[link.id, :len(ids)] = ids
    return dict(robot_dof=np.array(dof), robot_links=np.array([link.name for link in robot.links]),
                robot_joints=np.array([j.name for j in robot.joints]),
                robot_joint_types=np.array([type(j).__name__ for j in robot.joints]),
                robot_joint_parent=np.array([j.parent_link.id for j in robot.joints]),
                robot_joint_child=np.array([j.child_link.id for j in robot.joints]),
                robot_origins=torch.cat([j.origin for j in robot.joints]).numpy(),
                robot_axes=torch.stack([j.axis.view(6) if j.axis.numel() == 6 else torch.zeros(6) for j in robot.joints]).numpy(),
                robot_ancestors=anc)


def pose_angles(th, f, thetas, kw):
    """the rotation angle of the pose cost's error at every (K, B, dof) state"""
    obj, _, _, _ = build(th, f, **kw)
    out = []
    for x in thetas:
        obj.update({"theta": torch.from_numpy(np.ascontiguousarray(x))})
        out.append(obj.cost_functions["pose"].error()[:, 3:].norm(dim=1).detach().numpy())
    return np.stack(out)


def hinge_margin(f, thetas):
    if not has(f, "hinge_down"):
        return np.inf
    kinks = np.stack([f["hinge_down"] + f["hinge_thr"], f["hinge_up"] - f["hinge_thr"]])   # (2, 1, dof)
    return float(np.abs(np.asarray(thetas)[:, None] - kinks[None]).min())


def generate(th, name, f):
    kw = reference_builders(th)
    out = dict(f)
    obj, _, costs, model = build(th, f, **kw)
    names = list(obj.optim_vars.keys())
    out["var_order"], out["cost_order"] = np.array(names), np.array(costs)
    out.update(robot_table(model.robot))
    # forward kinematics of every link at the start
    full = th.eb.UrdfRobotModel(os.path.join(GOLDEN, str(f["urdf"])), dtype=torch.float64,
                                link_names=[link.name for link in model.robot.links])
    theta0 = torch.from_numpy(f["theta_0"])
    jb, js = {}, {}
    poses = full.forward_kinematics(theta0, jacobians=jb)
    full.forward_kinematics(theta0, jacobians=js, use_body_jacobians=False)
    out["fk_poses"] = np.stack([poses[n].tensor.numpy() for n in full.link_names])
    out["fk_body"] = np.stack([jb[n].numpy() for n in full.link_names])
    out["fk_spatial"] = np.stack([js[n].numpy() for n in full.link_names])
    obj.update()
    for cname, c in obj.cost_functions.items():
        jac, err = c.weighted_jacobians_error()
        out[f"we_{cname}"] = err.detach().numpy()
        for s, j in enumerate(jac):
            out[f"wj_{cname}_{s}"] = j.detach().numpy()
    lin = th.DenseLinearization(obj)
    lin.linearize()
    out.update(AtA=lin.AtA.detach().numpy(), Atb=lin.Atb.squeeze(2).detach().numpy(), error_metric=obj.error_metric().detach().numpy(),
               error=obj.error().detach().numpy())
    if has(f, "target_angles"):
        out["pose_target"] = obj.aux_vars["pose_target"].tensor.detach().numpy()
    # 5 LM iterations
    obj, _, _, _ = build(th, f, **kw)
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.CholeskyDenseSolver, vectorize=False, **LM_KW)
    with torch.no_grad():
        sol, info = th.TheseusLayer(opt).forward(optimizer_kwargs=dict(damping=LM_DAMPING, track_err_history=True, track_state_history=True))
    out["lm_iterates"] = torch.cat([info.state_history[k] for k in names], dim=1).permute(2, 0, 1).numpy()   # (K + 1, B, dof)
    out["lm_err_history"] = info.err_history.numpy()
    # implicit backward
    obj, leaves, _, _ = build(th, f, grad=True, **kw)
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.CholeskyDenseSolver, vectorize=False, **LM_KW)
    sol, info = th.TheseusLayer(opt).forward(optimizer_kwargs=dict(damping=LM_DAMPING, backward_mode="implicit"))
    final = torch.cat([sol[k] for k in names], dim=1)
    loss = (final ** 2).sum()
    loss.backward()
    out.update(implicit_final=final.detach().numpy(), implicit_loss=loss.item(), **{f"grad_{k}": v.grad.numpy() for k, v in leaves.items()})
    states = list(out["lm_iterates"]) + [out["implicit_final"]]
    angles = pose_angles(th, f, states, kw)
    assert 0.2 <= angles.min() and angles.max() <= 2.5, f"pose error angles {angles.min():.3f} ... {angles.max():.3f} rad"
    # the reference's revolute rotation is SO3.exp(angle * axis), whose branch below so3_near_zero_eps (5e-3 rad in fp64) replaces
    # sin(t) / t by (cos(t) + 1) / 2 -- off by t^3 / 12, 1e-8 at the switch; theseus_amd's closed form has no such branch
    revolute = out["robot_joint_types"][:int(out["robot_dof"])] == "RevoluteJoint"
    every = np.concatenate([np.asarray(states).reshape(-1, revolute.size), np.asarray(f["target_angles"]).reshape(-1, revolute.size)])
    small = float(np.abs(every[:, revolute]).min())
    assert small >= 6e-3, f"a revolute joint angle of {small:.2e} rad lies inside the reference's small-angle branch"
    margin = hinge_margin(f, states)
    assert margin >= 1e-3, f"a hinge argument lies {margin:.2e} from a kink"
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(name, "err", out["lm_err_history"][:, 0], "->", out["lm_err_history"][:, -1], "loss", loss.item(), "angles",
          angles.min(), angles.max(), "hinge margin", margin, {k: float(v.grad.abs().max()) for k, v in leaves.items()})


def ik_test_targets(batch_size):
    """the targets of the reference's tests/theseus_tests/embodied/kinematics/test_inverse_kinematics.py (its ``ee_pose_target``
    fixture, seed 1, float32 as that test runs): the reference's own function, loaded from its file"""
    path = os.path.join(REF, "tests", "theseus_tests", "embodied", "kinematics", "test_inverse_kinematics.py")
    spec = importlib.util.spec_from_file_location("reference_test_inverse_kinematics", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fixture = mod.ee_pose_target
    make = getattr(fixture, "__wrapped__", None) or fixture._get_wrapped_function()
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float32)
    try:
        return make(batch_size).tensor.double().numpy()
    finally:
        torch.set_default_dtype(old)


def panda_problem(th):
    rng = np.random.default_rng(11)
    theta0 = np.asarray(HOME_POSE)[None] + rng.normal(0, 0.01, (B, 7))
    home = np.asarray(HOME_POSE)[None]
    # (joints that rest near zero move away from it, so that no iterate enters the reference's small-angle branch)
    sign = np.where(np.abs(home) < 0.2, np.sign(home), rng.choice([-1.0, 1.0], (B, 7)))
    f = dict(urdf=np.asarray(PANDA_URDF), theta_0=theta0, pose_link=np.asarray(EE_NAME),
             target_angles=home + rng.uniform(0.35, 0.65, (B, 7)) * sign,
             w_pose=np.array([[1.0]]), prior_target=home + rng.normal(0, 0.01, (1, 7)), w_prior=np.array([[2.0]]))
    f["ik_target_b1"], f["ik_target_b3"] = ik_test_targets(1), ik_test_targets(3)
    return f


def tree_problem():
    rng = np.random.default_rng(12)
    dof = 6
    theta0 = rng.uniform(-0.8, 0.8, (B, dof))
    theta0[:, 2] *= 0.3   # (the prismatic joint, in metres)
    away = rng.uniform(0.5, 0.9, (B, dof)) * rng.choice([-1.0, 1.0], (B, dof))
    away[:, 2] *= 0.3
    down, up = np.full((1, dof), -0.5), np.full((1, dof), 0.5)
    up[0, 1] = np.inf   # (the continuous joint has no upper limit)
    return dict(urdf=np.asarray(TREE_URDF), theta_0=theta0, pose_link=np.asarray("tool_a"), target_angles=theta0 + away,
                w_pose=np.array([[1.0, 1.2, 0.8, 2.0, 2.5, 1.5]]), pos_link=np.asarray("tool_b"),
                pos_target=np.array([[0.35, -0.1, 0.55]]), w_pos=np.array([[1.5, 0.5, 1.0]]), hinge_down=down, hinge_up=up,
                hinge_thr=np.full((1, dof), 0.05), w_hinge=np.array([[0.8]]), prior_target=rng.uniform(-0.2, 0.2, (B, dof)),
                w_prior=np.linspace(1.0, 2.0, dof).reshape(1, dof))


def main():
    th, _ = import_reference()
    patch_urdf_parser()
    torch.set_default_dtype(torch.float64)
    generate(th, "kin_f64_panda", panda_problem(th))
    generate(th, "kin_f64_tree", tree_problem())


if __name__ == "__main__":
    main()
