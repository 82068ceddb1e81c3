"""Robot kinematics on URDF chains and inverse kinematics as a fused cost family (the reference's torchkin.Robot,
theseus.embodied.kinematics.UrdfRobotModel, examples/inverse_kinematics.py).

``Robot``            the kinematic tree of a URDF (revolute / continuous / prismatic / fixed joints), parsed with
                     xml.etree.ElementTree; fixed joints are folded into the origins of the joints behind them, ids come from a
                     breadth-first walk with the non-fixed joints first, so column k of a Jacobian is joint k.
``UrdfRobotModel``   forward kinematics with body / spatial Jacobians, differentiable torch on theseus_amd/se3_torch.py.
``LinkPoseCost``     6 rows, target.local(T_link(theta)) = log(target^-1 T_link), Jacobian Jlog J_body.  The reference example writes
                     pose.local(target), its negation: the same squared error and the same Gauss-Newton step.
``LinkPositionCost`` 3 rows, t_link(theta) - target, Jacobian R_link J_body[:3].
``PackedKinematics`` PackedEuclidean -- the (B, n) state, retraction by thx_vec_retract, implicit / unrolled / truncated backward
                     through the torch classes -- whose NON-differentiated evaluation is fused (theseus_amd/term_table.py):
                     ``assemble`` = thx_kin_eval into persistent block buffers + thx_block_assemble, ``error_metric`` =
                     thx_kin_error (csrc/kin_kernels.hip).  It accepts an objective whose optimisation variables are Vector(dof) of
                     ONE robot and whose costs are link costs, Difference on such a vector (rest-pose prior) and HingeCost on one
                     (joint limits), each with a Scale / DiagonalCostWeight, at least one of them a link cost.

The path of a link -- the joints from the root to it, fixed offsets folded in -- is extracted on the host into one device table of
thx_kin_joint entries that the packed class owns; a term's record names its path by offset and length (at most THX_KIN_MAX_PATH).
"""
import warnings
import xml.etree.ElementTree as ET
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, se3_torch
from .core import SE3, CostFunction, CostWeight, Point3, Vector
from .euclidean import PackedEuclidean, _is_euclidean
from .generic import _names
from .term_table import TermKind, TermTable, term_dtype, weight_var

KIN_TERM = term_dtype("var")   # var = (first state column of theta, first entry of the path, entries of the path, -1)
# thx_kin_joint of include/theseus_hip.h: fp64 in either dtype (the origins are evaluated in fp64 and cast to the run's dtype first)
KIN_JOINT = np.dtype([("type", "<i4"), ("theta", "<i4"), ("origin", "<f8", (12,)), ("axis", "<f8", (3,))])
assert KIN_JOINT.itemsize == 128
JOINT_TYPES = {"revolute": _lib.KIN_REVOLUTE, "continuous": _lib.KIN_REVOLUTE, "prismatic": _lib.KIN_PRISMATIC,
               "fixed": _lib.KIN_FIXED}


class Link:
    def __init__(self, name: str):
        self.name = name
        self.id: Optional[int] = None
        self.parent_joint: Optional["Joint"] = None
        self.child_joints: List["Joint"] = []
        self.ancestor_links: List["Link"] = []
        self.ancestor_non_fixed_joint_ids: List[int] = []

    @property
    def parent_link(self) -> Optional["Link"]:
        return self.parent_joint.parent_link if self.parent_joint is not None else None


class Joint:
    """``origin`` (3, 4) and ``axis`` (3,) are fp64 masters; ``Robot.tables`` casts them."""

    def __init__(self, name: str, kind: str, parent_link: Link, child_link: Link, origin: torch.Tensor, axis: Optional[torch.Tensor]):
        self.name, self.kind, self.parent_link, self.child_link = name, kind, parent_link, child_link
        self.type = JOINT_TYPES[kind]
        self.origin, self.axis = origin, axis if axis is not None else torch.zeros(3, dtype=torch.float64)
        self.id: Optional[int] = None

    @property
    def dof(self) -> int:
        return 0 if self.type == _lib.KIN_FIXED else 1


def _origin(xyz, rpy) -> torch.Tensor:
    """(3, 4) fp64 from a URDF origin: R = Rz(yaw) Ry(pitch) Rx(roll), t = xyz"""
    t = torch.tensor(xyz if xyz is not None else [0.0, 0.0, 0.0], dtype=torch.float64)
    if rpy is None:
        return torch.cat([torch.eye(3, dtype=torch.float64), t.view(3, 1)], dim=1)
    angles = torch.tensor(rpy, dtype=torch.float64)
    (cr, cp, cy), (sr, sp, sy) = angles.cos(), angles.sin()
    R = torch.stack([torch.stack([cy * cp, (cy * sp * sr) - (cr * sy), (sy * sr) + (cy * cr * sp)]),
                     torch.stack([cp * sy, (cy * cr) + (sy * sp * sr), (cr * sy * sp) - (cy * sr)]),
                     torch.stack([-sp, cp * sr, cp * cr])])
    return torch.cat([R, t.view(3, 1)], dim=1)


def _floats(text, what):
    vals = [float(x) for x in text.split()]
    if len(vals) != 3:
        raise ValueError(f"{what}: expected three numbers, got {text!r}")
    return vals


class Robot:
    def __init__(self, name: str, dtype: Optional[torch.dtype] = None, device=None):
        self.name = name
        self.dtype = dtype if dtype is not None else torch.get_default_dtype()
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.dof = 0
        self.links: List[Link] = []
        self.joints: List[Joint] = []
        self.link_map: Dict[str, Link] = {}
        self.joint_map: Dict[str, Joint] = {}
        self._tables = {}
        self._paths = {}

    # ---- construction ------------------------------------------------------------------------------------------------------
    @staticmethod
    def from_urdf_file(path: str, dtype: Optional[torch.dtype] = None, device=None) -> "Robot":
        with open(path) as f:
            return Robot.from_urdf_string(f.read(), dtype, device)

    @staticmethod
    def from_urdf_string(text: str, dtype: Optional[torch.dtype] = None, device=None) -> "Robot":
        root = ET.fromstring(text)
        if root.tag != "robot":
            raise ValueError(f"not a URDF: the root element is <{root.tag}>")
        links = [el.get("name") for el in root.findall("link")]
        specs = []
        for el in root.findall("joint"):
            name, kind = el.get("name"), el.get("type")
            o, a = el.find("origin"), el.find("axis")
            xyz = _floats(o.get("xyz"), f"joint {name} origin xyz") if o is not None and o.get("xyz") is not None else None
            rpy = _floats(o.get("rpy"), f"joint {name} origin rpy") if o is not None and o.get("rpy") is not None else None
            axis = _floats(a.get("xyz"), f"joint {name} axis") if a is not None and a.get("xyz") is not None else [1.0, 0.0, 0.0]
            specs.append((name, kind, el.find("parent").get("link"), el.find("child").get("link"), _origin(xyz, rpy),
                          torch.tensor(axis, dtype=torch.float64)))
        return Robot._build(root.get("name") or "robot", links, specs, dtype, device)

    @staticmethod
    def from_joints(parents: Sequence[int], types: Sequence[str], origins, axes, names: Optional[Sequence[str]] = None,
                    dtype: Optional[torch.dtype] = None, device=None) -> "Robot":
        """Joint i hangs link i + 1 on link ``parents[i]`` (link 0 is the root); ``origins`` (J, 3, 4), ``axes`` (J, 3) (ignored for a
        fixed joint); ``names``: the joints' names (links are link0, link1, ...)."""
        J = len(parents)
        origins = torch.as_tensor(np.asarray(origins), dtype=torch.float64).reshape(J, 3, 4)
        axes = torch.as_tensor(np.asarray(axes), dtype=torch.float64).reshape(J, 3)
        if len(types) != J or (names is not None and len(names) != J):
            raise ValueError("from_joints: parents, types, origins, axes and names must have one entry per joint")
        links = [f"link{k}" for k in range(J + 1)]
        specs = []
        for i in range(J):
            if not 0 <= int(parents[i]) <= J or int(parents[i]) == i + 1:
                raise ValueError(f"from_joints: joint {i} has no valid parent link")
            specs.append((names[i] if names is not None else f"joint{i}", types[i], links[int(parents[i])], links[i + 1],
                          origins[i].clone(), axes[i].clone()))
        return Robot._build("robot", links, specs, dtype, device)

    @staticmethod
    def _build(name, link_names, specs, dtype, device) -> "Robot":
        robot = Robot(name, dtype, device)
        for ln in link_names:
            robot.link_map[ln] = Link(ln)
        for jname, kind, parent, child, origin, axis in specs:
            if kind not in JOINT_TYPES:
                raise ValueError(f"joint {jname}: joint type {kind!r} is not supported (revolute, continuous, prismatic, fixed).")
            fixed = JOINT_TYPES[kind] == _lib.KIN_FIXED
            if not fixed and abs(float(axis.norm()) - 1.0) > 1e-9:
                raise ValueError(f"joint {jname}: the axis {axis.tolist()} is not a unit vector.")
            if parent not in robot.link_map or child not in robot.link_map:
                raise ValueError(f"joint {jname}: unknown link {parent if parent not in robot.link_map else child!r}")
            joint = Joint(jname, kind, robot.link_map[parent], robot.link_map[child], origin, None if fixed else axis)
            if joint.child_link.parent_joint is not None:
                raise ValueError(f"link {child} is the child of two joints")
            joint.child_link.parent_joint = joint
            joint.parent_link.child_joints.append(joint)
            robot.joint_map[jname] = joint
        roots = [ln for ln in robot.link_map.values() if ln.parent_joint is None]
        if len(roots) != 1:
            raise ValueError(f"a robot needs exactly one root link, found {[r.name for r in roots]}")
        # fold every fixed joint into the joints behind it: they become children of the fixed joint's parent link (the list grows
        # while it is walked, so a chain of fixed joints folds in one pass)
        for link in robot.link_map.values():
            for joint in link.child_joints:
                if joint.type == _lib.KIN_FIXED:
                    behind, joint.child_link.child_joints = joint.child_link.child_joints, []
                    for sub in behind:
                        sub.parent_link = link
                        sub.origin = se3_torch.compose(joint.origin.unsqueeze(0), sub.origin.unsqueeze(0))[0]
                        link.child_joints.append(sub)

        def number(joint):
            joint.id = len(robot.joints)
            robot.joints.append(joint)
            robot.dof += joint.dof
            joint.child_link.id = len(robot.links)
            robot.links.append(joint.child_link)
        # breadth first over the non-fixed joints, then the fixed ones in the order they were declared
        roots[0].id = 0
        robot.links.append(roots[0])
        queue = list(roots[0].child_joints)
        while queue:
            joint = queue.pop(0)
            if joint.type != _lib.KIN_FIXED:
                number(joint)
                queue += joint.child_link.child_joints
        for joint in robot.joint_map.values():
            if joint.id is None:
                if joint.type != _lib.KIN_FIXED:
                    raise ValueError(f"joint {joint.name} is not connected to the root link {roots[0].name}")
                number(joint)
        for link in robot.links:
            if link.parent_joint is not None:
                parent = link.parent_link
                link.ancestor_links = parent.ancestor_links + [parent]
                own = [] if link.parent_joint.type == _lib.KIN_FIXED else [link.parent_joint.id]
                link.ancestor_non_fixed_joint_ids = parent.ancestor_non_fixed_joint_ids + own
        return robot

    # ---- what the model and the packer read -----------------------------------------------------------------------------------
    @property
    def num_links(self) -> int:
        return len(self.links)

    @property
    def num_joints(self) -> int:
        return len(self.joints)

    @property
    def ancestor_non_fixed_joint_ids(self) -> List[List[int]]:
        return [list(link.ancestor_non_fixed_joint_ids) for link in self.links]

    def get_links(self, link_names: Optional[Sequence[str]] = None) -> List[Link]:
        return list(self.links) if link_names is None else [self.link_map[n] for n in link_names]

    def tables(self, dtype=None, device=None):
        """(origins (J, 3, 4), axes as tangents [prismatic; revolute] (J, 6)) by joint id, cast from the fp64 masters"""
        key = (dtype or self.dtype, torch.device(device) if device is not None else self.device)
        if key not in self._tables:
            origins = torch.stack([j.origin for j in self.joints]) if self.joints else torch.zeros(0, 3, 4, dtype=torch.float64)
            axes = torch.zeros(len(self.joints), 6, dtype=torch.float64)
            for j in self.joints:
                if j.type == _lib.KIN_REVOLUTE:
                    axes[j.id, 3:] = j.axis
                elif j.type == _lib.KIN_PRISMATIC:
                    axes[j.id, :3] = j.axis
            self._tables[key] = (origins.to(key[0]).to(key[1]), axes.to(key[0]).to(key[1]))
        return self._tables[key]

    def path(self, link_name: str) -> List[Joint]:
        """the joints from the root to the link, in that order (fixed joints in front of a joint are folded into its origin, so a
        fixed joint can only be the last one)"""
        if link_name not in self._paths:
            if link_name not in self.link_map:
                raise ValueError(f"robot {self.name} has no link {link_name!r}")
            path, joint = [], self.link_map[link_name].parent_joint
            while joint is not None:
                path.insert(0, joint)
                joint = joint.parent_link.parent_joint
            self._paths[link_name] = path
        return self._paths[link_name]

    def relative_pose(self, joint: Joint, q: Optional[torch.Tensor], origins, axes) -> torch.Tensor:
        """origin * motion(q): (B|1, 3, 4)"""
        o = origins[joint.id].unsqueeze(0)
        if joint.type == _lib.KIN_REVOLUTE:
            return torch.cat([o[:, :, :3] @ se3_torch.axis_rotation(axes[joint.id, 3:], q), o[:, :, 3:].expand(q.shape[0], 3, 1)], dim=2)
        if joint.type == _lib.KIN_PRISMATIC:
            t = o[:, :, :3] @ (q.view(-1, 1) * axes[joint.id, :3].view(1, 3)).unsqueeze(2) + o[:, :, 3:]
            return torch.cat([o[:, :, :3].expand(q.shape[0], 3, 3), t], dim=2)
        return o

    def link_fk(self, theta: torch.Tensor, link_name: str, jacobian: bool = True):
        """(T_link (B, 3, 4), body Jacobian (B, 6, dof) | None) along the link's path; columns of joints off the path are zero"""
        if theta.ndim != 2 or theta.shape[1] != self.dof:
            raise ValueError(f"Joint angles for {self.name} should be {self.dof}-D vectors")
        origins, axes = self.tables(theta.dtype, theta.device)
        B = theta.shape[0]
        T = torch.eye(3, 4, dtype=theta.dtype, device=theta.device).expand(B, 3, 4)
        cols = [None] * self.dof
        for joint in self.path(link_name):
            T = se3_torch.compose(T, self.relative_pose(joint, theta[:, joint.id] if joint.dof else None, origins, axes))
            if joint.dof and jacobian:
                cols[joint.id] = se3_torch.adjoint(T) @ axes[joint.id]
        if not jacobian:
            return T, None
        zero = torch.zeros(B, 6, dtype=theta.dtype, device=theta.device)
        Js = torch.stack([c if c is not None else zero for c in cols], dim=2) if self.dof else zero.new_zeros(B, 6, 0)
        return T, se3_torch.adjoint(se3_torch.inverse(T)) @ Js


class UrdfRobotModel:
    """theseus.embodied.kinematics.UrdfRobotModel: forward kinematics of the selected links (all of them by default)."""

    def __init__(self, urdf_path: str, device=None, dtype: torch.dtype = torch.float32, link_names: Optional[List[str]] = None,
                 robot: Optional[Robot] = None):
        self.robot = robot if robot is not None else Robot.from_urdf_file(urdf_path, dtype=dtype, device=device)
        self.link_names = list(link_names) if link_names is not None else [link.name for link in self.robot.links]
        for n in self.link_names:
            if n not in self.robot.link_map:
                raise ValueError(f"robot {self.robot.name} has no link {n!r}")

    def forward_kinematics(self, joint_states, jacobians: Optional[Dict[str, torch.Tensor]] = None,
                           use_body_jacobians: bool = True) -> Dict[str, SE3]:
        """{link name: SE3 pose}.  An empty ``jacobians`` dict is filled with the links' (B, 6, dof) body Jacobians (each in the frame
        of its link) or, ``use_body_jacobians=False``, spatial Jacobians (in the base frame)."""
        if jacobians is not None and len(jacobians) > 0:
            raise ValueError("Jacobians dictionary must be empty on input.")
        if joint_states.shape[-1] != self.robot.dof:
            raise ValueError(f"Robot model dofs ({self.robot.dof}) incompatible with input joint state dimensions "
                             f"({joint_states.shape[-1]}).")
        if isinstance(joint_states, torch.Tensor):
            theta = joint_states
        elif isinstance(joint_states, Vector):
            theta = joint_states.tensor
        else:
            raise Exception("Invalid input joint states data type. Valid types are torch.Tensor and th.Vector.")
        robot = self.robot
        if theta.ndim != 2:
            raise ValueError(f"Joint angles for {robot.name} should be {robot.dof}-D vectors")
        origins, axes = robot.tables(theta.dtype, theta.device)
        B = theta.shape[0]
        wanted = [robot.link_map[n] for n in self.link_names]
        related = sorted({a.id for link in wanted for a in link.ancestor_links} | {link.id for link in wanted})
        poses = {0: torch.eye(3, 4, dtype=theta.dtype, device=theta.device).expand(B, 3, 4)}
        for lid in related:
            if lid:
                joint = robot.links[lid].parent_joint
                rel = robot.relative_pose(joint, theta[:, joint.id] if joint.dof else None, origins, axes)
                poses[lid] = se3_torch.compose(poses[joint.parent_link.id], rel)
        if jacobians is not None:
            warnings.warn("The body Jacobian of a link is expressed in the frame of that link (the classical body Jacobian); set "
                          "`use_body_jacobians=False` for spatial Jacobians aligned with the base.", UserWarning)
            zero = torch.zeros(B, 6, dtype=theta.dtype, device=theta.device)
            spatial = {lid: se3_torch.adjoint(poses[lid]) @ axes[robot.links[lid].parent_joint.id]
                       for lid in related if lid and robot.links[lid].parent_joint.dof}
            for link in wanted:
                on_path = set(link.ancestor_non_fixed_joint_ids)
                Js = torch.stack([spatial[robot.joints[k].child_link.id] if k in on_path else zero for k in range(robot.dof)], dim=2)
                jacobians[link.name] = se3_torch.adjoint(se3_torch.inverse(poses[link.id])) @ Js if use_body_jacobians else Js
        return {link.name: SE3(tensor=poses[link.id]) for link in wanted}


# --------------------------------------------------------------------------------------------------------------------------------
# cost functions
# --------------------------------------------------------------------------------------------------------------------------------
class _LinkCost(CostFunction):
    def __init__(self, theta: Vector, target, cost_weight: CostWeight, robot_model, link_name: str, name: Optional[str] = None):
        super().__init__(cost_weight, name)
        self.robot = robot_model.robot if hasattr(robot_model, "robot") else robot_model
        if not _is_euclidean(theta) or theta.dof() != self.robot.dof:
            raise ValueError(f"{self.name}: theta must be a Vector of the robot's {self.robot.dof} degrees of freedom.")
        self.robot.path(link_name)   # (raises for an unknown link)
        self.theta, self.target, self.robot_model, self.link_name = theta, target, robot_model, link_name

    def optim_vars(self):
        return [self.theta]

    def aux_vars(self):
        return [self.target] + self.weight.aux_vars()


class LinkPoseCost(_LinkCost):
    """error = target.local(T_link(theta)) = log(target^-1 T_link) (6 rows, tangent order [v, w]); Jacobian = Jlog J_body.
    (examples/inverse_kinematics.py of the reference writes pose.local(target), the negation of this error: the same squared error,
    the same Gauss-Newton step.)"""

    def __init__(self, theta: Vector, target: SE3, cost_weight: CostWeight, robot_model, link_name: str, name: Optional[str] = None):
        if "SE3" not in _names(target):
            raise ValueError("LinkPoseCost expects a target of type SE3.")
        super().__init__(theta, target, cost_weight, robot_model, link_name, name)

    def dim(self) -> int:
        return 6

    def error(self) -> torch.Tensor:
        T, _ = self.robot.link_fk(self.theta.tensor, self.link_name, jacobian=False)
        return se3_torch.local(self.target.tensor, T)

    def jacobians(self):
        T, Jb = self.robot.link_fk(self.theta.tensor, self.link_name)
        err, Jlog = se3_torch.local(self.target.tensor, T, jac=True)
        return [Jlog @ Jb], err


class LinkPositionCost(_LinkCost):
    """error = t_link(theta) - target (3 rows); Jacobian = R_link J_body[:3]."""

    def __init__(self, theta: Vector, target: Point3, cost_weight: CostWeight, robot_model, link_name: str, name: Optional[str] = None):
        if not _is_euclidean(target) or target.dof() != 3:
            raise ValueError("LinkPositionCost expects a target of type Point3.")
        super().__init__(theta, target, cost_weight, robot_model, link_name, name)

    def dim(self) -> int:
        return 3

    def error(self) -> torch.Tensor:
        T, _ = self.robot.link_fk(self.theta.tensor, self.link_name, jacobian=False)
        return T[:, :, 3] - self.target.tensor

    def jacobians(self):
        T, Jb = self.robot.link_fk(self.theta.tensor, self.link_name)
        return [T[:, :, :3] @ Jb[:, :3]], T[:, :, 3] - self.target.tensor


# --------------------------------------------------------------------------------------------------------------------------------
# the packed family
# --------------------------------------------------------------------------------------------------------------------------------
_KINDS_MESSAGE = ("HIP backend, fused inverse kinematics: every optimisation variable must be a Vector of the degrees of freedom of "
                  "ONE robot and every cost one of four kinds: LinkPoseCost, LinkPositionCost, Difference on such a vector or "
                  "HingeCost on one -- each with a Scale / DiagonalCostWeight, and at least one of them a link cost.")


def _kin_kind(c):
    """THX_KIN_* of a cost function the fused kernels cover, else None."""
    names, w = _names(c), _names(c.weight)
    if not ("ScaleCostWeight" in w or "DiagonalCostWeight" in w):
        return None
    if "LinkPoseCost" in names:
        return _lib.KIN_POSE
    if "LinkPositionCost" in names:
        return _lib.KIN_POSITION
    if "HingeCost" in names:
        return _lib.KIN_HINGE if _is_euclidean(c.vector) else None
    if "Difference" in names:
        return _lib.KIN_PRIOR if _is_euclidean(c.var) else None
    return None


class PackedKinematics(TermTable, PackedEuclidean):
    family = "inverse kinematics"

    _TERM = KIN_TERM
    _KINDS = {
        _lib.KIN_POSE: TermKind(lambda c: [(c.target, 12), (weight_var(c), None)], weight=1),
        _lib.KIN_POSITION: TermKind(lambda c: [(c.target, 3), (weight_var(c), None)], weight=1),
        _lib.KIN_HINGE: TermKind(lambda c: [(c.down_limit, None), (c.up_limit, None), (c.threshold, None), (weight_var(c), None)],
                                 weight=3),
        _lib.KIN_PRIOR: TermKind(lambda c: [(c.target, None), (weight_var(c), None)], weight=1),
    }

    def __init__(self, objective, kernels=None, order=None):
        from .kernels import default_kernels
        from .packed import UnsupportedObjective
        K = kernels or default_kernels()
        if not hasattr(K, "kin_eval"):
            raise UnsupportedObjective("these kernels have no fused inverse-kinematics evaluation")
        self._paths_dev = None
        super().__init__(objective, K, order)

    def _check(self):
        from .packed import UnsupportedObjective
        self.kinds = [_kin_kind(c) for c in self.costs]
        links = [c for c, k in zip(self.costs, self.kinds) if k in (_lib.KIN_POSE, _lib.KIN_POSITION)]
        if not self.vars or any(k is None for k in self.kinds) or not links or any(not _is_euclidean(v) for v in self.vars):
            raise UnsupportedObjective(_KINDS_MESSAGE)
        self.robot = links[0].robot
        dof = self.robot.dof
        if any(c.robot is not self.robot for c in links) or any(v.dof() != dof for v in self.vars):
            raise UnsupportedObjective(_KINDS_MESSAGE)
        self._TANGENT = dof
        self._WEIGHT_WIDTHS = (tuple(sorted({1, 3, 6, dof})), "This cost needs a DiagonalCostWeight of the cost's own dimension.")
        # the path table: every distinct link once
        self.path_of, entries = {}, []
        for c in links:
            if c.link_name not in self.path_of:
                path = self.robot.path(c.link_name)
                if len(path) > _lib.THX_KIN_MAX_PATH:
                    raise ValueError(f"{c.name}: the path to {c.link_name} has {len(path)} joints, the fused kernels take "
                                     f"{_lib.THX_KIN_MAX_PATH}")
                ids = [j.id for j in path if j.dof]
                assert ids == sorted(set(ids)) and all(i < dof for i in ids)   # (breadth-first ids grow along a path)
                self.path_of[c.link_name] = (len(entries), len(path))
                entries += path
        self._path_joints = entries

    def _sync_aux(self, deep: bool = False):
        """... and a Scale / Diagonal weight is as wide as 1 or as the cost."""
        table = self._table
        super()._sync_aux(deep)
        if self._table is not table:
            for c in self.costs:
                if weight_var(c).tensor[0].numel() not in (1, c.dim()):
                    self._table = None
                    raise ValueError(f"{c.name}: this cost needs a {c.dim()}-dimensional DiagonalCostWeight.")

    def _term_vars(self, c):
        cost = self.costs[c]
        off, length = self.path_of[cost.link_name] if self.kinds[c] in (_lib.KIN_POSE, _lib.KIN_POSITION) else (0, 0)
        return [self.cols[self.cost_vars[c][0]][0], off, length]

    def _paths(self):
        """the device table of thx_kin_joint entries, values cast to the state's dtype first"""
        dev, dt = self._state.device, self._state.dtype
        if self._paths_dev is None or self._paths_dev[0] != (dev, dt):
            origins, axes = self.robot.tables(dt, "cpu")
            table = np.zeros(max(len(self._path_joints), 1), KIN_JOINT)
            for k, j in enumerate(self._path_joints):
                table[k]["type"], table[k]["theta"] = j.type, j.id if j.dof else -1
                table[k]["origin"] = origins[j.id].double().reshape(12).numpy()
                table[k]["axis"] = (axes[j.id, 3:] if j.type == _lib.KIN_REVOLUTE else axes[j.id, :3]).double().numpy()
            self._paths_dev = ((dev, dt), torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(dev))
        return self._paths_dev[1]

    def _launch_eval(self, state):
        self.K.kin_eval(self._table, len(self.costs), self._paths(), len(self._path_joints), state, self.n, self.robot.dof, self._J,
                        self.j_total, self._e)

    def _launch_error(self, state, err):
        self.K.kin_error(self._table, len(self.costs), self._paths(), len(self._path_joints), state, self.n, self.robot.dof, err)
