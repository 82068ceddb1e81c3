"""2D motion planning on theseus_amd's own API (``theseus_amd.eb``, as the reference's ``th.eb``): torch restatements of
  SignedDistanceField2D   theseus/embodied/collision/signed_distance_field.py:16-247
  Collision2D             theseus/embodied/collision/collision.py:17-92 (Point2 poses, the identity robot model)
  DoubleIntegrator        theseus/embodied/motionmodel/double_integrator.py:14-91 (Euclidean variables)
  GPCostWeight            :94-176
  GPMotionModel           :179-202
They implement ``error`` / ``jacobians`` / ``weighted_jacobians_error``, so an objective made of them runs through the generic
path (theseus_amd/euclidean.py: PackedEuclidean) with every backward mode; an objective made ONLY of Collision2D, GPMotionModel
and 2-dof Difference priors is evaluated by the fused kernels of csrc/traj_kernels.hip (PackedTrajectory2D below), for which these
classes are the fallback and the differentiable twin.  Collision2D and DoubleIntegrator / GPMotionModel also take SE2 poses (with
Vector(3) velocities): with Nonholonomic, HingeCost and XYDifference below they make the SE2 motion planner's objective, fused by
theseus_amd/planning_se2.py.  Further down: the planar-pushing costs on SE2 and HomographyAlignment, the
dense image-alignment cost of examples/homography_estimation.py, with their own fused families.
"""
from typing import List, Optional, Union

import torch

from . import _lib
from .core import CostFunction, CostWeight, Point2, ScaleCostWeight, Variable, Vector
from .euclidean import PackedEuclidean, _is_euclidean
from .generic import _names
from .term_table import TermKind, TermTable, term_dtype, weight_var


def _as_variable(x, dtype=None, name=None) -> Variable:
    if isinstance(x, Variable):
        return x
    if not isinstance(x, torch.Tensor):
        x = torch.tensor(float(x), dtype=dtype or torch.get_default_dtype())
    return Variable(x, name=name)


class SignedDistanceField2D:
    """A batch of grids ``sdf_data`` (B|1, rows, cols) with ``origin`` (B|1, 2) the position of cell (0, 0) and ``cell_size``
    (B|1, 1); x runs along the columns, y along the rows (signed_distance_field.py:163-188)."""

    def __init__(self, origin: Union[Point2, torch.Tensor], cell_size: Union[float, torch.Tensor, Variable],
                 sdf_data: Optional[Union[torch.Tensor, Variable]] = None, occupancy_map=None,
                 occupancy_threshold: float = 0.75, sdf_boundary_value: float = 0.0):
        if occupancy_map is not None:
            raise NotImplementedError("SignedDistanceField2D(occupancy_map=...) is out of scope on this back end (the reference "
                                      "runs scipy's distance transform on the host, signed_distance_field.py:51-102): pass sdf_data.")
        if sdf_data is None:
            raise ValueError("Either sdf_data or argument occupancy_map should be provided.")
        self.update_data(origin, sdf_data, cell_size)
        self.sdf_boundary_value = sdf_boundary_value

    @staticmethod
    def convert_origin(origin) -> Point2:
        if isinstance(origin, Point2):
            return origin
        if not isinstance(origin, torch.Tensor):
            raise ValueError("Argument origin to SignedDistanceField2D must be either a tensor or a Point2 variable.")
        try:
            return Point2(tensor=origin if origin.ndim == 2 else origin.view(1, -1))
        except ValueError:
            raise ValueError("Argument origin to SignedDistanceField2D must be a batch of 2D tensors.") from None

    @staticmethod
    def convert_cell_size(cell_size) -> Variable:
        if not isinstance(cell_size, Variable):
            if not isinstance(cell_size, torch.Tensor):
                if not isinstance(cell_size, float):
                    raise ValueError("Argument cell_size must be either a Variable, tensor, or float.")
                cell_size = torch.tensor(cell_size)
            return Variable(cell_size.view(-1, 1))
        if not (cell_size.ndim == 1 or (cell_size.ndim == 2 and cell_size.shape[1] == 1)):
            raise ValueError("Argument cell_size must be a batch of 0D or 1D tensors.")
        return cell_size

    @staticmethod
    def convert_sdf_data(sdf_data) -> Variable:
        sdf_data = _as_variable(sdf_data)
        if sdf_data.ndim != 3:
            raise ValueError("Argument sdf_data to SignedDistanceField2D must be a batch of matrices.")
        return sdf_data

    def update_data(self, origin, sdf_data, cell_size):
        self.origin = self.convert_origin(origin)
        self.cell_size = self.convert_cell_size(cell_size)
        self.sdf_data = self.convert_sdf_data(sdf_data)

    def signed_distance(self, points: torch.Tensor):
        """points (B, 2, P) -> distances (B, P), Jacobians (B, P, 2) = [d/dpx, d/dpy] (signed_distance_field.py:163-241)."""
        origin, cell = self.origin.tensor.unsqueeze(-1), self.cell_size.tensor.view(-1, 1)
        sdf = self.sdf_data.tensor
        R, C = sdf.shape[1], sdf.shape[2]
        px, py = points[:, 0], points[:, 1]
        oob = (px < origin[:, 0]) | (px > (origin[:, 0] + (C - 1.0) * cell)) | (py < origin[:, 1]) | (py > (origin[:, 1] + (R - 1.0) * cell))
        cols, rows = (px - origin[:, 0]) / cell, (py - origin[:, 1]) / cell
        lr, lc = torch.floor(rows), torch.floor(cols)
        hr, hc = lr + 1.0, lc + 1.0
        lri, hri = lr.long().clamp(0, R - 1), hr.long().clamp(0, R - 1)
        lci, hci = lc.long().clamp(0, C - 1), hc.long().clamp(0, C - 1)
        B = max(points.shape[0], sdf.shape[0])
        flat = sdf.reshape(sdf.shape[0], -1).expand(B, -1)

        def at(r, c):
            return flat.gather(1, (r * C + c).expand(B, -1))
        sll, shl, slh, shh = at(lri, lci), at(hri, lci), at(lri, hci), at(hri, hci)
        hrd, hcd, lrd, lcd = hr - rows, hc - cols, rows - lr, cols - lc
        dist = hrd * hcd * sll + lrd * hcd * shl + hrd * lcd * slh + lrd * lcd * shh
        jac1 = (hrd * (slh - sll) + lrd * (shh - shl)) / cell
        jac2 = (hcd * (shl - sll) + lcd * (shh - slh)) / cell
        oob = oob.expand_as(dist)
        dist = torch.where(oob, torch.full_like(dist, self.sdf_boundary_value), dist)
        zero = torch.zeros_like(dist)
        return dist, torch.stack([torch.where(oob, zero, jac1), torch.where(oob, zero, jac2)], dim=2)

    def to(self, *args, **kwargs):
        for v in (self.cell_size, self.origin, self.sdf_data):
            v.to(*args, **kwargs)


class Collision2D(CostFunction):
    """error = clamp(cost_eps - d(pose), min=0), Jacobian = -dd/dpose where d <= cost_eps (collision.py:44-73).  An SE2 pose is
    looked up at its translation: the 1 x 2 SDF Jacobian times d xy / d pose = [R, 0] (se2_torch.xy)."""

    def __init__(self, pose: Point2, sdf_origin, sdf_data, sdf_cell_size, cost_eps, cost_weight: CostWeight,
                 name: Optional[str] = None):
        if not isinstance(pose, Point2) and "SE2" not in _names(pose):
            raise ValueError("Collision2D only accepts Point2 or SE2 poses.")
        super().__init__(cost_weight, name)
        self.pose = pose
        self.sdf_origin = SignedDistanceField2D.convert_origin(sdf_origin)
        self.sdf_data = SignedDistanceField2D.convert_sdf_data(sdf_data)
        self.sdf_cell_size = SignedDistanceField2D.convert_cell_size(sdf_cell_size)
        self.cost_eps = _as_variable(cost_eps, dtype=pose.dtype)
        if self.cost_eps.tensor.ndim != 2:
            self.cost_eps._tensor = self.cost_eps.tensor.view(-1, 1)
        if not isinstance(pose, Point2):
            # the SE2 form is new here and strict from the start: one dtype for the pose, the grid and the weight, as Objective.add
            # and the fused family's term table ask anyway (a float32 weight on a float64 pose would be promoted silently by torch)
            for v in self.aux_vars():
                if v.tensor.is_floating_point() and v.dtype != pose.dtype:
                    raise ValueError(f"Collision2D on an SE2 pose ({pose.name}, {pose.dtype}): {v.name} has dtype {v.dtype}; the "
                                     "pose, the signed-distance field, cost_eps and the cost weight must share one dtype.")

    def optim_vars(self):
        return [self.pose]

    def aux_vars(self):
        return [self.sdf_origin, self.sdf_data, self.sdf_cell_size, self.cost_eps] + self.weight.aux_vars()

    def dim(self) -> int:
        return 1

    def _distances(self):
        # (the variables are read at every evaluation: Objective.update may have replaced their tensors)
        sdf = SignedDistanceField2D(self.sdf_origin, self.sdf_cell_size, self.sdf_data)
        if isinstance(self.pose, Point2):
            return sdf.signed_distance(self.pose.tensor.view(-1, 2, 1))
        from . import se2_torch as S
        xy, J_xy = S.xy(self.pose.tensor, jac=True)
        dist, jac = sdf.signed_distance(xy.reshape(-1, 2, 1))
        return dist, jac @ J_xy

    def error(self) -> torch.Tensor:
        return (self.cost_eps.tensor.view(-1, 1) - self._distances()[0]).clamp(min=0)

    def jacobians(self):
        dist, jac = self._distances()
        eps = self.cost_eps.tensor.view(-1, 1)
        jac = torch.where((dist > eps).unsqueeze(2), torch.zeros_like(jac), jac)
        return [-jac], (eps - dist).clamp(min=0)


class GPCostWeight(CostWeight):
    """The (B|1, 2 dof, 2 dof) matrix U = chol(W)^T, W = [[12/dt^3, -6/dt^2], [-6/dt^2, 4/dt]] (x) Qc_inv
    (double_integrator.py:131-152); differentiable in Qc_inv and dt."""

    def __init__(self, Qc_inv: Union[Variable, torch.Tensor], dt: Union[float, Variable, torch.Tensor], name: Optional[str] = None):
        super().__init__(name)
        Qc_inv = _as_variable(Qc_inv)
        dt = _as_variable(dt, dtype=Qc_inv.dtype)
        if dt.tensor.squeeze().ndim > 1:
            raise ValueError("dt must be a 0-D or 1-D tensor.")
        if dt.tensor.ndim != 2:
            dt._tensor = dt.tensor.view(-1, 1)
        if not (dt.tensor > 0).all():
            raise ValueError("dt must be greater than 0.")
        if Qc_inv.ndim not in (2, 3):
            raise ValueError("Qc_inv must be a single matrix or a batch of matrices.")
        if Qc_inv.shape[-2] != Qc_inv.shape[-1]:
            raise ValueError("Qc_inv must contain square matrices.")
        if Qc_inv.ndim == 2:
            Qc_inv._tensor = Qc_inv.tensor.unsqueeze(0)
        try:
            torch.linalg.cholesky(Qc_inv.tensor)
        except RuntimeError:
            raise ValueError("Qc_inv must be positive definite.") from None
        self.Qc_inv, self.dt = Qc_inv, dt

    def aux_vars(self):
        return [self.Qc_inv, self.dt]

    def sqrt_diag(self, dim):
        raise NotImplementedError("GPCostWeight is a full matrix: it weights through weight_jacobians_and_error()")

    def cost_weight_matrix(self) -> torch.Tensor:
        Q, dt = self.Qc_inv.tensor, self.dt.tensor.view(-1, 1, 1)
        q11, q12, q22 = 12.0 * dt.pow(-3.0) * Q, -6.0 * dt.pow(-2.0) * Q, 4.0 * dt.reciprocal() * Q
        W = torch.cat([torch.cat([q11, q12], dim=2), torch.cat([q12, q22], dim=2)], dim=1)
        return torch.linalg.cholesky(W.transpose(-2, -1)).transpose(-2, -1)

    def weight_error(self, error: torch.Tensor) -> torch.Tensor:
        return (self.cost_weight_matrix() @ error.unsqueeze(2)).squeeze(2)

    def weight_jacobians_and_error(self, jacobians: List[torch.Tensor], error: torch.Tensor):
        U = self.cost_weight_matrix()
        return [U @ j for j in jacobians], (U @ error.unsqueeze(2)).squeeze(2)


class DoubleIntegrator(CostFunction):
    """error = [pose1.local(pose2) - dt vel1 ; vel2 - vel1] (double_integrator.py:48-80): Euclidean variables, or SE2 poses with
    Vector(3) velocities -- then ``local`` and its two Jacobians are se2_torch.local's."""

    def __init__(self, pose1: Vector, vel1: Vector, pose2: Vector, vel2: Vector, dt, cost_weight: CostWeight,
                 name: Optional[str] = None):
        super().__init__(cost_weight, name)
        self._se2 = "SE2" in _names(pose1) and "SE2" in _names(pose2)
        for v in (vel1, vel2) if self._se2 else (pose1, vel1, pose2, vel2):
            if not _is_euclidean(v):
                raise ValueError(f"DoubleIntegrator: the variables must be Euclidean (Vector / Point2 / Point3), or the poses SE2 with "
                                 f"Vector velocities, on this back end; got {type(v).__name__} ({v.name}).")
        dof = pose1.dof()
        if not (vel1.dof() == pose2.dof() == vel2.dof() == dof):
            raise ValueError("All variables for a DoubleIntegrator must have the same dimension.")
        self.dt = _as_variable(dt, dtype=pose1.dtype)
        if self.dt.tensor.squeeze().ndim > 1:
            raise ValueError("dt data must be a 0-D or 1-D tensor with numel in {1, batch_size}.")
        if self.dt.tensor.ndim != 2:
            self.dt._tensor = self.dt.tensor.view(-1, 1)
        self.pose1, self.vel1, self.pose2, self.vel2 = pose1, vel1, pose2, vel2

    def optim_vars(self):
        return [self.pose1, self.vel1, self.pose2, self.vel2]

    def aux_vars(self):
        aux = [self.dt]
        return aux + [v for v in self.weight.aux_vars() if v is not self.dt]

    def dim(self) -> int:
        return 2 * self.pose1.dof()

    def _pose_diff(self, jac: bool):
        """pose1.local(pose2) [, its Jacobians w.r.t. pose1 and pose2, None for Euclidean poses: -I and I]"""
        if not self._se2:
            return self.pose1.local(self.pose2), None
        from . import se2_torch as S
        return S.local(self.pose1.tensor, self.pose2.tensor, jac=True) if jac else (S.local(self.pose1.tensor, self.pose2.tensor), None)

    def _error_from(self, diff):
        dt = self.dt.tensor.view(-1, 1)
        a, b = diff - dt * self.vel1.tensor, self.vel2.tensor - self.vel1.tensor
        B = max(a.shape[0], b.shape[0])
        return torch.cat([a.expand(B, -1), b.expand(B, -1)], dim=1)

    def error(self) -> torch.Tensor:
        return self._error_from(self._pose_diff(False)[0])

    def jacobians(self):
        diff, J_local = self._pose_diff(True)
        err = self._error_from(diff)
        B, dof = err.shape[0], self.pose1.dof()
        eye = torch.eye(dof, dtype=err.dtype, device=err.device).expand(B, dof, dof)
        zero = torch.zeros_like(eye)
        dt = self.dt.tensor.view(-1, 1, 1)
        J1, J2 = (-eye, eye) if J_local is None else (j.expand(B, dof, dof) for j in J_local)
        return [torch.cat([J1, zero], dim=1), torch.cat([-dt * eye, -eye], dim=1), torch.cat([J2, zero], dim=1),
                torch.cat([zero, eye], dim=1)], err

    def weighted_error(self) -> torch.Tensor:
        if hasattr(self.weight, "weight_error"):
            return self.weight.weight_error(self.error())
        return super().weighted_error()

    def weighted_jacobians_error(self):
        if hasattr(self.weight, "weight_jacobians_and_error"):
            return self.weight.weight_jacobians_and_error(*self.jacobians())
        return super().weighted_jacobians_error()


class GPMotionModel(DoubleIntegrator):
    def __init__(self, pose1: Vector, vel1: Vector, pose2: Vector, vel2: Vector, dt, cost_weight: GPCostWeight,
                 name: Optional[str] = None):
        if not isinstance(cost_weight, GPCostWeight):
            raise ValueError("GPMotionModel only accepts cost weights of type GPCostWeight. For other weight types, consider "
                             "using DoubleIntegrator instead.")
        super().__init__(pose1, vel1, pose2, vel2, dt, cost_weight, name=name)


# --------------------------------------------------------------------------------------------------------------------------------
# the SE2 motion planner (examples/se2_planning.py: MotionPlanner with pose_type=SE2): torch restatements of
#   Nonholonomic   theseus/embodied/motionmodel/misc.py:97-186
#   HingeCost      theseus/embodied/motionmodel/misc.py:14-94
#   XYDifference   the planner's private _XYDifference (theseus/utils/examples/motion_planning/motion_planner.py:15-54)
# With Collision2D / GPMotionModel on SE2 poses and Difference priors they make the planner's objective, which is evaluated by the
# fused kernels of csrc/trajse2_kernels.hip (theseus_amd/planning_se2.py: PackedTrajectorySE2); these classes are the
# differentiable twin.
# --------------------------------------------------------------------------------------------------------------------------------
class Nonholonomic(CostFunction):
    """The sideways velocity of a car-like robot.  SE2 pose: the velocity is in the body frame, error = vel_y, Jacobians 0 and
    [0, 1, 0].  Vector pose (x, y, theta): the velocity is in the world frame, error = vel_y cos(theta) - vel_x sin(theta)."""

    def __init__(self, pose, vel: Vector, cost_weight: CostWeight, name: Optional[str] = None):
        super().__init__(cost_weight, name)
        if vel.dof() != 3 or pose.dof() != 3:
            raise ValueError("Nonholonomic only accepts 3D velocity or poses (x, y, theta dims). "
                             "Poses can either be SE2 or Vector variables. Velocities only Vector.")
        if not _is_euclidean(vel) or not ("SE2" in _names(pose) or _is_euclidean(pose)):
            raise ValueError("Nonholonomic: poses can either be SE2 or Vector variables. Velocities only Vector.")
        self.pose, self.vel = pose, vel
        self._se2 = "SE2" in _names(pose)

    def optim_vars(self):
        return [self.pose, self.vel]

    def aux_vars(self):
        return self.weight.aux_vars()

    def dim(self) -> int:
        return 1

    def error(self) -> torch.Tensor:
        vel = self.vel.tensor
        if self._se2:
            return vel[:, 1].view(-1, 1)
        th = self.pose.tensor[:, 2]
        return (vel[:, 1] * th.cos() - vel[:, 0] * th.sin()).view(-1, 1)

    def jacobians(self):
        err, vel = self.error(), self.vel.tensor
        zero, one = torch.zeros_like(err[:, 0]), torch.ones_like(err[:, 0])
        if self._se2:
            return [torch.stack([zero, zero, zero], dim=1).unsqueeze(1), torch.stack([zero, one, zero], dim=1).unsqueeze(1)], err
        th = self.pose.tensor[:, 2]
        cos, sin = th.cos(), th.sin()
        J_pose = torch.stack([zero, zero, -(vel[:, 1] * sin + vel[:, 0] * cos) * one], dim=1).unsqueeze(1)
        return [J_pose, torch.stack([-sin * one, cos * one, zero], dim=1).unsqueeze(1)], err


class HingeCost(CostFunction):
    """error_i = down_i + thr_i - v_i where v_i < down_i + thr_i, v_i - (up_i - thr_i) where v_i > up_i - thr_i (this one wins
    where both hold), else 0; the Jacobian is diagonal: -1 / +1 / 0.  The limits may be +-inf."""

    def __init__(self, vector: Vector, down_limit, up_limit, threshold, cost_weight: CostWeight, name: Optional[str] = None):
        super().__init__(cost_weight, name)
        self.vector = vector
        dof = vector.dof()

        def convert(value, what):
            if isinstance(value, float):   # (a number: one value per component, where the vector lives)
                value = torch.full((1, dof), value, dtype=vector.dtype, device=vector.device)
            return _as_variable(value, name=f"{self.name}__{what}")
        self.down_limit, self.up_limit = convert(down_limit, "downlimit"), convert(up_limit, "uplimit")
        self.threshold = convert(threshold, "thres")
        for v in (self.down_limit, self.up_limit, self.threshold):
            if v.ndim != 2 or v.shape[1] != dof:
                raise ValueError(f"Limit and threshold must be 1D variables with dimension equal to `vector.dof()` ({dof}).")
        if not bool((self.down_limit.tensor <= self.up_limit.tensor).all()):
            raise ValueError("All down_limit must be <= than up_limit.")
        if self.threshold.tensor.max() < 0.0:
            raise ValueError("Threshold values must be positive numbers.")

    def optim_vars(self):
        return [self.vector]

    def aux_vars(self):
        return [self.down_limit, self.up_limit, self.threshold] + self.weight.aux_vars()

    def dim(self) -> int:
        return self.vector.dof()

    def _evaluate(self):
        v, thr = self.vector.tensor, self.threshold.tensor
        down, up = self.down_limit.tensor + thr, self.up_limit.tensor - thr
        below, above = v < down, v > up
        err = torch.where(below, down - v, torch.zeros_like(v))
        return torch.where(above, v - up, err), below, above

    def error(self) -> torch.Tensor:
        return self._evaluate()[0]

    def jacobians(self):
        err, below, above = self._evaluate()
        zero, one = torch.zeros_like(err), torch.ones_like(err)
        return [torch.diag_embed(torch.where(above, one, torch.where(below, -one, zero)))], err


class XYDifference(CostFunction):
    """error = xy(var) - target for an SE2 ``var`` and a Point2 ``target``; Jacobian = d xy / d var = [R, 0]."""

    def __init__(self, var, target: Point2, cost_weight: CostWeight, name: Optional[str] = None):
        super().__init__(cost_weight, name)
        if "SE2" not in _names(var) or not isinstance(target, Point2):
            raise ValueError("XYDifference expects var of type SE2 and target of type Point2.")
        self.var, self.target = var, target

    def optim_vars(self):
        return [self.var]

    def aux_vars(self):
        return [self.target] + self.weight.aux_vars()

    def dim(self) -> int:
        return 2

    def error(self) -> torch.Tensor:
        from . import se2_torch as S
        return S.xy(self.var.tensor) - self.target.tensor

    def jacobians(self):
        from . import se2_torch as S
        xy, J = S.xy(self.var.tensor, jac=True)
        err = xy - self.target.tensor
        return [J.expand(err.shape[0], 2, 3)], err


# --------------------------------------------------------------------------------------------------------------------------------
# planar pushing on SE2 (examples/tactile_pose_estimation.py): torch restatements on theseus_amd/se2_torch.py of
#   QuasiStaticPushingPlanar     theseus/embodied/motionmodel/quasi_static_pushing_planar.py
#   MovingFrameBetween           theseus/embodied/measurements/moving_frame_between.py (SE2 only)
#   EffectorObjectContactPlanar  theseus/embodied/collision/eff_obj_contact.py
# They run on CPU and on the device and autograd goes through them; an objective made only of them and of Difference priors on
# SE2 is evaluated by the fused kernels of csrc/push_kernels.hip (theseus_amd/pushing.py: PackedPlanarPushing), for which these
# classes are the differentiable twin.
# --------------------------------------------------------------------------------------------------------------------------------
def _require_se2(owner, *variables):
    for v in variables:
        if "SE2" not in _names(v):
            raise ValueError(f"{owner}: the poses must be SE2 on this back end; got {type(v).__name__} ({v.name}).")


class QuasiStaticPushingPlanar(CostFunction):
    """error = D V - Vp of the velocity-only quasi-static model (Zhou et al. 2017, Eqs. 3-7): V the object's velocity in its own
    frame [R2^T (t_obj2 - t_obj1); angle(obj1^-1 obj2)], Vp the contact point's [R2^T (t_eff2 - t_eff1); 0], D built from the
    contact point (eff2's xy) in obj2's frame and ``c_square``."""

    def __init__(self, obj1, obj2, eff1, eff2, c_square, cost_weight: CostWeight, name: Optional[str] = None):
        super().__init__(cost_weight, name)
        _require_se2("QuasiStaticPushingPlanar", obj1, obj2, eff1, eff2)
        self.obj1, self.obj2, self.eff1, self.eff2 = obj1, obj2, eff1, eff2
        if not isinstance(c_square, (Variable, torch.Tensor)):   # (a number: on the poses' device)
            c_square = torch.tensor(float(c_square), dtype=obj1.dtype, device=obj1.device)
        c_square = _as_variable(c_square, dtype=obj1.dtype, name=f"csquare_{self.name}")
        if c_square.tensor.squeeze().ndim > 1:
            raise ValueError("c_square must be a 0-D or 1-D tensor.")
        if c_square.tensor.ndim != 2:   # (a new Variable on a (B, 1) view: the caller's object is left as it is)
            c_square = Variable(c_square.tensor.view(-1, 1), name=c_square.name)
        self.c_square = c_square

    def optim_vars(self):
        return [self.obj1, self.obj2, self.eff1, self.eff2]

    def aux_vars(self):
        return [self.c_square] + self.weight.aux_vars()

    def dim(self) -> int:
        return 3

    def _evaluate(self, jac: bool):
        from . import se2_torch as S
        o1, o2, e1, e2 = torch.broadcast_tensors(self.obj1.tensor, self.obj2.tensor, self.eff1.tensor, self.eff2.tensor)
        R2 = o2[:, 2:]
        cp2, J_cp2_e2 = S.xy(e2, jac=True)
        cpo, (J_cpo_o2, J_cpo_cp2) = S.transform_to(o2, cp2, jac=True)
        px, py = cpo[:, 0], cpo[:, 1]
        one, zero = torch.ones_like(px), torch.zeros_like(px)
        D = S._mat([[one, zero, -py], [zero, one, px], [-py, px, -self.c_square.tensor.view(-1).expand_as(px)]])
        o1xy, J_o1xy = S.xy(o1, jac=True)
        o2xy, J_o2xy = S.xy(o2, jac=True)
        voo, (J_voo_ang, J_voo_vw) = S.unrotate(R2, o2xy - o1xy, jac=True)
        od, (J_od_o1, J_od_o2) = S.between(o1, o2, jac=True)
        omega, J_om = S.theta(od, jac=True)
        V = torch.cat([voo, omega], dim=1)
        e1xy, J_e1xy = S.xy(e1, jac=True)
        vco, (J_vco_ang, J_vco_vcw) = S.unrotate(R2, cp2 - e1xy, jac=True)
        Vp = torch.cat([vco, zero.unsqueeze(1)], dim=1)
        err = (D @ V.unsqueeze(2)).squeeze(2) - Vp
        if not jac:
            return None, err
        _, J_ang_o2 = S.theta(o2, jac=True)

        def dD_times_V(J_cpo_var):   # (B, 2, 3) -> (B, 3, 3): column d = (dD / d var_d) V
            dpx, dpy = J_cpo_var[:, 0], J_cpo_var[:, 1]
            return torch.stack([-dpy * V[:, 2:3], dpx * V[:, 2:3], -dpy * V[:, 0:1] + dpx * V[:, 1:2]], dim=1)

        def pad(J2):                 # (B, 2, 3) -> (B, 3, 3) with a zero third row
            return torch.cat([J2, torch.zeros_like(J2[:, :1])], dim=1)
        dV_o1 = torch.cat([J_voo_vw @ -J_o1xy, J_om @ J_od_o1], dim=1)
        dV_o2 = torch.cat([J_voo_ang @ J_ang_o2 + J_voo_vw @ J_o2xy, J_om @ J_od_o2], dim=1)
        J_cpo_e2 = J_cpo_cp2 @ J_cp2_e2
        J_o1 = D @ dV_o1
        J_o2 = dD_times_V(J_cpo_o2) + D @ dV_o2 - pad(J_vco_ang @ J_ang_o2)
        J_e1 = -pad(J_vco_vcw @ -J_e1xy)
        J_e2 = dD_times_V(J_cpo_e2) - pad(J_vco_vcw @ J_cp2_e2)
        return [J_o1, J_o2, J_e1, J_e2], err

    def error(self) -> torch.Tensor:
        return self._evaluate(False)[1]

    def jacobians(self):
        return self._evaluate(True)


class MovingFrameBetween(CostFunction):
    """error = measurement.local(between(between(frame1, pose1), between(frame2, pose2))) on SE2.  NB the optimisation variables
    are ordered frame1, frame2, pose1, pose2, and the Jacobians are the reference's: the chain of the three ``between``s
    (moving_frame_between.py:46-64)."""

    def __init__(self, frame1, frame2, pose1, pose2, measurement, cost_weight: CostWeight, name: Optional[str] = None):
        if len({type(x).__name__ for x in (frame1, frame2, pose1, pose2, measurement)}) > 1:
            raise ValueError("Inconsistent types between input variables.")
        super().__init__(cost_weight, name)
        _require_se2("MovingFrameBetween", frame1, frame2, pose1, pose2, measurement)
        self.frame1, self.frame2, self.pose1, self.pose2, self.measurement = frame1, frame2, pose1, pose2, measurement

    def optim_vars(self):
        return [self.frame1, self.frame2, self.pose1, self.pose2]

    def aux_vars(self):
        return [self.measurement] + self.weight.aux_vars()

    def dim(self) -> int:
        return 3

    def error(self) -> torch.Tensor:
        from . import se2_torch as S
        p1f = S.between(self.frame1.tensor, self.pose1.tensor)
        p2f = S.between(self.frame2.tensor, self.pose2.tensor)
        return S.local(self.measurement.tensor, S.between(p1f, p2f))

    def jacobians(self):
        from . import se2_torch as S
        p1f, (JB1_f1, JB1_p1) = S.between(self.frame1.tensor, self.pose1.tensor, jac=True)
        p2f, (JB2_f2, JB2_p2) = S.between(self.frame2.tensor, self.pose2.tensor, jac=True)
        diff, (JO_1, JO_2) = S.between(p1f, p2f, jac=True)
        err = S.local(self.measurement.tensor, diff)
        return [JO_1 @ JB1_f1, JO_2 @ JB2_f2, JO_1 @ JB1_p1, JO_2 @ JB2_p2], err


class EffectorObjectContactPlanar(CostFunction):
    """error = |d - eff_radius|, d the signed distance of the effector's xy in the object's frame; both Jacobians are negated
    where d < eff_radius (eff_obj_contact.py)."""

    def __init__(self, obj, eff, sdf_origin, sdf_data, sdf_cell_size, eff_radius, cost_weight: CostWeight,
                 name: Optional[str] = None, use_huber_loss: bool = False):
        super().__init__(cost_weight, name)
        _require_se2("EffectorObjectContactPlanar", obj, eff)
        self.obj, self.eff = obj, eff
        self.sdf_origin = SignedDistanceField2D.convert_origin(sdf_origin)
        self.sdf_data = SignedDistanceField2D.convert_sdf_data(sdf_data)
        self.sdf_cell_size = SignedDistanceField2D.convert_cell_size(sdf_cell_size)
        if not isinstance(eff_radius, (Variable, torch.Tensor)):   # (a number: on the poses' device)
            eff_radius = torch.tensor(float(eff_radius), dtype=obj.dtype, device=obj.device)
        self.eff_radius = _as_variable(eff_radius, dtype=obj.dtype)
        if self.eff_radius.tensor.squeeze().ndim > 1:
            raise ValueError("eff_radius must be a 0-D or 1-D tensor.")
        if self.eff_radius.tensor.ndim != 2:   # (a new Variable on a (B, 1) view: the caller's object is left as it is)
            self.eff_radius = Variable(self.eff_radius.tensor.view(-1, 1), name=self.eff_radius.name)
        self.sdf = SignedDistanceField2D(self.sdf_origin, self.sdf_cell_size, self.sdf_data)
        if use_huber_loss:
            raise NotImplementedError("Jacobians for huber loss are not yet implemented.")

    _AUX = ("sdf_origin", "sdf_data", "sdf_cell_size", "eff_radius")

    def optim_vars(self):
        return [self.obj, self.eff]

    def aux_vars(self):
        return [getattr(self, k) for k in self._AUX] + self.weight.aux_vars()

    def set_aux_var_at(self, index: int, variable: Variable):
        """Replace the ``index``-th auxiliary variable (sdf_origin, sdf_data, sdf_cell_size, eff_radius); the SDF container
        follows."""
        setattr(self, self._AUX[index], variable)
        self.sdf.update_data(self.sdf_origin, self.sdf_data, self.sdf_cell_size)

    def dim(self) -> int:
        return 1

    def _distances(self):
        from . import se2_torch as S
        cp, J_xy = S.xy(self.eff.tensor, jac=True)
        eo, (J_obj, J_pnt) = S.transform_to(self.obj.tensor, cp, jac=True)
        dist, J_dist = self.sdf.signed_distance(eo.view(-1, 2, 1))
        return dist, (J_dist @ J_obj, J_dist @ (J_pnt @ J_xy))

    def error(self) -> torch.Tensor:
        return (self._distances()[0] - self.eff_radius.tensor).abs()

    def jacobians(self):
        dist, (J_obj, J_eff) = self._distances()
        r = self.eff_radius.tensor
        sign = torch.where(dist < r, -torch.ones_like(dist), torch.ones_like(dist)).unsqueeze(2)
        return [J_obj * sign, J_eff * sign], (dist - r).abs()


# --------------------------------------------------------------------------------------------------------------------------------
# homography image alignment, dense Lucas-Kanade (examples/homography_estimation.py): a torch restatement of the example's
# homography_error_fn (:140-168) over theseus/third_party/utils.py grid_sample, with an analytic Jacobian.  An objective made only
# of it and of Difference priors on the 8-dof variable is evaluated by the fused kernels of csrc/homog_kernels.hip
# (theseus_amd/homography.py: PackedHomography), for which this class is the differentiable twin.
# --------------------------------------------------------------------------------------------------------------------------------
class HomographyAlignment(CostFunction):
    """error = sum m (s - feat_dst)^2 / sum m over all C Hh Ww elements: s is ``feat_src`` sampled bilinearly where the homography
    H = [h0 .. h7, 1] (row major, ``H8``'s tensor) sends each pixel of ``feat_dst``, m the mask "the four bilinear weights add up
    to more than 0.9".  Both feature maps are (B|1, C, Hh, Ww).  In the reference's operation order:
      pixel (i, j) -> x = 2 j / (Ww - 1) - 1, y = 2 i / (Hh - 1) - 1;  G = adj(H) / det(H) by the cofactor formula;
      q = G (x, y, 1), u = q_x / q_z, v = q_y / q_z;  ix = ((u + 1) / 2) (Ww - 1), iy = ((v + 1) / 2) (Hh - 1);
      the weights come from the UNCLAMPED corners floor(ix), floor(ix) + 1, ..., the four corner indices are clamped to the image.
    Two deliberate differences from the example: the inverse is the explicit cofactor formula (torch.inverse's LU rounding cannot
    be reproduced in a kernel, and a different last bit moves floor()), and u, v are plain divisions -- kornia's
    convert_points_from_homogeneous guards that division with an eps of 1e-8, a variant that is not reproduced here.
    ``jacobians()`` is the analytic 1 x 8 block with floor() and the mask held constant, written in torch operations that stay
    differentiable w.r.t. both feature maps.  For non-finite source coordinates (q_z = 0) the result is unspecified."""

    def __init__(self, H8: Vector, feat_src, feat_dst, cost_weight: Optional[CostWeight] = None, name: Optional[str] = None):
        if cost_weight is None:   # (scale 1, where H8 lives)
            cost_weight = ScaleCostWeight(torch.ones(1, 1, dtype=H8.dtype, device=H8.device))
        super().__init__(cost_weight, name)
        if not _is_euclidean(H8) or H8.dof() != 8:
            raise ValueError(f"HomographyAlignment ({self.name}): H8 must be a Vector of dof 8.")
        w = _names(self.weight)
        if not ("ScaleCostWeight" in w or "DiagonalCostWeight" in w):
            raise ValueError(f"HomographyAlignment ({self.name}): the weight must be a ScaleCostWeight or a DiagonalCostWeight of "
                             "width 1.")
        self.H8, self.feat_src, self.feat_dst = H8, _as_variable(feat_src), _as_variable(feat_dst)
        self.check_shapes()

    def check_shapes(self):
        """the feature maps are 4-D, of one shape (up to the batch) and at least 2 x 2; the weight has width 1"""
        s, d = self.feat_src.tensor, self.feat_dst.tensor
        if s.ndim != 4 or d.ndim != 4 or s.shape[1:] != d.shape[1:] or s.shape[2] < 2 or s.shape[3] < 2:
            raise ValueError(f"{self.name}: feat_src {tuple(s.shape)} and feat_dst {tuple(d.shape)} must be (B|1, C, Hh, Ww) feature "
                             "maps of the same C, Hh, Ww with Hh, Ww >= 2.")
        if "DiagonalCostWeight" in _names(self.weight) and self.weight.diagonal.tensor.shape[1] != 1:
            raise ValueError(f"{self.name}: this cost needs a 1-dimensional DiagonalCostWeight.")

    def optim_vars(self):
        return [self.H8]

    def aux_vars(self):
        return [self.feat_src, self.feat_dst] + self.weight.aux_vars()

    def dim(self) -> int:
        return 1

    @staticmethod
    def _inverse(h: torch.Tensor):
        """(B, 8) -> the nine entries of adj(H) / det(H), each (B, 1)"""
        a, b, c, d, e, f, g, k = (h[:, n:n + 1] for n in range(8))
        i = torch.ones_like(a)
        A = [e * i - f * k, c * k - b * i, b * f - c * e,
             f * g - d * i, a * i - c * g, c * d - a * f,
             d * k - e * g, b * g - a * k, a * e - b * d]
        det = (a * A[0] + b * A[3]) + c * A[6]
        return [x / det for x in A]

    def source_points(self):
        """-> (ix, iy), each (B, Hh Ww): where every destination pixel lands in feat_src, in pixels (not clamped)"""
        return self._geometry()[:2]

    def _geometry(self):
        h = self.H8.tensor
        Hh, Ww = self.feat_src.tensor.shape[2:]
        G = self._inverse(h)
        jj = torch.arange(Ww, dtype=h.dtype, device=h.device)
        ii = torch.arange(Hh, dtype=h.dtype, device=h.device)
        x = ((2 * jj) / (Ww - 1) - 1).repeat(Hh).unsqueeze(0)                 # (1, P), pixel = i Ww + j
        y = ((2 * ii) / (Hh - 1) - 1).repeat_interleave(Ww).unsqueeze(0)
        q = [(G[3 * r] * x + G[3 * r + 1] * y) + G[3 * r + 2] for r in range(3)]
        u, v = q[0] / q[2], q[1] / q[2]
        ix, iy = ((u + 1) / 2) * (Ww - 1), ((v + 1) / 2) * (Hh - 1)
        return ix, iy, G, q, u, v

    def _evaluate(self, jac: bool):
        src, dst = self.feat_src.tensor, self.feat_dst.tensor
        C, Hh, Ww = src.shape[1:]
        P = Hh * Ww
        ix, iy, G, q, u, v = self._geometry()
        B = max(ix.shape[0], src.shape[0], dst.shape[0])
        with torch.no_grad():
            x0, y0 = torch.floor(ix), torch.floor(iy)
            x1, y1 = x0 + 1, y0 + 1

            def index(t, hi):   # (clamped before the conversion, NaN -> 0: what the kernel's homog_idx does)
                return torch.where(t > 0, t, torch.zeros_like(t)).clamp(max=hi).long()
            xi0, xi1, yi0, yi1 = index(x0, Ww - 1), index(x1, Ww - 1), index(y0, Hh - 1), index(y1, Hh - 1)
        wx1, wx0, wy1, wy0 = x1 - ix, ix - x0, y1 - iy, iy - y0
        nw, ne, sw, se = wx1 * wy1, wx0 * wy1, wx1 * wy0, wx0 * wy0
        with torch.no_grad():
            m = ((((nw + ne) + sw) + se) > 0.9).to(ix.dtype).expand(B, P)
        flat = src.reshape(src.shape[0], C, P).expand(B, C, P)

        def at(r, c):
            return flat.gather(2, (r * Ww + c).expand(B, P).unsqueeze(1).expand(B, C, P))
        vnw, vne, vsw, vse = at(yi0, xi0), at(yi0, xi1), at(yi1, xi0), at(yi1, xi1)
        nw_, ne_, sw_, se_ = (t.unsqueeze(1) for t in (nw, ne, sw, se))
        s = ((vnw * nw_ + vne * ne_) + vsw * sw_) + vse * se_
        d = s - dst.reshape(dst.shape[0], C, P)
        count = m.sum(dim=1, keepdim=True) * C   # (the mask has the feature maps' shape: every channel counts)
        err = ((d * d).sum(dim=1) * m).sum(dim=1, keepdim=True) / count
        if not jac:
            return None, err
        dsx = (vne - vnw) * wy1.unsqueeze(1) + (vse - vsw) * wy0.unsqueeze(1)
        dsy = (vsw - vnw) * wx1.unsqueeze(1) + (vse - vne) * wx0.unsqueeze(1)
        gu = ((d * dsx).sum(dim=1) * m) * ((Ww - 1) / 2)
        gv = ((d * dsy).sum(dim=1) * m) * ((Hh - 1) / 2)
        # d s / d h_(3k+l) = -(G^T r)_k q_l with r = d s / d q, from d q / d H_kl = -G[:, k] q_l
        r = [gu / q[2], gv / q[2], -(gu * u + gv * v) / q[2]]
        cols = []
        for k in range(3):
            tk = (G[k] * r[0] + G[3 + k] * r[1]) + G[6 + k] * r[2]
            cols += [-(2 * (tk * q[l]).sum(dim=1, keepdim=True) / count) for l in range(3) if 3 * k + l < 8]
        return [torch.cat(cols, dim=1).unsqueeze(1)], err

    def error(self) -> torch.Tensor:
        return self._evaluate(False)[1]

    def jacobians(self):
        return self._evaluate(True)


# --------------------------------------------------------------------------------------------------------------------------------
# the packed family: csrc/traj_kernels.hip
# --------------------------------------------------------------------------------------------------------------------------------
TRAJ2_TERM = term_dtype("col")


def _traj2_kind(c):
    """THX_TRAJ2_* of a cost function the fused kernels cover, else None."""
    names, w = _names(c), _names(c.weight)
    if "Collision2D" in names and "ScaleCostWeight" in w and "Point2" in _names(c.pose):
        return _lib.TRAJ2_COLLISION
    if "GPMotionModel" in names and "GPCostWeight" in w and c.pose1.dof() == 2:
        return _lib.TRAJ2_GP
    if "Difference" in names and ("ScaleCostWeight" in w or "DiagonalCostWeight" in w) and _is_euclidean(c.var) and c.var.dof() == 2:
        return _lib.TRAJ2_PRIOR
    return None


class PackedTrajectory2D(TermTable, PackedEuclidean):
    """PackedEuclidean whose NON-differentiated evaluation is fused (theseus_amd/term_table.py): ``assemble(graph=False)`` =
    thx_traj2_eval into persistent block buffers + thx_block_assemble on them, ``error_metric`` = thx_traj2_error.  Everything
    differentiated (``assemble(graph=True)``, ``unrolled_step``) is the parent's."""

    _TERM, _TANGENT = TRAJ2_TERM, 2
    _KINDS = {
        _lib.TRAJ2_COLLISION: TermKind(lambda c: [(c.sdf_data, None), (c.sdf_origin, 2), (c.sdf_cell_size, 1), (c.cost_eps, 1),
                                                  (c.weight.scale, 1)], grid=0),
        _lib.TRAJ2_GP: TermKind(lambda c: [(c.dt, 1), (c.weight.dt, 1), (c.weight.Qc_inv, 4)]),
        _lib.TRAJ2_PRIOR: TermKind(lambda c: [(c.target, 2), (weight_var(c), None)], weight=1),
    }
    _WEIGHT_WIDTHS = ((1, 2), "This cost needs a 2-dimensional DiagonalCostWeight.")

    def __init__(self, objective, kernels=None, order=None):
        from .kernels import default_kernels
        from .packed import UnsupportedObjective
        K = kernels or default_kernels()
        if not hasattr(K, "traj2_eval"):
            raise UnsupportedObjective("these kernels have no fused trajectory evaluation")
        self.kinds = [_traj2_kind(c) for c in objective.cost_functions.values()]
        if not self.kinds or any(k is None for k in self.kinds):
            raise UnsupportedObjective("HIP backend, fused 2D motion planning: every cost must be a Collision2D on a Point2 with a "
                                       "ScaleCostWeight, a GPMotionModel with dof 2 or a Difference on a 2-dof Euclidean variable "
                                       "with a Scale / DiagonalCostWeight.")
        super().__init__(objective, K, order)

    def _term_vars(self, c):
        return [self.cols[k][0] for k in self.cost_vars[c]]   # (state columns)

    def _launch_eval(self, state):
        self.K.traj2_eval(self._table, len(self.costs), state, self.n, self._J, self.j_total, self._e)

    def _launch_error(self, state, err):
        self.K.traj2_error(self._table, len(self.costs), state, self.n, err)


# robot kinematics and the inverse-kinematics cost family live in theseus_amd/kinematics.py; theseus_amd.eb exports them
from .kinematics import (LinkPoseCost, LinkPositionCost, PackedKinematics, Robot, UrdfRobotModel)  # noqa: E402,F401
