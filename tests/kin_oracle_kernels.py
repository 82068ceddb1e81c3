"""TEST-ONLY: the CPU stand-in of tests/oracle_kernels.py extended by the two exports of csrc/kin_kernels.hip, restated in torch
from include/theseus_hip.h (thx_kin_term, thx_kin_joint) -- it decodes the SAME term table and path table the HIP kernels read (the
pointers are host pointers here), so the packer's tables are checked without a GPU.  The kinematics are written with 4 x 4
homogeneous matrices and the kernel's backward walk (Y = (rel_(k+1) ... rel_(n-1))^-1, column = Ad(Y) axis), not with the forward
spatial Jacobians of theseus_amd/kinematics.py; log and Jlog are theseus_amd/se3_torch.py's (checked against the reference's
fixtures by tests/test_kin_host.py on their own)."""
import ctypes

import numpy as np
import torch

from tests.oracle_kernels import OracleKernels
from theseus_amd import _lib, se3_torch
from theseus_amd.kinematics import KIN_JOINT, KIN_TERM

POSE, POSITION, HINGE, PRIOR = 0, 1, 2, 3
FIXED, REVOLUTE, PRISMATIC = 0, 1, 2


def _aux(term, k, B, per, np_dtype):
    """(B, per) host tensor of aux slot k (batch stride 0: broadcast)"""
    stride, item = int(term["aux_bstride"][k]), np.dtype(np_dtype).itemsize
    count = (B - 1) * stride + per
    base = np.frombuffer((ctypes.c_char * (count * item)).from_address(int(term["aux"][k])), dtype=np_dtype)
    return torch.from_numpy(np.lib.stride_tricks.as_strided(base, shape=(B, per), strides=(stride * item, item)).copy())


def _hom(R, t):
    """(B, 3, 3), (B, 3) -> (B, 4, 4)"""
    top = torch.cat([R, t.unsqueeze(2)], dim=2)
    last = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=R.dtype).expand(R.shape[0], 1, 4)
    return torch.cat([top, last], dim=1)


def _skew(a):
    return torch.tensor([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]], dtype=a.dtype)


def _relative(joint, q, dtype):
    """origin * motion(q) as (B, 4, 4); ``q`` (B,) or None"""
    O = torch.from_numpy(np.array(joint["origin"]).reshape(3, 4)).to(dtype)
    a = torch.from_numpy(np.array(joint["axis"])).to(dtype)
    B = 1 if q is None else q.shape[0]
    R, t = O[:, :3].expand(B, 3, 3), O[:, 3].expand(B, 3)
    if q is not None and int(joint["type"]) == REVOLUTE:
        K = _skew(a)
        R = R @ (torch.eye(3, dtype=dtype) + q.sin().view(-1, 1, 1) * K + (1 - q.cos()).view(-1, 1, 1) * (K @ K))
    elif q is not None and int(joint["type"]) == PRISMATIC:
        t = t + (O[:, :3] @ a).view(1, 3) * q.view(-1, 1)
    return _hom(R, t)


def _link(term, joints, x, B, np_dtype, dof):
    """-> (weighted error (B, dim), weighted block (B, dim, dof))"""
    col, p0, pn = (int(v) for v in term["var"][:3])
    dtype = x.dtype
    path = joints[p0:p0 + pn]
    assert pn <= _lib.THX_KIN_MAX_PATH and p0 + pn <= len(joints)
    moving = [int(j["theta"]) for j in path if int(j["type"]) != FIXED]
    assert moving == sorted(set(moving)) and all(0 <= k < dof for k in moving), "path components must grow and lie inside theta"
    rels = [_relative(j, x[:, col + int(j["theta"])] if int(j["type"]) != FIXED else None, dtype) for j in path]
    T = torch.eye(4, dtype=dtype).expand(B, 4, 4)
    for rel in rels:
        T = T @ rel
    pose = int(term["kind"]) == POSE
    if pose:
        target = _aux(term, 0, B, 12, np_dtype).reshape(B, 3, 4)
        w = _aux(term, 1, B, int(term["wdim"]), np_dtype).expand(B, 6)
        err, Jlog = se3_torch.local(target, T[:, :3], jac=True)
        M = Jlog
    else:
        target = _aux(term, 0, B, 3, np_dtype)
        w = _aux(term, 1, B, int(term["wdim"]), np_dtype).expand(B, 3)
        err = T[:, :3, 3] - target
        M = torch.cat([T[:, :3, :3], torch.zeros(B, 3, 3, dtype=dtype)], dim=2)
    J = torch.zeros(B, err.shape[1], dof, dtype=dtype)
    Y = torch.eye(4, dtype=dtype).expand(B, 4, 4)
    for joint, rel in zip(reversed(path), reversed(rels)):
        if int(joint["type"]) != FIXED:
            a = torch.from_numpy(np.array(joint["axis"])).to(dtype)
            Ra = Y[:, :3, :3] @ a
            if int(joint["type"]) == REVOLUTE:
                twist = torch.cat([torch.linalg.cross(Y[:, :3, 3], Ra, dim=1), Ra], dim=1)
            else:
                twist = torch.cat([Ra, torch.zeros_like(Ra)], dim=1)
            J[:, :, int(joint["theta"])] = (M @ twist.unsqueeze(2)).squeeze(2)
        Y = Y @ torch.linalg.inv(rel)
    return err * w, J * w.unsqueeze(2)


def _vector(term, x, B, np_dtype, dof):
    col = int(term["var"][0])
    v = x[:, col:col + dof]
    if int(term["kind"]) == HINGE:
        down, up, thr = (_aux(term, k, B, dof, np_dtype) for k in range(3))
        w = _aux(term, 3, B, int(term["wdim"]), np_dtype).expand(B, dof)
        lo, hi = down + thr, up - thr
        err = torch.where(v > hi, v - hi, torch.where(v < lo, lo - v, torch.zeros_like(v)))
        sign = torch.where(v > hi, torch.ones_like(v), torch.where(v < lo, -torch.ones_like(v), torch.zeros_like(v)))
        return err * w, torch.diag_embed(sign * w)
    target = _aux(term, 0, B, dof, np_dtype)
    w = _aux(term, 1, B, int(term["wdim"]), np_dtype).expand(B, dof)
    return (v - target) * w, torch.diag_embed(w)


class KinOracleKernels(OracleKernels):
    def __init__(self):
        super().__init__()
        self.calls = {"kin_eval": 0, "kin_error": 0}

    @staticmethod
    def _tables(table, n_terms, paths, n_paths):
        terms = table.numpy().view(KIN_TERM)[:n_terms]
        kinds = [int(t["kind"]) for t in terms]
        assert kinds == sorted(kinds) and any(k in (POSE, POSITION) for k in kinds)
        return terms, paths.numpy().view(KIN_JOINT)[:n_paths]

    @staticmethod
    def _term(term, joints, x, B, dof):
        np_dtype = x.numpy().dtype
        if int(term["kind"]) in (POSE, POSITION):
            return _link(term, joints, x, B, np_dtype, dof)
        return _vector(term, x, B, np_dtype, dof)

    def kin_eval(self, table, n_terms, paths, n_paths, x, n, dof, J, j_total, e):
        self.calls["kin_eval"] += 1
        B, xd = x.shape[0], x.detach()
        terms, joints = self._tables(table, n_terms, paths, n_paths)
        for term in terms:
            err, blk = self._term(term, joints, xd, B, dof)
            d, r0, off = err.shape[1], int(term["row0"]), int(term["j_off"])
            e[:, r0:r0 + d] = err
            J[off * B:(off + dof * d) * B] = blk.reshape(-1)

    def kin_error(self, table, n_terms, paths, n_paths, x, n, dof, err):
        self.calls["kin_error"] += 1
        B, xd = x.shape[0], x.detach()
        terms, joints = self._tables(table, n_terms, paths, n_paths)
        acc = torch.zeros(B, dtype=torch.float64)
        for term in terms:
            acc += (self._term(term, joints, xd, B, dof)[0].double() ** 2).sum(1)
        err.copy_((0.5 * acc).to(err.dtype))

    def block_assemble_strided(self, asm, jacobians, errors, H, g, cache):
        self.block_assemble(asm, jacobians, errors, H, g)
