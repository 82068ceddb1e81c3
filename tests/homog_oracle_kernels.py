"""TEST-ONLY: the CPU stand-in of tests/oracle_kernels.py extended by the two exports of csrc/homog_kernels.hip, restated in torch
from include/theseus_hip.h (thx_homog_term) -- it decodes the SAME term table the HIP kernels read (the pointers are host pointers
here), so the packer's table is checked without a GPU.  Written from the formulas of the header and of
theseus/third_party/utils.py grid_sample with the chain rule through q = G p spelled out per parameter; it shares no code with
theseus_amd/embodied.py's torch class."""
import ctypes

import numpy as np
import torch

from tests.oracle_kernels import OracleKernels
from theseus_amd import _lib
from theseus_amd.homography import HOMOG_TERM

ALIGN, PRIOR = 0, 1


def _aux(term, k, B, per, np_dtype):
    """(B, per) host tensor of aux slot k (batch stride 0: broadcast)"""
    stride, item = int(term["aux_bstride"][k]), np.dtype(np_dtype).itemsize
    count = (B - 1) * stride + per
    base = np.frombuffer((ctypes.c_char * (count * item)).from_address(int(term["aux"][k])), dtype=np_dtype)
    return torch.from_numpy(np.lib.stride_tricks.as_strided(base, shape=(B, per), strides=(stride * item, item)).copy())


def _align(term, x, B, np_dtype):
    """-> (weighted error (B, 1), weighted block (B, 1, 8)); G from the cyclic cofactor formula, the sums in fp64"""
    Hh, Ww, C, col = int(term["rows"]), int(term["cols"]), int(term["pad"]), int(term["col"][0])
    P = Hh * Ww
    src = _aux(term, 0, B, C * P, np_dtype).reshape(B, C, P)
    dst = _aux(term, 1, B, C * P, np_dtype).reshape(B, C, P)
    w = _aux(term, 2, B, 1, np_dtype)
    Hm = torch.cat([x[:, col:col + 8], torch.ones(B, 1, dtype=x.dtype)], dim=1).reshape(B, 3, 3)
    cof = torch.empty_like(Hm)
    for r in range(3):
        for c in range(3):
            r1, r2, c1, c2 = (r + 1) % 3, (r + 2) % 3, (c + 1) % 3, (c + 2) % 3
            cof[:, c, r] = Hm[:, r1, c1] * Hm[:, r2, c2] - Hm[:, r1, c2] * Hm[:, r2, c1]   # adj = cof^T
    det = (Hm[:, 0, 0] * cof[:, 0, 0] + Hm[:, 0, 1] * cof[:, 1, 0]) + Hm[:, 0, 2] * cof[:, 2, 0]
    G = cof / det.view(B, 1, 1)
    jj, ii = torch.arange(Ww, dtype=x.dtype), torch.arange(Hh, dtype=x.dtype)
    p = torch.stack([(2 * jj / (Ww - 1) - 1).repeat(Hh), (2 * ii / (Hh - 1) - 1).repeat_interleave(Ww), torch.ones(P, dtype=x.dtype)])
    q = [(G[:, r, 0:1] * p[0] + G[:, r, 1:2] * p[1]) + G[:, r, 2:3] for r in range(3)]
    u, v = q[0] / q[2], q[1] / q[2]
    ix, iy = ((u + 1) / 2) * (Ww - 1), ((v + 1) / 2) * (Hh - 1)
    x0, y0 = ix.floor(), iy.floor()
    fx, fy = ix - x0, iy - y0
    gx, gy = (x0 + 1) - ix, (y0 + 1) - iy
    wts = [gx * gy, fx * gy, gx * fy, fx * fy]
    mask = ((((wts[0] + wts[1]) + wts[2]) + wts[3]) > 0.9).to(x.dtype)
    xs = [x0.clamp(0, Ww - 1).long(), (x0 + 1).clamp(0, Ww - 1).long()]
    ys = [y0.clamp(0, Hh - 1).long(), (y0 + 1).clamp(0, Hh - 1).long()]
    vals = [src.gather(2, (ys[a] * Ww + xs[b]).unsqueeze(1).expand(B, C, P)) for a in (0, 1) for b in (0, 1)]
    s = ((vals[0] * wts[0].unsqueeze(1) + vals[1] * wts[1].unsqueeze(1)) + vals[2] * wts[2].unsqueeze(1)) + vals[3] * wts[3].unsqueeze(1)
    d = (s - dst).double()
    m = mask.double().unsqueeze(1)
    count = C * mask.double().sum(1, keepdim=True)
    err = (m * d * d).sum((1, 2)).unsqueeze(1) / count
    ds_dix = ((vals[1] - vals[0]) * gy.unsqueeze(1) + (vals[3] - vals[2]) * fy.unsqueeze(1)).double()
    ds_diy = ((vals[2] - vals[0]) * gx.unsqueeze(1) + (vals[3] - vals[1]) * fx.unsqueeze(1)).double()
    # per pixel: de/d(ix, iy) summed over the channels, then through (u, v) = (q_x, q_y) / q_z and d q / d H_kl = -G[:, k] q_l
    a = (m * d * ds_dix).sum(1) * ((Ww - 1) / 2)
    b = (m * d * ds_diy).sum(1) * ((Hh - 1) / 2)
    qd, Gd = [t.double() for t in q], G.double()
    de_dq = torch.stack([a / qd[2], b / qd[2], -(a * u.double() + b * v.double()) / qd[2]], dim=1)   # (B, 3, P)
    J = torch.zeros(B, 9, dtype=torch.float64)
    for k in range(3):
        for l in range(3):   # noqa: E741
            dq = -Gd[:, :, k].unsqueeze(2) * qd[l].unsqueeze(1)   # (B, 3, P)
            J[:, 3 * k + l] = 2 * (de_dq * dq).sum((1, 2)) / count[:, 0]
    wd = w.double()
    return (err * wd).to(x.dtype), (J[:, :8] * wd).unsqueeze(1).to(x.dtype)


def _prior(term, x, B, np_dtype):
    col = int(term["col"][0])
    target = _aux(term, 0, B, 8, np_dtype)
    w = _aux(term, 1, B, int(term["wdim"]), np_dtype).expand(B, 8)
    return (x[:, col:col + 8] - target) * w, torch.diag_embed(w)


class HomogOracleKernels(OracleKernels):
    def __init__(self):
        super().__init__()
        self.calls = {"homog_eval": 0, "homog_error": 0}

    @staticmethod
    def _terms(table, n_terms, n_align, scratch, chunks, B):
        terms = table.numpy().view(HOMOG_TERM)[:n_terms]
        kinds = [int(t["kind"]) for t in terms]
        assert kinds == sorted(kinds) and kinds.count(ALIGN) == n_align >= 1
        need = max(-(-(int(t["rows"]) * int(t["cols"])) // _lib.THX_HOMOG_CHUNK) for t in terms[:n_align])
        assert chunks >= need and scratch.dtype == torch.float64 and scratch.numel() >= n_align * B * chunks * _lib.THX_HOMOG_SUMS
        return terms

    @staticmethod
    def _term(term, x, B):
        np_dtype = x.numpy().dtype
        return (_align if int(term["kind"]) == ALIGN else _prior)(term, x, B, np_dtype)

    def homog_eval(self, table, n_terms, n_align, x, n, scratch, chunks, J, j_total, e):
        self.calls["homog_eval"] += 1
        B, xd = x.shape[0], x.detach()
        for term in self._terms(table, n_terms, n_align, scratch, chunks, B):
            err, blk = self._term(term, xd, B)
            d, r0, off = err.shape[1], int(term["row0"]), int(term["j_off"])
            e[:, r0:r0 + d] = err
            J[off * B:(off + 8 * d) * B] = blk.reshape(-1)

    def homog_error(self, table, n_terms, n_align, x, n, scratch, chunks, err):
        self.calls["homog_error"] += 1
        B, xd = x.shape[0], x.detach()
        acc = torch.zeros(B, dtype=torch.float64)
        for term in self._terms(table, n_terms, n_align, scratch, chunks, B):
            acc += (self._term(term, xd, B)[0].double() ** 2).sum(1)
        err.copy_((0.5 * acc).to(err.dtype))

    def block_assemble_strided(self, asm, jacobians, errors, H, g, cache):
        self.block_assemble(asm, jacobians, errors, H, g)
