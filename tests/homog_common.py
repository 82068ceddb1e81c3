"""The homography-alignment objective of the homog fixtures (tests/golden/homog_f64_shared.npz, homog_f64_batched.npz, written by
tools/gen_homog_golden.py from the REAL reference), built on either API: ``th`` is ``theseus_amd`` in the tests and ``theseus`` in
the generator (which passes its own ``align``: an AutoDiffCostFunction on the reference's grid_sample).  B = 3 problems, one
Vector(8) ``H8``, feature maps (B|1, 2, 6, 7); costs in objective order: the alignment cost (ScaleCostWeight) and a Difference prior
on H8 (shared: ScaleCostWeight, batched: DiagonalCostWeight of width 8).

Also here: homographies given by where they send the destination pixels (``h8_from_source_map``), the smooth feature maps and the
problems of the GPU tests, and the magnitudes the GPU tests' bound is made of."""
import numpy as np
import torch

FIXTURES = ("homog_f64_shared", "homog_f64_batched")
LM_KW = dict(max_iterations=5, step_size=1.0, abs_err_tolerance=0.0, rel_err_tolerance=0.0)
LM_DAMPING = 5.0
LEAVES = ("feat_src", "feat_dst")
MARGIN = 1e-3   # pixels: no source coordinate of an fp32 comparison may lie this close to an integer


def build(th, f, device="cpu", dtype=torch.float64, grad=False, align=None):
    """-> (objective, {leaf name: tensor}, [cost names in objective order]); ``grad``: the LEAVES require grad."""
    def t(key):
        return torch.from_numpy(np.asarray(f[key])).to(dtype).to(device)
    leaves = {k: t(k).clone().requires_grad_(grad) for k in LEAVES}
    H8 = th.Vector(tensor=t("H8_0").clone(), name="H8")
    src, dst = th.Variable(leaves["feat_src"], name="feat_src"), th.Variable(leaves["feat_dst"], name="feat_dst")
    w_align = th.ScaleCostWeight(th.Variable(t("w_align"), name="w_align"))
    wp = th.Variable(t("w_prior"), name="w_prior")
    w_prior = th.ScaleCostWeight(wp) if wp.shape[1] == 1 else th.DiagonalCostWeight(wp)
    obj = th.Objective(dtype=dtype)
    if align is None:
        obj.add(th.eb.HomographyAlignment(H8, src, dst, w_align, name="align"))
    else:
        obj.add(align(H8, src, dst, w_align, "align"))
    obj.add(th.Difference(H8, th.Vector(tensor=t("H8_prior"), name="H8_prior"), w_prior, name="prior"))
    return obj, leaves, list(obj.cost_functions.keys())


def h8_from_source_map(G):
    """(..., 3, 3) matrices G that send a destination pixel's normalised (x, y, 1) to its source point -> (..., 8): the first eight
    entries of H = G^-1 scaled to H[2, 2] = 1 (fp64)"""
    H = np.linalg.inv(np.asarray(G, dtype=np.float64))
    H = H / H[..., 2:3, 2:3]
    return H.reshape(*H.shape[:-2], 9)[..., :8]


def source_map(Hh, Ww, shift=(0.5, 0.5), scale=1.0, drift=(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)):
    """G: the destination pixel (i, j) comes from source pixel (scale (j - cx) + cx + shift_x, scale (i - cy) + cy + shift_y) plus
    a small affine and perspective ``drift`` = (a, b, c, d, g6, g7) in normalised coordinates"""
    a, b, c, d, g6, g7 = drift
    return np.array([[scale + a, b, 2.0 * shift[0] / (Ww - 1)], [c, scale + d, 2.0 * shift[1] / (Hh - 1)], [g6, g7, 1.0]])


def smooth_maps(B, C, Hh, Ww, seed, G=None):
    """(B, C, Hh, Ww) fp64 values of a smooth function (a few sinusoids per channel and problem) at the normalised pixel coordinates,
    or -- ``G`` (B, 3, 3) -- at the points G sends them to"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(2.0 * np.arange(Ww) / (Ww - 1) - 1.0, 2.0 * np.arange(Hh) / (Hh - 1) - 1.0)
    p = np.stack([x, y, np.ones_like(x)], axis=0).reshape(1, 3, -1)
    if G is not None:
        q = np.asarray(G) @ p
        p = q / q[:, 2:3]
    px, py = p[:, 0].reshape(-1, 1, Hh, Ww), p[:, 1].reshape(-1, 1, Hh, Ww)
    out = np.zeros((B, C, Hh, Ww))
    for _ in range(3):
        fx, fy, ph = rng.uniform(0.5, 2.5, (B, C, 1, 1)), rng.uniform(0.5, 2.5, (B, C, 1, 1)), rng.uniform(0, 6.28, (B, C, 1, 1))
        out = out + rng.uniform(0.3, 1.0, (B, C, 1, 1)) * np.sin(fx * px + fy * py + ph)
    return out


def drifts(B, size, seed):
    """(B, 6) small drifts: every source point stays within ``size`` pixels (per axis, roughly) of its shifted lattice point"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (B, 6)) * size


def kernel_problem(B, C, Hh, Ww, seed, scale=1.0, shared=False, shift=(0.5, 0.5)):
    """A problem for the kernels alone (no reference run), same keys as the fixtures: H8_0 sends every destination pixel to the
    middle of a source cell up to a drift of less than 0.3 pixel (0.15 from the affine part and 0.15 from the perspective part at
    the image's corners), so that no source coordinate comes near an integer; ``scale`` = 3 pushes a third of the pixels out of
    the image on each side."""
    half = max(Hh - 1, Ww - 1) / 2.0
    dr = drifts(B, 0.15 / (2.0 * half * max(scale, 1.0)), seed)
    G0 = np.stack([source_map(Hh, Ww, shift, scale, dr[k]) for k in range(B)])
    Gt = np.stack([source_map(Hh, Ww, (0.2, -0.3), 1.0, -dr[k]) for k in range(B)])
    Bf = 1 if shared else B
    return dict(H8_0=h8_from_source_map(G0), H8_prior=h8_from_source_map(G0) + 0.01, feat_src=smooth_maps(Bf, C, Hh, Ww, seed + 1),
                feat_dst=smooth_maps(Bf, C, Hh, Ww, seed + 1, Gt[:Bf]), w_align=np.array([[3.0]]),
                w_prior=np.linspace(0.5, 1.5, 8).reshape(1, 8))


def min_margin(cost):
    """the smallest distance, in pixels, of any source coordinate of ``cost`` (a HomographyAlignment) from an integer"""
    with torch.no_grad():
        ix, iy = cost.source_points()
    c = torch.cat([ix, iy]).double()
    return float((c - torch.round(c)).abs().min())


def outside_fractions(cost):
    """the fractions of the destination pixels whose source point lies left of / right of / above / below the image"""
    with torch.no_grad():
        ix, iy = cost.source_points()
    Hh, Ww = cost.feat_src.tensor.shape[2:]
    return [float(m.double().mean()) for m in (ix < 0, ix > Ww - 1, iy < 0, iy > Hh - 1)]


def term_magnitudes(cost):
    """What the GPU tests' bound is made of, from ``cost`` in fp64: (weight / sum m) * sum over all C Hh Ww elements of the magnitude
    of the element's term -- m d^2 for the error, 2 m d ds/dh_k for the k-th entry of the block -> ((B, 1), (B, 1, 8)) fp64"""
    c = cost
    assert c.H8.tensor.dtype == torch.float64
    with torch.no_grad():
        src, dst = c.feat_src.tensor, c.feat_dst.tensor
        C, Hh, Ww = src.shape[1:]
        P = Hh * Ww
        ix, iy, G, q, u, v = c._geometry()
        B = max(ix.shape[0], src.shape[0], dst.shape[0])
        x0, y0 = torch.floor(ix), torch.floor(iy)
        wx1, wx0, wy1, wy0 = x0 + 1 - ix, ix - x0, y0 + 1 - iy, iy - y0
        m = ((wx1 * wy1 + wx0 * wy1 + wx1 * wy0 + wx0 * wy0) > 0.9).double().expand(B, P)
        cl = lambda t, hi: t.clamp(0, hi).long()  # noqa: E731
        flat = src.reshape(src.shape[0], C, P).expand(B, C, P)
        at = lambda r, cc: flat.gather(2, (r * Ww + cc).expand(B, P).unsqueeze(1).expand(B, C, P))  # noqa: E731
        xi0, xi1, yi0, yi1 = cl(x0, Ww - 1), cl(x0 + 1, Ww - 1), cl(y0, Hh - 1), cl(y0 + 1, Hh - 1)
        vnw, vne, vsw, vse = at(yi0, xi0), at(yi0, xi1), at(yi1, xi0), at(yi1, xi1)
        wq = lambda t: t.unsqueeze(1)  # noqa: E731
        d = vnw * wq(wx1 * wy1) + vne * wq(wx0 * wy1) + vsw * wq(wx1 * wy0) + vse * wq(wx0 * wy0) - dst.reshape(dst.shape[0], C, P)
        dsx = (vne - vnw) * wq(wy1) + (vse - vsw) * wq(wy0)
        dsy = (vsw - vnw) * wq(wx1) + (vse - vne) * wq(wx0)
        w = c.weight.sqrt_diag(1).double().expand(B, 1)
        count = C * m.sum(1, keepdim=True)
        e_mag = w * (wq(m) * d * d).sum((1, 2)).unsqueeze(1) / count
        # ds/dh_(3k+l) = -(G^T r)_k q_l per element, r = (gu / q_z, gv / q_z, -(gu u + gv v) / q_z)
        gu, gv = dsx * ((Ww - 1) / 2), dsy * ((Hh - 1) / 2)
        r = [gu / wq(q[2]), gv / wq(q[2]), -(gu * wq(u) + gv * wq(v)) / wq(q[2])]
        mags = []
        for k in range(3):
            tk = wq(G[k]) * r[0] + wq(G[3 + k]) * r[1] + wq(G[6 + k]) * r[2]
            for l in range(3):   # noqa: E741
                if 3 * k + l < 8:
                    mags.append((2 * wq(m) * d * tk * wq(q[l])).abs().sum((1, 2)).unsqueeze(1) / count * w)
        return e_mag, torch.cat(mags, dim=1).unsqueeze(1)
