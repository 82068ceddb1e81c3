"""Homography estimation by dense feature alignment (the reference's examples/homography_estimation.py) on theseus_amd's own API:
a two-layer CNN turns two images into feature maps, Levenberg-Marquardt (50 iterations, step size 0.1) finds the homography that
aligns them -- HomographyAlignment plus a Difference regulariser towards the identity, on the fused path
(theseus_amd/homography.py: PackedHomography -- thx_homog_eval + thx_block_assemble + the Cholesky at n = 8) -- and Adam trains the
CNN through the implicit backward mode on the four-corner distance between the estimate and the known homography.
The data are synthetic: smooth images (a few sinusoids) and random homographies close to the identity, generated here; the second
image of a pair is the first one's function evaluated where the true homography sends each pixel.  No dataset, no kornia.
usage: python examples/homography_estimation.py [--batch 16] [--size 60 80] [--channels 4] [--outer 5] [--device cuda] [--dtype f32]
       (--kernels module:Class substitutes the kernel set -- the tests' CPU stand-in, for machines without a GPU)
"""
import argparse
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import theseus_amd as th  # noqa: E402

IDENTITY8 = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
REG_WEIGHT = 1e-2 ** 0.5   # the example's regulariser: sqrt(1e-2)


def pixel_grid(Hh, Ww, dtype, device):
    """(3, Hh Ww): the normalised homogeneous coordinates (x, y, 1) of every pixel, x = 2 j / (Ww - 1) - 1"""
    x = (2 * torch.arange(Ww, dtype=dtype, device=device) / (Ww - 1) - 1).repeat(Hh)
    y = (2 * torch.arange(Hh, dtype=dtype, device=device) / (Hh - 1) - 1).repeat_interleave(Ww)
    return torch.stack([x, y, torch.ones_like(x)])


def image_pairs(B, Hh, Ww, dtype, device, seed=0, strength=0.04):
    """-> img1, img2 (B, 1, Hh, Ww) and the true H8 (B, 8): img2 shows img1's scene through the homography (img2(p) = img1(H^-1 p))"""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64).to(dtype).to(device)  # noqa: E731
    H8 = torch.tensor(IDENTITY8, dtype=dtype, device=device) + strength * (2 * rnd(B, 8) - 1)
    Hm = torch.cat([H8, torch.ones(B, 1, dtype=dtype, device=device)], dim=1).view(B, 3, 3)
    p = pixel_grid(Hh, Ww, dtype, device)
    q = torch.linalg.inv(Hm) @ p
    waves = [(1 + 3 * rnd(B, 1), 1 + 3 * rnd(B, 1), 6.28 * rnd(B, 1), 0.3 + 0.7 * rnd(B, 1)) for _ in range(4)]

    def scene(x, y):
        return sum(a * torch.sin(fx * x + fy * y + ph) for fx, fy, ph, a in waves)
    img1 = scene(p[0].unsqueeze(0), p[1].unsqueeze(0)).view(B, 1, Hh, Ww)
    img2 = scene(q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]).view(B, 1, Hh, Ww)
    return img1, img2, H8


def make_objective(th, feat1, feat2, dtype, device):
    """H8 starts at the identity; feat1 is warped onto feat2"""
    B = max(feat1.shape[0], feat2.shape[0])
    eye = torch.tensor([IDENTITY8], dtype=dtype, device=device)
    H8 = th.Vector(tensor=eye.repeat(B, 1), name="H8_1_2")
    obj = th.Objective(dtype=dtype)
    obj.add(th.eb.HomographyAlignment(H8, th.Variable(feat1, name="feat1"), th.Variable(feat2, name="feat2"), name="alignment"))
    reg = th.ScaleCostWeight(th.Variable(torch.full((1, 1), REG_WEIGHT, dtype=dtype, device=device), name="reg_w"))
    obj.add(th.Difference(H8, th.Vector(tensor=eye.clone(), name="identity"), reg, name="reg_homography"))
    return obj


def four_corner_dist(H8, H8_gt):
    """mean distance, in normalised units, between the images of the four corners (+-1, +-1) under both homographies"""
    one = torch.ones(H8.shape[0], 1, dtype=H8.dtype, device=H8.device)
    corners = torch.tensor([[-1.0, 1.0, -1.0, 1.0], [-1.0, -1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0]], dtype=H8.dtype, device=H8.device)

    def warp(h):
        q = torch.cat([h, one], dim=1).view(-1, 3, 3) @ corners
        return q[:, :2] / q[:, 2:]
    return (warp(H8) - warp(H8_gt)).norm(dim=1).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, nargs=2, default=[60, 80])
    ap.add_argument("--channels", type=int, default=4)
    ap.add_argument("--outer", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--kernels", default=None)
    a = ap.parse_args()
    dtype = torch.float64 if a.dtype == "f64" else torch.float32
    kernels = None
    if a.kernels:
        mod, cls = a.kernels.split(":")
        kernels = getattr(importlib.import_module(mod), cls)()
    torch.manual_seed(0)
    Hh, Ww = a.size
    cnn = torch.nn.Sequential(torch.nn.Conv2d(1, a.channels, 3, padding=1), torch.nn.ReLU(),
                              torch.nn.Conv2d(a.channels, a.channels, 3, padding=1)).to(a.device).to(dtype)
    outer = torch.optim.Adam(cnn.parameters(), lr=a.lr)
    img1, img2, H8_gt = image_pairs(a.batch, Hh, Ww, dtype, a.device)
    obj = make_objective(th, cnn(img1).detach(), cnn(img2).detach(), dtype, a.device)
    opt = th.LevenbergMarquardt(obj, max_iterations=a.iters, step_size=0.1, abs_err_tolerance=0.0, rel_err_tolerance=0.0,
                                linearization_kwargs=dict(kernels=kernels) if kernels else None)
    layer = th.TheseusLayer(opt)
    print(f"batch {a.batch}, {a.channels} x {Hh} x {Ww} feature maps, packed family: "
          f"{type(opt.linear_solver.linearization.packed).__name__}")
    eye = torch.tensor([IDENTITY8], dtype=dtype, device=a.device).repeat(a.batch, 1)
    print(f"four-corner distance of the identity: {float(four_corner_dist(eye, H8_gt)):.4f}")
    for it in range(a.outer):
        outer.zero_grad()
        inputs = {"H8_1_2": eye.clone(), "feat1": cnn(img1), "feat2": cnn(img2)}   # new feature maps at every outer step
        sol, info = layer.forward(inputs, optimizer_kwargs=dict(backward_mode="implicit"))
        loss = four_corner_dist(sol["H8_1_2"], H8_gt)
        loss.backward()
        outer.step()
        print(f"outer step {it}: four-corner distance {loss.item():.4f}, alignment objective {float(obj.error_metric().mean()):.3e}")


if __name__ == "__main__":
    main()
