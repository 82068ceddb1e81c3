"""-m gpu: blocks of right-hand sides on HipSchurSolver (thx_ba_reduce_multi / thx_ba_backsub_multi, csrc/ba_multi_kernels.hip,
around the multi-vector solves of the reduced system's factor): solve_multi_with_factor, sample_deltas, marginal_covariance and
TheseusLayer.compute_samples in the solver's three modes.  Reference: the dense H of each problem rebuilt on the CPU in fp64 from
the linearization's Hcc / Hpp / W (+ the camera-camera blocks) with the damping the factor used, solved by torch.linalg in fp64.
Bar: 4 x the error of the existing single-vector ``solve_with_factor`` against the same reference on the same systems (the same
arithmetic in another order), measured in the test.  Measured on an MI355X (profiles/ba_multi/pytest_gpu_ba_multi.txt), max-norm
error relative to max|reference|, block path / single-vector path: undamped (condition ~1e9, both dominated by the shared factor)
fp32 8.6e-4 .. 2.1e-3 / the same, fp64 1.6e-7 / the same; damped fp32 4.4e-8 / 2.9e-8 (level mode, B 70, k 33) and 2.8e-8 / 2.3e-8
(dense + Between), fp64 1.3e-15 / 1.3e-15 and 9.4e-16 / 9.4e-16; X^T X against H^-1 at n = 54: fp32 2.6e-2 / 2.6e-2, fp64
3.8e-10 / 3.8e-10."""
import math

import numpy as np
import pytest
import torch

import theseus_amd as th
from oracle import lie
from theseus_amd.utils.synthetic_ba import make_ba_objective

pytestmark = pytest.mark.gpu
# fp64 retraction against the oracle's: a few hundred roundings of 1.1e-16, times the size of the sampled tangent vectors (the weak
# regularisation of the generator leaves standard deviations of tens of units)
RETRACT_BAR = 1e-10
MODES = dict(dense=dict(sparse_reduced_system=False), tile=dict(ordering="natural"), level=dict(ordering="nd"))


def relerr(got, want):
    return ((got.double().cpu() - want).abs().max() / want.abs().max()).item()


def dense_H(lin, lam=None, eps=1e-8):
    """(B, n, n) fp64 on the CPU: cameras then points, ellipsoidal damping ``lam`` (B,) as DenseSolver._apply_damping."""
    p, s = lin.packed, lin.packed.structure
    B, C, nc, n = lin.g.shape[0], s.num_cams, p.nc, lin.n
    blk = lambda x, *sh: x.double().cpu().permute(2, 0, 1).reshape(B, x.shape[0], *sh)   # noqa: E731  planar -> (B, N, ...)
    H = torch.zeros(B, n, n, dtype=torch.float64)
    for c, h in enumerate(blk(lin.Hcc, 6, 6).unbind(1)):
        H[:, 6 * c:6 * c + 6, 6 * c:6 * c + 6] = torch.tril(h) + torch.tril(h, -1).transpose(1, 2)
    for k, h in enumerate(blk(lin.Hpp, 6).unbind(1)):
        a = nc + 3 * k
        H[:, a:a + 3, a:a + 3] = torch.stack([h[:, [0, 1, 2]], h[:, [1, 3, 4]], h[:, [2, 4, 5]]], 1)
    W = blk(lin.W, 6, 3)
    for o in range(s.num_obs):
        c, k = int(s.t["obs_cam"][o]), int(s.t["obs_pt"][o])
        H[:, 6 * c:6 * c + 6, nc + 3 * k:nc + 3 * k + 3] += W[:, o]
    H[:, nc:, :nc] = H[:, :nc, nc:].transpose(1, 2)
    if p.cc_costs:
        off = torch.zeros_like(H)
        off.index_put_((torch.arange(B).view(-1, 1, 1, 1), lin._cc_rows.cpu().unsqueeze(0), lin._cc_cols.cpu().unsqueeze(0)),
                       lin._cc_off.double().cpu(), accumulate=True)
        H += off + off.transpose(1, 2)
    if lam is not None:
        d = H.diagonal(dim1=1, dim2=2)
        H = H + torch.diag_embed(lam.double().cpu().view(-1, 1) * d + eps)
    return H


def system(dtype, B, mode, damped=False, between=False, cams=48, points=96, seed=0):
    """-> (optimizer, solver, H^-1 (B, n, n) fp64 CPU) after one solve: the factor every test below uses."""
    obj, _ = make_ba_objective(cams, points, B, dtype=dtype, seed=seed)
    if between:
        a, b = obj.get_variable("Cam3"), obj.get_variable("Cam40")
        meas = th.SE3(tensor=torch.eye(3, 4, dtype=dtype, device="cuda").unsqueeze(0), name="odo")
        obj.add(th.Between(a, b, meas, th.ScaleCostWeight(torch.tensor(0.5, dtype=dtype, device="cuda")), name="between"))
    opt = th.LevenbergMarquardt(obj, max_iterations=1, linear_solver_kwargs=MODES[mode])
    solver = opt.linear_solver
    obj.update()
    solver.linearization.linearize()
    lam = torch.linspace(0.5, 2.0, B, dtype=dtype, device="cuda") if damped else None
    solver.solve(damping=lam)
    assert solver.levels == (mode == "level") and (mode == "level" or solver.sparse == (mode == "tile"))
    return opt, solver, torch.linalg.inv(dense_H(solver.linearization, lam))


def block(B, k, n, dtype, seed=1):
    return torch.randn(B, k, n, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()


def single_vector_error(solver, rhs, want):
    """The bar's yardstick: the existing single-vector path, one call per vector, against the same reference."""
    got = torch.stack([solver.solve_with_factor(rhs[:, j].contiguous()) for j in range(rhs.shape[1])], 1)
    return relerr(got, want)


CASES = [(m, B, k, {}) for m in MODES for B, k in ((3, 1), (70, 33))] + \
    [("level", 70, 33, dict(damped=True)), ("tile", 3, 5, dict(between=True)), ("dense", 3, 5, dict(damped=True, between=True))]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mode,B,k,kw", CASES, ids=[f"{m}-B{B}-k{k}" + "".join("-" + x for x in kw) for m, B, k, kw in CASES])
def test_block_solves_match_the_dense_fp64_inverse(dtype, mode, B, k, kw):
    """which = 0 against H^-1 rhs; which = 2 then 1 gives the same; two calls give the same bits.  48 cameras (three tiles, a real
    dissection order), 96 points of which some have a single observation."""
    _, solver, Hinv = system(dtype, B, mode, **kw)
    s = solver.linearization.packed.structure
    assert (np.diff(s.t["pt_ptr"]) == 1).any()
    rhs = block(B, k, solver.linearization.n, dtype)
    want = (Hinv @ rhs.double().cpu().transpose(1, 2)).transpose(1, 2)
    bar = 4 * single_vector_error(solver, rhs, want)
    x0 = solver.solve_multi_with_factor(rhs)
    x21 = solver.solve_multi_with_factor(solver.solve_multi_with_factor(rhs, 2), 1)
    e0, e21 = relerr(x0, want), relerr(x21, want)
    print(f"{mode} {dtype} B={B} k={k} {kw}: which=0 {e0:.3e}, 2 then 1 {e21:.3e}, bar (4 x single-vector) {bar:.3e}")
    assert e0 <= bar and e21 <= bar
    assert torch.equal(x0, solver.solve_multi_with_factor(rhs))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_the_square_root_is_exact_and_sample_deltas_uses_it(dtype):
    """n = 54, k = n: X = M^-T applied to the identity block has X^T X = H^-1 -- cameras, points and cross blocks."""
    B, T = 3, 0.5
    _, solver, _ = system(dtype, B, "dense", cams=4, points=10)
    n = solver.linearization.n
    assert n == 54
    noise = torch.randn(n, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).to(dtype).cuda()
    samples = solver.sample_deltas(7, temperature=T, noise=noise)              # (factorises undamped: that factor from here on)
    delta = solver.solve()
    Hinv = torch.linalg.inv(dense_H(solver.linearization))
    eye = torch.eye(n, dtype=dtype, device="cuda").expand(B, n, n)
    bar = 4 * single_vector_error(solver, eye, Hinv)
    X = solver.solve_multi_with_factor(eye, 1).double().cpu()
    e_cov = relerr(X.transpose(1, 2) @ X, Hinv)
    want = delta.double().cpu().unsqueeze(2) + math.sqrt(T) * (X.transpose(1, 2) @ noise.double().cpu())
    e_smp = relerr(samples, want)
    print(f"{dtype}: X^T X vs H^-1 {e_cov:.3e}, sample_deltas {e_smp:.3e}, bar {bar:.3e}")
    assert e_cov <= bar and e_smp <= bar


@pytest.mark.parametrize("mode", list(MODES))
def test_marginal_covariance_and_compute_samples(mode):
    dtype, B, k = torch.float64, 3, 4
    opt, solver, _ = system(dtype, B, mode)
    lin, p = solver.linearization, solver.linearization.packed
    names = [p.cam_vars[5].name, p.pt_vars[3].name, p.pt_vars[40].name]
    cols = [c for nm in names for i in [lin.ordering.index_of(nm)] for c in range(lin.var_start_cols[i], lin.var_start_cols[i] + lin.var_dims[i])]
    C = solver.marginal_covariance(names)                                        # (factorises undamped)
    Hinv = torch.linalg.inv(dense_H(lin))
    bar = 4 * single_vector_error(solver, torch.eye(lin.n, dtype=dtype, device="cuda")[cols].expand(B, -1, -1), Hinv[:, cols])
    assert torch.equal(C, C.transpose(1, 2)) and relerr(C, Hinv[:, cols][:, :, cols]) <= bar
    before = {v.name: v.tensor.clone() for v in p.cam_vars + p.pt_vars}
    noise = torch.randn(lin.n, k, dtype=dtype, generator=torch.Generator().manual_seed(5)).cuda()
    out = th.TheseusLayer(opt).compute_samples(solver, k, 0.7, noise=noise, return_dict=True)
    d = solver.sample_deltas(k, 0.7, noise=noise).transpose(1, 2).cpu()             # (B, k, n)
    for i, v in enumerate(p.cam_vars):
        want = lie.se3_compose(before[v.name].cpu().unsqueeze(1), lie.se3_exp(d[:, :, 6 * i:6 * i + 6]))
        assert out[v.name].shape == (B, k, 3, 4) and relerr(out[v.name], want) < RETRACT_BAR
    for i, v in enumerate(p.pt_vars):
        assert relerr(out[v.name], before[v.name].cpu().unsqueeze(1) + d[:, :, p.nc + 3 * i:p.nc + 3 * i + 3]) < RETRACT_BAR
    assert all(torch.equal(v.tensor, before[v.name]) for v in p.cam_vars + p.pt_vars)
