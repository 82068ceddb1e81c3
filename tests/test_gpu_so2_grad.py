"""-m gpu: gradients of SO2 pose graphs through the HIP kernels (thx_so2_retract_vjp, thx_pgso2_vjp, thx_pgso2_unroll_vjp and the
cached / copied Cholesky factors) -- backward_mode "implicit", "unroll" and "truncated" through theseus_amd's own loop against the
REAL reference's gradients (tests/golden/pgso2_f64_*.npz), an fp32 run against the fp64 reference, each kernel on its own against
torch autograd through the oracle on random SO2 graphs, and the dispatch: an SO2 buffer never reaches an SE3 / SE2 / SO3 entry
point.  CPU twins (stand-in kernels, the kernels' maths on the host): tests/test_so2_grad_host.py."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import lie_so2
from oracle import pose_graph as opg
from tests.helpers import load_golden
from tests import so2_grad_common as so2g

pytestmark = pytest.mark.gpu

IMPLICIT = [("pgso2_f64_implicit", False), ("pgso2_f64_robust_implicit", True)]
UNROLLED_TAGS = ["gn_unroll", "lm_trunc", "lm_ellips_unroll"]


@pytest.mark.parametrize("name,robust", IMPLICIT)
def test_implicit_gradients_of_an_so2_graph_on_the_gpu(name, robust):
    import theseus_amd as th
    g = load_golden(name)
    final, loss, grads, _ = so2g.run(th, g, "cuda", robust=robust)
    so2g.check_implicit(g, final, loss, grads, rel=2e-6)


@pytest.mark.parametrize("tag", UNROLLED_TAGS)
def test_unrolled_gradients_of_an_so2_graph_on_the_gpu(tag):
    import theseus_amd as th
    g = load_golden("pgso2_f64_unrolled")
    so2g.check_unrolled(g, tag, *so2g.run(th, g, "cuda", tag=tag))


@pytest.mark.parametrize("name,robust", IMPLICIT)
def test_implicit_fp32_gradients_close_to_fp64_reference(name, robust):
    """fp32 storage (the LM loop, its Cholesky and the records in fp32; the VJP kernels in fp64 registers) against the reference's
    fp64 gradients of the same problem.  The bound is the forward one, not rounding: the fp32 solves carry ~cond x 6e-8 into the
    final poses and from there into every gradient.  The all-fp32 CPU stand-in of this run lands at <= 3.5e-4 of each gradient's
    largest entry (log_loss_radius of the Welsch costs the worst) and 3e-7 on the poses; the bounds sit ~6x above that.  SO2's
    raw-entry gradients need no tangent projection across dtypes (there is no Taylor branch to switch)."""
    import theseus_amd as th
    g = load_golden(name)
    final, _, grads, _ = so2g.run(th, g, "cuda", robust=robust, dtype=torch.float32)
    assert float((final.double() - torch.from_numpy(g["final"])).abs().max()) < 2e-6
    for key, got in grads.items():
        want = g[f"grad_{key}"]
        d = float(np.abs(got.double().numpy() - want).max())
        assert d <= 2e-3 * np.abs(want).max(), (key, d)


# ---- each kernel against torch autograd through the oracle ------------------------------------------------------------------------
MIXED = [None, "welsch", "huber", "hinge", "gm", "welsch+flatten", "huber+flatten", "hinge+flatten", "gm+flatten"]


def _random_so2_graph(B, seed, robust, batched):
    """A random SO2 graph (oracle PGProblem, batch-major) whose records are spread over the circle and OFF it (norms 0.8 - 1.25,
    never re-normalised); robust: a per-cost mix of every loss code on both roles."""
    gen = torch.Generator().manual_seed(seed)
    f64 = torch.float64
    P, E = 9, 17
    rng = np.random.default_rng(seed)
    edges = [(i, i + 1) for i in range(P - 1)]
    while len(edges) < E:
        i, j = sorted(rng.choice(P, 2, replace=False).tolist())
        edges.append((j, i) if rng.random() < 0.3 else (i, j))
    rec = lambda *sh: (lie_so2.so2_exp(np.pi * (2 * torch.rand(*sh, 1, dtype=f64, generator=gen) - 1))   # noqa: E731
                       * (0.8 + 0.45 * torch.rand(*sh, 1, dtype=f64, generator=gen)))
    prior_idx = torch.tensor([0, 4, 7])
    Bw = B if batched else 1
    p = opg.PGProblem(num_poses=P, edges=torch.tensor(edges), meas=rec(B, E), w_between=0.5 + torch.rand(Bw, E, 1, dtype=f64, generator=gen),
                      prior_idx=prior_idx, prior_target=rec(Bw, 3), w_prior=0.5 + torch.rand(Bw, 3, 1, dtype=f64, generator=gen),
                      group="SO2")
    if robust:
        p = dataclasses.replace(p, robust_between=[MIXED[k % len(MIXED)] for k in range(E)],
                                log_radius_between=torch.rand(Bw, E, 1, dtype=f64, generator=gen) * 3 - 2.5,
                                robust_prior=["huber", None, "gm+flatten"],
                                log_radius_prior=torch.rand(Bw, 3, 1, dtype=f64, generator=gen) * 3 - 2.5)
    return p, rec(B, P)


def _r(x, dtype):
    """The same values on both sides: fp32 runs see the fp32-rounded inputs, widened for the fp64 checker."""
    return x if x is None or dtype == torch.float64 else x.float().double()


def _rounded(p, poses, dtype):
    r = lambda x: _r(x, dtype)  # noqa: E731
    return dataclasses.replace(p, meas=r(p.meas), w_between=r(p.w_between), prior_target=r(p.prior_target), w_prior=r(p.w_prior),
                               log_radius_between=r(p.log_radius_between), log_radius_prior=r(p.log_radius_prior)), r(poses)


def _cast(p, dtype):
    c = lambda x: None if x is None else x.to(dtype)  # noqa: E731
    return dataclasses.replace(p, meas=c(p.meas), w_between=c(p.w_between), prior_target=c(p.prior_target), w_prior=c(p.w_prior),
                               log_radius_between=c(p.log_radius_between), log_radius_prior=c(p.log_radius_prior))


TOL = {torch.float64: 1e-11, torch.float32: 5e-7}   # fp32: same inputs, fp64 registers, each output rounded once


def _close(got, want, what, dtype):
    want = want.double()
    assert got.shape == want.shape, what
    assert torch.isfinite(got).all(), what
    assert float((got.cpu().double() - want).abs().max()) <= TOL[dtype] * max(1.0, float(want.abs().max())), what


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("robust,batched", [(False, False), (True, True), (True, False)])
def test_so2_vjp_kernels_vs_oracle_autograd(dtype, robust, batched):
    """thx_pgso2_vjp and thx_so2_retract_vjp on their own (70 problems: two blocks of lanes) against the stand-in's torch autograd
    through the oracle (tests/oracle_kernels.py)."""
    from tests.gpu_helpers import to_device_problem
    from tests.oracle_kernels import OracleKernels
    from theseus_amd.kernels import default_kernels
    B = 70
    p, poses = _rounded(*_random_so2_graph(B, 11, robust, batched), dtype)
    s, t = to_device_problem(_cast(p, dtype), poses.to(dtype))
    s64, t64 = to_device_problem(p, poses, device="cpu")
    E, Kp, n = s.num_edges, s.num_priors, p.num_poses
    gen = torch.Generator().manual_seed(5)
    w = _r(torch.randn(B, n, dtype=torch.float64, generator=gen), dtype)
    shapes = [(E, B, 2), (E, B, 1), (Kp, B, 2), (Kp, B, 1)] + ([(E, B, 1), (Kp, B, 1)] if robust else [])
    got = [torch.full(sh, float("nan"), dtype=dtype, device="cuda") for sh in shapes]
    want = [torch.zeros(sh, dtype=torch.float64) for sh in shapes]
    lr = lambda outs: dict(g_lrb=outs[4], g_lrp=outs[5]) if robust else {}  # noqa: E731
    default_kernels().pg_vjp(s.on("cuda"), t, w.to(dtype).cuda(), *got[:4], **lr(got))
    OracleKernels().pg_vjp(s64.on("cpu"), t64, w, *want[:4], **lr(want))
    for a, b_, name in zip(got, want, ("meas", "w_between", "prior_target", "w_prior", "log_radius_between", "log_radius_prior")):
        _close(a, b_, name, dtype)
    # the retraction's VJP, with a step size
    delta = _r(0.7 * torch.randn(B, n, dtype=torch.float64, generator=gen), dtype)
    gout = _r(torch.randn(n, B, 2, dtype=torch.float64, generator=gen), dtype)
    gd = torch.full((B, n), float("nan"), dtype=dtype, device="cuda")
    X = poses.transpose(0, 1).contiguous()
    default_kernels().retract_vjp(X.to(dtype).cuda(), delta.to(dtype).cuda(), 0.75, gout.to(dtype).cuda(), gd)
    gref = torch.zeros(B, n, dtype=torch.float64)
    OracleKernels().retract_vjp(X, delta, 0.75, gout, gref)
    _close(gd, gref, "retract", dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("ellipsoidal", [False, True])
@pytest.mark.parametrize("robust,batched", [(False, True), (True, False)])
def test_so2_unroll_vjp_kernel_vs_oracle_autograd(dtype, ellipsoidal, robust, batched):
    """thx_pgso2_unroll_vjp on its own: per-cost gradients of phi = -(J w)(r + J delta) [- lambda sum_i w_i delta_i H_ii] w.r.t. both
    poses, the measurement / target, the weights and log_loss_radius, against the stand-in's autograd through the oracle."""
    from tests.gpu_helpers import to_device_problem
    from tests.oracle_kernels import OracleKernels
    from theseus_amd.kernels import default_kernels
    B = 70
    p, poses = _rounded(*_random_so2_graph(B, 13, robust, batched), dtype)
    s, t = to_device_problem(_cast(p, dtype), poses.to(dtype))
    s64, t64 = to_device_problem(p, poses, device="cpu")
    E, Kp, n = s.num_edges, s.num_priors, p.num_poses
    gen = torch.Generator().manual_seed(6)
    w, d = (_r(torch.randn(B, n, dtype=torch.float64, generator=gen), dtype) for _ in range(2))
    lam = _r(0.1 + torch.rand(B, dtype=torch.float64, generator=gen), dtype) if ellipsoidal else None
    shapes = [(E, B, 2), (E, B, 2), (E, B, 2), (E, B, 1), (Kp, B, 2), (Kp, B, 2), (Kp, B, 1)] + ([(E, B, 1), (Kp, B, 1)] if robust else [])
    got = [torch.full(sh, float("nan"), dtype=dtype, device="cuda") for sh in shapes]
    want = [torch.zeros(sh, dtype=torch.float64) for sh in shapes]
    lr = lambda outs: dict(g_lrb=outs[7], g_lrp=outs[8]) if robust else {}  # noqa: E731
    default_kernels().pg_unroll_vjp(s.on("cuda"), t, w.to(dtype).cuda(), d.to(dtype).cuda(), *got[:7],
                                    ell_damping=None if lam is None else lam.to(dtype).cuda(), **lr(got))
    OracleKernels().pg_unroll_vjp(s64.on("cpu"), t64, w, d, *want[:7], ell_damping=lam, **lr(want))
    for a, b_, name in zip(got, want, ("pose_i", "pose_j", "meas", "w_between", "pose_prior", "prior_target", "w_prior",
                                        "log_radius_between", "log_radius_prior")):
        _close(a, b_, name, dtype)


# ---- dispatch ---------------------------------------------------------------------------------------------------------------------
class _Spy:
    """Records every C entry point called through a HipKernels' library handle."""

    def __init__(self, lib):
        self._lib, self.called = lib, []

    def __getattr__(self, name):
        if name.startswith("thx_"):
            self.called.append(name)
        return getattr(self._lib, name)


OTHER_BACKWARD = {"thx_se3_retract_vjp", "thx_se2_retract_vjp", "thx_so3_retract_vjp", "thx_pg_vjp", "thx_pg2_vjp", "thx_pgso3_vjp",
                  "thx_pg_unroll_vjp", "thx_pg2_unroll_vjp", "thx_pgso3_unroll_vjp"}


@pytest.mark.parametrize("tag", [None, "gn_unroll"])
def test_so2_buffers_reach_only_the_so2_backward_entry_points(tag):
    import theseus_amd as th
    from theseus_amd.kernels import HipKernels
    K = HipKernels()
    K.lib = spy = _Spy(K.lib)
    g = load_golden("pgso2_f64_implicit" if tag is None else "pgso2_f64_unrolled")
    final, loss, grads, _ = so2g.run(th, g, "cuda", tag=tag, optimizer_kwargs=dict(linearization_kwargs=dict(kernels=K)))
    if tag is None:
        so2g.check_implicit(g, final, loss, grads)
        expect = {"thx_so2_retract_vjp", "thx_pgso2_vjp"}
    else:
        expect = {"thx_so2_retract_vjp", "thx_pgso2_unroll_vjp"}
    called = set(spy.called)
    assert expect <= called, called
    assert not called & OTHER_BACKWARD, called & OTHER_BACKWARD
    # an SO2 buffer handed to the entry points directly, too
    X = torch.from_numpy(g["poses0"]).transpose(0, 1).contiguous().cuda()
    B, P = X.shape[1], X.shape[0]
    spy.called.clear()
    K.retract_vjp(X, torch.zeros(B, P, dtype=X.dtype, device="cuda"), 1.0, torch.ones_like(X),
                  torch.empty(B, P, dtype=X.dtype, device="cuda"))
    assert spy.called == ["thx_so2_retract_vjp"]
    with pytest.raises(ValueError, match="no VJP kernel"):
        K.retract_vjp(X[..., :1].contiguous(), torch.zeros(B, P, dtype=X.dtype, device="cuda"), 1.0,
                      torch.ones(P, B, 1, dtype=X.dtype, device="cuda"), torch.empty(B, P, dtype=X.dtype, device="cuda"))
