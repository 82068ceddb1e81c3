"""A zoo of small bundle-adjustment problems that leave the corner the golden fixtures live in (B <= 4, ``feat`` batched and every
other auxiliary batch-shared, one generator): seeded generator, the theseus_amd objective and the oracle ``BAProblem`` of a
case, and ONE comparison of the first damped linear system with the oracle (oracle/ba.py, fp64, CPU) that the host tests
(tests/test_ba_zoo_host.py, stand-in kernels) and the GPU tests (tests/test_gpu_ba_zoo.py, HIP kernels) share.

Column order of every comparison = the linearization's: cameras, then points, each in the objective's insertion order.  The
oracle problem is built with that ``var_order``, worked out here from the cost add order (and asserted against the packer's)."""
import dataclasses

import numpy as np
import torch

from oracle import ba as oba
from oracle import lie
from oracle import pose_graph as opg

TOPOLOGIES = ("regular", "lonely_camera", "single_view_points", "two_islands", "repeated_observation", "no_priors_but_one",
              "odometry", "levels")
# the eight batch strides of thx_ba_data (focal / k1 / k2 share one by contract)
AUX = ("calib", "feat", "w_obs", "log_radius", "cam_prior_target", "w_cam_prior", "pt_prior_target", "w_pt_prior")
AUX_KEYS = dict(calib=("focal", "k1", "k2"), feat=("feat",), w_obs=("w_obs",), log_radius=("log_radius",),
                cam_prior_target=("cam_prior_target",), w_cam_prior=("w_cam_prior",), pt_prior_target=("pt_prior_target",),
                w_pt_prior=("w_pt_prior",))       # the case's arrays behind each stride
_MIXED_A = ("calib", "w_obs", "cam_prior_target", "w_pt_prior")
LAYOUTS = {"shared": (), "batched": AUX, "mixed_a": _MIXED_A, "mixed_b": tuple(a for a in AUX if a not in _MIXED_A)}
MIN_DEPTH = 5.0
# Smallest rotation angle of target^-1 camera over the camera priors.  The derivative of the SE3 log map's Jacobian cancels like
# eps / angle^3: at 0.004 rad the autograd reference's own gradient of a camera prior moves by 3e-10 of its scale under a one-ulp
# change of the cameras, above the 1e-10 gradient bar; at 0.05 rad that is 1e-13.
MIN_PRIOR_ANGLE = 0.05
MIN_KINK_GAP = 1e-9         # |x / radius - 1| of every robust term: the derivative of the Huber rescale jumps at x = radius


# ---- topologies ------------------------------------------------------------------------------------------------------------------
def _sample(rng, cams, k):
    return sorted(rng.choice(np.asarray(cams), size=k, replace=False).tolist())


def topology(name, rng):
    """-> dict(C, Np, obs [(camera, point)], cam_priors [camera], pt_priors [point], cc_edges [(i, j)], solver_kwargs)."""
    cc, kw = [], {}
    if name == "regular":
        C, Np = 6, 20
        obs = [(c, p) for p in range(Np) for c in _sample(rng, range(C), 3 + (p % 2))]
    elif name == "lonely_camera":          # camera 2: a prior and a Between, no Reprojection
        C, Np = 6, 16
        obs = [(c, p) for p in range(Np) for c in _sample(rng, (0, 1, 3, 4, 5), 3)]
        cc = [(1, 2)]
    elif name == "single_view_points":     # points 0..8: one camera each; point 9: every camera
        C, Np = 5, 18
        obs = [(p % C, p) for p in range(9)] + [(c, 9) for c in range(C)]
        obs += [(c, p) for p in range(10, Np) for c in _sample(rng, range(C), 2 + (p % 2))]
    elif name == "two_islands":
        C, Np = 6, 14
        obs = [(c, p) for p in range(Np) for c in _sample(rng, (0, 1, 2) if p < 7 else (3, 4, 5), 2 + (p % 2))]
    elif name == "repeated_observation":   # camera 1 observes point 3 twice
        C, Np = 4, 10
        obs = [(c, p) for p in range(Np) for c in _sample(rng, range(C), 2 + (p % 2))]
        obs = [o for o in obs if o != (1, 3)] + [(1, 3), (1, 3)]
    elif name == "no_priors_but_one":
        C, Np = 5, 14
        obs = [(c, p) for p in range(Np) for c in _sample(rng, range(C), 3)]
    elif name == "odometry":               # the islands again, joined by Between costs only: (3, 2) and (2, 5) share no point
        C, Np = 6, 14
        obs = [(c, p) for p in range(Np) for c in _sample(rng, (0, 1, 2) if p < 7 else (3, 4, 5), 2 + (p % 2))]
        cc = [(0, 1), (3, 2), (2, 5), (4, 5)]
    elif name == "levels":                 # cameras on a ring with local tracks, two Cholesky tiles, dissection order
        C, Np = 24, 60
        obs = [((p * C // Np + d) % C, p) for p in range(Np) for d in _sample(rng, range(-2, 3), 3)]
        kw = dict(ordering="nd")
    else:
        raise ValueError(name)
    cam_priors, pt_priors = list(range(C)), list(range(Np))
    if name == "no_priors_but_one":
        cam_priors, pt_priors = [0], []
    assert sorted({p for _, p in obs}) == list(range(Np))
    return dict(C=C, Np=Np, obs=obs, cam_priors=cam_priors, pt_priors=pt_priors, cc_edges=cc, solver_kwargs=kw)


# ---- generator -------------------------------------------------------------------------------------------------------------------
def _project(cams, pts, focal, k1, k2):
    pc = cams[..., 3] + (cams[..., :3] @ pts.unsqueeze(-1)).squeeze(-1)
    proj = -pc[..., :2] / pc[..., 2:3]
    q = (proj * proj).sum(-1, keepdim=True)
    return proj * (focal * (1.0 + q * (k1 + q * k2)))


def make_case(topology_name, B, layout, robust="huber", dtype=torch.float64, seed=0):
    """Fixture-style dict (numpy arrays; the keys tests/ba_common.build_ba_objective and tests/helpers.ba_problem read, the
    per-auxiliary batch sizes ``batch``, the cost add order, the damping vector).  Cameras near the identity look at points at depth
    7..10; initial perturbations as in theseus_amd/utils/synthetic_ba.py scaled to that size; batched tensors are independent
    draws per batch item."""
    rng = np.random.default_rng(1000 * seed + TOPOLOGIES.index(topology_name))
    gen = torch.Generator().manual_seed(int(rng.integers(1 << 31)))
    rnd = lambda *s: 2.0 * torch.rand(*s, generator=gen, dtype=torch.float64) - 1.0   # noqa: E731
    top = topology(topology_name, rng)
    C, Np, obs = top["C"], top["Np"], top["obs"]
    obs = [obs[k] for k in rng.permutation(len(obs))]
    O, Kc, Kp, E = len(obs), len(top["cam_priors"]), len(top["pt_priors"]), len(top["cc_edges"])
    nb = {a: (B if a in LAYOUTS[layout] else 1) for a in AUX}
    oc, op = torch.tensor([c for c, _ in obs]), torch.tensor([p for _, p in obs])
    gt_cams = lie.se3_exp(torch.cat([2.0 * rnd(C, 2), 0.3 * rnd(C, 1), 0.1 * rnd(C, 3)], 1))   # (a baseline: depth is observable)
    gt_pts = torch.cat([2.0 * rnd(Np, 2), 8.5 + 1.5 * rnd(Np, 1)], 1)
    focal0, k10, k20 = 50.0 + 5.0 * rnd(1, C, 1), 0.05 * rnd(1, C, 1), 0.01 * rnd(1, C, 1)
    focal = focal0 + 2.0 * rnd(nb["calib"], C, 1) * (nb["calib"] > 1)
    k1 = k10 + 0.01 * rnd(nb["calib"], C, 1) * (nb["calib"] > 1)
    k2 = k20 + 0.002 * rnd(nb["calib"], C, 1) * (nb["calib"] > 1)
    feat = _project(gt_cams[oc], gt_pts[op], focal0[0, oc], k10[0, oc], k20[0, oc]).unsqueeze(0) + 0.3 * rnd(nb["feat"], O, 2)
    w_obs = 1.0 + 0.5 * rnd(nb["w_obs"], O, 2)
    pert = lie.se3_exp(torch.cat([0.1 * rnd(B * C, 3), 0.01 * rnd(B * C, 3)], 1)).view(B, C, 3, 4)
    cams0 = lie.se3_compose(gt_cams.unsqueeze(0).expand(B, C, 3, 4), pert)
    pts0 = gt_pts.unsqueeze(0) + 0.1 * rnd(B, Np, 3)
    cpi, ppi = torch.tensor(top["cam_priors"], dtype=torch.long), torch.tensor(top["pt_priors"], dtype=torch.long)
    nt = nb["cam_prior_target"]
    # (prior targets a fixed angle of 0.1..0.2 rad away from their camera: the gradients of log(target^-1 camera) lose eps / angle^3
    #  near the identity, in the reference as in any kernel -- see MIN_PRIOR_ANGLE)
    axis = torch.nn.functional.normalize(rnd(nt * Kc, 3) + 1e-3, dim=1)
    cam_prior_target = lie.se3_compose(gt_cams[cpi].unsqueeze(0).expand(nt, Kc, 3, 4),
                                       lie.se3_exp(torch.cat([0.05 * rnd(nt * Kc, 3), (0.15 + 0.05 * rnd(nt * Kc, 1)) * axis], 1)).view(nt, Kc, 3, 4))
    w_cam_prior = 4.0 + 2.0 * rnd(nb["w_cam_prior"], Kc, 6)
    pt_prior_target = gt_pts[ppi].unsqueeze(0) + 0.2 * rnd(nb["pt_prior_target"], Kp, 3)
    w_pt_prior = 1.0 + 0.4 * rnd(nb["w_pt_prior"], Kp, 3)
    cc = torch.tensor(top["cc_edges"], dtype=torch.long).view(E, 2)
    rel = lie.se3_compose(lie.se3_inverse(gt_cams[cc[:, 0]]), gt_cams[cc[:, 1]])
    cc_meas = lie.se3_compose(rel.unsqueeze(0).expand(B, E, 3, 4),
                              lie.se3_exp(torch.cat([0.02 * rnd(B * E, 3), 0.01 * rnd(B * E, 3)], 1)).view(B, E, 3, 4))
    w_cc = 4.0 + 2.0 * rnd(1, E, 6)
    # cost add order: every kind interleaved (the row tables of Av, the variables' insertion order)
    costs = [(0, k) for k in range(O)] + [(1, k) for k in range(Kc)] + [(2, k) for k in range(Kp)] + [(3, k) for k in range(E)]
    costs = [costs[k] for k in rng.permutation(len(costs))]
    cam_order, pt_order = [], []
    for kind, k in costs:                  # insertion order of the optimisation variables
        cams_k = [obs[k][0]] if kind == 0 else [top["cam_priors"][k]] if kind == 1 else list(top["cc_edges"][k]) if kind == 3 else []
        pts_k = [obs[k][1]] if kind == 0 else [top["pt_priors"][k]] if kind == 2 else []
        cam_order += [c for c in cams_k if c not in cam_order]
        pt_order += [p for p in pts_k if p not in pt_order]
    assert sorted(cam_order) == list(range(C)) and sorted(pt_order) == list(range(Np))
    damping = 1.0 + 1.5 * torch.rand(B, generator=gen, dtype=torch.float64)
    cast = lambda x: x.to(dtype).numpy()   # noqa: E731
    case = dict(topology=topology_name, layout=layout, B=B, C=C, Np=Np, robust=robust or "", batch=nb, dtype=dtype,
                obs_cam=oc.numpy(), obs_pt=op.numpy(), cams0=cast(cams0), pts0=cast(pts0), feat=cast(feat), w_obs=cast(w_obs),
                focal=cast(focal), k1=cast(k1), k2=cast(k2), cam_prior_idx=cpi.numpy(), cam_prior_target=cast(cam_prior_target),
                w_cam_prior=cast(w_cam_prior), pt_prior_idx=ppi.numpy(), pt_prior_target=cast(pt_prior_target),
                w_pt_prior=cast(w_pt_prior), cc_edges=cc.numpy(), cc_meas=cast(cc_meas), w_cc=cast(w_cc),
                cost_kind=np.array([k for k, _ in costs]), cost_idx=np.array([i for _, i in costs]),
                var_kind=np.array([0] * C + [1] * Np), var_idx=np.array(cam_order + pt_order), cam_order=cam_order, pt_order=pt_order,
                damping=cast(damping), solver_kwargs=top["solver_kwargs"],
                opt_kwargs=repr(dict(gauss_newton=False, max_iterations=1, step_size=1.0, ellipsoidal_damping=True)))
    case["log_radius"] = _choose_radii(case) if robust else None
    _assert_conditions(case)
    return case


def _with(d, **kw):
    out = dict(d)
    out.update(kw)
    return out


def _weighted_sq_residuals(case):
    """(B, O, 2) squared weighted reprojection residuals of the initial state, from the oracle without a loss."""
    p, state = oracle_problem(_with(case, robust="", log_radius=None))
    return p.terms(state)[3] ** 2


def _choose_radii(case):
    """log radii from the oracle's own weighted residuals, so that both branches of the loss are taken: one shared variable
    (1, 1, 1) in the ``shared`` layout, else one per observation with batch 1 | B."""
    x2 = _weighted_sq_residuals(case)
    B, O = x2.shape[:2]
    stat = x2.mean(-1, keepdim=True) if case["robust"].endswith("+flatten") else x2.sum(-1, keepdim=True)   # (B, O, 1)
    if case["layout"] == "shared":
        srt = stat.reshape(-1).sort().values
        r = (srt[srt.numel() // 2 - 1] * srt[srt.numel() // 2]).sqrt().view(1, 1, 1) if srt.numel() > 1 else 1.5 * srt.view(1, 1, 1)
    elif case["batch"]["log_radius"] == 1:
        r = stat.median(0, keepdim=True).values * torch.where(torch.arange(O) % 2 == 0, 1.5, 1 / 1.5).view(1, O, 1)
    else:
        flip = (torch.arange(B).view(B, 1) + torch.arange(O).view(1, O)) % 2 == 0
        r = stat * torch.where(flip, 2.0, 0.5).view(B, O, 1)
    return r.log().to(case["dtype"]).numpy()


def radius_shares(case):
    """(share of the weighted residual terms inside the loss radius, share outside), in the oracle."""
    x2 = _weighted_sq_residuals(case)
    x = x2 if case["robust"].endswith("+flatten") else x2.sum(-1, keepdim=True)
    inside = (x <= torch.from_numpy(case["log_radius"]).double().exp()).double().mean().item()
    return inside, 1.0 - inside


def min_depth(case):
    p, (cams, pts) = oracle_problem(case)
    c, x = cams[:, p.obs_cam], pts[:, p.obs_pt]
    return (c[..., 3] + (c[..., :3] @ x.unsqueeze(-1)).squeeze(-1))[..., 2].abs().min().item()


def min_prior_angle(case):
    p, (cams, _) = oracle_problem(case)
    if p.cam_prior_idx.numel() == 0:
        return float("inf")
    D = lie.se3_compose(lie.se3_inverse(p.cam_prior_target), cams[:, p.cam_prior_idx])
    return lie.se3_log(D)[..., 3:].norm(dim=-1).min().item()


def _assert_conditions(case):
    assert min_depth(case) >= MIN_DEPTH
    assert min_prior_angle(case) >= MIN_PRIOR_ANGLE
    if case["robust"]:
        inside, outside = radius_shares(case)
        assert inside >= 0.2 and outside >= 0.2, (inside, outside)
        x2 = _weighted_sq_residuals(case)
        x = x2 if case["robust"].endswith("+flatten") else x2.sum(-1, keepdim=True)
        assert ((x / torch.from_numpy(case["log_radius"]).double().exp() - 1.0).abs() >= MIN_KINK_GAP).all()
    assert (case["w_obs"][..., 0] != case["w_obs"][..., 1]).all() and case["pt_prior_target"].all()
    assert all(len(set(row.tolist())) == 6 for row in case["w_cam_prior"].reshape(-1, 6))
    B = case["B"]
    for k in ("cams0", "pts0") + tuple(k for a, ks in AUX_KEYS.items() if case["batch"][a] == B for k in ks):
        x = case[k]
        if x is None or x.shape[1] == 0 or x.shape[0] != B:
            continue
        items = sorted({0, min(63, B - 1), min(64, B - 1), B - 1})
        for i in items:
            for j in items:
                assert i == j or not np.array_equal(x[i], x[j]), (k, i, j)


# ---- builders --------------------------------------------------------------------------------------------------------------------
def build_objective(th, case, device="cpu"):
    """-> (objective, camera variables, point variables) in the case's own numbering; costs added in the case's add order."""
    t = lambda a: torch.from_numpy(a).to(device)   # noqa: E731
    dtype = case["dtype"]
    C, Np, O = case["C"], case["Np"], case["obs_cam"].shape[0]
    cams0, pts0, feat, w_obs = t(case["cams0"]), t(case["pts0"]), t(case["feat"]), t(case["w_obs"])
    obj = th.Objective(dtype=dtype)
    cam_v = [th.SE3(tensor=cams0[:, i].clone(), name=f"Cam{i}") for i in range(C)]
    pt_v = [th.Point3(tensor=pts0[:, i].clone(), name=f"Pt{i}") for i in range(Np)]
    fl = [th.Vector(tensor=t(case["focal"])[:, i].clone(), name=f"fl{i}") for i in range(C)]
    k1 = [th.Vector(tensor=t(case["k1"])[:, i].clone(), name=f"k1_{i}") for i in range(C)]
    k2 = [th.Vector(tensor=t(case["k2"])[:, i].clone(), name=f"k2_{i}") for i in range(C)]
    robust = case["robust"]
    if robust:
        lr = t(case["log_radius"])
        radius = [th.Vector(tensor=lr[:, o if lr.shape[1] > 1 else 0].clone(), name=f"log_radius_{o}") for o in range(lr.shape[1])]
    loss = {"huber": th.HuberLoss, "welsch": th.WelschLoss}.get(robust.split("+")[0])
    diag = lambda x, name: th.DiagonalCostWeight(th.Variable(x.clone(), name=name))   # noqa: E731
    for kind, k in zip(case["cost_kind"].tolist(), case["cost_idx"].tolist()):
        if kind == 0:
            c, p = int(case["obs_cam"][k]), int(case["obs_pt"][k])
            cf = th.Reprojection(camera_pose=cam_v[c], world_point=pt_v[p], focal_length=fl[c], calib_k1=k1[c], calib_k2=k2[c],
                                 image_feature_point=th.Point2(tensor=feat[:, k].clone(), name=f"Feat{k}"),
                                 weight=diag(w_obs[:, k], f"w_obs_{k}"), name=f"reproj_{k}")
            if robust:
                cf = th.RobustCostFunction(cf, loss, radius[k if len(radius) > 1 else 0], name=f"robust_{k}",
                                           flatten_dims=robust.endswith("+flatten"))
            obj.add(cf)
        elif kind == 1:
            obj.add(th.Difference(cam_v[int(case["cam_prior_idx"][k])],
                                  th.SE3(tensor=t(case["cam_prior_target"])[:, k].clone(), name=f"cam_target_{k}"),
                                  diag(t(case["w_cam_prior"])[:, k], f"w_cam_prior_{k}"), name=f"cam_prior_{k}"))
        elif kind == 2:
            obj.add(th.Difference(pt_v[int(case["pt_prior_idx"][k])],
                                  th.Point3(tensor=t(case["pt_prior_target"])[:, k].clone(), name=f"pt_target_{k}"),
                                  diag(t(case["w_pt_prior"])[:, k], f"w_pt_prior_{k}"), name=f"pt_prior_{k}"))
        else:
            i, j = case["cc_edges"][k].tolist()
            obj.add(th.Between(cam_v[i], cam_v[j], th.SE3(tensor=t(case["cc_meas"])[:, k].clone(), name=f"odo_{k}"),
                               diag(t(case["w_cc"])[:, k], f"w_odo_{k}"), name=f"odometry_{k}"))
    return obj, cam_v, pt_v


def oracle_problem(case, **replace):
    """-> (oracle BAProblem in fp64 with the LINEARIZATION's numbering -- cameras / points re-indexed to their insertion order, columns
    cameras then points --, (cams0, pts0)).  ``replace``: BAProblem fields to overwrite (the self-checks of the comparison)."""
    d = lambda a: torch.from_numpy(a).double()   # noqa: E731
    C, Np = case["C"], case["Np"]
    cpos = {c: k for k, c in enumerate(case["cam_order"])}
    ppos = {p: k for k, p in enumerate(case["pt_order"])}
    ci = lambda a: torch.tensor([cpos[int(c)] for c in np.asarray(a).reshape(-1)], dtype=torch.long)   # noqa: E731
    pi = lambda a: torch.tensor([ppos[int(p)] for p in np.asarray(a).reshape(-1)], dtype=torch.long)   # noqa: E731
    cam_perm = torch.tensor(case["cam_order"])
    E = case["cc_edges"].shape[0]
    robust = case["robust"] or None
    p = oba.BAProblem(
        num_cams=C, num_points=Np, obs_cam=ci(case["obs_cam"]), obs_pt=pi(case["obs_pt"]), feat=d(case["feat"]), w_obs=d(case["w_obs"]),
        focal=d(case["focal"])[:, cam_perm], k1=d(case["k1"])[:, cam_perm], k2=d(case["k2"])[:, cam_perm],
        cam_prior_idx=ci(case["cam_prior_idx"]), cam_prior_target=d(case["cam_prior_target"]), w_cam_prior=d(case["w_cam_prior"]),
        pt_prior_idx=pi(case["pt_prior_idx"]), pt_prior_target=d(case["pt_prior_target"]), w_pt_prior=d(case["w_pt_prior"]),
        var_order=[("cam", k) for k in range(C)] + [("pt", k) for k in range(Np)],
        cost_order=[(("obs", "cam_prior", "pt_prior", "cam_between")[k], int(i)) for k, i in zip(case["cost_kind"].tolist(), case["cost_idx"].tolist())],
        robust_obs=robust, log_radius_obs=d(case["log_radius"]) if robust else None,
        cc_edges=ci(case["cc_edges"]).view(E, 2) if E else None, cc_meas=d(case["cc_meas"]) if E else None,
        w_cc=d(case["w_cc"]) if E else None)
    if replace:
        p = dataclasses.replace(p, **replace)
    return p, (d(case["cams0"])[:, cam_perm], d(case["pts0"])[:, torch.tensor(case["pt_order"])])


# ---- the first damped linear system: oracle side ----------------------------------------------------------------------------------
def _blocks(M, r0, nr, dr, c0, nc, dc):
    """(B, n, n) -> (B, nr, nc, dr, dc): the blocks at rows r0 + dr * i, columns c0 + dc * j."""
    B = M.shape[0]
    return M[:, r0:r0 + nr * dr, c0:c0 + nc * dc].reshape(B, nr, dr, nc, dc).permute(0, 1, 3, 2, 4)


def oracle_system(case, problem=None, state=None, damping=None, v=None):
    """Everything check_first_system compares, from the oracle's dense A, b (fp64, CPU)."""
    if problem is None:
        problem, state = oracle_problem(case)
    lam = torch.from_numpy(case["damping"]).double() if damping is None else damping.double().cpu()
    C, Np = case["C"], case["Np"]
    nc = 6 * C
    A, b = problem.dense_linearize(state)
    AtA, Atb = opg.hessian(A, b)
    g = Atb[..., 0]
    Hd = opg.apply_damping(AtA, lam, True, 1e-8)
    Hpp_inv = torch.zeros_like(Hd[:, nc:, nc:])
    for k in range(Np):
        Hpp_inv[:, 3 * k:3 * k + 3, 3 * k:3 * k + 3] = torch.linalg.inv(Hd[:, nc + 3 * k:nc + 3 * k + 3, nc + 3 * k:nc + 3 * k + 3])
    Hcp = Hd[:, :nc, nc:]
    out = dict(g=g, diag=AtA.diagonal(dim1=1, dim2=2), err=problem.error_metric(state),
               Hcc=torch.stack([AtA[:, 6 * c:6 * c + 6, 6 * c:6 * c + 6] for c in range(C)], 1),
               Hpp=torch.stack([AtA[:, nc + 3 * k:nc + 3 * k + 3, nc + 3 * k:nc + 3 * k + 3] for k in range(Np)], 1),
               W=_blocks(AtA, 0, C, 6, nc, Np, 3), S=torch.tril(Hd[:, :nc, :nc] - Hcp @ Hpp_inv @ Hcp.transpose(1, 2)),
               rhs=g[:, :nc] - (Hcp @ Hpp_inv @ g[:, nc:].unsqueeze(2)).squeeze(2), delta=opg.solve(AtA, Atb, lam, True, 1e-8),
               damped=Hd, A=A)
    if v is not None:
        out["Av"] = (A @ v.double().cpu().unsqueeze(2)).squeeze(2)
    return out


def absent_blocks(case):
    """Camera pairs (c1 > c2, the linearization's numbering) that share neither a point nor a Between cost: S is zero there."""
    cpos = {c: k for k, c in enumerate(case["cam_order"])}
    seen = {}
    for c, p in zip(case["obs_cam"].tolist(), case["obs_pt"].tolist()):
        seen.setdefault(p, set()).add(cpos[c])
    linked = {(max(a, b), min(a, b)) for s in seen.values() for a in s for b in s}
    linked |= {(max(cpos[i], cpos[j]), min(cpos[i], cpos[j])) for i, j in case["cc_edges"].tolist()}
    return [(a, b) for a in range(case["C"]) for b in range(a) if (a, b) not in linked]


# ---- the first damped linear system: theseus_amd side ------------------------------------------------------------------------------
def _dense_S(solver, C):
    """tril of the reduced camera system (B, 6C, 6C) in the linearization's camera order, from either store of the solver: the
    dense frame, or (level mode) the block list -- the solver's camera order and the bit-30 transposition undone here."""
    if not solver.levels:
        return torch.tril(solver.S[:, :6 * C, :6 * C]).double().cpu().clone()
    s = solver.linearization.packed.structure
    K = s.num_blocks
    Sc = solver.Sc[:, :36 * (C + K)].reshape(-1, C + K, 6, 6).double().cpu()
    t = solver._level_t
    diag_blk, dst = t["diag_blk"].cpu().numpy(), t["blk_dst"].cpu().numpy()
    S = torch.zeros(Sc.shape[0], 6 * C, 6 * C, dtype=torch.float64)
    for c in range(C):
        S[:, 6 * c:6 * c + 6, 6 * c:6 * c + 6] = torch.tril(Sc[:, int(diag_blk[c])])
    c1, c2 = s.t["blk_c1"][:K].astype(np.int64), s.t["blk_c2"][:K].astype(np.int64)
    for k in range(K):
        blk = Sc[:, int(dst[k]) & 0x3fffffff]
        assert c1[k] > c2[k]
        S[:, 6 * c1[k]:6 * c1[k] + 6, 6 * c2[k]:6 * c2[k] + 6] = blk.transpose(1, 2) if (int(dst[k]) >> 30) & 1 else blk
    return S


def first_system(th, case, device="cpu", kernels=None, second_solve=False):
    """LevenbergMarquardt(max_iterations=1) on the case's objective: linearize, solve with the case's damping vector, Av.
    -> (dict of CPU fp64 tensors in the layout of ``oracle_system``, optimizer, objective).  ``second_solve``: after the first solve,
    move the variables (half the oracle-independent first step), linearize again and solve with the damping reversed: the entries
    ``S2`` / ``rhs2`` / ``delta2`` / ``state2`` / ``damping2`` are that second system's."""
    obj, cam_v, pt_v = build_objective(th, case, device)
    okw = dict(max_iterations=1, linear_solver_kwargs=dict(case["solver_kwargs"]) or None)
    if kernels is not None:
        okw["linearization_kwargs"] = dict(kernels=kernels)
    opt = th.LevenbergMarquardt(obj, **okw)
    solver, lin = opt.linear_solver, opt.linear_solver.linearization
    obj.update()
    lin.linearize()
    packed = lin.packed
    assert [v.name for v in packed.cam_vars] == [f"Cam{i}" for i in case["cam_order"]]
    assert [v.name for v in packed.pt_vars] == [f"Pt{i}" for i in case["pt_order"]]
    C, Np, B = case["C"], case["Np"], case["B"]
    cpu = lambda x: x.detach().double().cpu().clone()   # noqa: E731  (a copy on every device)
    bm = lambda x, *sh: cpu(x).permute(2, 0, 1).reshape(B, x.shape[0], *sh)   # noqa: E731  planar (N, comps, B) -> (B, N, ...)
    got = dict(g=cpu(lin.g), diag=cpu(lin.diag), err=cpu(obj.error_metric()), Hcc=bm(lin.Hcc, 6, 6))
    h = bm(lin.Hpp, 6)
    got["Hpp"] = torch.stack([torch.stack([h[..., 0], h[..., 1], h[..., 2]], -1), torch.stack([h[..., 1], h[..., 3], h[..., 4]], -1),
                              torch.stack([h[..., 2], h[..., 4], h[..., 5]], -1)], -2)
    O = case["obs_cam"].shape[0]
    W = bm(lin.W[:O], 6, 3)
    s = packed.structure
    got["W"] = torch.zeros(B, C, Np, 6, 3, dtype=torch.float64).index_put_(
        (torch.arange(B).view(B, 1), torch.from_numpy(s.t["obs_cam"][:O].astype(np.int64)).view(1, O),
         torch.from_numpy(s.t["obs_pt"][:O].astype(np.int64)).view(1, O)), W, accumulate=True)
    lam = torch.from_numpy(case["damping"]).to(lin.g.dtype).to(device)
    delta = solver.solve(damping=lam, ellipsoidal_damping=True, damping_eps=1e-8)
    got.update(S=_dense_S(solver, C), rhs=cpu(solver.rhs), delta=cpu(delta))
    v = torch.randn(B, lin.n, dtype=torch.float64, generator=torch.Generator().manual_seed(7)).to(lin.g.dtype)
    got["v"] = v.double()
    got["Av"] = cpu(lin.Av(v.to(device)))
    assert got["Av"].shape == (B, packed.m)
    if second_solve:
        p, state = oracle_problem(case)
        state2 = p.retract(state, 0.5 * got["delta"])
        cpos, ppos = {c: k for k, c in enumerate(case["cam_order"])}, {q: k for k, q in enumerate(case["pt_order"])}
        new = {f"Cam{i}": state2[0][:, cpos[i]].to(case["dtype"]).to(device).contiguous() for i in range(C)}
        new.update({f"Pt{i}": state2[1][:, ppos[i]].to(case["dtype"]).to(device).contiguous() for i in range(Np)})
        obj.update(new)
        lin.linearize()
        lam2 = lam.flip(0) * 3.0
        delta2 = solver.solve(damping=lam2, ellipsoidal_damping=True, damping_eps=1e-8)
        got.update(S2=_dense_S(solver, C), rhs2=cpu(solver.rhs), delta2=cpu(delta2), damping2=cpu(lam2),
                   state2=(torch.stack([cpu(v_.tensor) for v_ in packed.cam_vars], 1), torch.stack([cpu(v_.tensor) for v_ in packed.pt_vars], 1)),
                   S2_raw=None if solver.levels else cpu(solver.S))
    return got, opt, obj


# ---- bars (the issue's; none comes from the kernels' output) --------------------------------------------------------------------
FP64_BLOCK_BAR = 1e-11      # g, diag, Hcc, Hpp, W, S, rhs, Av: max|got - want| <= bar * max|want| (tests/test_gpu_ba.py's bar on g)
FP64_ERR_RTOL = 1e-12
FP64_DELTA_BAR = 1e-8       # * max(1, max|want|): tests/test_gpu_edge_cases.py; the damped system's condition number is <= 1e6
FP32_BAR = 3e-7             # one fp32 rounding of a value the kernels evaluate in fp64 registers (test_ba_first_linear_system_...)
MAX_COND = 1e6


def _rel(got, want):
    return ((got - want).abs().max() / want.abs().max()).item()


def compare(got, want, f32=False, log=None):
    """Assert the issue's bars on every array of the first system; ``log`` collects (name, measured, bar) for printing."""
    log = [] if log is None else log

    def check(name, g, w, bar, scale=None):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        sc = w.abs().max().item() if scale is None else scale
        d = (g - w).abs().max().item()
        log.append((name, d / sc if sc else d, bar))
        assert d <= bar * sc, f"{name}: max|got - want| = {d:.3e} > {bar:g} * {sc:.3e}"
    bar = FP32_BAR if f32 else FP64_BLOCK_BAR
    for k in ("g", "diag", "Hcc", "Hpp", "W", "S", "rhs"):
        check(k, got[k], want[k], bar)
    if f32:
        check("err", got["err"], want["err"], FP32_BAR)
    else:
        check("Av", got["Av"], want["Av"], FP64_BLOCK_BAR)
        np.testing.assert_allclose(got["err"].numpy(), want["err"].numpy(), rtol=FP64_ERR_RTOL)
        check("delta", got["delta"], want["delta"], FP64_DELTA_BAR, scale=max(1.0, want["delta"].abs().max().item()))
    return log


def compare_second_system(got, case, f32=False):
    """The system of the SECOND solve on one solver (first_system(second_solve=True)): re-linearised at a moved state, other
    damping.  S / rhs / delta against the oracle at that state, and the blocks of the dense frame that no cost fills -- zeroed once
    when the frame is allocated, or (blocks only Between costs fill) before every scatter-add -- exactly zero."""
    p, _ = oracle_problem(case)
    want = oracle_system(case, p, got["state2"], damping=got["damping2"])
    bar = FP32_BAR if f32 else FP64_BLOCK_BAR
    for k in ("S", "rhs"):
        d, sc = (got[k + "2"] - want[k]).abs().max().item(), want[k].abs().max().item()
        assert d <= bar * sc, f"second solve, {k}: max|got - want| = {d:.3e} > {bar:g} * {sc:.3e}"
    if not f32:
        d = (got["delta2"] - want["delta"]).abs().max().item()
        assert d <= FP64_DELTA_BAR * max(1.0, want["delta"].abs().max().item()), d
    absent = absent_blocks(case)
    assert absent
    for a, b in absent:
        assert not want["S"][:, 6 * a:6 * a + 6, 6 * b:6 * b + 6].any()
        assert not got["S2_raw"][:, 6 * a:6 * a + 6, 6 * b:6 * b + 6].any(), f"block ({a}, {b}) of S is not exactly zero"
    return want


def fp32_delta_ratio(got, want):
    """fp32 ``delta``: its distance from the exact solution in units of the distance of a CPU fp32 LAPACK Cholesky solve of the same
    damped system (cast to fp32).  -> (ratio, bound check passes)."""
    Hd, g, exact = want["damped"], want["g"], want["delta"]
    L = torch.linalg.cholesky(Hd.float())
    ref32 = torch.cholesky_solve(g.float().unsqueeze(2), L).squeeze(2).double()
    d_ref = (ref32 - exact).abs().max().item()
    d = (got["delta"] - exact).abs().max().item()
    return d / d_ref, d <= 4.0 * d_ref + 1e-6 * max(1.0, exact.abs().max().item())


def condition_number(want):
    return torch.linalg.cond(want["damped"]).max().item()


# ---- gradients: thx_ba_vjp / thx_ba_unroll_vjp / ba_vjp_grads against autograd through the oracle ---------------------------------
GRAD_BAR = 1e-10            # * max|want| per gradient array (the looser of the existing fp64 gradient bars)
_NAME_AUX = dict(feat="feat", w_obs="w_obs", focal="calib", k1="calib", k2="calib", log_radius="log_radius",
                 cam_prior_target="cam_prior_target", w_cam_prior="w_cam_prior", pt_prior_target="pt_prior_target",
                 w_pt_prior="w_pt_prior")


def _grad_check(name, got, want, log):
    got, want = got.detach().double().cpu(), want.double()
    if want.numel() == 0:                  # (no cost of this kind: the packer keeps an empty (0, 1, ...) tensor)
        assert got.numel() == 0, (name, got.shape)
        return
    assert got.shape == want.shape, (name, got.shape, want.shape)
    sc = want.abs().max().item()
    if sc == 0.0:
        assert not got.any(), f"{name}: the exact gradient is identically zero"
        log.append((name, 0.0, 0.0))
        return
    d = (got - want).abs().max().item()
    log.append((name, d / sc, GRAD_BAR))
    assert d <= GRAD_BAR * sc, f"{name}: max|got - want| = {d:.3e} > {GRAD_BAR:g} * {sc:.3e}"


def check_vjp(th, case, device="cpu", kernels=None):
    """K.ba_vjp, K.ba_unroll_vjp and ba_vjp_grads of the case's packed problem against the CPU stand-ins' autograd through the oracle
    (tests/oracle_kernels.py) on the same packed tensors.  -> [(name, measured, bar)]."""
    from tests.oracle_kernels import OracleKernels
    from theseus_amd import _lib
    from theseus_amd.ba import BAImplicitStep, ba_vjp_grads
    obj, _, _ = build_objective(th, case, device)
    okw = dict(max_iterations=1)
    if kernels is not None:
        okw["linearization_kwargs"] = dict(kernels=kernels)
    opt = th.LevenbergMarquardt(obj, **okw)
    lin = opt.linear_solver.linearization
    obj.update()
    lin.linearize()
    packed = lin.packed
    K, t, s = packed.K, packed.tensors, packed.structure
    B, n, C = case["B"], lin.n, case["C"]
    O, Kc, Kp = s.num_obs, s.num_cam_priors, s.num_pt_priors
    gen = torch.Generator().manual_seed(11)
    w, delta = torch.randn(B, n, dtype=torch.float64, generator=gen), 0.1 * torch.randn(B, n, dtype=torch.float64, generator=gen)
    lam = torch.from_numpy(case["damping"]).double()
    t_cpu = dataclasses.replace(t, **{f.name: getattr(t, f.name).detach().cpu() for f in dataclasses.fields(t)
                                      if isinstance(getattr(t, f.name), torch.Tensor)})
    s_cpu, ref = s.on("cpu"), OracleKernels()
    oc = torch.from_numpy(s.t["obs_cam"][:O].astype(np.int64))
    log = []

    def vjp_bufs(dev):
        new = lambda *sh: torch.zeros(*sh, dtype=torch.float64, device=dev)  # noqa: E731
        return dict(feat=new(max(O, 1), B, 2), w_obs=new(max(O, 1), B, 2), focal=new(max(O, 1), B), k1=new(max(O, 1), B),
                    k2=new(max(O, 1), B), log_radius=new(max(O, 1), B, 1) if t.robust_obs else None,
                    cam_prior_target=new(max(Kc, 1), B, 3, 4), w_cam_prior=new(max(Kc, 1), B, 6),
                    pt_prior_target=new(max(Kp, 1), B, 3), w_pt_prior=new(max(Kp, 1), B, 3))
    counts = dict(feat=O, w_obs=O, focal=O, k1=O, k2=O, log_radius=O, cam_prior_target=Kc, w_cam_prior=Kc, pt_prior_target=Kp,
                  w_pt_prior=Kp)
    per_cam = lambda g: torch.zeros(C, B, dtype=torch.float64).index_add_(0, oc, g[:O].double().cpu()).unsqueeze(2)  # noqa: E731
    got, want = vjp_bufs(device), vjp_bufs("cpu")
    K.ba_vjp(packed.dstruct, t, w.to(device).contiguous(), got)
    ref.ba_vjp(s_cpu, t_cpu, w, want)
    for k in BAImplicitStep.NAMES:
        if got[k] is None:
            continue
        if k in ("focal", "k1", "k2"):     # per observation in any split that sums to the camera's: compare per camera
            _grad_check("ba_vjp." + k, per_cam(got[k]), per_cam(want[k]), log)
        else:
            _grad_check("ba_vjp." + k, got[k][:counts[k]], want[k][:counts[k]], log)
    # ba_vjp_grads: the packed shapes -- summed over the batch for a batch-shared input, passed through for a batched one
    packed_grads = ba_vjp_grads(K, packed, t, w.to(device).contiguous())
    for k, g in zip(BAImplicitStep.NAMES, packed_grads):
        if g is None:
            continue
        full = per_cam(want[k]) if k in ("focal", "k1", "k2") else want[k][:counts[k]]
        nb = case["batch"][_NAME_AUX[k]]
        exp = full.sum(1, keepdim=True) if nb == 1 and B != 1 else full
        like = t.log_radius_obs if k == "log_radius" else getattr(t, k)
        assert tuple(g.shape) == tuple(like.shape), (k, g.shape, like.shape)
        _grad_check("ba_vjp_grads." + k, g, exp, log)

    def unroll_bufs(dev):
        new = lambda *sh: torch.zeros(*sh, dtype=torch.float64, device=dev)  # noqa: E731
        return dict(cam_obs=new(max(O, 1), B, 3, 4), pt_obs=new(max(O, 1), B, 3), feat=new(max(O, 1), B, 2), w_obs=new(max(O, 1), B, 2),
                    focal=new(max(O, 1), B), k1=new(max(O, 1), B), k2=new(max(O, 1), B),
                    log_radius_obs=new(max(O, 1), B, 1) if t.robust_obs else None,
                    cam_prior_cam=new(max(Kc, 1), B, 3, 4), cam_prior_target=new(max(Kc, 1), B, 3, 4), w_cam_prior=new(max(Kc, 1), B, 6),
                    pt_prior_pt=new(max(Kp, 1), B, 3), pt_prior_target=new(max(Kp, 1), B, 3), w_pt_prior=new(max(Kp, 1), B, 3))
    ucount = dict(cam_obs=O, pt_obs=O, feat=O, w_obs=O, focal=O, k1=O, k2=O, log_radius_obs=O, cam_prior_cam=Kc, cam_prior_target=Kc,
                  w_cam_prior=Kc, pt_prior_pt=Kp, pt_prior_target=Kp, w_pt_prior=Kp)
    assert set(ucount) == set(_lib.BA_UNROLL_GRADS)
    got, want = unroll_bufs(device), unroll_bufs("cpu")
    K.ba_unroll_vjp(packed.dstruct, t, w.to(device).contiguous(), delta.to(device).contiguous(), got, ell_damping=lam.to(device))
    ref.ba_unroll_vjp(s_cpu, t_cpu, w, delta, want, ell_damping=lam)
    for k in _lib.BA_UNROLL_GRADS:
        if got[k] is not None:
            _grad_check("ba_unroll_vjp." + k, got[k][:ucount[k]], want[k][:ucount[k]], log)
    return log
