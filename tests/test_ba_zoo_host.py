"""The bundle-adjustment zoo (tests/ba_zoo_common.py) through the host path on the CPU: PackedBA / BAStructure / the Schur solver's
tables with the TEST stand-in kernels, against the oracle's dense A, b.  What runs here is every table the host builds on the odd
structures -- CSR lists, pair list, pair_dptr, block ranges, level-mode block destinations, the row tables of Av -- and the
generator's own conditions.  GPU twin (the HIP kernels on the same cases): tests/test_gpu_ba_zoo.py."""
import pytest
import torch

from tests import ba_zoo_common as zoo


def _kernels():
    from tests.oracle_kernels import OracleKernels
    from tests.test_ba_host import _LevelStandIns

    class K(_LevelStandIns, OracleKernels):
        pass
    return K()


@pytest.mark.parametrize("B", [3, 65])
@pytest.mark.parametrize("layout", list(zoo.LAYOUTS))
@pytest.mark.parametrize("topology", zoo.TOPOLOGIES)
def test_zoo_first_system_on_the_host(topology, layout, B):
    import theseus_amd as th
    case = zoo.make_case(topology, B, layout, robust="huber")
    # the generator's conditions (make_case asserts depth / shares too; stated here with their figures)
    assert zoo.min_depth(case) >= zoo.MIN_DEPTH
    inside, outside = zoo.radius_shares(case)
    assert inside >= 0.2 and outside >= 0.2, (inside, outside)
    assert {case[k].shape[0] for a in zoo.AUX for k in zoo.AUX_KEYS[a]} == ({1} if layout == "shared" or B == 1 else
                                                                              {B} if layout == "batched" else {1, B})
    second = topology in ("two_islands", "odometry")
    got, opt, _ = zoo.first_system(th, case, "cpu", _kernels(), second_solve=second)
    want = zoo.oracle_system(case, v=got["v"])
    cond = zoo.condition_number(want)
    assert cond <= zoo.MAX_COND, cond
    zoo.compare(got, want)
    solver = opt.linear_solver
    s = solver.linearization.packed.structure
    assert solver.levels == (topology == "levels")
    if topology == "levels":
        dst = solver._level_t["blk_dst"].numpy()
        assert ((dst >> 30) & 1).any() and not ((dst >> 30) & 1).all()
    if topology == "lonely_camera":
        lonely = case["cam_order"].index(2)
        assert s.t["cam_ptr"][lonely] == s.t["cam_ptr"][lonely + 1] and s.t["pair_ptr"][lonely] == s.t["pair_ptr"][lonely + 1]
    if topology == "single_view_points":
        assert s.num_pairs == sum(n * (n + 1) // 2 for n in [1] * 9 + [5] + [2 + (p % 2) for p in range(10, 18)])
    if topology == "no_priors_but_one":
        assert (s.num_cam_priors, s.num_pt_priors) == (1, 0)
    if topology in ("two_islands", "odometry"):
        pos = {c: k for k, c in enumerate(case["cam_order"])}
        cross = {(max(pos[a], pos[b]), min(pos[a], pos[b])) for a in (0, 1, 2) for b in (3, 4, 5)}
        assert not cross & set(zip(s.t["blk_c1"].tolist(), s.t["blk_c2"].tolist()))
        zoo.compare_second_system(got, case)
    if topology == "odometry":
        assert solver._odo_only and solver._odo_only[0].shape[0] == 2     # (3, 2) and (2, 5) share no point


# ---- the comparison can reveal a wrong stride / a wrong width ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def batched_regular():
    import theseus_amd as th
    case = zoo.make_case("regular", 65, "batched", robust="huber")
    got, _, _ = zoo.first_system(th, case, "cpu", _kernels())
    zoo.compare(got, zoo.oracle_system(case, v=got["v"]))
    return case, got


@pytest.mark.parametrize("field", ["feat", "w_obs", "focal", "log_radius_obs", "cam_prior_target", "w_cam_prior", "pt_prior_target",
                                   "w_pt_prior"])
def test_comparison_fails_when_batch_items_0_and_64_of_one_auxiliary_are_swapped(batched_regular, field):
    case, got = batched_regular
    p, state = zoo.oracle_problem(case)
    x = getattr(p, field).clone()
    x[[0, 64]] = x[[64, 0]]
    wrong, _ = zoo.oracle_problem(case, **{field: x})
    with pytest.raises(AssertionError):
        zoo.compare(got, zoo.oracle_system(case, wrong, state, v=got["v"]))


def test_comparison_fails_when_the_components_of_w_obs_are_swapped(batched_regular):
    case, got = batched_regular
    p, state = zoo.oracle_problem(case)
    wrong, _ = zoo.oracle_problem(case, w_obs=p.w_obs.flip(-1))
    with pytest.raises(AssertionError):
        zoo.compare(got, zoo.oracle_system(case, wrong, state, v=got["v"]))


def test_gradient_helper_runs_on_the_stand_in():
    """check_vjp's plumbing (buffers, counts, the packed shapes of ba_vjp_grads in both directions of its batch reduction) with the
    stand-in on both sides; the HIP kernels take the first side in tests/test_gpu_ba_zoo.py."""
    import theseus_amd as th
    from tests.oracle_kernels import OracleKernels
    for topology, layout in (("lonely_camera", "mixed_a"), ("no_priors_but_one", "mixed_b")):
        log = zoo.check_vjp(th, zoo.make_case(topology, 3, layout, robust="huber"), "cpu", OracleKernels())
        assert len(log) >= 20 and all(torch.isfinite(torch.tensor(m)) for _, m, _ in log)
