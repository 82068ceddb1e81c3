"""-m gpu: the bundle-adjustment kernels (thx_ba_assemble, thx_ba_schur / thx_ba_schur_blocks, thx_ba_backsub, thx_ba_error, thx_ba_av,
thx_ba_vjp, thx_ba_unroll_vjp) on the zoo of tests/ba_zoo_common.py against the fp64 oracle (oracle/ba.py) on the CPU: more than
one wave of problems along the batch axis (B = 65, 130), each of the eight auxiliary batch strides in both states, DiagonalCostWeight
/ per-observation radii with distinct values, and the odd structures the packer has code for.  Host twin: tests/test_ba_zoo_host.py.

Bars (tests/ba_zoo_common.py, none derived from the kernels' output): fp64 blocks 1e-11 * max|want|, error metric rtol 1e-12, delta
1e-8 * max(1, |want|) at an asserted condition number <= 1e6, gradients 1e-10 * max|want|; fp32 3e-7 * max|exact| against the oracle on
the fp32-rounded inputs, delta within 4x the distance of a CPU fp32 LAPACK solve of the same system (+ 1e-6 * max(1, |exact|))."""
import pytest
import torch

from tests import ba_zoo_common as zoo
from tests.helpers import f32_thresholds

pytestmark = pytest.mark.gpu


def check_first_system(case):
    import theseus_amd as th
    f32 = case["dtype"] == torch.float32
    second = case["topology"] in ("two_islands", "odometry")
    got, opt, _ = zoo.first_system(th, case, "cuda", second_solve=second)
    solver = opt.linear_solver
    assert type(solver).__name__ == "HipSchurSolver" and solver.levels == (case["topology"] == "levels")
    if solver.levels:
        dst = solver._level_t["blk_dst"].cpu().numpy()
        assert ((dst >> 30) & 1).any()
    assert int(solver.info.abs().sum()) == 0
    if f32:
        with f32_thresholds():
            want = zoo.oracle_system(case, v=got["v"])
    else:
        want = zoo.oracle_system(case, v=got["v"])
    cond = zoo.condition_number(want)
    assert cond <= zoo.MAX_COND, cond
    log = []
    try:
        zoo.compare(got, want, f32=f32, log=log)
    finally:
        print(f"[BA zoo {case['topology']} {case['layout']} B={case['B']} {case['robust'] or 'none'} {'f32' if f32 else 'f64'}] cond {cond:.1e}; "
              + ", ".join(f"{k} {m:.1e}" for k, m, _ in log))
    if f32:
        ratio, ok = zoo.fp32_delta_ratio(got, want)
        print(f"[BA zoo fp32 delta] {case['topology']} {case['layout']} B={case['B']}: |delta - exact| / |fp32 LAPACK - exact| = {ratio:.3f}")
        assert ok, ratio
    if second:
        if f32:
            with f32_thresholds():
                zoo.compare_second_system(got, case, f32=True)
        else:
            zoo.compare_second_system(got, case)


_FIRST_F64 = ([(t, 65, "mixed_a", "huber") for t in zoo.TOPOLOGIES]
              + [("regular", B, layout, "huber") for layout in zoo.LAYOUTS for B in (1, 65, 130) if (B, layout) != (65, "mixed_a")]
              + [("regular", 65, "batched", r) for r in ("", "welsch", "huber+flatten")]
              + [("odometry", 65, "mixed_b", "huber"), ("levels", 65, "mixed_b", "huber")])


@pytest.mark.parametrize("topology,B,layout,robust", _FIRST_F64, ids=lambda v: str(v) if v != "" else "none")
def test_zoo_first_system_fp64(topology, B, layout, robust):
    check_first_system(zoo.make_case(topology, B, layout, robust=robust, dtype=torch.float64))


@pytest.mark.parametrize("topology", ["regular", "single_view_points", "levels"])
def test_zoo_first_system_fp32(topology):
    check_first_system(zoo.make_case(topology, 65, "mixed_b", robust="huber", dtype=torch.float32))


@pytest.mark.parametrize("topology,layout", [("regular", "shared"), ("regular", "batched"), ("regular", "mixed_a"), ("regular", "mixed_b"),
                                             ("lonely_camera", "mixed_a"), ("no_priors_but_one", "batched"), ("odometry", "mixed_b")])
def test_zoo_vjp_fp64(topology, layout):
    import theseus_amd as th
    case = zoo.make_case(topology, 65, layout, robust="huber", dtype=torch.float64)
    log = []
    try:
        log = zoo.check_vjp(th, case, "cuda")
    finally:
        print(f"[BA zoo vjp {topology} {layout}] worst {max((m for _, m, _ in log), default=float('nan')):.1e} of {len(log)} arrays")
