"""CPU-side (-m "not gpu") checks of the multi-vector surface of the banded solver: header, library, ctypes table and INTEGRATION.md
agree on thx_pb_solve_multi / thx_pb_inverse_band; the entry points refuse bad arguments before any launch; samples and marginal
covariances of HipBandedCholeskySolver on the numpy stand-ins (tests/band_multi_oracle_kernels.py) against an fp64 inverse of the
linearization's AtA (``check_solver_surface``, which tests/test_gpu_band_multi.py runs on the device)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import traj2_common, trajse2_common
from tests.conftest import ROOT
from tests.helpers import load_golden
from tests.test_cabi_and_host import declared_symbols, lib_path  # noqa: F401  (lib_path: the session fixture that builds)

NAMES = {"thx_pb_solve_multi": 13, "thx_pb_inverse_band": 7}   # name: number of arguments
FAMILIES = {"traj2": (traj2_common, "BandMultiTraj2OracleKernels", 28), "trajse2": (trajse2_common, "BandMultiTrajSE2OracleKernels", 36)}


def test_header_library_ctypes_table_and_build_agree_on_the_two_names(lib_path):  # noqa: F811
    from theseus_amd import _lib, build as thx_build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "theseus_hip.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = ctypes.CDLL(lib_path)
    for name, nargs in NAMES.items():
        assert name in declared_symbols() and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and name in doc
        proto = re.search(rf"\b{name}\s*\(([^)]*)\)", header).group(1)
        assert len(proto.split(",")) == nargs == len(_lib._SIGNATURES[name])
    assert _lib.ABI_VERSION == 30 and "band_multi_kernels.hip" in thx_build.SOURCES


def test_bad_arguments_are_refused_before_any_launch(lib_path):  # noqa: F811
    from theseus_amd import _lib
    lib = _lib.load()
    one, two, three, four = (ctypes.c_void_p(a) for a in (16, 4096, 8192, 12288))
    lim = _lib.THX_BAND_MAX_KD

    def multi(Lb=one, n=6, kd=2, B=1, perm=two, rhs=three, x=four, nrhs=2, ldv=6, bstride=12, which=0, dtype=0):
        return lib.thx_pb_solve_multi(Lb, n, kd, B, perm, rhs, x, nrhs, ldv, bstride, which, dtype, None), lib.thx_last_error()

    def inverse(Lb=one, n=6, kd=2, B=1, Zb=two, dtype=0):
        return lib.thx_pb_inverse_band(Lb, n, kd, B, Zb, dtype, None), lib.thx_last_error()
    cases = [(multi, dict(Lb=None), b"null pointer"), (multi, dict(perm=None), b"null pointer"), (multi, dict(rhs=None), b"null pointer"),
             (multi, dict(x=None), b"null pointer"), (multi, dict(kd=-1), b"kd"), (multi, dict(kd=6), b"kd"),
             (multi, dict(n=100, kd=lim + 1, ldv=100, bstride=200), str(lim).encode()), (multi, dict(nrhs=0), b"nrhs < 1"),
             (multi, dict(ldv=5), b"ldv < n"), (multi, dict(bstride=11), b"bstride < nrhs * ldv"), (multi, dict(which=3), b"which"),
             (multi, dict(which=-1), b"which"), (multi, dict(dtype=7), b"dtype"),
             (inverse, dict(Lb=None), b"null pointer"), (inverse, dict(Zb=None), b"null pointer"), (inverse, dict(kd=-1), b"kd"),
             (inverse, dict(kd=6), b"kd"), (inverse, dict(n=100, kd=lim + 1), str(lim).encode()), (inverse, dict(dtype=7), b"dtype"),
             (inverse, dict(Zb=one), b"alias")]
    for fn, kw, text in cases:
        rc, err = fn(**kw)
        assert rc == -1 and text in err and (b"thx_pb_solve_multi" if fn is multi else b"thx_pb_inverse_band") in err, (kw, err)


def check_solver_surface(th, family, fixture, kernels, device):
    """Samples and marginal covariances of HipBandedCholeskySolver on a golden trajectory fixture against inv(AtA) in fp64 (two
    evaluations of the same maths in fp64: 1e-9 of the largest entry, as tests/test_gpu_band.py compares solvers) and against
    HipCholeskySolver.marginal_covariance on the same objective."""
    common, _, n = FAMILIES[family]
    kw = dict(linearization_kwargs=dict(kernels=kernels)) if kernels is not None else {}
    obj, _, _ = common.build(th, load_golden(fixture), device=device)
    solver, dense = th.HipBandedCholeskySolver(obj, **kw), th.HipCholeskySolver(obj, **kw)
    lin = solver.linearization
    obj.update()
    lin.linearize()
    dense.linearization.linearize()
    assert lin.n == n
    Hinv = torch.linalg.inv(lin.AtA.double().cpu())
    B, tol = Hinv.shape[0], 1e-9 * float(Hinv.abs().max())
    close = lambda a, want: float((a.double().cpu() - want).abs().max()) <= tol  # noqa: E731
    temperature, eye = 0.7, torch.eye(n, dtype=torch.float64, device=device)
    S = solver.sample_deltas(n, temperature, noise=eye)
    delta = solver.solve()
    assert tuple(S.shape) == (B, n, n)
    D = (S - delta.unsqueeze(2)).double().cpu()
    assert close(D @ D.transpose(1, 2) / temperature, Hinv)
    # which = 2 then 1 is which = 0, on the factor solve() left
    R = torch.randn(B, 3, n, dtype=torch.float64, generator=torch.Generator().manual_seed(0)).to(device)
    x0 = solver.solve_multi_with_factor(R, 0)
    assert close(x0, R.cpu() @ Hinv) and torch.equal(solver.solve_multi_with_factor(solver.solve_multi_with_factor(R, 2), 1), x0)
    names = [v.name for v in lin.ordering]
    every = solver.marginal_covariances()
    assert sorted(every) == sorted(names)
    for k, name in enumerate(names):
        c = slice(lin.var_start_cols[k], lin.var_start_cols[k] + lin.var_dims[k])
        assert close(every[name], Hinv[:, c, c]) and tuple(every[name].shape) == (B, lin.var_dims[k], lin.var_dims[k])
    pick = [names[-1], names[0], names[len(names) // 2]]                     # any set, any order: off-diagonal blocks too
    cols = [c for p in pick for c in range(lin.var_start_cols[names.index(p)], lin.var_start_cols[names.index(p)] + lin.var_dims[names.index(p)])]
    joint = solver.marginal_covariance(pick)
    assert close(joint, Hinv[:, cols][:, :, cols]) and close(dense.marginal_covariance(pick), joint.double().cpu())
    return obj, solver, delta


@pytest.mark.parametrize("family,fixture", [(f, fx) for f, v in FAMILIES.items() for fx in v[0].FIXTURES])
def test_samples_and_marginals_on_the_stand_in_kernels(family, fixture):
    import theseus_amd as th
    import tests.band_multi_oracle_kernels as oracle
    check_solver_surface(th, family, fixture, getattr(oracle, FAMILIES[family][1])(), "cpu")


def check_compute_samples(th, obj, solver, delta, kernels=None):
    """TheseusLayer.compute_samples with the banded solver: documented shapes, and the mean over the draw pair +-y (identity noise)
    of every variable whose tensor is as wide as its dof is the solved state x + delta."""
    lin = solver.linearization
    n = lin.n
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.HipBandedCholeskySolver,
                                **(dict(linearization_kwargs=dict(kernels=kernels)) if kernels is not None else {}))
    eye = torch.eye(n, dtype=delta.dtype, device=delta.device)
    out = th.TheseusLayer(opt).compute_samples(solver, 2 * n, 1.0, noise=torch.cat([eye, -eye], dim=1), return_dict=True)
    for k, v in enumerate(lin.ordering):
        assert tuple(out[v.name].shape) == (delta.shape[0], 2 * n, *v.tensor.shape[1:])
        if v.tensor.shape[1] == lin.var_dims[k]:
            want = v.tensor + delta[:, lin.var_start_cols[k]:lin.var_start_cols[k] + lin.var_dims[k]]
            np.testing.assert_allclose(out[v.name].mean(dim=1).cpu().numpy(), want.cpu().numpy(), rtol=0, atol=1e-9 * float(want.abs().max()))


def test_compute_samples_runs_with_the_banded_solver_on_the_stand_in_kernels(family="traj2"):
    """(traj2 only: compute_samples has no retraction for the mixed SE2 + velocity state of trajse2, with any solver)"""
    import theseus_amd as th
    import tests.band_multi_oracle_kernels as oracle
    K = getattr(oracle, FAMILIES[family][1])()
    obj, solver, delta = check_solver_surface(th, family, FAMILIES[family][0].FIXTURES[1], K, "cpu")
    check_compute_samples(th, obj, solver, delta, K)
