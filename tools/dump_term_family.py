"""What the fused cost families compute, to a file -- for a before / after comparison of a change that must not move a bit: J, e of
thx_traj2_eval / thx_push2_eval and the metric of thx_traj2_error / thx_push2_error, in fp32 and fp64, at the committed fixtures of
both families and at one seeded random problem each (the sizes of tests/test_gpu_traj2.py / tests/test_gpu_push2.py).

    python tools/dump_term_family.py --out a.pt [--root <another checkout of this repository>]
    python tools/dump_term_family.py --compare a.pt b.pt        # torch.equal on every array; exit status 1 on any difference
"""
import argparse
import os
import sys

import torch


def dump(out):
    import theseus_amd as th
    from tests import push2_common, traj2_common
    from tests.helpers import load_golden
    cases = [(f, traj2_common, load_golden(f), {}) for f in traj2_common.FIXTURES]
    cases.append(("traj2_random_B70_N40", traj2_common, traj2_common.random_problem(70, 40, seed=5), dict(N=40)))
    cases += [(f, push2_common, load_golden(f), {}) for f in push2_common.FIXTURES]
    cases.append(("push2_random_B70_T12", push2_common, push2_common.random_problem(70, 12, seed=5), dict(T=12)))
    arrays = {}
    for name, common, data, kw in cases:
        for dtype in (torch.float32, torch.float64):
            obj = common.build(th, data, device="cuda", dtype=dtype, **kw)[0]
            packed = th.HipLinearization(obj).packed
            packed._eval()
            tag = f"{name}/{type(packed).__name__}/{str(dtype).split('.')[1]}"
            arrays[tag + "/J"], arrays[tag + "/e"] = packed._J.cpu().clone(), packed._e.cpu().clone()
            arrays[tag + "/metric"] = packed.error_metric().cpu().clone()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    torch.save(arrays, out)
    print(f"{len(arrays)} arrays of {os.path.dirname(th.__file__)} -> {out}")


def compare(a, b):
    A, B = torch.load(a), torch.load(b)
    bad = sorted(set(A) ^ set(B))
    for k in sorted(set(A) & set(B)):
        same = A[k].dtype == B[k].dtype and A[k].shape == B[k].shape and torch.equal(A[k], B[k])
        finite = bool(torch.isfinite(A[k]).all())
        print(f"{'equal    ' if same else 'DIFFERENT'} {k:70s} {str(tuple(A[k].shape)):14s} finite={finite} max|.|={float(A[k].abs().max()):.6g}")
        if not same:
            bad.append(k)
    print(f"{len(A)} / {len(B)} arrays, {len(bad)} differ or are missing on one side" + (": " + ", ".join(bad) if bad else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--compare", nargs=2)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    sys.path.insert(0, os.path.abspath(a.root))
    dump(a.out)
