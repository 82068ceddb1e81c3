"""Builds libtheseus_hip.so (the C ABI of include/theseus_hip.h) with hipcc for gfx950, in-tree.

hipcc cross-compiles without a GPU.  The .so is git-ignored but travels to the GPU box with the
gpurun snapshot.  Usage:  python -m theseus_amd.build [--force]
"""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libtheseus_hip.so")
SOURCES = ["pg_kernels.hip", "chol_kernels.hip", "hblock_order.hip", "pg_vjp_kernels.hip", "block_kernels.hip", "pg2_kernels.hip", "ba_kernels.hip", "pgso3_kernels.hip", "pgso2_kernels.hip", "ba_vjp_kernels.hip", "vjp_unroll_ba_kernels.hip", "lu_kernels.hip", "multi_solve_kernels.hip", "traj_kernels.hip", "push_kernels.hip", "trajse2_kernels.hip", "homog_kernels.hip", "kin_kernels.hip", "dcem_kernels.hip", "band_kernels.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-pass-failed"]


def _mtime(p):
    return os.path.getmtime(p) if os.path.exists(p) else 0.0


def deps(path):
    """`path` and every file it reaches through `#include "..."` lines, each resolved against the including file's folder."""
    seen, todo = set(), [os.path.normpath(path)]
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        with open(f) as fh:
            for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', fh.read(), re.M):
                todo.append(os.path.normpath(os.path.join(os.path.dirname(f), inc)))
    return seen


def build(force: bool = False, verbose: bool = True) -> str:
    os.makedirs(LIBDIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(LIBDIR, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _mtime(o) < max(_mtime(d) for d in deps(s)):
            cmd = [hipcc, *FLAGS, "-c", s, "-o", o]
            if verbose:
                print("[theseus_amd.build]", " ".join(cmd), flush=True)
            subprocess.check_call(cmd)
    if force or _mtime(LIB) < max(_mtime(o) for o in objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-o", LIB, *objs]
        if verbose:
            print("[theseus_amd.build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
