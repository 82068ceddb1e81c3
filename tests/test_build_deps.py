"""CPU-side (-m "not gpu"), no compiler: theseus_amd/build.py rebuilds an object when anything its source reaches through
`#include "..."` is newer.  The dependency sets it computes are checked against an independent scan of the same files, so a header
that is added and not picked up (a stale library with no error) cannot go unnoticed."""
import glob
import os
import re

from theseus_amd import build

INCLUDE = re.compile(r'#\s*include\s*"([^"]+)"')


def reachable(path):
    """Every file `path` reaches through quoted includes (itself included), scanned without build.py's code."""
    found, frontier = {os.path.realpath(path)}, [os.path.realpath(path)]
    while frontier:
        here = frontier.pop()
        with open(here) as f:
            names = [m.group(1) for line in f for m in [INCLUDE.search(line.split("//")[0])] if m]
        for name in names:
            target = os.path.realpath(os.path.join(os.path.dirname(here), name))
            assert os.path.isfile(target), f"{here} includes {name}: no such file"
            if target not in found:
                found.add(target)
                frontier.append(target)
    return found


def deps_of(src):
    return {os.path.realpath(p) for p in build.deps(os.path.join(build.CSRC, src))}


def test_every_source_depends_on_all_it_includes():
    for src in build.SOURCES:
        got = deps_of(src)
        assert all(os.path.isfile(p) for p in got), (src, sorted(got))
        missing = reachable(os.path.join(build.CSRC, src)) - got
        assert not missing, (src, sorted(missing))


def test_no_orphan_headers():
    used = set().union(*(deps_of(src) for src in build.SOURCES))
    headers = {os.path.realpath(p) for p in glob.glob(os.path.join(build.CSRC, "*.cuh"))}
    assert headers and not headers - used, sorted(headers - used)


def test_cholesky_depends_on_its_headers_and_the_c_header():
    names = ["chol_base", "chol_engine", "chol_potrf", "chol_tiles", "chol_diag", "chol_offdiag_f32", "chol_offdiag_f64",
             "chol_solve", "chol_small"]
    want = {os.path.realpath(os.path.join(build.CSRC, n + ".cuh")) for n in names}
    want.add(os.path.realpath(os.path.join(build.HERE, "..", "include", "theseus_hip.h")))
    assert want <= deps_of("chol_kernels.hip"), sorted(want - deps_of("chol_kernels.hip"))
