"""Bytes per problem that the dense-frame backward substitution (chol_bwd_kernel<T, false>) reads from L and the solve panels,
before and after the row-envelope path (thx_chol_solve_backward_env) -- from the host table thx_hblock_layout.row_first alone, no GPU.

before: every row of every strictly-lower tile in full, twelve whole 128 x 128 panels (at 256 poses).
after : of row r only the 16-byte groups that reach to or past row_first[r], and the ten lower 32 x 32 sub-blocks of every panel.
Counted in units of 16 bytes (the loads themselves), 64 bytes (an HBM sector) and 128 bytes (a cache line); rows of the frame start
on 512-byte boundaries (ld is a multiple of 128), so a row's segment touches ceil(end / G) - floor(start / G) units.

usage: python tools/model_solve_bytes.py [--poses 256 --edges 1024 --topology-seed 0]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TILE = 128


def solve_bytes(row_first: np.ndarray, es: int, gran: int):
    """(before, after) bytes per problem of L's strictly-lower tiles + the panels, element size ``es``, counted in ``gran``-byte units."""
    n = int(row_first.shape[0])
    nt = (n + TILE - 1) // TILE
    vec = 16 // es
    r = np.arange(n)
    end = (r // TILE) * TILE * es                          # a row's segment ends where its diagonal tile begins
    start_env = (np.minimum(row_first, (r // TILE) * TILE) // vec) * vec * es
    units = lambda s: int((-(-end // gran) - s // gran).sum()) * gran   # noqa: E731
    sub = 32 * es                                          # one sub-block row: a multiple of 128 bytes in both precisions
    panel_before, panel_after = nt * 16 * 32 * sub, nt * 10 * 32 * sub
    return units(np.zeros(n, np.int64)) + panel_before, units(start_env) + panel_after


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=256)
    ap.add_argument("--edges", type=int, default=1024)
    ap.add_argument("--topology-seed", type=int, default=0)
    a = ap.parse_args()
    from theseus_amd.compiler import PoseGraphStructure
    from theseus_amd.utils.synthetic import pose_graph_topology
    s = PoseGraphStructure.build(a.poses, pose_graph_topology(a.poses, a.edges, a.topology_seed), [0], dof=6)
    first = s.hessian_blocks().row_first.astype(np.int64)
    print(f"{a.poses} poses / {a.edges} edges (topology seed {a.topology_seed}): n = {first.shape[0]}")
    for name, es in (("fp32", 4), ("fp64", 8)):
        for gran in (16, 64, 128):
            before, after = solve_bytes(first, es, gran)
            print(f"{name} {gran:4d}-byte units: {before:10d} -> {after:10d} bytes per problem, ratio {after / before:.3f}")


if __name__ == "__main__":
    main()
