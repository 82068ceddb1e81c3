"""Model of the regrouped fp32 column pairs (thx_hblock_layout.rg_*) from the REAL host tables: per pair the share of
the pair K-loop's 32x32 block products that the regrouped schedule leaves out, next to what the sub-block masks alone skip, and
the factor's K-loops in 128^3 tile products.  No GPU.
usage: python tools/model_row_groups.py [--poses 256] [--edges 1024] [--topology-seed 0]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def zero_solves(rg, m):
    """thx_chol_schedule.skip_zero_solves (RowGroups.zero_solve_model): per pair the substitution + coupling products and the K-loop
    products, today -> with every wave skipping what its strip's first chunk makes zero, and the leading zero sub-blocks per wave."""
    model = rg.zero_solve_model(m)
    print(f"{'pair':>5s} {'subst + coupling':>18s} {'K-loop':>14s}   leading zero 32-column sub-blocks per wave (of 8), group by group")
    tot = [0, 0, 0, 0]
    for j, r in model.items():
        zs = " ".join("[" + ",".join(str(v) for v in g) + "]" for g in r["z"]) or "natural tiles"
        print(f"j={j:<3d} {r['solve'][0]:>8d} -> {r['solve'][1]:<7d} {r['kloop'][0]:>6d} -> {r['kloop'][1]:<5d}   {zs}")
        tot = [a + b for a, b in zip(tot, r["solve"] + r["kloop"])]
    pct = lambda a, b: f"{100 * (b / a - 1):+.1f} %" if a else "-"   # noqa: E731
    print(f"all   {tot[0]:>8d} -> {tot[1]:<7d} {tot[2]:>6d} -> {tot[3]:<5d}   ({pct(tot[0], tot[1])} substitution + coupling, {pct(tot[2], tot[3])} K-loop)")
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=256)
    ap.add_argument("--edges", type=int, default=1024)
    ap.add_argument("--topology-seed", type=int, default=0)
    a = ap.parse_args()
    from theseus_amd.compiler import PoseGraphStructure
    from theseus_amd.utils.synthetic import pose_graph_topology
    hb = PoseGraphStructure.build(a.poses, pose_graph_topology(a.poses, a.edges, a.topology_seed), [0], dof=6).hessian_blocks()
    rg, m, nt = hb.row_groups(), hb.l_mask(), hb.ntiles
    if rg is None:
        print("no pair of this layout would start a K-loop late: no row groups")
        return
    zero_solves(rg, m)
    if rg.ngroups == 0:
        print("no pair of this layout would start a K-loop late: pair 0's groups only")
        return
    pop = lambda x: bin(int(x) & 15).count("1")   # noqa: E731
    per, total = rg.skipped_fraction(m)
    print(f"n = {6 * a.poses}, {nt} block columns, {rg.ngroups} groups, at most {rg.max_tile_pieces} pieces per (group, block column), "
          f"{int(np.diff(rg.tile_ptr).reshape(-1, 2).sum(1).max())} per group")
    print(f"{'pair':>5s} {'first chunks of the groups':40s} {'left out, regrouped':>20s} {'masks alone':>12s} {'column side':>12s}")
    all_p = today = cols_only = 0
    for jp in range(rg.npairs):
        j = 2 * jp
        cols = [pop(m[j, kc]) + pop(m[j + 1, kc]) for kc in range(4 * j)]
        allp = (nt - 2 - j) * 4 * j * 32
        run = sum(pop(m[i, kc]) * cols[kc] for i in range(j + 2, nt) for kc in range(4 * j))
        unif = sum(4 * cols[kc] for i in range(j + 2, nt) for kc in range(4 * j))
        k0 = rg.k0[rg.group_ptr[jp]:rg.group_ptr[jp + 1]].tolist()
        f = lambda x: f"{1 - x / allp:.3f}" if allp else "-"   # noqa: E731
        print(f"j={j:<3d} {str(k0) if k0 else 'natural tiles':40s} {per[j]:20.3f} {f(run):>12s} {f(unif):>12s}")
        all_p, today, cols_only = all_p + allp, today + run, cols_only + unif
    print(f"all pairs: {100 * total:.1f} % of the pair K-loop products left out (masks alone {100 * (1 - today / all_p):.1f} %, "
          f"of which {100 * (1 - cols_only / all_p):.1f} % on the column side)")
    # the factor's K-loops in 128^3 tile products, counted dense: per block column j the SYRK of the diagonal tile (j) and the
    # off-diagonal tiles' K-loops ((nt - 1 - j) j); substitutions and tile factorisations are not K-loop work
    kloops = sum(j + (nt - 1 - j) * j for j in range(nt))
    pair_k = all_p / 64.0              # of which in the pair kernel (a tile product = 4 chunks x 4 waves x 4 sub-blocks)
    print(f"K-loops of the factor: {kloops} tile products, {pair_k:.0f} of them in the pair kernel; left out {pair_k * total:.1f} "
          f"regrouped, {pair_k * (1 - today / all_p):.1f} by the masks alone: {kloops - pair_k * (1 - today / all_p):.1f} -> "
          f"{kloops - pair_k * total:.1f} executed ({100 * pair_k * (total - (1 - today / all_p)) / (kloops - pair_k * (1 - today / all_p)):.1f} % fewer)")
    # thx_chol_schedule.sort_pair_columns (PairColumns, thx_hblock_layout.sc_*): the pair's 256 columns sorted by first, 8 blocks of 32
    pc = hb.pair_columns()
    if pc is None:
        print("sorted pair columns: no pair has a table")
        return
    pcper, (ex_a, ex_b) = pc.executed_fraction(rg)
    print(f"{'pair':>5s} {'executed, regrouped':>20s} {'with sorted columns':>20s}   first chunks of the 8 sorted blocks")
    for j, (xa, xb) in pcper.items():
        fc = pc.first_chunk[j // 2].tolist() if pc.has[j // 2] else "no table"
        print(f"j={j:<3d} {xa:20.3f} {xb:20.3f}   {fc}")
    print(f"all pair K-loops: {ex_a:.3f} -> {ex_b:.3f} executed; {pair_k * (ex_a - ex_b):.1f} of the factor's {kloops - pair_k * total:.1f} "
          f"executed tile products left out")

if __name__ == "__main__":
    main()
