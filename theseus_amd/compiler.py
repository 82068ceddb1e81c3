"""Problem compiler: objective structure -> int32 index tables for the HIP kernels.

Runs once per objective (host side, numpy).  Structure parity with the reference is bit exact:
column layout = variable order * dof (``Linearization.var_start_cols``,
theseus/optimizer/linearization.py:31-41, default ``VariableOrdering`` = insertion order,
theseus/optimizer/variable_ordering.py:19-27) and row layout = cost-function add order
(theseus/optimizer/dense_linearization.py:41-56).
"""
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

DOF = 6


@dataclass
class PoseGraphStructure:
    """Immutable topology of a pose graph (SE3: dof 6, SE2: dof 3): P poses, E Between edges, K Difference priors."""

    num_poses: int
    edge_i: np.ndarray  # (E,) int32  v0 pose of edge e
    edge_j: np.ndarray  # (E,) int32  v1 pose of edge e
    prior_pose: np.ndarray  # (K,) int32
    # row start (in A / b / error vector) of every cost, in add order
    edge_row_start: np.ndarray = None  # (E,) int64
    prior_row_start: np.ndarray = None  # (K,) int64
    # derived CSR tables
    inc_ptr: np.ndarray = field(default=None, repr=False)
    inc_edge: np.ndarray = field(default=None, repr=False)
    inc_side: np.ndarray = field(default=None, repr=False)
    inc_other: np.ndarray = field(default=None, repr=False)
    pri_ptr: np.ndarray = field(default=None, repr=False)
    pri_id: np.ndarray = field(default=None, repr=False)
    _dev: dict = field(default_factory=dict, repr=False)
    dof: int = DOF

    @staticmethod
    def build(num_poses: int, edges: Sequence[Tuple[int, int]], priors: Sequence[int],
              edge_row_start: Optional[Sequence[int]] = None,
              prior_row_start: Optional[Sequence[int]] = None, dof: int = DOF) -> "PoseGraphStructure":
        P = int(num_poses)
        e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
        E = e.shape[0]
        pr = np.asarray(priors, dtype=np.int64).reshape(-1)
        K = pr.shape[0]
        if E and (e.min() < 0 or e.max() >= P):
            raise ValueError("edge endpoint out of range")
        if K and (pr.min() < 0 or pr.max() >= P):
            raise ValueError("prior pose out of range")
        if E and np.any(e[:, 0] == e[:, 1]):
            raise ValueError("Between cost with v0 is v1 (self loop) is not supported")
        if edge_row_start is None:
            edge_row_start = dof * np.arange(E)
        if prior_row_start is None:
            prior_row_start = dof * (E + np.arange(K))
        # incident-edge CSR per pose, entries sorted by (other endpoint, edge id)
        ent_pose = np.concatenate([e[:, 0], e[:, 1]])
        ent_other = np.concatenate([e[:, 1], e[:, 0]])
        ent_edge = np.concatenate([np.arange(E), np.arange(E)])
        ent_side = np.concatenate([np.zeros(E, np.int64), np.ones(E, np.int64)])
        order = np.lexsort((ent_edge, ent_other, ent_pose))
        inc_ptr = np.zeros(P + 1, np.int64)
        np.add.at(inc_ptr, ent_pose + 1, 1)
        inc_ptr = np.cumsum(inc_ptr)
        porder = np.argsort(pr, kind="stable")
        pri_ptr = np.zeros(P + 1, np.int64)
        np.add.at(pri_ptr, pr + 1, 1)
        pri_ptr = np.cumsum(pri_ptr)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
        return PoseGraphStructure(
            num_poses=P, edge_i=i32(e[:, 0]), edge_j=i32(e[:, 1]), prior_pose=i32(pr),
            edge_row_start=np.asarray(edge_row_start, np.int64), prior_row_start=np.asarray(prior_row_start, np.int64),
            inc_ptr=i32(inc_ptr), inc_edge=i32(ent_edge[order]), inc_side=i32(ent_side[order]),
            inc_other=i32(ent_other[order]), pri_ptr=i32(pri_ptr), pri_id=i32(porder), dof=int(dof),
        )

    # ---- sizes -------------------------------------------------------------------------------
    @property
    def num_edges(self) -> int:
        return int(self.edge_i.shape[0])

    @property
    def num_priors(self) -> int:
        return int(self.prior_pose.shape[0])

    @property
    def num_cols(self) -> int:
        return self.dof * self.num_poses

    @property
    def num_rows(self) -> int:
        return self.dof * (self.num_edges + self.num_priors)

    @property
    def var_start_cols(self) -> List[int]:
        return [self.dof * k for k in range(self.num_poses)]

    def lower_block_pattern(self) -> np.ndarray:
        """(nblocks, 2) sorted unique (row pose, col pose) of the non-zero 6x6 blocks of tril(H)."""
        blocks = {(p, p) for p in range(self.num_poses)}
        for i, j in zip(self.edge_i.tolist(), self.edge_j.tolist()):
            blocks.add((max(i, j), min(i, j)))
        return np.array(sorted(blocks), dtype=np.int64)

    def hessian_blocks(self) -> "HessianBlocks":
        """Block-compact layout of tril(H) for this structure (built once)."""
        hb = self._dev.get("__hblocks__")
        if hb is None:
            hb = self._dev["__hblocks__"] = HessianBlocks(self)
        return hb

    # ---- device side ---------------------------------------------------------------------------
    def on(self, device) -> "DeviceStructure":
        key = str(device)
        if key not in self._dev:
            self._dev[key] = DeviceStructure(self, device)
        return self._dev[key]


class DeviceStructure:
    """The int32 tables on one device + the ctypes struct that points at them."""

    _FIELDS = ["edge_i", "edge_j", "inc_ptr", "inc_edge", "inc_side", "inc_other", "prior_pose", "pri_ptr", "pri_id"]

    def __init__(self, s: PoseGraphStructure, device):
        self.host = s
        self.device = torch.device(device)
        self.t = {}
        for f in self._FIELDS:
            a = getattr(s, f)
            if a.size == 0:
                a = np.zeros(1, np.int32)  # keep a valid pointer
            self.t[f] = torch.from_numpy(a.copy()).to(self.device)
        c = _lib.PGStructure()
        c.num_poses, c.num_edges, c.num_priors = s.num_poses, s.num_edges, s.num_priors
        for f in self._FIELDS:
            setattr(c, f, self.t[f].data_ptr())
        self.c = c


TILE = _lib.THX_TILE


class HessianBlocks:
    """Block-compact storage of tril(H) (include/theseus_hip.h: thx_hblock_layout): the non-zero dof x dof blocks -- one per
    variable (diagonal) and one per connected variable pair -- ordered by the 128 x 128 Cholesky tile of their top-left element,
    then by (row variable, column variable), so that the blocks of a tile are one contiguous run of the list; per lower tile the
    PIECES that fall into it (a block straddles up to four tiles: 128 is not a multiple of 6)."""

    def __init__(self, s: PoseGraphStructure):
        d, P = s.dof, s.num_poses
        pat = s.lower_block_pattern()                                   # (nb, 2) sorted by (p, q), q <= p
        p, q = pat[:, 0], pat[:, 1]
        order = np.lexsort((q, p, (d * q) // TILE, (d * p) // TILE))    # by (tile row, tile col, p, q)
        self.blocks = pat[order]
        self.nblocks, self.bd, self.nvars = int(pat.shape[0]), d, P
        self.ntiles = (d * P + TILE - 1) // TILE
        ident = {(int(a), int(b)): k for k, (a, b) in enumerate(self.blocks.tolist())}
        self.diag_blk = np.array([ident[(k, k)] for k in range(P)], dtype=np.int32)
        pose_of_entry = np.repeat(np.arange(P), np.diff(s.inc_ptr))
        self.inc_blk = np.array([ident[(int(a), int(o))] if o < a else -1 for a, o in zip(pose_of_entry.tolist(), s.inc_other.tolist())],
                                dtype=np.int32)
        # pieces per lower tile t = i (i + 1) / 2 + j
        per_tile = [[] for _ in range(self.ntiles * (self.ntiles + 1) // 2)]
        for k, (a, b) in enumerate(self.blocks.tolist()):
            r, c = d * a, d * b
            for ti in sorted({r // TILE, (r + d - 1) // TILE}):
                for tj in sorted({c // TILE, (c + d - 1) // TILE}):
                    if tj > ti:
                        continue   # (the part of a straddling DIAGONAL block above the tile diagonal: never read)
                    per_tile[ti * (ti + 1) // 2 + tj].append((k, r - TILE * ti, c - TILE * tj))
        self.tile_ptr = np.zeros(len(per_tile) + 1, dtype=np.int32)
        self.tile_ptr[1:] = np.cumsum([len(x) for x in per_tile])
        flat = [x for lst in per_tile for x in lst]
        self.piece_blk = np.array([x[0] for x in flat], dtype=np.int32)
        self.piece_rc = np.array([((x[1] & 0xFFFF) << 16) | (x[2] & 0xFFFF) for x in flat], dtype=np.int64).astype(np.uint32).view(np.int32)
        self.elems = self.nblocks * d * d
        self.bstride = (self.elems + 3) // 4 * 4     # elements per problem (16-byte aligned in fp32)
        # (n) first non-zero column of every row of H -- and of L, which fills inside the envelope of H only (thx_hblock_layout.row_first)
        firstp = np.arange(P)
        np.minimum.at(firstp, p, q)
        self.row_first = np.repeat(d * firstp, d).astype(np.int32)
        self._dev = {}
        self._l_mask = None
        self._row_groups = None
        self._pair_columns = None
        self._tile_rows = None

    def l_mask(self) -> np.ndarray:
        """(ntiles, 4 * ntiles) int32: bit s of [t, c] set when the 32x32 sub-block (rows 128 t + 32 s, columns 32 c) of the
        natural-order Cholesky factor can be non-zero (thx_hblock_fill_mask, host only)."""
        if self._l_mask is None:
            self._l_mask = _lib.hblock_fill_mask(self.blocks, self.nvars, self.bd)
        return self._l_mask

    def row_groups(self) -> Optional["RowGroups"]:
        """The regrouped rows of the fp32 column pairs (thx_hblock_layout.rg_*), None when no pair would start a K-loop late and
        pair 0 has no strip of rows that begins behind column 32."""
        if self._row_groups is None:
            rg = RowGroups(self)
            self._row_groups = rg if rg.ngroups > 0 or rg.ngroups0 > 0 else False
        return self._row_groups or None

    def pair_columns(self) -> Optional["PairColumns"]:
        """The sorted columns of the fp32 column pairs (thx_hblock_layout.sc_*), None when no pair has a table."""
        if self._pair_columns is None:
            pc = PairColumns(self, self.row_groups())
            self._pair_columns = pc if pc.npairs_sorted > 0 else False
        return self._pair_columns or None

    def tile_rows(self) -> Optional["TileRows"]:
        """The sorted rows of the diagonal tiles (thx_hblock_layout.tr_*), None when the layout has no row groups above a pair
        (regroup_rows cannot apply) or no tile has a table."""
        if self._tile_rows is None:
            rg = self.row_groups()
            tr = TileRows(self) if rg is not None and rg.ngroups > 0 else None
            self._tile_rows = tr if tr is not None and tr.ntables > 0 else False
        return self._tile_rows or None

    def on(self, device) -> "DeviceHessianBlocks":
        key = str(device)
        if key not in self._dev:
            self._dev[key] = DeviceHessianBlocks(self, device)
        return self._dev[key]

    # ---- host-side reference of the layout (tests) ---------------------------------------------------------------
    def pack_dense(self, H: np.ndarray) -> np.ndarray:
        """(B, >= n, >= n) dense (lower) -> (B, bstride) block list."""
        B, d = H.shape[0], self.bd
        out = np.zeros((B, self.bstride), dtype=H.dtype)
        for k, (a, b) in enumerate(self.blocks.tolist()):
            out[:, k * d * d:(k + 1) * d * d] = H[:, d * a:d * a + d, d * b:d * b + d].reshape(B, -1)
        return out

    def expand(self, Hc: np.ndarray, ld: int) -> np.ndarray:
        """(B, bstride) -> dense (B, ld, ld) the way the device kernels gather it: tile by tile, piece by piece."""
        B, d = Hc.shape[0], self.bd
        H = np.zeros((B, ld, ld), dtype=Hc.dtype)
        for ti in range(self.ntiles):
            for tj in range(ti + 1):
                t = ti * (ti + 1) // 2 + tj
                for pc in range(self.tile_ptr[t], self.tile_ptr[t + 1]):
                    rc = int(self.piece_rc[pc]) & 0xFFFFFFFF
                    r0, c0 = np.array(rc >> 16, dtype=np.uint16).view(np.int16), np.array(rc & 0xFFFF, dtype=np.uint16).view(np.int16)
                    blk = Hc[:, self.piece_blk[pc] * d * d:(self.piece_blk[pc] + 1) * d * d].reshape(B, d, d)
                    for e in range(d * d):
                        r, c = int(r0) + e // d, int(c0) + e % d
                        if 0 <= r < TILE and 0 <= c < TILE and TILE * ti + r < ld and TILE * tj + c < ld:
                            H[:, TILE * ti + r, TILE * tj + c] = blk[:, e // d, e % d]
        return H


class RowGroups:
    """Rows below every fp32 column pair regrouped by their first non-zero column (thx_hblock_layout.rg_*).

    Row r of the natural-order factor is zero left of ``first[r]``, the first non-zero column of row r of H (L fills inside the
    envelope of H only).  In the column-pair kernel every row of L is independent, so the rows below pair (j, j + 1) -- j even,
    j + 2 < ntiles -- need not be dealt to workgroups tile by tile: they are sorted by ``first`` (stable: a variable's rows stay
    adjacent and in order), cut into groups of 128, and a group's K-loop starts at chunk ``k0 = min(min first // 32, 4 j)``.
    The rows of a variable that the pair's lower edge cuts (128 is no multiple of 6) move up to slot 0 of their group -- or of
    the nearest group before it whose slot 0 no straddling variable holds -- so that the missing part of its blocks falls in
    front of slot 0 and is clipped like any straddling piece.  A pair whose groups all start at chunk 0 keeps its natural tiles
    (no groups).

    group_ptr  (npairs + 1)      groups of pair j / 2: [group_ptr[j / 2], group_ptr[j / 2 + 1])
    rows       (ngroups, 128)    matrix row of every slot, -1 behind the last row
    k0         (ngroups)         first 32-column chunk of the group's K-loop
    tile_ptr   (2 ngroups + 1)   pieces of (group g, column tile j + s): [tile_ptr[2 g + s], tile_ptr[2 g + s + 1])
    piece_blk, piece_rc          as HessianBlocks', the row relative to the group's slot 0
    zf         (ngroups, 4)      per 32-slot strip (= wave of the workgroup) min first // 32, NOT capped (a strip without rows:
                                 4 j + 8): what of the strip's substitutions and coupling is a product with zeros
                                 (thx_chol_schedule.skip_zero_solves)

    Pair 0 has no K-loop and keeps group_ptr[0:2] == 0; its rows, sorted and cut the same way, are in tables of their own --
    ngroups0, rows0, zf0, tile_ptr0, piece_blk0, piece_rc0, max_tile_pieces0 -- present when some strip begins behind chunk 0.
    """

    def __init__(self, hb: "HessianBlocks"):
        d, P, nt = hb.bd, hb.nvars, hb.ntiles
        n = d * P
        by_row = [[] for _ in range(P)]
        for k, (a, b) in enumerate(hb.blocks.tolist()):
            by_row[a].append((b, k))
        self.first = hb.row_first.astype(np.int64)      # (n) first non-zero column of every row of H (and of L)
        self.npairs = max(0, (nt - 1) // 2)
        group_ptr, rows, k0s, zfs, tile_ptr, pblk, prc = [0], [], [], [], [0], [], []
        self.max_tile_pieces = 0

        def sorted_rows(j):
            r0 = (j + 2) * TILE
            rr = np.arange(r0, n)
            srows = rr[np.argsort(self.first[rr], kind="stable")]
            if r0 % d:   # the variable cut by the pair's lower edge: nothing may sit in the slots in front of its rows
                head = srows // d == r0 // d
                g = int(np.argmax(head)) // TILE
                while g > 0 and not head[TILE * g] and srows[TILE * g] % d:   # (a variable straddling into group g has its slot 0)
                    g -= 1
                rest = srows[~head]
                cut = int((~head[:TILE * g]).sum())
                srows = np.concatenate([rest[:cut], srows[head], rest[cut:]])
            assert self._slots_ok(srows, d)
            return srows

        def strip_chunks(slots, j):   # per 32-slot strip (= wave) min first // 32, uncapped; a strip without rows: behind the pair
            return [int(self.first[slots[s:s + 32]].min()) // 32 if slots.size > s else 4 * j + 8 for s in range(0, TILE, 32)]

        def add_group(slots, j, rows, tile_ptr, pblk, prc):   # -> the largest piece count of (this group, one block column)
            rows.append(np.concatenate([slots, np.full(TILE - slots.size, -1)]))
            pose = slots // d
            starts = [s for s in range(slots.size) if s == 0 or pose[s] != pose[s - 1]]
            most = 0
            for tj in (j, j + 1):
                cnt = 0
                for s in starts:
                    s0 = s - int(slots[s]) % d       # slot of the variable's row 0 (negative: it starts in the group before)
                    for q, k in by_row[int(pose[s])]:
                        c0 = d * q - TILE * tj
                        if c0 + d > 0 and c0 < TILE:
                            pblk.append(k)
                            prc.append(((s0 & 0xFFFF) << 16) | (c0 & 0xFFFF))
                            cnt += 1
                tile_ptr.append(tile_ptr[-1] + cnt)
                most = max(most, cnt)
            return most

        for jp in range(self.npairs):
            j = 2 * jp
            srows = sorted_rows(j)
            ng = (srows.size + TILE - 1) // TILE
            k0 = [min(int(self.first[srows[TILE * g:TILE * g + TILE]].min()) // 32, 4 * j) for g in range(ng)]
            if max(k0) == 0:
                group_ptr.append(group_ptr[-1])
                continue
            for g in range(ng):
                slots = srows[TILE * g:TILE * g + TILE]
                k0s.append(k0[g])
                zfs.append(strip_chunks(slots, j))
                self.max_tile_pieces = max(self.max_tile_pieces, add_group(slots, j, rows, tile_ptr, pblk, prc))
            group_ptr.append(group_ptr[-1] + ng)
        self.ngroups = group_ptr[-1]
        self.group_ptr = np.array(group_ptr, dtype=np.int32)
        self.rows = np.array(rows, dtype=np.int32).reshape(-1, TILE)
        self.k0 = np.array(k0s, dtype=np.int32)
        self.zf = np.array(zfs, dtype=np.int32).reshape(-1, 4)
        self.tile_ptr = np.array(tile_ptr, dtype=np.int32)
        self.piece_blk = np.array(pblk, dtype=np.int32)
        self.piece_rc = np.array(prc, dtype=np.int64).astype(np.uint32).view(np.int32)
        # pair 0, in tables of its own (group_ptr keeps it empty): no K-loop to shorten, but sorted rows put the rows whose X0 / X1
        # are structurally zero into the same strips and groups
        rows0, zf0, tile_ptr0, pblk0, prc0 = [], [], [0], [], []
        self.max_tile_pieces0 = 0
        if self.npairs > 0:
            srows = sorted_rows(0)
            groups = [srows[TILE * g:TILE * g + TILE] for g in range((srows.size + TILE - 1) // TILE)]
            if any(int(self.first[sl[s:s + 32]].min()) >= 32 for sl in groups for s in range(0, sl.size, 32)):   # (a strip starts late)
                for slots in groups:
                    zf0.append(strip_chunks(slots, 0))
                    self.max_tile_pieces0 = max(self.max_tile_pieces0, add_group(slots, 0, rows0, tile_ptr0, pblk0, prc0))
        self.ngroups0 = len(rows0)
        self.rows0 = np.array(rows0, dtype=np.int32).reshape(-1, TILE)
        self.zf0 = np.array(zf0, dtype=np.int32).reshape(-1, 4)
        self.tile_ptr0 = np.array(tile_ptr0, dtype=np.int32)
        self.piece_blk0 = np.array(pblk0, dtype=np.int32)
        self.piece_rc0 = np.array(prc0, dtype=np.int64).astype(np.uint32).view(np.int32)
        self._hb = hb

    @staticmethod
    def _slots_ok(srows: np.ndarray, d: int) -> bool:
        """A piece lands all d rows of its block on consecutive slots: a run of a variable's rows may begin behind the variable's
        row 0 only at slot 0 of a group and end before its last row only at a group's last slot (what falls outside is clipped)."""
        r = srows.tolist()
        for s in range(len(r)):
            begins = s == 0 or s % TILE == 0 or r[s - 1] != r[s] - 1 or r[s] % d == 0
            ends = s == len(r) - 1 or s % TILE == TILE - 1 or r[s + 1] != r[s] + 1 or r[s] % d == d - 1
            if (begins and r[s] % d and s % TILE) or (ends and r[s] % d != d - 1 and s % TILE != TILE - 1 and s != len(r) - 1):
                return False
        return True

    def expand(self, Hc: np.ndarray, ld: int) -> np.ndarray:
        """(B, bstride) -> dense (B, ld, ld), the way the regrouped column-pair workgroups gather it: rows [128 (j + 2), n) of
        column tiles j, j + 1 of every regrouped pair, group by group, piece by piece (everything else stays zero)."""
        H = np.zeros((Hc.shape[0], ld, ld), dtype=Hc.dtype)
        for jp in range(self.npairs):
            self._expand_groups(H, Hc, 2 * jp, range(self.group_ptr[jp], self.group_ptr[jp + 1]), self.rows, self.tile_ptr,
                                self.piece_blk, self.piece_rc)
        return H

    def expand0(self, Hc: np.ndarray, ld: int) -> np.ndarray:
        """``expand`` for pair 0's own tables: rows [256, n) of column tiles 0, 1."""
        H = np.zeros((Hc.shape[0], ld, ld), dtype=Hc.dtype)
        self._expand_groups(H, Hc, 0, range(self.ngroups0), self.rows0, self.tile_ptr0, self.piece_blk0, self.piece_rc0)
        return H

    def _expand_groups(self, H, Hc, j, groups, rows, tile_ptr, piece_blk, piece_rc):
        B, d = Hc.shape[0], self._hb.bd
        for g in groups:
            for s in range(2):
                for pc in range(tile_ptr[2 * g + s], tile_ptr[2 * g + s + 1]):
                    rc = int(piece_rc[pc]) & 0xFFFFFFFF
                    r0 = int(np.array(rc >> 16, dtype=np.uint16).view(np.int16))
                    c0 = int(np.array(rc & 0xFFFF, dtype=np.uint16).view(np.int16))
                    blk = Hc[:, piece_blk[pc] * d * d:(piece_blk[pc] + 1) * d * d].reshape(B, d, d)
                    for e in range(d * d):
                        r, c = r0 + e // d, c0 + e % d
                        if 0 <= r < TILE and 0 <= c < TILE and rows[g, r] >= 0:
                            H[:, rows[g, r], TILE * (j + s) + c] = blk[:, e // d, e % d]

    def skipped_fraction(self, l_mask: np.ndarray):
        """Model: the share of the pair K-loops' 32x32 block products (chol_offdiag2_f32_kernel: per row tile and k-chunk four waves
        times the four + four sub-blocks of tiles j, j + 1) that the regrouped schedule leaves out -- the chunks in front of a
        group's k0 and, behind it, the column-side zero sub-blocks of ``l_mask``.  Pairs without groups count with the
        natural-tile skip (row-side and column-side masks).  Returns ({j: fraction}, fraction over all pairs)."""
        nt = l_mask.shape[0]
        pop = lambda m: bin(int(m) & 15).count("1")   # noqa: E731
        per, tot_all, tot_run = {}, 0, 0
        for jp in range(self.npairs):
            j = 2 * jp
            cols = [pop(l_mask[j, kc]) + pop(l_mask[j + 1, kc]) for kc in range(4 * j)]
            allp = (nt - 2 - j) * 4 * j * 32
            run = 0
            if self.group_ptr[jp + 1] > self.group_ptr[jp]:
                for g in range(self.group_ptr[jp], self.group_ptr[jp + 1]):
                    run += sum(4 * cols[kc] for kc in range(int(self.k0[g]), 4 * j))
            else:
                for i in range(j + 2, nt):
                    run += sum(pop(l_mask[i, kc]) * cols[kc] for kc in range(4 * j))
            per[j] = 1.0 - run / allp if allp else 0.0
            tot_all += allp
            tot_run += run
        return per, (1.0 - tot_run / tot_all if tot_all else 0.0)

    def zero_solve_model(self, l_mask: np.ndarray):
        """Model of thx_chol_schedule.skip_zero_solves in 32x32x32 block products, per pair j: a wave's two substitutions are
        10 + 10 products and its coupling 16; with z0 / z1 leading zero sub-blocks of its strip in tiles (i, j) / (i, j + 1) they
        are (4 - z0)(5 - z0) / 2 + (4 - z1)(5 - z1) / 2 and 4 (4 - z0).  The K-loop counts as in ``skipped_fraction``, a wave
        starting at its own strip's first chunk.  Pairs without groups keep their natural tiles (nothing changes).  Returns
        {j: dict(solve=(today, proposed), kloop=(today, proposed), z=[[z of the four waves] per group])}."""
        nt = l_mask.shape[0]
        pop = lambda m: bin(int(m) & 15).count("1")   # noqa: E731
        tri = lambda m: m * (m + 1) // 2              # noqa: E731
        out = {}
        for jp in range(self.npairs):
            j = 2 * jp
            cols = [pop(l_mask[j, kc]) + pop(l_mask[j + 1, kc]) for kc in range(4 * j)]
            g0, g1 = int(self.group_ptr[jp]), int(self.group_ptr[jp + 1])
            zf = self.zf[g0:g1] if g1 > g0 else (self.zf0 if j == 0 else np.zeros((0, 4), np.int32))
            solve_today = (nt - 2 - j) * 4 * 36
            if zf.shape[0] == 0:   # natural tiles
                k = sum(pop(l_mask[i, kc]) * cols[kc] for i in range(j + 2, nt) for kc in range(4 * j))
                out[j] = dict(solve=(solve_today, solve_today), kloop=(k, k), z=[])
                continue
            z = np.clip(zf - 4 * j, 0, 8)
            z0, z1 = np.minimum(z, 4), z - np.minimum(z, 4)
            solve = int(sum(tri(4 - a) + 4 * (4 - a) + tri(4 - b) for a, b in zip(z0.reshape(-1).tolist(), z1.reshape(-1).tolist())))
            k0 = np.minimum(zf.min(1), 4 * j)
            k_today = sum(4 * cols[kc] for g in range(zf.shape[0]) for kc in range(int(k0[g]), 4 * j))
            k_new = sum(cols[kc] for g in range(zf.shape[0]) for w in range(4) for kc in range(min(int(zf[g, w]), 4 * j), 4 * j))
            out[j] = dict(solve=(solve_today, solve), kloop=(k_today, k_new), z=z.tolist())
        return out


class PairColumns:
    """The 256 columns of every fp32 column pair sorted by their first non-zero column (thx_hblock_layout.sc_*).

    The K-loop of pair (j, j + 1) multiplies row r below the pair with row c of tiles j, j + 1 over the columns k < 128 j; the
    product is structurally zero for k < max(first[r], first[c]).  ``RowGroups`` sorts the r side.  Here the c side: the pair's 256
    matrix rows 128 j ... 128 j + 255, stably sorted by ``first`` (a variable's rows stay adjacent), are cut into eight blocks of 32
    sorted slots; block u is zero in every k-chunk before ``first_chunk[u] = min first // 32`` (a value >= 4 j: never active in
    this pair).  Pairs j >= 2 that have row groups (the kernel variant is the row groups'); a pair whose eight blocks all start at
    chunk 0 has no table.

    has          (npairs)              1: the pair has tables
    perm         (npairs, 256)         sorted slot -> column of the pair, 0 ... 255 (matrix row 128 j + value); identity without tables
    first_chunk  (npairs, 8)           per block min first // 32
    mask         (npairs, 4 ntiles)    per k-chunk kc < 4 j: bit u set when block u is active (kc >= first_chunk[u]); 255 elsewhere
    """

    def __init__(self, hb: "HessianBlocks", rg: Optional[RowGroups]):
        nt = hb.ntiles
        first = hb.row_first.astype(np.int64)
        self.npairs = max(0, (nt - 1) // 2)
        self.has = np.zeros(self.npairs, dtype=np.int32)
        self.perm = np.tile(np.arange(2 * TILE, dtype=np.int32), (self.npairs, 1))
        self.first_chunk = np.zeros((self.npairs, 8), dtype=np.int32)
        self.mask = np.full((self.npairs, 4 * nt), 255, dtype=np.int32)
        for jp in range(1, self.npairs):
            if rg is None or rg.group_ptr[jp + 1] == rg.group_ptr[jp]:
                continue
            j = 2 * jp
            f = first[TILE * j:TILE * j + 2 * TILE]
            order = np.argsort(f, kind="stable")
            fc = f[order].reshape(8, 32).min(1) // 32
            if fc.max() == 0:
                continue
            self.has[jp] = 1
            self.perm[jp] = order
            self.first_chunk[jp] = fc
            for kc in range(4 * j):
                self.mask[jp, kc] = sum(1 << u for u in range(8) if kc >= fc[u])
        self.npairs_sorted = int(self.has.sum())

    def executed_fraction(self, rg: RowGroups):
        """Model in 32x32x32 block products, per pair j: the K-loop's products executed with the row groups and the natural-order
        column masks (``l_mask``; what ``RowGroups.skipped_fraction`` counts) against the row groups and the sorted blocks, both as
        shares of the dense count.  Returns ({j: (today, sorted)}, (today, sorted) over all pairs with a K-loop)."""
        hb = rg._hb
        l_mask, nt = hb.l_mask(), hb.ntiles
        pop = lambda m: bin(int(m)).count("1")   # noqa: E731
        per, tot, run_a, run_b = {}, 0, 0, 0
        for jp in range(1, self.npairs):
            j = 2 * jp
            allp = (nt - 2 - j) * 4 * j * 32
            g0, g1 = int(rg.group_ptr[jp]), int(rg.group_ptr[jp + 1])
            nat = [pop(l_mask[j, kc] & 15) + pop(l_mask[j + 1, kc] & 15) for kc in range(4 * j)]
            srt = [pop(self.mask[jp, kc] & 255) for kc in range(4 * j)] if self.has[jp] else nat
            if g1 > g0:
                a = sum(4 * nat[kc] for g in range(g0, g1) for kc in range(int(rg.k0[g]), 4 * j))
                b = sum(4 * srt[kc] for g in range(g0, g1) for kc in range(int(rg.k0[g]), 4 * j))
            else:
                a = b = sum(pop(l_mask[i, kc] & 15) * nat[kc] for i in range(j + 2, nt) for kc in range(4 * j))
            per[j] = (a / allp, b / allp)
            tot, run_a, run_b = tot + allp, run_a + a, run_b + b
        return per, ((run_a / tot, run_b / tot) if tot else (0.0, 0.0))


class TileRows:
    """The 128 rows of every diagonal tile sorted by their first non-zero column (thx_hblock_layout.tr_*).

    The SYRK of diagonal tile j multiplies rows r and c of the tile over the columns k < 128 j; the product is structurally zero for
    k < max(first[r], first[c]).  The tile's rows, stably sorted by ``first`` (a variable's rows stay adjacent; rows at or behind n
    are never active and go last), are cut into eight rank blocks of 16.  The kernel's four waves meet at two barriers per
    k-chunk, wave g owning block rows 4 + g and 3 - g of the 8 x 8 block grid, so a chunk costs what its busiest wave executes:
    rank block q is staged at block row ``PLACE[q]``, the fixed placement with the lowest such cost on the headline graph (0.738
    of dense against 0.847 for the identity; ``model``).  Block row u is zero in every k-chunk before ``first_chunk[u]``; a value
    >= 4 j: never active.  A tile whose blocks all begin at chunk 0 (tile 0 always) has no table.

    has          (ntiles)              1: the tile has tables
    perm         (ntiles, 128)         staged slot -> row of the tile, 0 ... 127 (matrix row 128 j + value); identity without tables
    first_chunk  (ntiles, 8)           per staged block row min first // 32
    mask         (ntiles, 4 ntiles)    per k-chunk kc < 4 j: bit u set when block row u is active (kc >= first_chunk[u]); 255 elsewhere
    """

    PLACE = (1, 2, 3, 7, 6, 5, 4, 0)
    NEVER = 1 << 30   # ``first`` of a row at or behind n

    def __init__(self, hb: "HessianBlocks", place=PLACE):
        nt, n = hb.ntiles, hb.bd * hb.nvars
        first = np.full(nt * TILE, self.NEVER, dtype=np.int64)
        first[:n] = hb.row_first
        self.place = tuple(place)
        self.has = np.zeros(nt, dtype=np.int32)
        self.perm = np.tile(np.arange(TILE, dtype=np.int32), (nt, 1))
        self.first_chunk = np.zeros((nt, 8), dtype=np.int32)
        self.mask = np.full((nt, 4 * nt), 255, dtype=np.int32)
        for j in range(1, nt):
            f = first[TILE * j:TILE * j + TILE]
            order = np.argsort(f, kind="stable")
            fc_rank = np.minimum(f[order].reshape(8, 16).min(1) // 32, 4 * nt)
            if fc_rank.max() == 0:
                continue
            self.has[j] = 1
            for q in range(8):
                u = self.place[q]
                self.perm[j, 16 * u:16 * u + 16] = order[16 * q:16 * q + 16]
                self.first_chunk[j, u] = fc_rank[q]
            for kc in range(4 * j):
                self.mask[j, kc] = sum(1 << u for u in range(8) if kc >= self.first_chunk[j, u])
        # the head tiles (j + 1, j) of the column pairs: tile j's rows in the plain stable sort, four blocks of 32
        self.has32 = np.zeros(nt, dtype=np.int32)
        self.perm32 = np.tile(np.arange(TILE, dtype=np.int32), (nt, 1))
        self.first_chunk32 = np.zeros((nt, 4), dtype=np.int32)
        self.mask32 = np.full((nt, 4 * nt), 15, dtype=np.int32)
        self.k0h = np.zeros(nt, dtype=np.int32)
        for j in range(2, nt - 1, 2):
            f = first[TILE * j:TILE * j + TILE]
            order = np.argsort(f, kind="stable")
            fc = np.minimum(f[order].reshape(4, 32).min(1) // 32, 4 * nt)
            k0 = min(max(int(first[TILE * (j + 1):TILE * (j + 2)].min()) // 32, int(fc.min())), 4 * j)
            if fc.max() == 0 and k0 == 0:
                continue
            self.has32[j], self.perm32[j], self.first_chunk32[j], self.k0h[j] = 1, order, fc, k0
            for kc in range(4 * j):
                self.mask32[j, kc] = sum(1 << u for u in range(4) if kc >= fc[u])
        self.ntables = int(self.has.sum()) + int(self.has32.sum())

    @staticmethod
    def wave_blocks(m: int):
        """Per wave g the 16x16 block products of chunk mask ``m`` in Engine<float>::syrk36: block (u, v), v <= u, of block rows
        u = 4 + g and 3 - g, executed when bits u and v are both set."""
        bit = lambda u: (m >> u) & 1   # noqa: E731
        return [sum(bit(u) & bit(v) for u in (4 + g, 3 - g) for v in range(u + 1)) for g in range(4)]

    def model(self):
        """Model in 16x16 block products per 32-column k-chunk, per tile j >= 1: ({j: (executed, slowest wave)}, (executed, slowest
        wave) over all tiles), as shares of the dense count (36 products, 9 per wave and chunk).  Tiles without tables count dense."""
        per, tot, ex, slow = {}, 0, 0, 0
        for j in range(1, self.has.size):
            w = [self.wave_blocks(int(self.mask[j, kc]) if self.has[j] else 255) for kc in range(4 * j)]
            e, sl = sum(sum(x) for x in w), sum(max(x) for x in w)
            per[j] = (e / (36 * 4 * j), sl / (9 * 4 * j))
            tot, ex, slow = tot + 4 * j, ex + e, slow + sl
        return per, ((ex / (36 * tot), slow / (9 * tot)) if tot else (1.0, 1.0))

    def head_model(self):
        """Model of the head tiles (j + 1, j), j even >= 2, in 32x32 block products per k-chunk (16 dense: four waves times four
        blocks), skipped by the whole workgroup: ({j: executed}, executed over all of them), as shares of dense."""
        per, tot, ex = {}, 0, 0
        for j in range(2, self.has32.size - 1, 2):
            e = sum(4 * bin(int(self.mask32[j, kc]) & 15).count("1") for kc in range(int(self.k0h[j]), 4 * j))
            per[j] = e / (64 * j)
            tot, ex = tot + 64 * j, ex + e
        return per, (ex / tot if tot else 1.0)


class DeviceHessianBlocks:
    _FIELDS = ["diag_blk", "inc_blk", "tile_ptr", "piece_blk", "piece_rc"]

    def __init__(self, hb: HessianBlocks, device):
        self.host = hb
        self.t = {}
        for f in self._FIELDS:
            a = getattr(hb, f)
            if a.size == 0:
                a = np.zeros(1, np.int32)
            self.t[f] = torch.from_numpy(np.ascontiguousarray(a)).to(device)
        c = _lib.HBlockLayout()
        c.nblocks, c.bd, c.nvars, c.ntiles = hb.nblocks, hb.bd, hb.nvars, hb.ntiles
        for f in self._FIELDS:
            setattr(c, f, self.t[f].data_ptr())
        c.max_tile_pieces = _lib.max_offdiag_tile_pieces(hb.tile_ptr, hb.ntiles)
        # the structurally non-zero 32x32 sub-blocks of the natural-order factor (thx_hblock_layout.l_mask), once per layout and device
        self.t["l_mask"] = torch.from_numpy(hb.l_mask()).to(device)
        c.l_mask = self.t["l_mask"].data_ptr()
        # the row envelope of H and L for the dense-frame solves (thx_hblock_layout.row_first), with or without row groups
        self.t["row_first"] = torch.from_numpy(hb.row_first).to(device)
        c.row_first = self.t["row_first"].data_ptr()
        # the row groups of the fp32 column pairs (thx_hblock_layout.rg_*); none: the fields stay NULL
        rg = hb.row_groups()
        if rg is not None and rg.ngroups > 0:
            self.rg_group_ptr_host = np.ascontiguousarray(rg.group_ptr)   # (host table: kept alive here)
            c.rg_group_ptr_host = self.rg_group_ptr_host.ctypes.data
            for f in ("rows", "k0", "tile_ptr", "piece_blk", "piece_rc", "zf"):
                self.t["rg_" + f] = torch.from_numpy(np.ascontiguousarray(getattr(rg, f))).to(device)
                setattr(c, "rg_" + f, self.t["rg_" + f].data_ptr())
            c.rg_max_tile_pieces = rg.max_tile_pieces
        if rg is not None and rg.ngroups0 > 0:   # pair 0's groups (thx_hblock_layout.rg0_*)
            for f in ("rows", "zf", "tile_ptr", "piece_blk", "piece_rc"):
                self.t["rg0_" + f] = torch.from_numpy(np.ascontiguousarray(getattr(rg, f + "0"))).to(device)
                setattr(c, "rg0_" + f, self.t["rg0_" + f].data_ptr())
            c.rg0_ngroups, c.rg0_max_tile_pieces = rg.ngroups0, rg.max_tile_pieces0
        pc = hb.pair_columns()   # the sorted columns of the pairs that have row groups (thx_hblock_layout.sc_*); none: NULL
        if pc is not None:
            self.sc_pair_host = np.ascontiguousarray(pc.has)   # (host table: kept alive here)
            c.sc_pair_host = self.sc_pair_host.ctypes.data
            for f in ("perm", "mask"):
                self.t["sc_" + f] = torch.from_numpy(np.ascontiguousarray(getattr(pc, f))).to(device)
                setattr(c, "sc_" + f, self.t["sc_" + f].data_ptr())
        tr = hb.tile_rows()      # the sorted rows of the diagonal tiles (thx_hblock_layout.tr_*); none: NULL
        if tr is not None:
            self.tr_tile_host = np.ascontiguousarray(tr.has)   # (host table: kept alive here)
            c.tr_tile_host = self.tr_tile_host.ctypes.data
            for f in ("perm", "mask"):
                self.t["tr_" + f + "16"] = torch.from_numpy(np.ascontiguousarray(getattr(tr, f))).to(device)
                setattr(c, "tr_" + f + "16", self.t["tr_" + f + "16"].data_ptr())
            self.th_tile_host = np.ascontiguousarray(tr.has32)   # (host table: kept alive here)
            c.th_tile_host = self.th_tile_host.ctypes.data
            for f in ("perm32", "mask32", "k0h"):
                self.t["th_" + f] = torch.from_numpy(np.ascontiguousarray(getattr(tr, f))).to(device)
                setattr(c, "th_" + f, self.t["th_" + f].data_ptr())
        self.c = c


class _OrderedPattern:
    """What HessianBlocks reads of a structure, for a block pattern given directly (no cost tables: the layout is never assembled
    into, its blocks arrive by thx_hblocks_permute)."""

    def __init__(self, dof: int, nvars: int, pattern: np.ndarray):
        self.dof, self.num_poses, self._pattern = dof, nvars, pattern
        self.inc_ptr = np.zeros(nvars + 1, dtype=np.int32)
        self.inc_other = np.zeros(0, dtype=np.int32)

    def lower_block_pattern(self) -> np.ndarray:
        return self._pattern


class OrderedHessianBlocks:
    """A block layout of the SAME matrix under another order of its variables (thx_hblock_order): ``perm[k]`` = the variable of
    ``hb`` at position k.  ``layout`` is a HessianBlocks of P H P^T in its own right -- every table of it (pieces, l_mask, row
    groups, sorted columns and rows, row_first) is built from the permuted positions by the code that builds the natural one.

    block_map (layout.nblocks) int32: (block of ``hb`` << 1) | transposed -- block k of the layout is that block of the
                                      linearization's list, transposed when its two variables swap sides of the diagonal
    to_perm   (n) int32: column of the linearization at every column of the permuted order (g -> P g by thx_vec_gather)
    from_perm (n) int32: the inverse (x of the permuted order -> delta)"""

    def __init__(self, hb: HessianBlocks, perm: np.ndarray):
        d, P = hb.bd, hb.nvars
        perm = np.asarray(perm, dtype=np.int64)
        if perm.shape != (P,) or not np.array_equal(np.sort(perm), np.arange(P)):
            raise ValueError("OrderedHessianBlocks: perm is not a permutation of the layout's variables")
        pos = np.empty(P, dtype=np.int64)
        pos[perm] = np.arange(P)
        a, b = pos[hb.blocks[:, 0]], pos[hb.blocks[:, 1]]
        swapped = a < b
        pat = np.stack([np.maximum(a, b), np.minimum(a, b)], axis=1)
        self.base, self.perm, self.pos = hb, perm.astype(np.int32), pos.astype(np.int32)
        self.layout = HessianBlocks(_OrderedPattern(d, P, pat[np.lexsort((pat[:, 1], pat[:, 0]))]))
        ident = {(int(p), int(q)): k for k, (p, q) in enumerate(self.layout.blocks.tolist())}
        self.block_map = np.zeros(hb.nblocks, dtype=np.int32)
        for k, ((p, q), t) in enumerate(zip(pat.tolist(), swapped.tolist())):
            self.block_map[ident[(p, q)]] = (k << 1) | int(t)
        self.nswapped = int(swapped.sum())
        self.to_perm = (d * perm[:, None] + np.arange(d)[None, :]).reshape(-1).astype(np.int32)
        self.from_perm = (d * pos[:, None] + np.arange(d)[None, :]).reshape(-1).astype(np.int32)
        self._dev = {}

    def on(self, device):
        """(DeviceHessianBlocks of the layout, {block_map, to_perm, from_perm} on the device)."""
        key = str(device)
        if key not in self._dev:
            maps = {f: torch.from_numpy(getattr(self, f)).to(device) for f in ("block_map", "to_perm", "from_perm")}
            self._dev[key] = (self.layout.on(device), maps)
        return self._dev[key]


def ordered_hessian_blocks(hb: HessianBlocks) -> Optional[OrderedHessianBlocks]:
    """The layout of ``hb``'s matrix under thx_hblock_order's order, None when that is the insertion order (built once per layout)."""
    cached = getattr(hb, "_ordered", None)
    if cached is None:
        perm, score, natural = _lib.hblock_order(hb.blocks, hb.nvars, hb.bd)
        cached = hb._ordered = OrderedHessianBlocks(hb, perm) if score < natural else False
    return cached or None
