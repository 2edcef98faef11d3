"""hard_voxelize's border lattice (a helper module like tests/sparse_lattice.py, not a conftest).

* plan() restates vt_plan / vw_plan / v3_plan and the *_applicable functions of csrc/voxelize.hip: for every (case, form)
  pair it says which pipeline runs, with which route tile and group split, or that the form answers status -3.
* ref_cells is the reference's fp32 cell rule in NumPy, ref_hard_voxelize a sequential restatement on those cells
  (np.unique + stable sorts, no loop over points).  tests/test_voxel_lattice_cpu.py holds the oracle port to it on every
  case, so what the GPU is compared with does not rest on one implementation.
* the case families are crosses, not products; every builder draws its points from a seed derived from the case id and
  shuffles only where the family says so.  Structural families use unit grids (minimum 0, size 1: cell = floor(p), points
  at cell + 1/4, 1/2 or 3/4 are exact) so that a case's claim -- records of a group, first points of a tile -- is exact.

Everything here runs on the CPU except run / run_raw / run_index / run_dynamic, which the GPU tests use.
"""
from __future__ import annotations

import re
import zlib
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

FORMS = {"auto": 0, "sort": 1, "tiled": 2, "gather": 3, "wave": 5, "s0": 6, "s1": 7, "s2": 8, "s3": 9, "s4": 10,
         "prio": 11, "split": 12, "prio_split": 13, "w3d": 14, "w3d_s1": 15, "w3d_s2": 16, "payload": 17}
F2D = ("tiled", "gather", "wave", "s0", "s1", "s2", "s3", "s4", "prio", "split", "prio_split", "payload")
F3D = ("w3d", "w3d_s1", "w3d_s2")
FAST = F2D + F3D
SKEW = 37                              # kVtSkew
ROW_LIMIT = (1 << 24) - 4096           # max_voxels * rowq stays below it
MAX_PTS = 254                          # kVtMaxPts
ASSIGN_CAP, HOLD, ASSIGN_THREADS = 4096, 8, 512   # kVwAssignCap, kHold, kVwAssignThreads
VW_REG, V3_REG, V3_LOAD = 40 * 64, 12 * 64, 768   # kVwRegSteps * 64, kV3RegSteps * 64, kV3Load
WAVE_SHAPES = ((512, 8), (1024, 8), (1024, 10), (512, 10), (1024, 5))
TILE_OF = {"tiled": 4096, "gather": 4096, "s0": 4096, "payload": 4096, "s1": 8192, "w3d_s1": 8192, "s2": 10240,
           "w3d_s2": 10240, "s3": 5120, "s4": 5120}


# ---- the plans, restated from voxelize_tiled.hpp / voxelize_wave.hpp / voxelize_wave3d.hpp / voxelize.hip ------------------
@dataclass(frozen=True)
class Plan:
    kind: str            # sort / tiled / wave / wave3d: the pipeline that runs (where ok)
    ok: bool             # False: the form answers status -3
    low: int = 0
    gbits: int = 0
    groups: int = 0
    cpg: int = 0
    tile: int = 0
    tiles: int = 0


def _ceil_div(a, b):
    return -(-a // b)


def _bits(ncells):
    b = 0
    while (1 << b) < ncells:
        b += 1
    return b


def _low(bits, max_low, n):
    low = max(min(bits - 2, max_low), 0)
    while low > 0 and n >= (1 << (32 - low)) - 1:   # a record = (point index << low) | cell
        low -= 1
    return low


def _rowq(p, d, vec4=True):
    """Units of a row in the row writer: float4s where P * D % 4 == 0 and the float4 writer runs, else floats."""
    return p * d // 4 if p * d % 4 == 0 and vec4 else p * d


def _common_ok(tiles, n, p):
    return tiles <= 1024 and n < 0x3FFFFF - 1 and p <= MAX_PTS


def _tiled(ncells, n, p, v, d, aligned=True):
    bits = _bits(ncells)
    low = _low(bits, 12, n)
    gbits = max(bits - low, 2)
    tiles = _ceil_div(n, 4096)
    ok = gbits <= 10 and _common_ok(tiles, n, p) and v * _rowq(p, d, aligned) < ROW_LIMIT
    return Plan("tiled", ok, low, gbits, 1 << gbits, 1 << low, 4096, tiles)


def _wave(ncells, n, p, v, d, batch, shape, aligned=True):
    bits = _bits(ncells)
    low = _low(bits, 10, n)
    gbits = max(bits - low, 2)
    if not 0 <= shape < len(WAVE_SHAPES):
        shape = 0
        for k in (1, 2):
            if _ceil_div(n, WAVE_SHAPES[k][0] * WAVE_SHAPES[k][1]) * batch >= 384:
                shape = k
    tile = WAVE_SHAPES[shape][0] * WAVE_SHAPES[shape][1]
    tiles = _ceil_div(n, tile)
    vec4 = aligned or d in (4, 5)    # D = 4 / 5 leave through the slot-per-lane writer whatever the alignment
    ok = bits <= 20 and gbits <= 10 and _common_ok(tiles, n, p) and v * _rowq(p, d, vec4) < ROW_LIMIT
    return Plan("wave", ok, low, gbits, 1 << gbits, 1 << low, tile, tiles)


def _wave3d(ncells, n, p, v, d, batch, shape):
    bits = _bits(ncells)
    if not 0 <= shape < 3:
        shape = 0
        for k in (1, 2):
            if _ceil_div(n, WAVE_SHAPES[k][0] * WAVE_SHAPES[k][1]) * batch >= 192:
                shape = k
    tile = WAVE_SHAPES[shape][0] * WAVE_SHAPES[shape][1]
    tiles = _ceil_div(n, tile)
    ok = 20 < bits <= 28 and _common_ok(tiles, n, p) and d in (4, 5) and v * p < ROW_LIMIT
    return Plan("wave3d", ok, 18, 10, 1024, 0, tile, tiles)


def plan(form, ncells, n, p, v, d, batch, aligned=True):
    """What pd3_hard_voxelize_path does with `form` on these sizes (n = max_points of a frame).  aligned: the voxels tensor
    lies at a multiple of 16 bytes (else the scalar row writer runs, with four times the units where P * D % 4 == 0)."""
    path = FORMS[form]
    if path == 1:
        return Plan("sort", True)
    if path == 0:
        for pl in (_wave(ncells, n, p, v, d, batch, -1, aligned), _wave3d(ncells, n, p, v, d, batch, -1),
                   _tiled(ncells, n, p, v, d, aligned)):
            if pl.ok:
                return pl
        return Plan("sort", True)
    if path in (2, 3):
        return _tiled(ncells, n, p, v, d, aligned)
    if path == 17:   # the carried payload: 4096-point tiles, its LDS slice within 160 KiB, its run within the voxels tensor
        pl = _wave(ncells, n, p, v, d, batch, 0, aligned)
        lds = (4096 + 8 * pl.groups + 8 + 2) * 4 + 4096 * d * 4
        ok = pl.ok and lds <= 160 * 1024 and pl.tiles * 4096 <= v * p
        return Plan("wave", ok, pl.low, pl.gbits, pl.groups, pl.cpg, pl.tile, pl.tiles)
    if path >= 14:
        return _wave3d(ncells, n, p, v, d, batch, -1 if path == 14 else path - 14)
    if path >= 11:
        return _wave(ncells, n, p, v, d, batch, -1, aligned)
    return _wave(ncells, n, p, v, d, batch, path - 6, aligned)


def index_plan(ncells, n, p, v, d, batch):
    """pd3_hard_voxelize_index: the 2-D wave form, else the 3-D one, else None (status -3)."""
    for pl in (_wave(ncells, n, p, v, d, batch, -1), _wave3d(ncells, n, p, v, d, batch, -1)):
        if pl.ok:
            return pl
    return None


def group_of(key, gbits):
    """vt_key_to_group: cell key = local * G + lo  ->  group (lo + 37 * local) mod G."""
    key = np.asarray(key, np.int64)
    gm = (1 << gbits) - 1
    return ((key & gm) + SKEW * (key >> gbits)) & gm


def keys_of_group(group, gbits, ncells):
    """Every cell key below ncells that vt_key_to_group deals to `group`, ascending."""
    local = np.arange(_ceil_div(ncells, 1 << gbits), dtype=np.int64)
    keys = (local << gbits) | ((group - SKEW * local) & ((1 << gbits) - 1))
    return keys[keys < ncells]


# ---- the two references ----------------------------------------------------------------------------------------------------
def grid_of(vs, pr):
    """voxelize_op.cc:97-102: round((max - min) / size) on fp32 operands."""
    vs, pr = np.asarray(vs, np.float32), np.asarray(pr, np.float32)
    return tuple(int(np.round(np.float64((pr[3 + a] - pr[a]) / vs[a]))) for a in range(3))


def ref_cells(points, vs, pr):
    """The fp32 cell rule: subtract, divide, floor, 0 <= q < extent per axis (false for NaN and +-inf).
    Returns (cells [N, 3] int64 (x, y, z), -1 rows where the point lies outside; inside [N] bool)."""
    pts = np.asarray(points, np.float32)[:, :3]
    vs, pr = np.asarray(vs, np.float32), np.asarray(pr, np.float32)
    grid = np.asarray(grid_of(vs, pr), np.float32)
    with np.errstate(all="ignore"):
        q = np.floor((pts - pr[:3]) / vs)
        assert q.dtype == np.float32
        inside = np.all((q >= 0) & (q < grid), axis=1)
    cells = np.where(inside[:, None], q, -1).astype(np.int64)
    return cells, inside


def keys_of_points(points, vs, pr):
    """(linear cell key per point, -1 outside; inside)."""
    gx, gy, _ = grid_of(vs, pr)
    cells, inside = ref_cells(points, vs, pr)
    return np.where(inside, (cells[:, 2] * gy + cells[:, 1]) * gx + cells[:, 0], -1), inside


def ref_hard_voxelize(points, vs, pr, p, v):
    """hard_voxelize from its definition on ref_cells: voxels in the order their cells first occur, the first `v` of them,
    the first `p` points of each.  (voxels [v, p, D], coords [v, 3] (z, y, x), counts [v], num_voxels)."""
    pts = np.ascontiguousarray(points, np.float32)
    d = pts.shape[1]
    gx, gy, _ = grid_of(vs, pr)
    key, inside = keys_of_points(pts, vs, pr)
    idx = np.nonzero(inside)[0]
    k = key[idx]
    voxels, coords, counts = np.zeros((v, p, d), np.float32), np.zeros((v, 3), np.int32), np.zeros((v,), np.int32)
    if len(k) == 0:
        return voxels, coords, counts, 0
    uniq, first, inv = np.unique(k, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")            # cells in the order of their first points
    rank = np.empty(len(uniq), np.int64)
    rank[order] = np.arange(len(uniq))
    vid = rank[inv.reshape(-1)]                         # voxel of every inside point, before the cap
    s = np.argsort(vid, kind="stable")                  # by voxel, points of one voxel in input order
    vs_ = vid[s]
    slot = np.arange(len(s)) - np.searchsorted(vs_, vs_, side="left")
    sel = (vs_ < v) & (slot < p)
    voxels[vs_[sel], slot[sel]] = pts[idx[s[sel]]]
    nv = min(len(uniq), v)
    counts[:nv] = np.minimum(np.bincount(vid, minlength=len(uniq))[:nv], p)
    ck = uniq[order][:nv]
    coords[:nv] = np.stack([ck // (gx * gy), (ck // gx) % gy, ck % gx], 1)
    return voxels, coords, counts, nv


# ---- cases -----------------------------------------------------------------------------------------------------------------
def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


@dataclass(frozen=True, eq=False)
class Case:
    id: str
    family: str
    vs: tuple
    pr: tuple
    P: int
    V: int
    D: int
    forms: tuple                 # the forms the case is meant for (every case also runs on auto and sort)
    build: object = field(repr=False, default=None)   # rng -> (frames [B, N, D] fp32, num_points list or None)
    claim: tuple = ()            # sorted (key, value) pairs the CPU file verifies
    index: bool = False          # also runs through hard_voxelize_index_batch

    def c(self, key, default=None):
        return dict(self.claim).get(key, default)

    @property
    def grid(self):
        return grid_of(self.vs, self.pr)

    @property
    def ncells(self):
        gx, gy, gz = self.grid
        return gx * gy * gz


_DATA = {}


def data(case: Case):
    """(frames [B, N, D] fp32 read-only, num_points list or None); made once per case."""
    if case.id not in _DATA:
        frames, lens = case.build(np.random.default_rng(_seed(case.id)))
        frames = np.ascontiguousarray(frames, np.float32)
        if frames.ndim == 2:
            frames = frames[None]
        assert frames.shape[2] == case.D, case.id
        frames.setflags(write=False)
        _DATA[case.id] = (frames, None if lens is None else [int(x) for x in lens])
    return _DATA[case.id]


def sizes(case: Case):
    frames, _ = data(case)
    return frames.shape[0], frames.shape[1]


def case_plan(case: Case, form, aligned=True):
    b, n = sizes(case)
    return plan(form, case.ncells, n, case.P, case.V, case.D, b, aligned)


def case_index_plan(case: Case):
    b, n = sizes(case)
    return index_plan(case.ncells, n, case.P, case.V, case.D, b)


def frame_points(case: Case, b):
    frames, lens = data(case)
    return frames[b] if lens is None else frames[b, : lens[b]]


def unit_grid(gx, gy, gz=1):
    return (1.0, 1.0, 1.0), (0.0, 0.0, 0.0, float(gx), float(gy), float(gz))


def pts_of_keys(keys, grid, d, rng):
    """fp32 points [N, d] in the cells `keys` of a unit grid (-1: a point outside it), at cell + 1/4, 1/2 or 3/4; feature 3
    is the point's serial number, the others are random."""
    keys = np.asarray(keys, np.int64)
    gx, gy, gz = grid
    n = len(keys)
    out = rng.standard_normal((n, d)).astype(np.float32)
    off = rng.integers(1, 4, (n, 3)) * 0.25
    k = np.where(keys < 0, 0, keys)
    out[:, 0] = k % gx + off[:, 0]
    out[:, 1] = (k // gx) % gy + off[:, 1]
    out[:, 2] = k // (gx * gy) + off[:, 2]
    bad = keys < 0
    out[bad, 0] = np.where(rng.random(int(bad.sum())) < 0.5, -3.5, gx + 2.5)
    if d > 3:
        out[:, 3] = np.arange(n)
    return out


def _unit_case(cid, family, grid, keys_fn, P, V, D=4, forms=FAST, claim=(), index=True, lens=None):
    """A case on a unit grid whose frames come from cell keys: keys_fn(rng) -> [N] or [B, N] int64 keys."""
    vs, pr = unit_grid(*grid)

    def build(rng):
        keys = np.asarray(keys_fn(rng), np.int64)
        if keys.ndim == 1:
            return pts_of_keys(keys, grid, D, rng), lens
        return np.stack([pts_of_keys(k, grid, D, rng) for k in keys]), lens

    return Case(cid, family, vs, pr, P, V, D, tuple(forms), build, tuple(sorted(dict(claim).items())), index)


PILLAR = (64, 64, 1)          # 4096 cells: 4 groups in the wave form, cells fill and open throughout
BIG = (2048, 1024, 1)         # 2^21 cells: the 3-D wave form (and the tiled form)
_BIG_POOL = 4096              # occupied cells of BIG are drawn from a pool of this many


def _pool(rng, grid, size=_BIG_POOL):
    ncells = grid[0] * grid[1] * grid[2]
    if ncells <= size:
        return np.arange(ncells, dtype=np.int64)
    pool = rng.choice(ncells, size, replace=False).astype(np.int64)
    pool[0], pool[1] = 0, ncells - 1
    return pool


def _random_keys(rng, grid, n, outside=0.05, fresh_at=()):
    """n keys drawn from the grid's pool, a share of them outside the grid; the points at `fresh_at` open cells that no other
    point visits (the last point of a stream is then visible whatever the cells before it hold)."""
    pool = _pool(rng, grid)
    spare = min(8, len(pool) - 1)
    keys = pool[rng.integers(0, len(pool) - spare, n)]
    keys[rng.random(n) < outside] = -1
    for j, at in enumerate(fresh_at):
        if spare and 0 <= at < n:
            keys[at] = pool[len(pool) - 1 - j % spare]
    return keys


# -- family 2: points ---------------------------------------------------------------------------------------------------------
def point_counts(t):
    return sorted({1, 63, 64, 65, t - 1, t, t + 1, 2 * t, 2 * t + 1})


def points_cases():
    out = []
    for t, f2, f3 in ((4096, ("tiled", "gather", "s0", "payload", "wave", "prio"), ("w3d", "tiled", "gather")),
                      (8192, ("s1",), ("w3d_s1",)), (10240, ("s2",), ("w3d_s2",)), (5120, ("s3", "s4"), ())):
        counts = point_counts(t)
        if t == 4096:
            counts = sorted(set(counts) | {2047, 2048, 2049, 64 * 4096 + 1, 65 * 4096 + 1})   # the sort path's tiles; the
        for n in counts:                                    # directory scan's second round of 64 tiles, vw_pow2_above 64 / 128
            for gname, grid, forms in (("pillar", PILLAR, f2), ("big", BIG, f3)):
                if not forms or (n > 3 * t and gname == "big"):
                    continue
                out.append(_unit_case(f"points-{gname}-T{t}-N{n}", "points", grid,
                                      lambda rng, grid=grid, n=n: _random_keys(rng, grid, n, fresh_at=(n - 1,)), 5, 5000,
                                      forms=forms, claim={"T": t, "N": n}))
        for gname, grid, forms in (("pillar", PILLAR, f2), ("big", BIG, f3)):
            if forms:
                n = 2 * t + 1
                out.append(_unit_case(f"points-{gname}-T{t}-ragged", "points", grid,
                                      lambda rng, grid=grid, n=n, t=t: np.stack(
                                          [_random_keys(rng, grid, n, fresh_at=(m - 1,)) for m in (0, 1, t, n)]),
                                      5, 5000, forms=forms, claim={"T": t, "N": n}, lens=[0, 1, t, n]))
    return out


# -- family 3: groups ---------------------------------------------------------------------------------------------------------
GROUP_GRID_2D = (512, 512, 1)      # 2^18 cells: 256 groups of 1024 cells in the wave form, 64 groups in the tiled form
GROUP_GRID_3D = (512, 512, 16)     # 2^22 cells: 4096 possible cells per group of the 3-D form
GROUP_T = 4096
LAYOUTS = ("one", "spread", "end")


def _group_stream(rng, grid, gbits, group, records, cells, layout, t=GROUP_T):
    """Keys of one frame in which `group` receives exactly `records` records in `cells` distinct cells; the rest are
    shuffled background points of other groups.  one: all in route tile 0; spread: over tiles 0, 2 and 5 of six and a half,
    tiles 1, 3, 4 and 6 without any; end: a run ending exactly at tile 0's last point, the rest in tile 2."""
    ncells = grid[0] * grid[1] * grid[2]
    gk = keys_of_group(group, gbits, ncells)
    mine = gk[rng.choice(len(gk), cells, replace=False)]
    fresh = min(3, cells)     # the stream's last records open cells of their own: a lost last step shows
    body = cells - fresh
    rec = np.concatenate([mine[:body], mine[rng.integers(0, body, records - cells)] if body else mine[:0]])
    rng.shuffle(rec)
    rec = np.concatenate([rec, mine[body:]])
    assert len(rec) == records
    n = {"one": 2 * t, "spread": 6 * t + 17, "end": 3 * t}[layout]
    bg = _pool(rng, grid, 6000)
    bg = bg[group_of(bg, gbits) != group]
    keys = bg[rng.integers(0, len(bg), n)]
    keys[rng.random(n) < 0.03] = -1
    if layout == "one":
        assert records <= t
        pos = np.sort(rng.choice(t, records, replace=False))
    elif layout == "spread":
        share = [records // 3, records // 3, records - 2 * (records // 3)]
        pos = np.concatenate([np.sort(rng.choice(t, min(s, t), replace=False)) + tile * t
                              for s, tile in zip(share, (0, 2, 5))])
    else:
        run = min(records, 64 + records // 2)
        pos = np.concatenate([np.arange(t - run, t), 2 * t + np.sort(rng.choice(t, records - run, replace=False))])
    keys[pos] = rec
    return keys


def groups_cases():
    out = []
    f2 = ("wave", "s0", "s1", "prio", "payload", "tiled", "gather")
    for r in (1, 63, 64, 65, VW_REG - 1, VW_REG, VW_REG + 1, 2625):
        for layout in LAYOUTS:
            cells = min(r, 150)
            out.append(_unit_case(f"groups-2d-R{r}-{layout}", "groups", GROUP_GRID_2D,
                                  lambda rng, r=r, cells=cells, layout=layout: _group_stream(
                                      rng, GROUP_GRID_2D, 8, 77, r, cells, layout),
                                  4, 9000, forms=f2, claim={"gbits": 8, "group": 77, "records": r, "cells": cells,
                                                            "layout": layout}))
    f3 = ("w3d", "w3d_s1", "tiled", "gather")
    for r, cells in ((V3_REG - 1, 100), (V3_REG, 100), (V3_REG + 1, 100),
                     (2 * V3_LOAD, V3_LOAD - 1), (2 * V3_LOAD, V3_LOAD), (2 * V3_LOAD, V3_LOAD + 1)):
        for layout in LAYOUTS:
            out.append(_unit_case(f"groups-3d-R{r}-C{cells}-{layout}", "groups", GROUP_GRID_3D,
                                  lambda rng, r=r, cells=cells, layout=layout: _group_stream(
                                      rng, GROUP_GRID_3D, 10, 5, r, cells, layout),
                                  4, 9000, forms=f3, claim={"gbits": 10, "group": 5, "records": r, "cells": cells,
                                                            "layout": layout}))
    return out


# -- family 4: slots ----------------------------------------------------------------------------------------------------------
def _slot_keys(rng, grid, mults):
    pool = _pool(rng, grid)
    cells = pool[rng.choice(len(pool), len(mults) + 50, replace=False)]
    keys = np.concatenate([np.repeat(cells[: len(mults)], mults), cells[len(mults):]])
    rng.shuffle(keys)
    return keys


def slots_cases():
    out = []
    for p in (1, 2, 20, 254, 255):
        mults = sorted({m for m in (p - 1, p, p + 1, 2 * p, 300) if m > 0}) * 3
        for gname, grid in (("pillar", PILLAR), ("big", BIG)):
            out.append(_unit_case(f"slots-{gname}-P{p}", "slots", grid,
                                  lambda rng, grid=grid, mults=mults: _slot_keys(rng, grid, mults), p, 40,
                                  claim={"mults": tuple(mults), "refused": p > MAX_PTS}))
    return out


# -- family 5: voxels ---------------------------------------------------------------------------------------------------------
CAP_GRID = (128, 128, 1)      # 16384 cells


def _cap_keys(rng, grid, t, base, opens):
    """Two route tiles of t points: tile 0 opens `base` cells, tile 1 opens `opens` more (its other points fall into cells
    of tile 0); a third, short tile revisits kept and dropped cells."""
    pool = _pool(rng, grid, 16384)
    cells = pool[rng.permutation(len(pool))[: base + opens]]
    a, b = cells[:base], cells[base:]
    t0 = np.concatenate([a, a[rng.integers(0, base, t - base)]])
    t1 = np.concatenate([b, a[rng.integers(0, base, t - opens)]])
    rng.shuffle(t0)
    rng.shuffle(t1)
    t2 = cells[rng.integers(0, base + opens, 300)]
    return np.concatenate([t0, t1, t2])


def _hold_keys(rng, grid, gbits, t, wanted):
    """Tile 0 and tile 1 of t points each: in both, group g opens exactly wanted[g] cells (other groups open what the
    background gives them)."""
    ncells = grid[0] * grid[1] * grid[2]
    tiles = []
    for tile in range(2):
        firsts = np.concatenate([keys_of_group(g, gbits, ncells)[tile * 300: tile * 300 + c] for g, c in wanted.items()])
        bgp = _pool(rng, grid, 3000)
        bgp = bgp[~np.isin(group_of(bgp, gbits), list(wanted))]
        body = np.concatenate([firsts, firsts[rng.integers(0, len(firsts), 200)], bgp[rng.integers(0, len(bgp), t)]])[:t]
        rng.shuffle(body)
        tiles.append(body)
    return np.concatenate(tiles)


def voxels_cases():
    out = []
    c = 300
    for v in (1, c - 1, c, c + 1):     # the cut inside a route tile
        out.append(_unit_case(f"voxels-inside-C{c}-V{v}", "voxels", CAP_GRID,
                              lambda rng: _slot_keys(rng, CAP_GRID, [3] * (c - 50)), 2, v, claim={"cells": c}))
    for gname, grid in (("pillar", CAP_GRID), ("big", BIG)):
        for v in (999, 1000, 1001):    # the cut exactly at tile 0's end (it opens 1000 cells)
            out.append(_unit_case(f"voxels-{gname}-tile-end-V{v}", "voxels", grid,
                                  lambda rng, grid=grid: _cap_keys(rng, grid, 4096, 1000, 700), 2, v,
                                  claim={"T": 4096, "firsts": (1000, 700)}))
    for t, f2, f3 in ((8192, ("s1",), ("w3d_s1",)), (10240, ("s2",), ("w3d_s2",))):
        for opens in (ASSIGN_CAP - 1, ASSIGN_CAP, ASSIGN_CAP + 1, t):
            if opens == t and t == 10240:
                base = 0   # a pool of 16384 cells: the whole tile of 10240 points opens cells, nothing before it
            else:
                base = 100
            for gname, grid, forms in (("pillar", CAP_GRID, f2), ("big", BIG, f3)):
                for v in (base + opens + 10, base + ASSIGN_CAP, base + ASSIGN_CAP + 1, base + ASSIGN_CAP + 50):
                    if base == 0:
                        keys_fn = lambda rng, grid=grid, t=t: (   # noqa: E731
                            lambda opened: np.concatenate([opened, opened[rng.integers(0, t, 300)]]))(
                                _pool(rng, grid, 16384)[rng.permutation(16384)[:t]])
                    else:
                        keys_fn = lambda rng, grid=grid, t=t, base=base, opens=opens: _cap_keys(  # noqa: E731
                            rng, grid, t, base, opens)
                    out.append(_unit_case(f"voxels-{gname}-T{t}-opens{opens}-V{v}", "voxels", grid, keys_fn, 2, v,
                                          forms=forms + ("wave", "gather"),
                                          claim={"T": t, "firsts": (base, opens) if base else (opens,)}))
    # kHold: first points of a (tile, group) piece per thread.  1024 groups: a thread per group, pieces of 8 and 9;
    # 256 groups: two threads per group, pieces of 16 / 17 / 18 (shares 8 + 8, 8 + 9, 9 + 9); 16 groups: 32 threads per
    # group, pieces of 256, 261 and 288 (shares of 8, 8 or 9, 9)
    for name, grid, gbits, wanted in (("g1024", (1024, 1024, 1), 10, {3: 8, 700: 9, 512: 7, 1023: 16, 0: 17}),
                                      ("g256", GROUP_GRID_2D, 8, {3: 16, 100: 17, 255: 18}),
                                      ("g16", CAP_GRID, 4, {3: 256, 9: 261, 15: 288})):
        out.append(_unit_case(f"voxels-hold-{name}", "voxels", grid,
                              lambda rng, grid=grid, gbits=gbits, wanted=wanted: _hold_keys(rng, grid, gbits, 4096, wanted),
                              2, 9000, forms=("wave", "s0", "prio", "payload"),
                              claim={"T": 4096, "gbits": gbits, "hold": tuple(sorted(wanted.items()))}))
    return out


# -- family 6: grids ----------------------------------------------------------------------------------------------------------
GRIDS = [(1, 1, 1), (2, 1, 1), (4, 4, 1), (3, 5, 7), (1023, 1, 1), (1, 1024, 1), (1024, 1024, 1), (1025, 1024, 1),
         (2048, 2048, 1), (2049, 2048, 1), (16384, 16384, 1), (16385, 16384, 1)]
ROWQ_CASES = [(ROW_LIMIT - 1, True), (ROW_LIMIT, False)]   # (V at P = 1, D = 4; taken by the fast forms)


def _grid_keys(rng, grid, n=3000):
    ncells = grid[0] * grid[1] * grid[2]
    pool = _pool(rng, grid, 1000)
    keys = pool[rng.integers(0, len(pool), n)]
    keys[rng.random(n) < 0.05] = -1
    keys[7], keys[n // 2] = ncells - 1, 0
    return keys


def grids_cases():
    out = []
    for grid in GRIDS:
        name = "x".join(map(str, grid))
        for d in ((4, 3) if grid == (1025, 1024, 1) else (4,)):
            out.append(_unit_case(f"grids-{name}-D{d}", "grids", grid, lambda rng, grid=grid: _grid_keys(rng, grid), 3,
                                  1200, D=d, claim={"ends": True}))
    return out


# -- family 7: rows -----------------------------------------------------------------------------------------------------------
def rows_cases():
    out = []
    for d in (3, 4, 5, 6, 7, 8):
        for p in (3, 4):
            for gname, grid in (("pillar", PILLAR), ("big", BIG)):
                if gname == "big" and d not in (4, 5):
                    continue
                out.append(_unit_case(f"rows-{gname}-D{d}-P{p}", "rows", grid,
                                      lambda rng, grid=grid: _random_keys(rng, grid, 3000), p, 1500, D=d, index=False,
                                      claim={"rowmod": (p * d) % 4}))
    return out


# -- family 8: batch ----------------------------------------------------------------------------------------------------------
def batch_cases():
    out = []
    n = 5000
    for b in (1, 2, 3, 8, 9):
        lens = [n, 0, 4097, 1, 63, n, 2048, 4096, 333][:b] if b > 1 else [n]
        for gname, grid in (("pillar", PILLAR), ("big", BIG)):
            if gname == "big" and b not in (3, 8):
                continue
            out.append(_unit_case(f"batch-{gname}-B{b}", "batch", grid,
                                  lambda rng, grid=grid, b=b: np.stack([_random_keys(rng, grid, n) for _ in range(b)]),
                                  4, 2500, index=False, lens=lens, claim={"B": b}))
    return out


# -- family 1: cells ----------------------------------------------------------------------------------------------------------
CELL_GRIDS = [
    # name, voxel size, range, dyadic axes (the bare multiply is exact there)
    ("nusc-pillar", (0.2, 0.2, 8.0), (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0), (2,)),
    ("kitti-pillar", (0.16, 0.16, 4.0), (0.0, -39.68, -3.0, 69.12, 39.68, 1.0), (2,)),
    ("nusc-0075", (0.075, 0.075, 0.2), (-54.0, -54.0, -5.0, 54.0, 54.0, 3.0), ()),
    ("dyadic-025", (0.25, 0.25, 8.0), (-50.0, -50.0, 0.0, 50.0, 50.0, 8.0), (0, 1, 2)),
    ("third", (1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0), (0.0, 0.0, 0.0, 20.0, 20.0, 20.0), ()),
]
ULPS = 6
DENORM = float(np.finfo(np.float32).smallest_subnormal)
FLT_MAX = float(np.finfo(np.float32).max)


def _ulp_walk(x, k):
    """fp32 x moved k ulps (k < 0: down)."""
    x = np.asarray(x, np.float32).copy()
    to = np.float32(np.inf if k > 0 else -np.inf)
    for _ in range(abs(k)):
        x = np.nextafter(x, to)
    return x


def single_cell_bounds(size):
    """vt_single_cell_bounds in NumPy: [lo, hi] = { t : floor(fp32(t / size)) == 0 }."""
    s = np.float32(size)
    h = np.float32(size)
    while not np.float32(h / s) < np.float32(1.0):
        h = np.nextafter(h, np.float32(-np.inf))
    lo = np.float32(-0.0)
    for _ in range(64):
        nxt = np.nextafter(lo, np.float32(-np.inf))
        if np.float32(nxt / s) == 0:
            lo = nxt
        else:
            break
    return lo, h


def axis_values(vs, pr, axis):
    """The fp32 coordinates the cells family puts on `axis`: every boundary -2 .. extent + 2, computed in fp32 and in float64
    then rounded, each at 0, +-1 .. +-6 ulps; the two bounds of the single-cell z test and their outer neighbours; around
    a zero minimum +-0, +-1 / 4 / 5 / 8 x the smallest denormal, +-1e-40; size * 2^20 and its neighbours, 1e30, +-FLT_MAX;
    NaN and +-inf."""
    lo32, s32 = np.float32(pr[axis]), np.float32(vs[axis])
    extent = grid_of(vs, pr)[axis]
    k = np.arange(-2, extent + 3)
    b32 = (lo32 + k.astype(np.float32) * s32).astype(np.float32)
    b64 = (np.float64(pr[axis]) + k * np.float64(vs[axis])).astype(np.float32)
    base = np.concatenate([b32, b64])
    vals = [_ulp_walk(base, u) for u in range(-ULPS, ULPS + 1)]
    zlo, zhi = single_cell_bounds(s32)
    with np.errstate(all="ignore"):
        edge = [np.float32(lo32 + t) for t in (zlo, np.nextafter(zlo, np.float32(-np.inf)), zhi,
                                               np.nextafter(zhi, np.float32(np.inf)))]
        big = np.float32(lo32 + s32 * np.float32(2.0 ** 20))
    special = edge + [_ulp_walk(big, u) for u in (-1, 0, 1)] + [1e30, -1e30, FLT_MAX, -FLT_MAX, np.nan, np.inf, -np.inf]
    if pr[axis] == 0.0:
        for m in (0.0, 1 * DENORM, 4 * DENORM, 5 * DENORM, 8 * DENORM, 1e-40):
            special += [m, -m]
    return np.concatenate([np.concatenate(vals), np.asarray(special, np.float32)]).astype(np.float32)


def edge_cells(points, vs, pr):
    """Per axis the cell of the fp32 rule clamped into the grid (NaN -> 0): a point's own cell, or the edge cell a point
    outside the range would join if a kernel took it in.  [N, 3] int64 (x, y, z)."""
    pts = np.asarray(points, np.float32)[:, :3]
    vs, pr = np.asarray(vs, np.float32), np.asarray(pr, np.float32)
    grid = np.asarray(grid_of(vs, pr), np.float64)
    with np.errstate(all="ignore"):
        q = np.floor((pts - pr[:3]) / vs).astype(np.float64)
    q = np.nan_to_num(q, nan=0.0, posinf=1e30, neginf=-1e30)
    return np.clip(q, 0, grid - 1).astype(np.int64)


def earlier_inside(points, vs, pr):
    """For every point the number of EARLIER points inside the range in its edge_cells cell.  Below P for every point means
    that every point is decisive: an inside point holds a slot, an outside point wrongly taken in would get one."""
    gx, gy, _ = grid_of(vs, pr)
    e = edge_cells(points, vs, pr)
    key = (e[:, 2] * gy + e[:, 1]) * gx + e[:, 0]
    _, inside = ref_cells(points, vs, pr)
    order = np.argsort(key, kind="stable")
    ks, ins = key[order], inside[order].astype(np.int64)
    cum = np.cumsum(ins) - ins                                   # inside points before this one, over the whole order
    start = np.searchsorted(ks, ks, side="left")                 # first position of the point's cell
    out = np.empty(len(key), np.int64)
    out[order] = cum - cum[start]
    return out


def cell_points(vs, pr, axis, rng, d=4):
    """Points [N, d] with axis_values on `axis`, every one ALONE in its cell: the n-th point of a cell along `axis` (for a
    point outside, of the edge cell it would join) lies in the n-th cell of the plane of the other two axes, at a random
    mid-cell offset.  With three sweeps in a frame a cell holds at most three points, so P = 3 hides none."""
    vals = axis_values(vs, pr, axis)
    grid = grid_of(vs, pr)
    probe = np.zeros((len(vals), 3), np.float32)
    probe[:, axis] = vals
    own = edge_cells(probe, vs, pr)[:, axis]
    order = np.argsort(own, kind="stable")
    so = own[order]
    nth = np.empty(len(vals), np.int64)
    nth[order] = np.arange(len(vals)) - np.searchsorted(so, so, side="left")
    a1, a2 = [a for a in range(3) if a != axis]
    assert nth.max() < grid[a1] * grid[a2], (axis, int(nth.max()))
    pts = rng.standard_normal((len(vals), d)).astype(np.float32)
    pts[:, axis] = vals
    for a, cells in ((a1, nth % grid[a1]), (a2, nth // grid[a1])):
        pts[:, a] = (np.float64(pr[a]) + (cells + rng.uniform(0.3, 0.7, len(vals))) * np.float64(vs[a])).astype(np.float32)
    return pts


def cells_cases():
    out = []
    for name, vs, pr, _ in CELL_GRIDS:
        def build(rng, vs=vs, pr=pr):
            return np.concatenate([cell_points(vs, pr, a, rng) for a in range(3)]), None

        key, inside = keys_of_points(build(np.random.default_rng(_seed(f"cells-{name}")))[0], vs, pr)
        occupied = len(np.unique(key[inside]))
        out.append(Case(f"cells-{name}", "cells", vs, pr, 3, occupied + 7, 4, FAST, build,
                        (("occupied", occupied),), False))
    return out


# the rule of vt_axis_cell and the bare multiply, emulated in fp32 NumPy (the CPU file compares both with ref_cells)
def axis_cell_band(p, lo, size, extent, fallback=True):
    p, lo, size = np.asarray(p, np.float32), np.float32(lo), np.float32(size)
    inv = np.float32(1.0 / np.float64(size))
    with np.errstate(all="ignore"):
        t = p - lo
        m = t * inv
        q = np.floor(m)
        frac = m - q
        tol = np.abs(m) * np.float32(2.0 ** -21) + np.float32(2.0 ** -30)
        sure = (frac >= tol) & (frac <= np.float32(1.0) - tol) & (np.abs(m) < np.float32(1048576.0))
        if fallback:
            q = np.where(sure, q, np.floor(t / size))
        assert q.dtype == np.float32 and tol.dtype == np.float32
        inside = (q >= 0) & (q < np.float32(extent))
    return np.where(inside, q, -1).astype(np.int64)


@lru_cache(maxsize=None)
def all_cases():
    cases = (cells_cases() + points_cases() + groups_cases() + slots_cases() + voxels_cases() + grids_cases() +
             rows_cases() + batch_cases())
    return tuple(cases)


def family(name):
    return [c for c in all_cases() if c.family == name]


def index_cases():
    return [c for c in all_cases() if c.index]


# ---- references per case, made once ----------------------------------------------------------------------------------------
_PORT = {}


def port_reference(oracle, case: Case, b=0):
    """The oracle port's (voxels, coords, counts, num_voxels) of frame b's own points; made once and shared."""
    if (case.id, b) not in _PORT:
        pts = np.ascontiguousarray(frame_points(case, b))
        if len(pts) == 0:
            _PORT[case.id, b] = ref_hard_voxelize(pts.reshape(0, case.D), case.vs, case.pr, case.P, case.V)
        else:
            _PORT[case.id, b] = oracle.hard_voxelize(pts, case.vs, case.pr, case.P, case.V, "port")
    return _PORT[case.id, b]


def first_points(case: Case, b=0):
    """(keys of frame b's inside points in input order, positions of those points, True where a point opens its cell)."""
    pts = frame_points(case, b)
    key, inside = keys_of_points(pts, case.vs, case.pr)
    pos = np.nonzero(inside)[0]
    k = key[pos]
    first = np.zeros(len(k), bool)
    first[np.unique(k, return_index=True)[1]] = True
    return k, pos, first


# ---- device calls (GPU tests only) -----------------------------------------------------------------------------------------
def status_of(exc):
    m = re.search(r"status (-?\d+)", str(exc))
    return int(m.group(1)) if m else None


def misaligned(t):
    """A contiguous copy of `t` whose data_ptr() % 16 == 4."""
    import torch

    step = 4 // t.element_size()
    buf = torch.empty(t.numel() + step, dtype=t.dtype, device=t.device)
    view = buf[step:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def device_input(case: Case, misalign=False):
    import torch

    frames, lens = data(case)
    pts = torch.from_numpy(frames.copy()).cuda()   # (the cached frames are read-only)
    if misalign:
        pts = misaligned(pts)
    num = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
    return pts, num


def run(case: Case, form, coors=False, misalign=False, inputs=None):
    """The case through ops.voxelize.hard_voxelize_batch on `form`: (status, host arrays or None).  Status 0, or the
    negative status the library answered with."""
    import torch

    from paddle3d_amd._lib import Paddle3DAmdError
    from paddle3d_amd.ops import voxelize

    pts, num = inputs if inputs is not None else device_input(case, misalign)
    try:
        out = voxelize.hard_voxelize_batch(pts, list(case.vs), list(case.pr), case.P, case.V, num_points=num,
                                           with_batch_coors=coors, path=FORMS[form])
    except Paddle3DAmdError as e:
        status = status_of(e)
        if status is None:
            raise
        return status, None
    torch.cuda.synchronize()
    return 0, [o.cpu().numpy() for o in out]


def run_raw(case: Case, form, misalign_voxels=False, inputs=None):
    """pd3_hard_voxelize_path through the C ABI, the way ops/voxelize.py calls it: (status, device tensors).  The outputs have
    their full size and start out filled with -7 (a refusal must leave them so); misalign_voxels: the voxels tensor at
    data_ptr() % 16 == 4."""
    import torch

    from paddle3d_amd.ops._common import host_f32, lib, ptr, stream_ptr, workspace

    pts, num = inputs if inputs is not None else device_input(case)
    b, n, d = pts.shape
    vs, pr = host_f32(case.vs, 3), host_f32(case.pr, 6)
    L = lib()
    ws_bytes = L.pd3_hard_voxelize_workspace(b, n, d, ptr(vs), ptr(pr), case.P, case.V)
    assert ws_bytes > 0, case.id
    ws = workspace(ws_bytes, pts.device)
    voxels = torch.full((b, case.V, case.P, d), -7.0, dtype=torch.float32, device=pts.device)
    if misalign_voxels:
        voxels = misaligned(voxels)
    coords = torch.full((b, case.V, 3), -7, dtype=torch.int32, device=pts.device)
    npv = torch.full((b, case.V), -7, dtype=torch.int32, device=pts.device)
    nv = torch.full((b,), -7, dtype=torch.int32, device=pts.device)
    status = L.pd3_hard_voxelize_path(ptr(pts), ptr(num), b, n, d, ptr(vs), ptr(pr), case.P, case.V, ptr(voxels), ptr(coords),
                                      ptr(npv), ptr(nv), None, ptr(ws), ws.numel(), stream_ptr(pts.device), FORMS[form])
    torch.cuda.synchronize()
    return status, (voxels, coords, npv, nv)


def run_index(case: Case, inputs=None):
    """The case through hard_voxelize_index_batch: None where the library answers None, else host arrays (voxels rebuilt from
    (vox_span, point_list) [B, V, P, D], coords, counts, num_voxels, coors)."""
    import torch

    from paddle3d_amd.ops import voxelize

    pts, num = inputs if inputs is not None else device_input(case)
    out = voxelize.hard_voxelize_index_batch(pts, list(case.vs), list(case.pr), case.P, case.V, num_points=num)
    if out is None:
        return None
    torch.cuda.synchronize()
    span, plist, coords, npv, nv, c4 = [o.cpu().numpy() for o in out]
    frames, _ = data(case)
    b, n, d = frames.shape
    voxels = np.zeros((b, case.V, case.P, d), np.float32)
    for f in range(b):
        m = int(nv[f])
        start, count = span[f, :m, 0].astype(np.int64), span[f, :m, 1].astype(np.int64)
        assert (count >= 0).all() and (count <= case.P).all() and (start >= 0).all() and (start + count <= n).all(), case.id
        vox = np.repeat(np.arange(m), count)
        slot = np.arange(len(vox)) - np.repeat(np.cumsum(count) - count, count)
        src = plist[f * n + np.repeat(start, count) + slot]
        assert ((src >= 0) & (src < n)).all(), case.id
        voxels[f, vox, slot] = frames[f, src]
    return voxels, coords, npv, nv, c4


def run_dynamic(case: Case):
    import torch

    from paddle3d_amd.ops import voxelize

    frames, _ = data(case)
    co = voxelize.dynamic_voxelize(torch.from_numpy(frames[0].copy()).cuda(), list(case.vs), list(case.pr))
    torch.cuda.synchronize()
    return co.cpu().numpy()
