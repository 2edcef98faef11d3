"""The camera-to-BEV chain's border lattice: stable argsort, voxel_pooling_prepare, bev_pool_v2 forward / backward and
frustum_to_lidar (a helper module like tests/voxel_lattice.py, not a conftest).

* plan() restates radix_plan (csrc/radix_sort.hpp) and scan_num_tiles / scan_partials_kernel's `per` (csrc/scan.hpp) for the
  [digit][tile] table, so that every case can say which plan it runs; source_constants() reads the constants this module
  restates out of the kernels' sources, and tests/test_pool_lattice_cpu.py holds the two together.
* ref_argsort, ref_prepare, ref_pool_fwd / ref_pool_bwd and ref_frustum_to_lidar are plain NumPy restatements of the
  operations; the CPU file holds each to a second implementation (torch.argsort, oracle.pyoracle, the oracle port).
* the case families are crosses, not products; every builder draws from a seed derived from the case id.  Structural
  families use unit grids (lower 0, step 1, points at cell + 0.5), so that a case's claim is exact.

Everything here runs on the CPU except the run_* wrappers, which the GPU tests use.
"""
from __future__ import annotations

import os
import re
import zlib
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

# ---- the constants of radix_sort.hpp / scan.hpp / bev_pool.hip, restated -----------------------------------------------------
RS_THREADS, RS_ROUNDS, RS_MAX_BINS = 256, 8, 1024      # kRsThreads, kRsRounds, kRsMaxBins
RS_TILE = RS_THREADS * RS_ROUNDS                       # kRsTile: 2048 keys per workgroup
SCAN_THREADS, SCAN_ITEMS = 256, 16                     # kScanThreads, kScanItems
SCAN_TILE = SCAN_THREADS * SCAN_ITEMS                  # kScanTile: 4096 ints
PARTIALS_THREADS = 1024                                # scan_partials_kernel's one workgroup
DIGIT_MAX = 10                                         # radix_plan: passes = ceil(bits / 10)
BLOCK = 256                                            # the launch blocks of argsort.hip / bev_pool.hip
POOL_U = 16                                            # the load batch of the three pool kernels
MAX_CELLS = 1 << 31                                    # pd3_voxel_pooling_prepare: cells - 1 must fit int32
CLAMP = 9.2e18                                         # vpp_key_kernel: quotients beyond it count as outside

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "paddle3d_amd", "csrc")


def source_constants():
    """The constants above as the kernels' sources state them (every pattern must match: a renamed or removed constant is
    an error here, not a silent pass)."""
    def read(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()

    def one(text, pattern):
        m = re.findall(pattern, text)
        assert len(m) >= 1 and len(set(m)) == 1, (pattern, m)
        return int(m[0])

    rs, sc, bp, ar = read("radix_sort.hpp"), read("scan.hpp"), read("bev_pool.hip"), read("argsort.hip")
    out = {
        "RS_THREADS": one(rs, r"constexpr int kRsThreads = (\d+);"),
        "RS_ROUNDS": one(rs, r"constexpr int kRsRounds = (\d+);"),
        "RS_MAX_BINS": one(rs, r"constexpr int kRsMaxBins = (\d+);"),
        "SCAN_THREADS": one(sc, r"constexpr int kScanThreads = (\d+);"),
        "SCAN_ITEMS": one(sc, r"constexpr int kScanItems = (\d+);"),
        "PARTIALS_THREADS": one(sc, r"ceil_div\(ntiles, (\d+)\)"),
        "DIGIT_MAX": one(rs, r"p\.passes = \(bits \+ 9\) / (\d+);"),
        "POOL_U": one(bp, r"constexpr int U = (\d+);"),
        "MAX_CELLS": 1 << one(bp, r"constexpr int64_t kMaxCells = \(int64_t\)1 << (\d+);"),
    }
    assert "kRsTile = kRsThreads * kRsRounds" in rs and "kScanTile = kScanThreads * kScanItems" in sc
    assert one(sc, r"__launch_bounds__\((\d+)\) void scan_partials_kernel") == out["PARTIALS_THREADS"]
    assert one(sc, r"block_exclusive_scan<(\d+)>\(sum, smem, total\);\n  for") == out["PARTIALS_THREADS"]
    blocks = set(re.findall(r"__launch_bounds__\((\d+)\)", bp + ar))
    assert blocks == {str(BLOCK)}, blocks
    assert len(re.findall(r"constexpr int U = \d+;", bp)) == 2 and bp.count("9.2e18f") == 2    # fwd + bwd feat share U
    return out


def _ceil_div(a, b):
    return -(-a // b)


@dataclass(frozen=True)
class Plan:
    bits: int
    passes: int
    digit_bits: int
    bins: int
    tiles: int        # radix tiles of RS_TILE keys
    hist_ints: int    # the [digit][tile] table
    scan_tiles: int   # scan tiles of SCAN_TILE ints over that table
    per: int          # table tiles per thread of scan_partials_kernel

    @property
    def name(self):
        return f"{self.passes}x{self.digit_bits}"


def plan(max_key, n):
    """radix_plan(max_key, n) and the scan over its [digit][tile] table."""
    assert 0 <= max_key <= 0xFFFFFFFF and n >= 1
    bits = 1
    while bits < 32 and (max_key >> bits) != 0:
        bits += 1
    passes = (bits + DIGIT_MAX - 1) // DIGIT_MAX
    digit_bits = (bits + passes - 1) // passes
    bins = 1 << digit_bits
    assert bins <= RS_MAX_BINS
    tiles = _ceil_div(n, RS_TILE)
    hist = bins * tiles
    st = _ceil_div(hist, SCAN_TILE)
    return Plan(bits, passes, digit_bits, bins, tiles, hist, st, _ceil_div(st, PARTIALS_THREADS))


PLANS = ("1x10", "2x6", "2x10", "3x7", "3x10", "4x8")
NS = (1, 2, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 6145)
MAX_KEYS = (0, 1, 1023, 1024, (1 << 20) - 1, 1 << 20, (1 << 30) - 1, 1 << 30, (1 << 31) - 1)
# the smallest n at which scan_partials_kernel runs with per = 2: the widest table is 1024 bins x tiles, i.e. one scan tile
# of 4096 ints per four radix tiles, and the kernel's 1024 threads take one scan tile each up to 4096 radix tiles
BIG_N, BIG_MAX_KEY = RS_TILE * (PARTIALS_THREADS * SCAN_TILE // RS_MAX_BINS) + 1, RS_MAX_BINS - 1


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def _rng(cid):
    return np.random.default_rng(_seed(cid))


# ---- references --------------------------------------------------------------------------------------------------------------
def ref_argsort(keys, mode):
    """mode 0: stable ascending order of int keys.  mode 1: stable descending order of fp32 keys from an explicit rank:
    every NaN (class 0), +inf (1), finite values by descending value with -0 == +0 (2), -inf (3)."""
    if mode == 0:
        return np.argsort(np.asarray(keys).astype(np.int64), kind="stable").astype(np.int64)
    k = np.asarray(keys, np.float32)
    cls = np.full(k.shape, 2, np.int64)
    cls[np.isnan(k)] = 0
    cls[np.isposinf(k)] = 1
    cls[np.isneginf(k)] = 3
    # fp32 -> float64 is exact; + 0.0 turns -0.0 into +0.0
    neg = np.where(cls == 2, -np.where(cls == 2, k, 0).astype(np.float64), 0.0) + 0.0
    return np.lexsort((neg, cls)).astype(np.int64)                 # lexsort is stable; the last key is the primary one


def ref_quotient(coor, lower, step):
    """fp32 (coor - lower) / step, the reference's rule."""
    c = np.asarray(coor, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        q = (c - np.asarray(lower, np.float32)) / np.asarray(step, np.float32)
    assert q.dtype == np.float32
    return q


def ref_cells(coor, lower, step, size):
    """(cells [n, 3] int64 (x, y, z), -1 rows where dropped; kept [n]): truncation toward zero, 0 <= cell < size per axis;
    NaN, infinite and beyond-int64 quotients are dropped explicitly."""
    q = ref_quotient(coor, lower, step)
    ok = np.isfinite(q) & (np.abs(q) <= np.float32(CLAMP))
    t = np.trunc(np.where(ok, q, np.float32(-1.0)))                # fp32, exact
    kept = np.all(ok & (t >= 0) & (t < np.asarray(size, np.float32)), axis=1)
    return np.where(kept[:, None], t, -1).astype(np.int64), kept


def ref_prepare(coor, batch, depth_bins, feat_hw, lower, step, size, mode):
    """(ranks_bev, ranks_depth, ranks_feat, interval_starts, interval_lengths) int32."""
    c = np.asarray(coor, np.float32).reshape(-1, 3)
    n = len(c)
    assert n % batch == 0
    gx, gy, gz = (int(s) for s in size)
    cells, kept = ref_cells(c, lower, step, size)
    idx = np.nonzero(kept)[0].astype(np.int64)
    x, y, z = cells[idx, 0], cells[idx, 1], cells[idx, 2]
    b = idx // (n // batch)
    key = ((b * gz + z) * gy + y) * gx + x if mode == 0 else ((b * gz + z) * gx + x) * gy + y
    assert len(key) == 0 or key.max() < (1 << 31), "the grid's cell ids do not fit int32"
    order = np.argsort(key, kind="stable")
    rb, rd = key[order], idx[order]
    rf = rd if mode == 1 else rd // (depth_bins * feat_hw) * feat_hw + rd % feat_hw
    head = np.ones(len(rb), bool)
    head[1:] = rb[1:] != rb[:-1]
    starts = np.nonzero(head)[0]
    lengths = np.diff(np.append(starts, len(rb)))
    return tuple(a.astype(np.int32) for a in (rb, rd, rf, starts, lengths))


def _interval_walk(starts, lengths):
    """For t = 0, 1, ...: (intervals longer than t, their t-th position)."""
    starts, lengths = np.asarray(starts, np.int64), np.asarray(lengths, np.int64)
    for t in range(int(lengths.max()) if len(lengths) else 0):
        live = np.nonzero(lengths > t)[0]
        yield live, starts[live] + t


def ref_pool_fwd(depth, feat, rd, rf, rb, lengths, starts, cells):
    """out [cells, C]: per interval and channel acc = f32(acc + f32(feat * depth)) in interval order."""
    d, f = np.asarray(depth, np.float32).reshape(-1), np.asarray(feat, np.float32)
    f = f.reshape(-1, f.shape[-1])
    acc = np.zeros((len(lengths), f.shape[1]), np.float32)
    with np.errstate(all="ignore"):
        for live, pos in _interval_walk(starts, lengths):
            prod = f[rf[pos]] * d[rd[pos]][:, None]
            acc[live] = acc[live] + prod
    assert acc.dtype == np.float32
    out = np.zeros((cells, f.shape[1]), np.float32)
    out[np.asarray(rb)[np.asarray(starts, np.int64)]] = acc
    return out


def ref_pool_bwd(out_grad, depth, feat, rd, rf, rb, lengths, starts):
    """(depth_grad like depth: per point, serial over channels; feat_grad like feat: per (interval, channel))."""
    d = np.asarray(depth, np.float32)
    f = np.asarray(feat, np.float32)
    f2 = f.reshape(-1, f.shape[-1])
    g = np.asarray(out_grad, np.float32).reshape(-1, f.shape[-1])
    dflat = d.reshape(-1)
    with np.errstate(all="ignore"):
        acc = np.zeros(len(rd), np.float32)
        gp, fp = g[rb], f2[rf]
        for ch in range(f2.shape[1]):
            acc = acc + gp[:, ch] * fp[:, ch]
        dg = np.zeros(dflat.shape, np.float32)
        dg[rd] = acc
        acc = np.zeros((len(lengths), f2.shape[1]), np.float32)
        for live, pos in _interval_walk(starts, lengths):
            acc[live] = acc[live] + g[rb[pos]] * dflat[rd[pos]][:, None]
        fg = np.zeros(f2.shape, np.float32)
        fg[np.asarray(rf)[np.asarray(starts, np.int64)]] = acc
    assert acc.dtype == np.float32 and dg.dtype == np.float32
    return dg.reshape(d.shape), fg.reshape(f.shape)


def resort_by_feat(rd, rf, rb):
    """The re-sort in front of bev_pool_v2_bkwd (BevPoolV2.backward): stable by ranks_feat, run-length encoded."""
    order = np.argsort(np.asarray(rf).astype(np.int64), kind="stable")
    rd2, rf2, rb2 = rd[order], rf[order], rb[order]
    head = np.ones(len(rf2), bool)
    head[1:] = rf2[1:] != rf2[:-1]
    starts = np.nonzero(head)[0]
    lengths = np.diff(np.append(starts, len(rf2)))
    return rd2, rf2, rb2, lengths.astype(np.int32), starts.astype(np.int32)


def ref_frustum_to_lidar(frustum, cams_per_batch, inv_post_rot, post_trans, cam_to_ego, trans, bda):
    """frustum [per_cam, 3], matrices [cams, 3, 3], vectors [cams, 3], bda [B, 3, 3] -> [cams * per_cam, 3], every step
    a separate fp32 operation in the kernel's order."""
    f32 = np.float32
    fr, a, c = np.asarray(frustum, f32), np.asarray(inv_post_rot, f32), np.asarray(cam_to_ego, f32)
    pt, tr, bd = np.asarray(post_trans, f32), np.asarray(trans, f32), np.asarray(bda, f32)
    cams = len(a)
    bd = bd[np.arange(cams) // cams_per_batch]

    def dot3(m, v, k):   # m [cams, 3, 3], v three [cams, per_cam] arrays: ((m0 * v0 + m1 * v1) + m2 * v2)
        return m[:, k, 0, None] * v[0] + m[:, k, 1, None] * v[1] + m[:, k, 2, None] * v[2]

    p = [fr[None, :, k] - pt[:, k, None] for k in range(3)]
    q = [dot3(a, p, k) for k in range(3)]
    p = [q[0] * q[2], q[1] * q[2], q[2]]
    q = [dot3(c, p, k) + tr[:, k, None] for k in range(3)]
    out = np.stack([dot3(bd, q, k) for k in range(3)], -1)
    assert out.dtype == f32
    return out.reshape(-1, 3)


# ---- family A: argsort -------------------------------------------------------------------------------------------------------
@dataclass(frozen=True, eq=False)
class SortCase:
    id: str
    mode: int
    n: int
    max_key: int
    build: object = field(repr=False, default=None)   # rng -> keys (int64 for mode 0, uint32 bit patterns for mode 1)
    kind: str = ""

    @property
    def plan(self):
        return plan(0xFFFFFFFF if self.mode == 1 else self.max_key, self.n)


_KEYS = {}


def sort_keys(case: SortCase):
    """mode 0: int32 keys; mode 1: float32 keys (made from bit patterns).  Made once, read-only."""
    if case.id not in _KEYS:
        k = np.asarray(case.build(_rng(case.id)))
        if case.mode == 0:
            assert len(k) == case.n and k.min() >= 0 and k.max() <= case.max_key, case.id
            k = k.astype(np.int32)
        else:
            assert len(k) == case.n and k.dtype == np.uint32, case.id
            k = k.view(np.float32)
        k.setflags(write=False)
        _KEYS[case.id] = k
    return _KEYS[case.id]


def digit_extremes(max_key):
    """Keys <= max_key whose single digits are all-zero or all-one under max_key's plan: per digit j the key with only
    digit j set to all ones, and max_key's own value with digit j cleared / filled (where that stays <= max_key)."""
    p = plan(max_key, 1)
    mask = (1 << p.digit_bits) - 1
    out = {0, max_key}
    for j in range(p.passes):
        m = mask << (j * p.digit_bits)
        for k in (m, max_key & ~m, max_key | m, m >> 1 & m, (m & max_key)):
            if 0 <= k <= max_key:
                out.add(int(k))
    return sorted(out)


def _sort_family_keys(kind, n, mk, rng):
    p = plan(mk, n)
    top_shift = (p.passes - 1) * p.digit_bits
    if kind == "equal":
        return np.full(n, mk // 3)
    if kind == "two":
        return np.where(rng.random(n) < 0.5, 0, mk)
    if kind == "top":        # only the top digit differs (the lower digits are one fixed pattern)
        low = (mk // 3) & ((1 << top_shift) - 1)
        hi = rng.integers(0, (mk >> top_shift) + 1, n)
        k = (hi << top_shift) | low
        return np.where(k > mk, low, k)
    if kind == "bottom":     # only the bottom digit differs (the upper digits are those of max_key / 2: no key exceeds max_key)
        mask = (1 << p.digit_bits) - 1
        return ((mk >> 1) & ~mask) | rng.integers(0, min(mask, mk) + 1, n)
    if kind == "extremes":
        pool = np.asarray(digit_extremes(mk), np.int64)
        return pool[rng.integers(0, len(pool), n)]
    if kind == "maxkey":
        k = rng.integers(0, mk + 1, n)
        k[rng.choice(n, max(1, n // 16), replace=False)] = mk
        k[0] = mk
        return k
    k = np.sort(rng.integers(0, mk + 1, n))
    return k if kind == "sorted" else k[::-1].copy()


SORT_KINDS = ("equal", "two", "top", "bottom", "extremes", "maxkey", "sorted", "reverse")
# bit patterns planted among the quantised scores of mode 1
F32_SPECIALS = np.array([
    0x80000000, 0x00000000,                                        # -0.0, +0.0: a tie in input order
    0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FA12345, 0xFFD54321,   # NaNs
    0x7F800000, 0xFF800000,                                        # +-inf
    0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,                # smallest / largest denormals
    0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF,                # smallest / largest normals
    0x3F800000, 0x3F800001, 0xBF800000, 0xBF800001, 0x00800001, 0x007FFFFE, 0x7F7FFFFE, 0xFF7FFFFE,   # adjacent in bits
], np.uint32)


def _f32_keys(n, rng):
    k = (np.round(rng.standard_normal(n) * 8) / 8).astype(np.float32).view(np.uint32).copy()
    m = min(n, 3 * len(F32_SPECIALS))
    pos = rng.choice(n, m, replace=False) if n > 2 else np.arange(m)
    k[pos] = np.resize(F32_SPECIALS, m)
    return k


def sort_cases():
    out = []
    for n in NS:
        for mk in (1023, 1 << 20, 1 << 30):     # 1x10, 3x7, 4x8 at every size
            out.append(SortCase(f"sort-n{n}-mk{mk}", 0, n, mk,
                                lambda rng, n=n, mk=mk: _sort_family_keys("maxkey", n, mk, rng), "sizes"))
        out.append(SortCase(f"sort-f32-n{n}", 1, n, 0xFFFFFFFF, lambda rng, n=n: _f32_keys(n, rng), "f32"))
    for n in (4 * RS_TILE, 4 * RS_TILE + 1):    # the [digit][tile] table of 1024 bins at one scan tile exactly, and at two
        out.append(SortCase(f"sort-table-n{n}", 0, n, RS_MAX_BINS - 1,
                            lambda rng, n=n: _sort_family_keys("maxkey", n, RS_MAX_BINS - 1, rng), "table"))
    n = RS_TILE + 1
    for mk in MAX_KEYS:
        kinds = ("equal",) if mk == 0 else (("equal", "two", "sorted", "reverse") if mk == 1 else SORT_KINDS)
        for kind in kinds:
            out.append(SortCase(f"sort-mk{mk}-{kind}", 0, n, mk,
                                lambda rng, kind=kind, mk=mk: _sort_family_keys(kind, n, mk, rng), kind))
    return out


def big_sort_case():
    """n = 2048 * 4096 + 1 keys below 1024: one pass, 1024 bins, 4097 radix tiles = 1025 scan tiles of the [digit][tile]
    table, so scan_partials_kernel runs with per = 2 -- the smallest n at which that branch runs at all (one pass of 1024
    bins is the widest table per key; 4096 radix tiles give exactly 1024 scan tiles, per = 1).  Keys (i * 389) % 1024:
    key k belongs to i = (k * 389^-1) % 1024 + 1024 * j, so the expected order is stated in closed form (big_sort_expected)
    and the case is never materialised on the host."""
    return SortCase("sort-big-per2", 0, BIG_N, BIG_MAX_KEY, None, "big")


BIG_MUL = 389


def big_sort_expected(p, n=BIG_N, mul=BIG_MUL, bins=BIG_MAX_KEY + 1):
    """order[p] of the big case for positions p (an integer array of any library with // and %): key 0 holds the indices
    0, 1024, .. (one more than the others when n % 1024 == 1), key k > 0 the indices i0(k) + 1024 * j."""
    assert n % bins == 1
    per = n // bins
    inv = pow(mul, -1, bins)
    q = p - (per + 1)                       # position among the keys >= 1
    k = 1 + q // per
    rest = (k * inv) % bins + bins * (q % per)
    return (p < per + 1) * (p * bins) + (p >= per + 1) * rest


# ---- families B, C, D: prepare -----------------------------------------------------------------------------------------------
@dataclass(frozen=True, eq=False)
class PrepCase:
    id: str
    family: str
    mode: int
    batch: int
    depth_bins: int
    feat_hw: int
    lower: tuple
    step: tuple
    size: tuple                  # (gx, gy, gz)
    build: object = field(repr=False, default=None)   # rng -> coor [n, 3] fp32
    claim: tuple = ()

    def c(self, key, default=None):
        return dict(self.claim).get(key, default)

    @property
    def cells(self):
        return self.batch * int(self.size[0]) * int(self.size[1]) * int(self.size[2])

    @property
    def plan(self):
        return plan(self.cells, len(coor_of(self)))


_COOR, _PREP = {}, {}


def coor_of(case: PrepCase):
    if case.id not in _COOR:
        c = np.ascontiguousarray(case.build(_rng(case.id)), np.float32).reshape(-1, 3)
        assert len(c) % case.batch == 0, case.id
        c.setflags(write=False)
        _COOR[case.id] = c
    return _COOR[case.id]


def prep_reference(case: PrepCase):
    """ref_prepare of the case, made once and shared (read-only)."""
    if case.id not in _PREP:
        ref = ref_prepare(coor_of(case), case.batch, case.depth_bins, case.feat_hw, case.lower, case.step, case.size,
                          case.mode)
        for a in ref:
            a.setflags(write=False)
        _PREP[case.id] = ref
    return _PREP[case.id]


UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def local_to_xyz(local, size, mode):
    """Cell id within one batch entry -> (x, y, z) under the mode's order."""
    gx, gy, gz = size
    local = np.asarray(local, np.int64)
    if mode == 0:
        return local % gx, (local // gx) % gy, local // (gx * gy)
    return (local // gy) % gx, local % gy, local // (gx * gy)


def unit_coor(local, size, mode, rng=None):
    """fp32 points [n, 3] at cell + 0.5 of a unit grid for per-point local cell ids (-1: outside the grid)."""
    local = np.asarray(local, np.int64)
    x, y, z = local_to_xyz(np.where(local < 0, 0, local), size, mode)
    out = np.stack([x, y, z], 1).astype(np.float32) + np.float32(0.5)
    bad = np.nonzero(local < 0)[0]
    if len(bad):   # outside on one axis, below or above, the other axes inside
        axis = np.arange(len(bad)) % 3 if rng is None else rng.integers(0, 3, len(bad))
        side = np.arange(len(bad)) % 2 if rng is None else rng.integers(0, 2, len(bad))
        out[bad, axis] = np.where(side == 0, -1.5, np.asarray(size, np.float32)[axis] + 1.5)
    return out


def _unit_case(cid, family, mode, batch, size, keys_fn, dhw=(1, 1), claim=()):
    """keys_fn(rng) -> [batch, per] local cell ids (the batch entry of a point is its position)."""
    def build(rng):
        local = np.asarray(keys_fn(rng), np.int64).reshape(batch, -1)
        return unit_coor(local.reshape(-1), size, mode, rng)

    return PrepCase(cid, family, mode, batch, dhw[0], dhw[1], UNIT[0], UNIT[1], tuple(float(s) for s in size), build,
                    tuple(sorted(dict(claim).items())))


def _random_local(rng, per_batch_cells, n, specials=(), outside=0.05, pool=300):
    cells = rng.integers(0, per_batch_cells, pool)
    k = cells[rng.integers(0, pool, n)]
    k[rng.random(n) < outside] = -1
    sp = np.asarray(sorted(specials), np.int64)
    if len(sp):
        reps = np.resize(sp, min(n, 3 * len(sp)))
        k[rng.choice(n, len(reps), replace=False)] = reps
    return k


SIZE_GRID, SIZE_BATCH = (16, 8, 4), 1
# cells = B * gx * gy * gz at the plan borders (the sort's largest key is `cells`, the key of a point outside the grid) and
# at the int32 border of ranks_bev: (gx, gy, gz, B)
PLAN_GRIDS = {
    1023: (33, 31, 1, 1), 1024: (32, 16, 2, 1), (1 << 20) - 1: (1025, 1023, 1, 1), 1 << 20: (1024, 512, 2, 1),
    (1 << 30) - 1: (32767, 32769, 1, 1), 1 << 30: (1024, 1024, 512, 2), 2047 << 20: (2047, 1024, 512, 2),
    1 << 31: (2048, 1024, 1024, 1),
}
# refused: the largest cell id does not fit int32 (2049 x 1024 x 1024 came back with negative ranks before the check moved),
# 2^32 - 1 and 2^32 cells (the former bound), and a product that wraps int64 (2^90 = 0 mod 2^64)
REFUSED_GRIDS = {
    "2049x1024x1024": (2049, 1024, 1024, 1), "1024x1024x1024xB3": (1024, 1024, 1024, 3),
    "65535x65537x1": (65535, 65537, 1, 1), "65536x65536x1": (65536, 65536, 1, 1),
    "2^30x2^30x2^30": (1 << 30, 1 << 30, 1 << 30, 1),
}
GRID_N = 3002


def _grid_keys(rng, grid, mode):
    """[B, per] local ids: random cells of a small pool, points outside, and -- as full keys b * cpb + local -- cell 0, the
    last cell and the digit extremes of the grid's plan, each in the batch entry it belongs to."""
    gx, gy, gz, b = grid
    cpb = gx * gy * gz
    special = [k for k in digit_extremes(cpb * b) if k < cpb * b] + [cpb * b - 1, 0]
    rows = []
    for e in range(b):
        mine = [k - e * cpb for k in special if e * cpb <= k < (e + 1) * cpb]
        rows.append(_random_local(rng, cpb, GRID_N // b, mine))
    return np.stack(rows)


def prep_size_cases():
    out = []
    gx, gy, gz = SIZE_GRID
    for n in NS:
        for mode in (0, 1, 2):
            out.append(_unit_case(f"prep-n{n}-m{mode}", "sizes", mode, SIZE_BATCH, SIZE_GRID,
                                  lambda rng, n=n: _random_local(rng, gx * gy * gz, n, (0, gx * gy * gz - 1)
                                                                 if n > 2 else ()), claim={"n": n}))
    for cells, grid in PLAN_GRIDS.items():
        for mode in (0, 1, 2):
            out.append(_unit_case(f"prep-cells{cells}-m{mode}", "grids", mode, grid[3], grid[:3],
                                  lambda rng, grid=grid, mode=mode: _grid_keys(rng, grid, mode), claim={"cells": cells}))
    return out


def refused_cases():
    out = []
    for name, grid in REFUSED_GRIDS.items():
        out.append(_unit_case(f"prep-refused-{name}", "refused", 0, grid[3], grid[:3],
                              lambda rng, grid=grid: np.zeros((grid[3], 100), np.int64)))
    return out


# -- family C: the coordinate rule on the real grids -----------------------------------------------------------------------------
def real_grids():
    from paddle3d_amd.bevfusion import gen_dx_bx
    from paddle3d_amd.ops.bev_pool_v2 import _lss_lower

    out = [("bevdet", (-51.2, -51.2, -5.0), (0.8, 0.8, 8.0), (128.0, 128.0, 1.0))]
    for name, bounds in (("lss-05", ([-50, 50, 0.5], [-50, 50, 0.5], [-5, 3, 0.5])),
                         ("lss-08", ([-51.2, 51.2, 0.8], [-51.2, 51.2, 0.8], [-10.0, 10.0, 20.0]))):
        dx, bx, nx = gen_dx_bx(*bounds)
        lower, dxn = _lss_lower(dx, bx)
        out.append((name, tuple(float(v) for v in lower), tuple(float(v) for v in dxn), tuple(float(v) for v in nx)))
    return out


def boundary_pair(lower, step, k, strict=False):
    """The two fp32 neighbours (lo, hi) between which the reference's quotient f32(f32(x - lower) / step) crosses k:
    quotient(lo) < k <= quotient(hi), hi = nextafter(lo, +inf); strict: quotient(lo) <= k < quotient(hi)."""
    lo32, s32, k32 = np.float32(lower), np.float32(step), np.float32(k)

    def at_or_above(x):
        q = np.float32(np.float32(x - lo32) / s32)
        return q > k32 if strict else q >= k32

    x = np.float32(lo32 + k32 * s32)
    for _ in range(4096):
        if at_or_above(x):
            below = np.nextafter(x, np.float32(-np.inf))
            if not at_or_above(below):
                return below, x
            x = below
        else:
            x = np.nextafter(x, np.float32(np.inf))
    raise AssertionError(("no crossing found", lower, step, k))


def axis_plants(lower, step, size, axis):
    """[(value, label, k)] for one axis: around lower + k * step for k in {-1, 0, 1, size - 1, size} the crossing pair of
    boundary_pair ('lo' / 'hi'; at k = -1 the strict pair: a quotient of exactly -1 truncates to -1 and is dropped, anything
    above it truncates to cell 0), the nominal fp32 boundary and its two neighbours ('near'); and the specials."""
    lo, st, sz = lower[axis], step[axis], int(size[axis])
    out = []
    for k in sorted({-1, 0, 1, sz - 1, sz}):
        a, b = boundary_pair(lo, st, k, strict=k < 0)
        out += [(a, "lo", k), (b, "hi", k)]
        x = np.float32(np.float32(lo) + np.float32(k) * np.float32(st))
        out += [(v, "near", k) for v in (np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf)))]
    big = np.float32(np.float32(CLAMP) * np.float32(st))
    specials = [-0.0, 0.0, np.nan, np.inf, -np.inf, 1e30, -1e30]
    for sgn in (1.0, -1.0):
        x = big
        specials += [sgn * v for v in (np.nextafter(np.nextafter(x, np.float32(0)), np.float32(0)),
                                       np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(np.inf)),
                                       np.nextafter(np.nextafter(x, np.float32(np.inf)), np.float32(np.inf)))]
    out += [(np.float32(v), "special", None) for v in specials]
    return out


def coord_points(lower, step, size, rng):
    """(coor [n, 3], plants [(point, axis, label, k)]): every planted value on its axis, the other two axes at the middle
    of a random cell."""
    rows, plants = [], []
    for axis in range(3):
        for v, label, k in axis_plants(lower, step, size, axis):
            p = [np.float32(np.float64(lower[a]) + (rng.integers(0, int(size[a])) + 0.5) * np.float64(step[a]))
                 for a in range(3)]
            p[axis] = v
            plants.append((len(rows), axis, label, k))
            rows.append(p)
    return np.asarray(rows, np.float32), plants


def coord_cases():
    out = []
    for name, lower, step, size in real_grids():
        for mode in (0, 1, 2):
            out.append(PrepCase(f"coord-{name}-m{mode}", "coord", mode, 1, 1, 1, lower, step, size,
                                lambda rng, g=(lower, step, size): coord_points(*g, rng)[0], (("grid", name),)))
    return out


def coord_plants(case: PrepCase):
    return coord_points(case.lower, case.step, case.size, _rng(case.id))[1]


# -- family D: occupancy ---------------------------------------------------------------------------------------------------------
ODD_GRID = (5, 3, 2)          # gx != gy != gz: modes 0 and 1 order its cells differently
WIDE_GRID = (71, 29, 2)       # 4118 cells: room for 4097 points in distinct cells
DHW = ((1, 1), (1, 7), (3, 5), (59, 1))


def _only_at(n, where, cell):
    k = np.full(n, -1, np.int64)
    k[list(where)] = cell
    return k


def occupancy_cases():
    out = []
    odd = ODD_GRID[0] * ODD_GRID[1] * ODD_GRID[2]
    wide = WIDE_GRID[0] * WIDE_GRID[1] * WIDE_GRID[2]
    for mode in (0, 1, 2):
        m = f"m{mode}"
        out.append(_unit_case(f"occ-none-{m}", "occupancy", mode, 1, ODD_GRID, lambda rng: np.full(300, -1),
                              claim={"kept": 0, "intervals": 0}))
        out.append(_unit_case(f"occ-onecell-{m}", "occupancy", mode, 1, ODD_GRID, lambda rng: np.full(4097, 17),
                              claim={"kept": 4097, "intervals": 1}))
        for n in (SCAN_TILE, SCAN_TILE + 1):
            out.append(_unit_case(f"occ-distinct{n}-{m}", "occupancy", mode, 1, WIDE_GRID,
                                  lambda rng, n=n: rng.permutation(wide)[:n], claim={"kept": n, "intervals": n}))
        for name, at in (("first", 0), ("last", 4096)):
            out.append(_unit_case(f"occ-{name}-{m}", "occupancy", mode, 1, ODD_GRID,
                                  lambda rng, at=at: _only_at(4097, (at,), 11), claim={"kept": 1, "intervals": 1}))
        out.append(_unit_case(f"occ-lastbatch-{m}", "occupancy", mode, 3, ODD_GRID,
                              lambda rng: np.stack([np.full(700, -1), np.full(700, -1), rng.integers(0, odd, 700)]),
                              claim={"kept": 700}))
        out.append(_unit_case(f"occ-interleave-{m}", "occupancy", mode, 2, ODD_GRID,
                              lambda rng: np.where(np.arange(4098) % 2 == 0, rng.integers(0, odd, 4098), -1),
                              claim={"kept": 2049}))
        for d, hw in DHW:
            per = {(1, 1): 257, (1, 7): 37 * 7, (3, 5): 19 * 15, (59, 1): 5 * 59}[d, hw]
            out.append(_unit_case(f"occ-order-D{d}-HW{hw}-{m}", "occupancy", mode, 2, ODD_GRID,
                                  lambda rng, per=per: np.stack([_random_local(rng, odd, per, range(odd), pool=30)
                                                                 for _ in range(2)]),
                                  dhw=(d, hw), claim={"dhw": (d, hw)}))
    return out


# ---- family E: pool tables -----------------------------------------------------------------------------------------------------
LENGTH_MIX = (1, 2, 15, 16, 17, 31, 32, 33, 48, 49)
POOL_CHANNELS = (1, 3, 64, 80, 255, 256, 257)


@dataclass(frozen=True, eq=False)
class PoolCase:
    id: str
    channels: int
    lengths: tuple
    source: str = ""             # id of the prepare case whose index sets are pooled (chain cases), else a built table


@dataclass(eq=False)
class PoolData:
    depth: np.ndarray            # [n_depth]
    feat: np.ndarray             # [rows, C]
    out_grad: np.ndarray         # [cells, C]
    cells: int
    fwd: tuple                   # (rd, rf, rb, lengths, starts): intervals by ranks_bev
    bwd: tuple                   # (rd, rf, rb, lengths, starts): intervals by ranks_feat


def _table(lengths, rng, group_space, other_space):
    """Points of intervals with the given lengths: `group` is constant per interval, distinct between intervals and not
    monotone; `other` is drawn from a small space (rows shared between intervals); `rd` a permutation into a depth array
    with unused entries."""
    lengths = np.asarray(lengths, np.int32)
    n = int(lengths.sum())
    starts = (np.cumsum(lengths) - lengths).astype(np.int32)
    group = np.repeat(rng.permutation(group_space)[: len(lengths)], lengths).astype(np.int32)
    other = rng.integers(0, other_space, n).astype(np.int32)
    rd = rng.permutation(n + 37)[:n].astype(np.int32)
    return rd, group, other, lengths, starts


def _values(rng, shape, specials=True):
    """Normal deviates; with `specials` two -0.0, and in arrays of 256 values or more one +inf and one -inf (few enough that
    most sums stay finite: a sum that has met an inf no longer shows what else went into it)."""
    v = rng.standard_normal(shape).astype(np.float32)
    if specials and v.size >= 8:
        flat = v.reshape(-1)
        pos = rng.choice(flat.size, 4, replace=False)
        flat[pos[:2]] = -0.0
        if flat.size >= 256:
            flat[pos[2]], flat[pos[3]] = np.inf, -np.inf
    return v


_POOL = {}


def pool_data(case: PoolCase):
    if case.id in _POOL:
        return _POOL[case.id]
    rng = _rng(case.id)
    c = case.channels
    if case.source:
        prep = {p.id: p for p in prepare_cases()}[case.source]
        rb, rd, rf, starts, lengths = (np.asarray(a) for a in prep_reference(prep))
        n = len(coor_of(prep))
        rows = n if prep.mode == 1 else ((n - 1) // (prep.depth_bins * prep.feat_hw)) * prep.feat_hw + prep.feat_hw
        cells, n_depth = prep.cells, n
        fwd = (rd, rf, rb, lengths, starts)
        bwd = resort_by_feat(rd, rf, rb)
        special = False
    else:
        ni = len(case.lengths)
        cells, rows = 2 * ni + 5, max(ni // 3, 4)
        rd, rb, rf, lengths, starts = _table(case.lengths, rng, cells, rows)
        fwd, n_depth = (rd, rf, rb, lengths, starts), len(rd) + 37
        lb = rng.permutation(np.asarray(case.lengths))
        rd2, rf2, rb2, l2, s2 = _table(lb, rng, 2 * ni + 5, cells)     # group = ranks_feat (rows 2 ni + 5), other = ranks_bev
        bwd = (rd2, rf2, rb2, l2, s2)
        special = ni > 1     # (an inf in the one interval of a single-interval table would turn every sum into inf / NaN)
    feat_rows = max(rows, int(bwd[1].max()) + 1 if len(bwd[1]) else 1)
    data = PoolData(_values(rng, (n_depth,), special), _values(rng, (feat_rows, c), special),
                    _values(rng, (cells, c), special), cells, fwd, bwd)
    _POOL[case.id] = data
    return data


_POOL_REF = {}


def pool_reference(case: PoolCase):
    """(out, depth_grad, feat_grad) of ref_pool_fwd / ref_pool_bwd on the case's data, made once and shared."""
    if case.id not in _POOL_REF:
        d = pool_data(case)
        _POOL_REF[case.id] = (ref_pool_fwd(d.depth, d.feat, *d.fwd, d.cells),) + ref_pool_bwd(d.out_grad, d.depth, d.feat,
                                                                                              *d.bwd)
    return _POOL_REF[case.id]


def pool_cases():
    out = []
    rng = _rng("pool-lengths")
    for c in POOL_CHANNELS:
        counts = (255, 256, 257) if c == 1 else (max(BLOCK // c + 2, len(LENGTH_MIX) + 1),)
        for ni in counts:
            lengths = np.resize(np.asarray(LENGTH_MIX), ni)
            out.append(PoolCase(f"pool-C{c}-I{ni}", c, tuple(int(v) for v in rng.permutation(lengths))))
    for c in (3, 64):
        out.append(PoolCase(f"pool-single100-C{c}", c, (100,)))
    return out


CHAIN_MAX_CELLS = 1 << 20     # the pooled output is [cells, C] fp32: larger grids stay with the prepare families


def chain_cases():
    """The index sets of families B-D (grids of up to 2^20 cells; the coordinate family on its real grids) pooled with
    three channels."""
    return [PoolCase(f"chain-{p.id}", 3, (), p.id) for p in prepare_cases() if p.cells <= CHAIN_MAX_CELLS]


# ---- family F: frustum ---------------------------------------------------------------------------------------------------------
@dataclass(frozen=True, eq=False)
class FrustumCase:
    id: str
    batch: int
    cams: int
    per_cam: int


def frustum_cases():
    return [FrustumCase(f"frustum-P{p}", 2, 3, p) for p in (1, 255, 257, 1000)]


def frustum_data(case: FrustumCase):
    """(frustum [per_cam, 3], inv_post_rot, post_trans, cam_to_ego, trans [B * N, ...], bda [B, 3, 3]) fp32: matrices are
    the identity plus a perturbation of at most 0.3 per entry (well conditioned), bda differs per batch entry."""
    rng = _rng(case.id)
    cams = case.batch * case.cams

    def mats(m):
        return (np.eye(3)[None] + rng.uniform(-0.3, 0.3, (m, 3, 3))).astype(np.float32)

    fr = np.stack([rng.uniform(0, 703, case.per_cam), rng.uniform(0, 255, case.per_cam),
                   rng.uniform(1, 60, case.per_cam)], 1).astype(np.float32)
    bda = mats(case.batch)
    assert not np.array_equal(bda[0], bda[1])
    return (fr, mats(cams), rng.uniform(-20, 20, (cams, 3)).astype(np.float32), mats(cams),
            rng.uniform(-2, 2, (cams, 3)).astype(np.float32), bda)


# ---- case lists ----------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def prepare_cases():
    return tuple(prep_size_cases() + coord_cases() + occupancy_cases())


@lru_cache(maxsize=None)
def all_sort_cases():
    return tuple(sort_cases())


@lru_cache(maxsize=None)
def all_pool_cases():
    return tuple(pool_cases() + chain_cases())


# ---- device calls (GPU tests only) ---------------------------------------------------------------------------------------------
def run_argsort(case: SortCase, raw=False):
    """The case through ops.sort.stable_argsort (or pd3_stable_argsort itself): the order as a host int64 array."""
    import torch

    from paddle3d_amd.ops.sort import stable_argsort

    keys = torch.from_numpy(sort_keys(case).copy()).cuda()
    if not raw:
        out = stable_argsort(keys, descending=case.mode == 1, max_key=None if case.mode == 1 else case.max_key)
    else:
        out = raw_argsort(keys, case.mode, case.max_key)
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64)


def raw_argsort(keys, mode, max_key):
    """pd3_stable_argsort on a device tensor of int32 / float32 keys: the int32 order tensor (no range check, no copies)."""
    import torch

    from paddle3d_amd.ops._common import check, lib, ptr, stream_ptr, workspace

    n = int(keys.numel())
    order = torch.full((n,), -7, dtype=torch.int32, device=keys.device)
    L = lib()
    ws = workspace(L.pd3_stable_argsort_workspace(n, max_key), keys.device)
    check(L.pd3_stable_argsort(ptr(keys), n, mode, max_key, ptr(order), ptr(ws), ws.numel(), stream_ptr(keys.device)),
          "stable_argsort")
    return order


def run_prepare(case: PrepCase):
    """pd3_voxel_pooling_prepare through the C ABI the way ops/bev_pool_v2.py calls it: (status, five host arrays cut to
    the counts -- whole where the call was refused --, counts).  The outputs have their full size and start out filled with -7."""
    import torch

    from paddle3d_amd.ops._common import host_f32, lib, ptr, stream_ptr, workspace

    c = torch.from_numpy(coor_of(case).copy()).cuda()
    n = int(c.shape[0])
    outs = [torch.full((n,), -7, dtype=torch.int32, device=c.device) for _ in range(5)]
    counts = torch.full((2,), -7, dtype=torch.int32, device=c.device)
    L = lib()
    ws = workspace(L.pd3_voxel_pooling_prepare_workspace(n), c.device)
    hlo, hiv, hsz = host_f32(case.lower, 3), host_f32(case.step, 3), host_f32(case.size, 3)
    status = L.pd3_voxel_pooling_prepare(ptr(c), n, case.batch, case.depth_bins, case.feat_hw, ptr(hlo), ptr(hiv), ptr(hsz),
                                         case.mode, *[ptr(o) for o in outs], ptr(counts), ptr(ws), ws.numel(),
                                         stream_ptr(c.device))
    torch.cuda.synchronize()
    cn = counts.cpu().numpy()
    host = [o.cpu().numpy() for o in outs]
    if status != 0:
        return status, host, cn
    kept, nint = int(cn[0]), int(cn[1])
    return status, [host[0][:kept], host[1][:kept], host[2][:kept], host[3][:nint], host[4][:nint]], cn


def run_pool(data: PoolData):
    """(out, depth_grad, feat_grad) host arrays through ops.bev_pool_v2.bev_pool_v2 / bev_pool_v2_bkwd."""
    import torch

    from paddle3d_amd.ops import bev_pool_v2 as bp

    def dev(a):
        return torch.from_numpy(np.array(a, copy=True)).cuda()   # (the cached arrays are read-only)

    d, f, g = dev(data.depth), dev(data.feat), dev(data.out_grad)
    rd, rf, rb, ln, st = (dev(a) for a in data.fwd)
    out = bp.bev_pool_v2(d, f, rd, rf, rb, ln, st, (data.cells, f.shape[1]))
    rd, rf, rb, ln, st = (dev(a) for a in data.bwd)
    dg, fg = bp.bev_pool_v2_bkwd(g, d, f, rd, rf, rb, ln, st)
    torch.cuda.synchronize()
    return out.cpu().numpy(), dg.cpu().numpy(), fg.cpu().numpy()


def run_frustum(case: FrustumCase):
    import torch

    from paddle3d_amd.ops._common import check, lib, ptr, stream_ptr

    dev = [torch.from_numpy(a).cuda() for a in frustum_data(case)]
    out = torch.full((case.batch * case.cams * case.per_cam, 3), float("nan"), dtype=torch.float32, device="cuda")
    check(lib().pd3_frustum_to_lidar(ptr(dev[0]), case.per_cam, case.batch, case.cams, ptr(dev[1]), ptr(dev[2]), ptr(dev[3]),
                                     ptr(dev[4]), ptr(dev[5]), ptr(out), stream_ptr(out.device)), "frustum_to_lidar")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same_bits(a, b):
    """Equal as uint32, except where both are NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
