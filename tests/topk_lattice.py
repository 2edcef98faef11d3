"""The shared block top-K selection's border lattice (csrc/block_topk.hpp through pd3_selfcheck_block_topk): a helper
module like tests/pool_lattice.py, not a conftest.

* the constants of block_topk.hpp and its callers' sentinels are restated here; source_constants() reads each out of the
  sources by pattern, and tests/test_topk_lattice_cpu.py holds the two together.
* ref_select is the contract (a stable argsort, first K); walk() restates block_topk_cut's radix walk and says at which
  depth it stops and with which r; compact_plan() / sort_plan() restate the partitions of the two compactions and the
  sort's size, so that every case can say which borders it lies on.
* model() is the restated pipeline (walk, take, order); it accepts a MUTANT, a one-line wrong version of itself.  The CPU
  file asserts that every mutant disagrees with ref_select somewhere on the lattice: the lattice's discriminating power
  is measured on the model, never with a wrong kernel.
* the cases are crosses, not products: a GROUP fixes what one launch of the probe fixes (n, K, key_bits, leave_out) and
  holds one set per key family; every family builds its keys constructively from a seed derived from the case id and
  states its claim (the depth the walk stops at, r) instead of hoping for it.

Everything here runs on the CPU except run_probe, which the GPU tests use.
"""
from __future__ import annotations

import os
import re
import zlib
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

# ---- block_topk.hpp and its callers, restated ------------------------------------------------------------------------
TOPK_THREADS = 1024          # kTopkThreads
TOPK_MAX_K = 1024            # kTopkMaxK
TOPK_COPIES = 8              # kTopkCopies: histogram replicas
WAVE = 64                    # kWave
WAVES = TOPK_THREADS // WAVE
Q = 4                        # block_topk_compact's kQ: keys per lane in flight (a wave walks Q * WAVE keys a step)
DIGIT = 10                   # block_topk_cut: min(hi, 10) bits at a time
SORT_BARRIER_STRIDE = 2 * WAVE   # block_topk_sort: a stride >= 2 * kWave crosses waves
LDS_MAX_N = 16384            # form 1 of the probe (cp_topk_kernel's kTopkMaxHw)
ONE_BITS = 0x3F800000        # bits of 1.0f
KEY_OUT = 0x3FFFFFFF         # postprocess.hip kKeyOut
SSD_KEY_OUT = 0x3FFFFFFF     # ssd_head.hip kSsdKeyOut
BD_KEY_NAN = 0x3FFFFFFF      # bevdet_postprocess.hip kBdKeyNan
KEY_NAN = 0x3FFFFFFF         # bevformer_decoder.hip kKeyNan
KEY_ALL = ONE_BITS + 2       # block_topk.hpp kScoreKeyAll
TAKE_ALL = 0xFFFFFFFF        # the probe's skip_cut cut-off; also what it writes for a refused set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "paddle3d_amd", "csrc")


def source_constants():
    """The constants above as the sources state them (every pattern must match: a renamed or removed constant is an
    error here, not a silent pass)."""
    def read(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()

    def one(text, pattern):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return int(m[0], 0)

    bt, cm = read("block_topk.hpp"), read("common.hpp")
    pp, ssd, bd, dec, a3d = (read(f) for f in ("postprocess.hip", "ssd_head.hip", "bevdet_postprocess.hip",
                                               "bevformer_decoder.hip", "anchor3d_head.hip"))
    out = {
        "TOPK_THREADS": one(bt, r"constexpr int kTopkThreads = (\d+);"),
        "TOPK_MAX_K": one(bt, r"constexpr int kTopkMaxK = (\d+);"),
        "TOPK_COPIES": one(bt, r"constexpr int kTopkCopies = (\d+);"),
        "WAVE": one(cm, r"constexpr int kWave = (\d+);"),
        "Q": one(bt, r"constexpr int kQ = (\d+);"),
        "DIGIT": one(bt, r"const int w = min\(hi, (\d+)\), shift = hi - w;"),
        "ONE_BITS": one(bt, r"constexpr uint32_t kScoreKeyOne = (0x[0-9A-Fa-f]+)u;"),
        "KEY_OUT": one(pp, r"constexpr uint32_t kKeyOut = (0x[0-9A-Fa-f]+)u;"),
        "SSD_KEY_OUT": one(ssd, r"constexpr uint32_t kSsdKeyOut = (0x[0-9A-Fa-f]+)u;"),
        "BD_KEY_NAN": one(bd, r"constexpr uint32_t kBdKeyNan = (0x[0-9A-Fa-f]+)u;"),
        "KEY_NAN": one(dec, r"constexpr uint32_t kKeyNan = (0x[0-9A-Fa-f]+)u;"),
        "KEY_ALL": one(bt, r"constexpr uint32_t kScoreKeyOne = (0x[0-9A-Fa-f]+)u;")
                   + one(bt, r"constexpr uint32_t kScoreKeyAll = kScoreKeyOne \+ (\d+)u;"),
        "LDS_MAX_N": one(read("selfcheck.hip"), r"constexpr int kProbeMaxLdsKeys = (\d+);"),
    }
    # the rules that are not a number: the barrier rule of the sort, the histogram's bins and replicas, the partition
    assert "if (stride >= 2 * kWave || (stride == 1 && size >= 2 * kWave))" in bt
    assert "constexpr int kTopkHistWords = kTopkCopies * 1024;" in bt and "hist + (t & (kTopkCopies - 1)) * 1024" in bt
    assert "const int per = (int)ceil_div(ceil_div(n, kWaves), kWave) * kWave;" in bt
    assert "for (int ib = i0; ib < i1; ib += kQ * kWave)" in bt
    assert "const int ept = (n + kTopkThreads - 1) / kTopkThreads;" in bt
    assert "int n2 = 64;\n  while (n2 < K) n2 <<= 1;" in bt
    assert one(pp, r"constexpr int kTopkMaxHw = (\d+);") == out["LDS_MAX_N"]
    assert "return i + (i >> 4); }  // postprocess.hip kidx" in read("selfcheck.hip")
    assert "__device__ __forceinline__ int kidx(int i) { return i + (i >> 4); }" in pp
    assert "block_topk_cut(K, kScoreKeyBits, hist, scr, visit) : TopkCut{kScoreKeyAll, 0}" in a3d
    for text, name in ((bd, "kBdKeyBits"), (dec, "kKeyBits"), (bt, "kScoreKeyBits")):
        assert one(text, rf"constexpr int {name} = (\d+);") == 30
    return out


def f32_bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def bits_f32(b):
    return float(np.array([b], np.uint32).view(np.float32)[0])


def topk_key_bits(score_threshold):
    """topk_key_bits of block_topk.hpp: the bits a key bits(1.0f) - bits(score) can have above the threshold."""
    thr = np.float32(score_threshold)
    tb = f32_bits(thr)
    span = ONE_BITS - tb if (thr > 0 and tb < ONE_BITS) else ONE_BITS   # NaN: the comparison is false
    return int(span).bit_length()


def score_key(score, nan_key=KEY_NAN):
    """bits(1.0f) - bits(s) for s in [0, 1], the NaN key otherwise (bevformer_decoder.hip score_key and its kin)."""
    b = np.asarray(score, np.float32).view(np.uint32).astype(np.int64)
    return np.where(b <= ONE_BITS, ONE_BITS - b, nan_key).astype(np.uint32)


# ---- the contract ----------------------------------------------------------------------------------------------------
def counted_mask(keys, key_bits, leave_out=None):
    c = (keys.astype(np.int64) >> key_bits) == 0
    if leave_out is not None:
        c &= keys != np.uint32(leave_out)
    return c


def ref_select(keys, K, counted):
    """Indices of the K smallest counted keys in ascending (key, index) order: a stable argsort, first K."""
    k = np.where(counted, keys.astype(np.int64), np.int64(1) << 32)
    order = np.argsort(k, kind="stable")[:K]
    assert counted[order].all(), "fewer than K keys counted"
    return order.astype(np.int64)


# ---- block_topk_cut --------------------------------------------------------------------------------------------------
def digit_plan(key_bits, mutant=None):
    hi, out = key_bits, []
    while hi > 0:
        w = DIGIT if mutant == "digit-always-10" else min(hi, DIGIT)
        out.append(w)
        hi -= w
    return tuple(out)


@dataclass(frozen=True)
class Walk:
    kc: int
    r: int
    depth: int        # digits walked
    plan: tuple       # widths of all digits of this key_bits
    in_bin: int       # keys in the last bin looked at

    @property
    def r_class(self):
        """whole: the bin holding rank K taken whole (r = 0); 1; max: in_bin - 1; mid: anything between."""
        if self.r == 0:
            return "whole"
        if self.r == 1:   # (in_bin == 2 is both 1 and max: counted as 1, and as max where asked)
            return "1"
        return "max" if self.r == self.in_bin - 1 else "mid"


def walk(keys, K, key_bits, leave_out=None, mutant=None):
    """block_topk_cut restated: (kc, r), the depth at which it stopped and the digit plan."""
    k = keys.astype(np.int64)
    visited = np.ones(len(k), bool)
    if leave_out is not None and mutant != "left-out-counted":
        visited &= k != leave_out
    k = k[visited]
    prefix, need, hi, depth, in_bin = 0, K, key_bits, 0, 0
    while hi > 0:
        w = DIGIT if mutant == "digit-always-10" else min(hi, DIGIT)
        shift = hi - w
        in_prefix = (k >> hi) == prefix
        if mutant == "high-keys-counted" and depth == 0:
            in_prefix = np.ones(len(k), bool)
        dig = ((k >> shift) if shift >= 0 else (k << -shift)) & ((1 << w) - 1)
        hist = np.bincount(dig[in_prefix], minlength=1 << w)
        cum = np.cumsum(hist) - hist
        hit = np.nonzero((need > cum) & (need <= cum + hist))[0]
        assert len(hit) == 1, "more than K keys must be visited"
        b = int(hit[0])
        in_bin, need = int(hist[b]), need - int(cum[b])
        prefix = (prefix << w) | b
        hi = shift
        depth += 1
        if need == in_bin:
            prefix = (prefix + 1) << max(hi, 0)
            need = 0
            break
    return Walk(int(prefix), int(need), depth, digit_plan(key_bits), in_bin)


# ---- the compactions' partitions and the sort's size -------------------------------------------------------------------
def _ceil_div(a, b):
    return -(-a // b)


@dataclass(frozen=True)
class CompactPlan:
    per: int          # block_topk_compact: indices per wave
    waves: tuple      # ((i0, i1),) * WAVES
    ept: int          # block_topk_compact_chunks: indices per thread

    def wave_of(self, i):
        return np.minimum(np.asarray(i) // self.per, WAVES - 1)

    def chunk_of(self, i):
        return np.asarray(i) // self.ept


def compact_plan(n):
    per = _ceil_div(_ceil_div(n, WAVES), WAVE) * WAVE
    waves = tuple((min(w * per, n), min(min(w * per, n) + per, n)) for w in range(WAVES))
    return CompactPlan(per, waves, _ceil_div(n, TOPK_THREADS))


def sort_plan(K):
    """(n2, whether a step of the network has a stride that crosses waves and so takes block barriers)."""
    n2 = 64
    while n2 < K:
        n2 <<= 1
    return n2, n2 // 2 >= SORT_BARRIER_STRIDE


# ---- the restated pipeline, and its one-line wrong versions --------------------------------------------------------------
MUTANTS = ("ties-from-end", "r-plus-1", "r-minus-1", "digit-always-10", "high-keys-counted", "left-out-counted",
           "wave-ties-not-offset", "order-by-key-alone", "every-set-reads-set-0")


def take(keys, kc, r, mutant=None):
    """What the compaction takes: every key below kc and the first r keys equal to kc in index order."""
    less = np.nonzero(keys.astype(np.int64) < kc)[0]
    eq = np.nonzero(keys.astype(np.int64) == kc)[0]
    if mutant == "r-plus-1":
        r = r + 1
    elif mutant == "r-minus-1":
        r = r - 1
    if mutant == "ties-from-end":
        ties = eq[len(eq) - r:] if r > 0 else eq[:0]
    elif mutant == "wave-ties-not-offset":      # pos_eq counted inside each wave's share only
        w = compact_plan(len(keys)).wave_of(eq)
        rank_in_wave = np.arange(len(eq)) - np.searchsorted(w, w, side="left")
        slot = {int(j): int(i) for i, j in zip(eq, rank_in_wave) if j < r}      # waves collide; one writer stays
        ties = np.array(sorted(slot.values()), np.int64)
    else:
        ties = eq[:max(r, 0)]
    return np.concatenate([less, ties])


def model(sets, K, key_bits, leave_out=None, mutant=None):
    """The sorted list of every set of a group, [sets][TOPK_MAX_K] indices with -1 where the list is empty: walk, take,
    order by (key, index).  The probe returns the first K entries; an exact selection leaves nothing behind them
    (expected())."""
    out = []
    for s, keys in enumerate(sets):
        if mutant == "every-set-reads-set-0":
            keys = sets[0]
        wk = walk(keys, K, key_bits, leave_out, mutant)
        idx = take(keys, wk.kc, wk.r, mutant)
        kk = keys[idx].astype(np.int64)
        if mutant == "order-by-key-alone":      # the index dropped from the entry: equal keys in no defined order
            order = np.lexsort((-idx, kk))
        else:
            order = np.lexsort((idx, kk))
        idx = idx[order][:TOPK_MAX_K]
        out.append(np.concatenate([idx, np.full(TOPK_MAX_K - len(idx), -1, np.int64)]))
    return np.stack(out)


def expected(keys, K, key_bits, leave_out=None):
    """ref_select as a whole list: K entries, nothing after them."""
    ref = ref_select(keys, K, counted_mask(keys, key_bits, leave_out))
    return np.concatenate([ref, np.full(TOPK_MAX_K - K, -1, np.int64)])


# ---- the lattice -----------------------------------------------------------------------------------------------------
KEY_BITS = (1, 2, 9, 10, 11, 19, 20, 21, 29, 30)
KS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)
NS = (65, 959, 960, 961, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 16383, 16384)
NS_GLOBAL_ONLY = (16385, 107136)     # form 0 alone: past the LDS form's limit, and KITTI's anchor count
FAMILIES = ("spread", "equal", "low", "tie-r1", "tie-rmax", "tie-fit", "whole-1", "whole-2", "first-bin", "last-bin",
            "hot-bin", "sentinel", "ascending", "descending")
FORMS = (0, 1)


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


@dataclass(frozen=True)
class Group:
    """What one launch of the probe fixes; its sets are the families that can be built at these parameters."""
    n: int
    K: int
    key_bits: int
    lo: str            # "none", "below" (leave_out < 2^key_bits) or "above"

    @property
    def id(self):
        return f"n{self.n}-K{self.K}-b{self.key_bits}-{self.lo}"

    @property
    def leave_out(self):
        if self.lo == "none":
            return None
        if self.lo == "below":
            return (1 << self.key_bits) - 1
        return SSD_KEY_OUT if self.key_bits < 30 else 0x7FFFFFFF

    @property
    def forms(self):
        return FORMS if self.n <= LDS_MAX_N else (0,)

    @property
    def values(self):
        """Counted keys are drawn from [0, values)."""
        return (1 << self.key_bits) - (1 if self.lo == "below" else 0)


@dataclass(frozen=True)
class Case:
    group: Group
    family: str
    keys: np.ndarray
    claim: dict        # what the construction guarantees of walk(): any of depth, r, r_class, counted

    @property
    def id(self):
        return f"{self.group.id}-{self.family}"


def _uncounted(g, rng, count):
    """Keys that are never counted: at or above 2^key_bits (0xFFFFFFFF among them), or the left-out value."""
    lim = 1 << g.key_bits
    hi = rng.integers(lim, 1 << 32, count, dtype=np.int64)
    if count:
        hi[0] = 0xFFFFFFFF
    if g.lo != "none":
        hi[rng.random(count) < (1.0 if g.lo == "below" else 0.5)] = g.leave_out
    return hi


def _place(g, rng, counted_vals, cluster=None, in_order=None):
    """n keys: the counted values at random indices (sorted by index if `in_order`), the cluster's members on both
    sides of a wave border and of a chunk border of compact_plan(n), uncounted keys everywhere else."""
    n = g.n
    m = len(counted_vals) + (cluster[1] if cluster else 0)
    assert m <= n
    keys = np.full(n, -1, np.int64)
    free = np.ones(n, bool)
    if cluster:
        val, T = cluster
        cp = compact_plan(n)
        mid = (n // 2 // cp.ept) * cp.ept
        anchors = [i for i in (cp.per - 1, cp.per, mid - 1, mid, cp.per + 1, 0, n - 1) if 0 <= i < n]
        anchors = list(dict.fromkeys(anchors))[:T]
        rest = np.setdiff1d(np.arange(n), anchors)
        pos = np.concatenate([anchors, rng.choice(rest, T - len(anchors), replace=False)]).astype(np.int64)
        keys[pos] = val
        free[pos] = False
    slots = np.nonzero(free)[0]
    pos = np.sort(rng.choice(slots, len(counted_vals), replace=False))
    vals = np.asarray(counted_vals, np.int64)
    if in_order == "ascending":
        vals = np.sort(vals)
    elif in_order == "descending":
        vals = np.sort(vals)[::-1]
    else:
        vals = rng.permutation(vals)
    keys[pos] = vals
    rest = keys < 0
    keys[rest] = _uncounted(g, rng, int(rest.sum()))
    return keys.astype(np.uint32)


def _build(g, family, rng):
    """(keys, claim) of one family at a group's parameters, or None where the width or the sizes leave no room."""
    n, K, B, V = g.n, g.K, g.key_bits, g.values
    plan = digit_plan(B)
    D = len(plan)
    # counted keys: all of them at n = K + 1, otherwise seven eighths of what is above K + 1
    m = K + 1 + (n - K - 1) * 7 // 8
    s1 = B - plan[0]                      # shift of digit 1
    wl = plan[-1]                         # width of the last digit
    if family in ("spread", "ascending", "descending"):
        order = family if family != "spread" else None
        return _place(g, rng, rng.integers(0, V, m), in_order=order), {"counted": m}
    if family == "equal":
        return _place(g, rng, np.full(m, rng.integers(0, V))), {"counted": m, "depth": D, "r": K}
    if family == "low":
        base = int(rng.integers(0, V)) >> wl << wl
        top = min(base + (1 << wl), V)
        return _place(g, rng, rng.integers(base, top, m)), {"counted": m}
    if family == "hot-bin":
        b = int(rng.integers(0, 1 << plan[0]))
        lo = min(b << s1, V - 1) >> s1 << s1
        return _place(g, rng, rng.integers(lo, min(lo + (1 << s1), V), m)), {"counted": m}
    if family == "sentinel":
        if n == K + 1:
            return None
        return _place(g, rng, rng.integers(0, V, K + 1)), {"counted": K + 1}
    if family in ("tie-r1", "tie-rmax", "tie-fit"):
        T = min({"tie-r1": m - K + 1, "tie-rmax": K + 1, "tie-fit": K}[family], 40)     # L + T <= m, L >= 0
        if T < 2:
            return None
        r = {"tie-r1": 1, "tie-rmax": T - 1, "tie-fit": T}[family]
        L, above = K - r, m - (K - r) - T
        c = int(rng.integers(V // 4, max(3 * V // 4, V // 4 + 1)))
        if family == "tie-fit" and (c & ((1 << wl) - 1)) == (1 << wl) - 1:
            c -= 1                         # room for c + 1 in the same bin of every digit but the last
        if L > 0:
            c = max(c, 1)
        if above > 0:
            c = min(c, V - 2)
        if not 0 <= c < V or (L > 0 and c < 1) or (above > 0 and c > V - 2) or (family == "tie-fit" and ((c + 1) >> wl != c >> wl or c + 1 >= V)):
            return None
        vals = np.concatenate([rng.integers(0, max(c, 1), L), rng.integers(c + 1, max(V, c + 2), above)])
        if family == "tie-fit":
            vals[L] = c + 1                # the bin of every earlier digit holds more than the walk needs of it
            return _place(g, rng, vals, cluster=(c, T)), {"counted": m, "depth": D, "r": 0, "r_class": "whole"}
        return _place(g, rng, vals, cluster=(c, T)), {"counted": m, "depth": D, "r": r}
    if family == "whole-1":
        nb = min(1 << plan[0], _ceil_div(V, 1 << s1))     # digit-1 bins that hold a counted value
        if nb < 2:
            return None
        b1 = int(rng.integers(0, nb - 1))
        lo_vals = rng.integers(0, (b1 + 1) << s1, K)
        lo_vals[0] = (b1 << s1) + int(rng.integers(0, 1 << s1))   # bin b1 is not empty
        hi_vals = rng.integers((b1 + 1) << s1, V, m - K)
        return (_place(g, rng, np.concatenate([lo_vals, hi_vals])),
                {"counted": m, "depth": 1, "r": 0, "r_class": "whole"})
    if family == "whole-2":
        if D < 2 or K < 2 or m < K + 1:
            return None
        w2 = plan[1]
        s2 = s1 - w2
        b1 = int(rng.integers(0, max(1, min(1 << plan[0], V >> s1) - 1)))
        b2 = int(rng.integers(0, (1 << w2) - 1))
        base = b1 << s1
        if base + ((b2 + 2) << s2) > V:
            return None
        A = int(rng.integers(0, K - 1)) if b1 > 0 else 0          # keys in earlier bins of digit 1
        below = rng.integers(0, max(base, 1), A)
        inside = rng.integers(base, base + ((b2 + 1) << s2), K - A)
        inside[0] = base + (b2 << s2) + int(rng.integers(0, 1 << s2))          # bin (b1, b2) is not empty
        after = rng.integers(base + ((b2 + 1) << s2), V, m - K)
        after[0] = base + ((b2 + 1) << s2) + int(rng.integers(0, 1 << s2))     # bin b1 of digit 1 is not taken whole
        return (_place(g, rng, np.concatenate([below, inside, after])),
                {"counted": m, "depth": 2, "r": 0, "r_class": "whole"})
    if family == "first-bin":
        if V < 2 or m < K + 2:
            return None
        nk = min(m - 1, K + 1 + (m - K) // 2)                     # rank K lies inside bin 0 of digit 1
        vals = np.concatenate([rng.integers(0, min(1 << s1, V), nk), rng.integers(0, V, m - nk)])
        vals[0], vals[-1] = 0, V - 1
        return _place(g, rng, vals), {"counted": m, "first_bin": True}
    if family == "last-bin":
        top = (V - 1) >> s1 << s1
        nk = (K - 1) // 2 if top > 0 else 0                       # fewer than K keys below the highest bin
        vals = np.concatenate([rng.integers(0, max(top, 1), nk), rng.integers(top, V, m - nk)])
        vals[-1] = V - 1
        if nk:
            vals[0] = 0
        return _place(g, rng, vals), {"counted": m, "last_bin": True}
    raise ValueError(family)


def _groups():
    out, los = [], ("none", "below", "above")
    for i, K in enumerate(KS):                       # n = K + 1 at every K
        out.append(Group(K + 1, K, KEY_BITS[i % len(KEY_BITS)], los[i % 3]))
    for i, n in enumerate(NS + NS_GLOBAL_ONLY):       # every n border, K and key_bits cycling out of step
        ks = [K for K in KS if K + 1 < n]
        out.append(Group(n, ks[(5 * i + 3) % len(ks)], KEY_BITS[(3 * i + 1) % len(KEY_BITS)], los[(i + 1) % 3]))
    for i, B in enumerate(KEY_BITS):                 # every width at a size with several chunks and full waves
        n = (2049, 4097, 1025, 16384)[i % 4]
        out.append(Group(n, KS[(7 * i + 2) % len(KS)], B, los[(i + 2) % 3]))
    for i, K in enumerate(KS):                       # every K (every sort size) again at three full digits
        out.append(Group((4096, 1025, 2047)[i % 3] if K < 1023 else 4096, K, (30, 21, 29)[i % 3], los[i % 3]))
    seen = {}
    for g in out:
        seen.setdefault(g.id, g)
    return tuple(seen.values())


GROUPS = _groups()


@lru_cache(maxsize=None)
def group_cases(gid):
    g = next(g for g in GROUPS if g.id == gid)
    cases = []
    for family in FAMILIES:
        built = _build(g, family, np.random.default_rng(_seed(g.id, family)))
        if built is not None:
            keys, claim = built
            keys.setflags(write=False)
            cases.append(Case(g, family, keys, claim))
    return tuple(cases)


def all_cases(form=None):
    return [c for g in GROUPS if form is None or form in g.forms for c in group_cases(g.id)]


def tie_split(case, wk, form):
    """Whether the keys equal to kc that are taken and those that are not lie in different partitions of the form's
    compaction (waves of form 0, chunks of form 1), and whether the taken ones span two partitions."""
    eq = np.nonzero(case.keys.astype(np.int64) == wk.kc)[0]
    if wk.r <= 0 or wk.r >= len(eq):
        return False, False
    cp = compact_plan(case.group.n)
    part = cp.wave_of(eq) if form == 0 else cp.chunk_of(eq)
    return bool(part[wk.r - 1] != part[wk.r] or part[0] != part[-1]), bool(part[0] != part[wk.r - 1])


# ---- the probe ---------------------------------------------------------------------------------------------------------
def run_probe(sets, K, key_bits, form, leave_out=None, skip_cut=False, stream=None):
    """pd3_selfcheck_block_topk on [sets][n] uint32 keys: (idx [sets][K], key [sets][K], cut [sets][2]) as int64."""
    import torch

    from paddle3d_amd.ops._common import check, lib, ptr, stream_ptr

    dev = torch.device("cuda", 0)
    keys = np.ascontiguousarray(np.stack(sets).astype(np.uint32))
    s, n = keys.shape
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream(dev))
    with ctx:
        dk = torch.from_numpy(keys.view(np.int32)).to(dev)
        idx = torch.full((s, K), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        key = torch.full((s, K), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        cut = torch.full((s, 2), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        check(lib().pd3_selfcheck_block_topk(ptr(dk), s, n, K, key_bits, form, -1 if leave_out is None else leave_out,
                                             int(skip_cut), ptr(idx), ptr(key), ptr(cut), stream_ptr(dev)),
              "selfcheck_block_topk")
        outs = [t.cpu().numpy().view(np.uint32).astype(np.int64) for t in (idx, key, cut)]
    return outs


# ---- call-site cases: logits through the public ops, keys restated on the CPU -----------------------------------------
F32 = np.float32
CP_THRESHOLDS = {          # name -> (score_threshold, the key_bits it must give)
    "default": (0.1, 25), "b10": (bits_f32(ONE_BITS - 1023), 10), "b11": (bits_f32(ONE_BITS - 1024), 11),
    "b20": (bits_f32(ONE_BITS - ((1 << 20) - 1)), 20), "b21": (bits_f32(ONE_BITS - (1 << 20)), 21),
    "zero": (0.0, 30), "minus-one": (-1.0, 30)}
CP_PRES = (63, 65, 129, 256, 257, 513, 1023)
CP_HW = (64, 64)           # 4096 cells: four cells per thread of block_topk_compact_chunks
CP_KINDS = ("continuous", "quantised", "tie-cluster", "pre-plus-1", "masked", "equal")      # task t of a case
CP_CASES = tuple((f"pre{p}", p, "default") for p in CP_PRES) + tuple(
    (f"thr-{t}", p, t) for t, p in (("b10", 63), ("b11", 129), ("b20", 257), ("b21", 513), ("zero", 256),
                                    ("minus-one", 1023)))


def sigmoid_f32(x, expf):
    """1 / (1 + expf(-x)) in float32, the heads' score (postprocess.hip cp_best_class and its kin)."""
    x = np.ascontiguousarray(x, F32)
    with np.errstate(all="ignore"):
        e = expf((-x).reshape(-1)).reshape(x.shape).astype(F32)
        return (F32(1) / (F32(1) + e)).astype(F32)


def cp_case(name):
    """(hm [6][hw] class-0 logits, masked [6][hw] cells to put outside the centre range, pre, threshold) of a
    CenterPoint case: task t is of kind CP_KINDS[t], so one launch runs six sets with six different cuts."""
    _, pre, tname = next(c for c in CP_CASES if c[0] == name)
    thr, bits = CP_THRESHOLDS[tname]
    hw = CP_HW[0] * CP_HW[1]
    rng = np.random.default_rng(_seed("cp", name))
    span = ONE_BITS - f32_bits(thr) if 0 < thr < 1 else None
    # logits whose scores exceed the threshold: sigmoid(x) > thr  <=>  x > log(thr / (1 - thr)), with a margin
    lo = float(np.log(thr / (1 - thr))) + 0.25 if 0 < thr < 1 else -4.0
    hi = lo + 7.0
    below = lo - 3.0 if 0 < thr < 1 else None      # (no score is below a threshold <= 0)
    hm, masked = [], []
    cp = compact_plan(hw)
    for kind in CP_KINDS:
        x = rng.uniform(lo, hi, hw).astype(F32)
        m = np.zeros(hw, bool)
        if kind == "quantised":
            x = (np.round(x * 2) / 2 + F32(0.5)).astype(F32)
        elif kind == "tie-cluster":          # pre - 5 cells above a cluster of ten equal logits around a chunk border
            x = rng.uniform(lo, lo + 2.0, hw).astype(F32)
            order = rng.permutation(hw)
            mid = (hw // 2 // cp.ept) * cp.ept
            cluster = np.array([mid - 2, mid - 1, mid, mid + 1, 5, 6, hw - 1, cp.per - 1, cp.per, mid + 2 * cp.ept])
            top = np.setdiff1d(order, cluster, assume_unique=False)[:max(pre - 5, 0)]
            x[top] = rng.uniform(lo + 4.0, hi, len(top)).astype(F32)
            x[cluster] = F32(lo + 3.0)
        elif kind == "pre-plus-1":
            if below is None:                # every cell passes a threshold <= 0: all but pre + 1 are masked instead
                m[rng.permutation(hw)[pre + 1:]] = True
            else:
                x[rng.permutation(hw)[pre + 1:]] = F32(below)
        elif kind == "masked":
            m[rng.random(hw) < 0.6] = True
        elif kind == "equal":
            x[:] = F32(lo + 1.0)
        hm.append(x)
        masked.append(m)
    return np.stack(hm), np.stack(masked), pre, thr, bits, span


def cp_keys(hm, masked, thr, expf):
    """cp_cell_key restated for one class: bits(1.0f) - bits(score), kKeyOut for a cell that is masked out."""
    s = sigmoid_f32(hm, expf)
    return np.where((s > F32(thr)) & ~masked, score_key(s), np.uint32(KEY_OUT)).astype(np.uint32)


DECODE_CASES = {           # name -> (Q, K, max_num, kind): Q * K = max_num + 1
    "m1": (1, 2, 1, "continuous"), "m64": (13, 5, 64, "quantised"), "m65": (33, 2, 65, "ties"),
    "m300": (43, 7, 300, "quantised"), "m1024": (205, 5, 1024, "continuous"), "m300-nan": (43, 7, 300, "nan"),
    "m64-nan": (13, 5, 64, "nan")}


def decode_logits(name):
    """cls [2][Q][K] of an nms_free_decode case: Q * K = max_num + 1 candidates per frame."""
    Q, K, max_num, kind = DECODE_CASES[name]
    rng = np.random.default_rng(_seed("decode", name))
    cls = rng.uniform(-5.0, 3.0, (2, Q, K)).astype(F32)
    if kind in ("quantised", "nan"):
        cls = (np.round(cls * 2) / 2).astype(F32)
    if kind == "ties":                       # the cut inside a cluster of equal logits, the lowest of the frame
        flat = cls.reshape(2, -1)
        for b in range(2):
            flat[b, rng.choice(Q * K, 7, replace=False)] = F32(-6.0)
    if kind == "nan":                        # fewer numbers than max_num: the cut lies among the NaN keys
        flat = cls.reshape(2, -1)
        for b in range(2):
            flat[b, rng.choice(Q * K, 4 + b, replace=False)] = np.nan
    return cls, max_num


def decode_keys(cls, expf):
    B = cls.shape[0]
    return score_key(sigmoid_f32(cls, expf)).reshape(B, -1)


BD_CASES = {               # name -> (ncls, h, w, max_num, plant): n = ncls * h * w keys per frame, two frames; the op
                           # takes max_num <= h * w (the reference's per-class topk), so n = K + 1 needs one class
    "k+1": (1, 7, 9, 62, "quantised"),                  # n = K + 1
    "k+1-nan": (1, 7, 10, 69, "nan"),                   # n = K + 1, fewer numbers than K: the cut among kBdKeyNan
    "1023": (3, 11, 31, 300, "quantised"),              # 1024 - 1
    "1025-saturated": (5, 5, 41, 200, "saturated"),     # 1024 + 1, more than K scores of exactly 1.0 across classes
    "2047": (1, 23, 89, 513, "continuous"),             # 2048 - 1
    "4095-saturated": (3, 35, 39, 1000, "saturated"),   # 4096 - 1
    "1025-nan": (5, 5, 41, 129, "nan-cut"),             # NaN scores present, the cut among the numbers
}


def bd_heatmap(name):
    """heatmap [2][ncls][h][w] of a BEVDet case (the other head maps come from bevdet_head_numpy.head_maps)."""
    ncls, h, w, K, plant = BD_CASES[name]
    rng = np.random.default_rng(_seed("bevdet", name))
    n = ncls * h * w
    hm = rng.uniform(-2.0, 4.0, (2, n)).astype(F32)
    if plant in ("quantised", "nan", "nan-cut"):
        hm = (np.round(hm * 2) / 2).astype(F32)
    for b in range(2):
        if plant == "nan":
            hm[b, rng.choice(n, 3 + b, replace=False)] = np.nan
        elif plant == "nan-cut":
            hm[b, rng.choice(n, 40, replace=False)] = np.nan
        elif plant == "saturated":       # sigmoid(30) == 1.0f: K + 7 of them, in every class, on both sides of wave borders
            hm[b, rng.choice(n, K + 7 + b, replace=False)] = F32(30.0)
    return hm.reshape(2, ncls, h, w)


SSD_GRIDS = {"n&3==0": None, "n&3!=0": [0.0, -4.96, -3.0, 8.0, 4.96, 1.0]}      # point-cloud range (None: the golden's)
SSD_THRESHOLDS = {"zero": 0.0, "minus-one": -1.0, "low": 0.05}                     # `low` derives a width below 30
SSD_CASES = tuple((g, t, p) for g in SSD_GRIDS for t, p in (("zero", "cluster"), ("minus-one", "count-1"),
                                                            ("low", "cluster"), ("low", "count-1")))


@lru_cache(maxsize=None)
def ssd_setup(grid):
    """(generator arguments, pillar coordinates [25][4], anchor masks [2][a]) of the small SSD grids: 25 pillars keep a
    few hundred of the ~4600 anchors, every other anchor gets kSsdKeyOut."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_ssd_golden as G
    from oracle import pyoracle as O

    from paddle3d_amd.pointpillars import AnchorGenerator

    c = G.CASES["b"]
    args = (2, SSD_GRIDS[grid] or c["pcr"], c["vs"], c["anchor_configs"], 1)
    gen = AnchorGenerator(*args)
    rng = np.random.default_rng(9)
    nx, ny = gen.grid_size
    cells = rng.choice(nx * ny, 25, replace=False)
    co = np.zeros((25, 4), np.int32)
    co[:, 0], co[:, 2], co[:, 3] = rng.integers(0, 2, 25), cells // nx, cells % nx
    bv = gen.anchors_bv.cpu().numpy().astype(np.int64)
    masks = np.stack([O.ssd_anchor_mask_numpy(co[co[:, 0] == b][:, 1:], bv, gen.grid_size, 1.0) for b in range(2)])
    return args, co, masks, c["num_classes"]


def ssd_case(grid, tname, pre_kind):
    """(cls [2][a][ncls] logits, pre, threshold, cluster [2][10] anchor indices) of an SSD case.  `cluster`: pre - 5
    kept anchors with distinct high logits, then ten kept anchors with one logit on both sides of a wave border of
    block_topk_compact (r = 5), every other kept anchor below; `count-1`: pre is the smaller frame's kept count - 1.
    The logits are gaps apart that no one-ulp difference of expf closes, so the labels hold for the device's scores."""
    args, co, masks, ncls = ssd_setup(grid)
    a = masks.shape[1]
    rng = np.random.default_rng(_seed("ssd", grid, tname, pre_kind))
    counts = masks.sum(1)
    pre = 129 if pre_kind == "cluster" else int(counts.min()) - 1
    cp = compact_plan(a)
    cls = np.full((2, a, ncls), F32(-2.0), F32)
    x = rng.uniform(-2.5, 0.0, (2, a)).astype(F32)
    clusters = []
    for b in range(2):
        kept = np.nonzero(masks[b])[0]
        waves = cp.wave_of(kept)
        # the wave border with the most kept anchors on its two sides: five members before it, five behind
        w = max(range(1, WAVES), key=lambda w: min((waves < w).sum(), (waves >= w).sum(), 5) * 1000
                + min((waves == w - 1).sum(), (waves == w).sum()))
        before, behind = kept[waves < w][-5:], kept[waves >= w][:5]
        cluster = np.concatenate([before, behind])
        rest = np.setdiff1d(kept, cluster)
        top = rng.permutation(rest)[:pre - 5]
        x[b, top] = np.linspace(2.0, 5.0, len(top)).astype(F32)[rng.permutation(len(top))]
        x[b, cluster] = F32(1.0)
        clusters.append(cluster)
    cls[:, :, 0] = x
    cls[:, :, 1:] = x[:, :, None] - F32(8.0)          # class 0 is every anchor's best class
    return cls, pre, SSD_THRESHOLDS[tname], np.stack(clusters)


def ssd_keys(cls, masks, thr, expf):
    """ssd_score kernel's key restated (no centre range): bits(1.0f) - bits(best score) of a kept anchor, else
    kSsdKeyOut; kept = inside the pillar mask and score >= threshold (pointpillars_head.py's test)."""
    s = sigmoid_f32(cls, expf).max(-1)
    return np.where(masks & (s >= F32(thr)), score_key(s), np.uint32(SSD_KEY_OUT)).astype(np.uint32)


A3D_NMS_PRE = (63, 64, 65, 129, 1024)
A3D_GRIDS = {"N&3==0": (24, 23, 2), "N&3!=0": (23, 25, 2)}       # H, W, A: N = 1104 and 1150 anchors, both above 1024
A3D_NC, A3D_CS = 3, 7
A3D_SET_SIZES = (64, 65, 129)


def a3d_maps(H, W, A, x, seed):
    """(cls [1][A * nc][H][W], reg, dirs) with class logit x[i, c] at anchor i = pixel * A + a (cls row a * nc + c)."""
    rng = np.random.default_rng(seed)
    nc = x.shape[1]
    cls = np.ascontiguousarray(x.reshape(H * W, A, nc).transpose(1, 2, 0)).reshape(1, A * nc, H, W).astype(F32)
    reg = (rng.standard_normal((1, A * A3D_CS, H, W)) * 0.05).astype(F32)
    dirs = rng.standard_normal((1, A * 2, H, W)).astype(F32)
    return cls, reg, dirs


def a3d_select_case(grid, nms_pre):
    """x [N][nc] logits for a3d_topk_kernel: nms_pre - 5 anchors with distinct high logits (spread over the classes),
    ten anchors with one logit on both sides of the first wave border of block_topk_compact (r = 5), the rest lower."""
    H, W, A = A3D_GRIDS[grid]
    N = H * W * A
    rng = np.random.default_rng(_seed("a3d", grid, nms_pre))
    per = compact_plan(N).per
    cluster = np.arange(per - 5, per + 5)
    x = np.full((N, A3D_NC), F32(-6.0), F32)
    best = rng.uniform(-2.0, 0.0, N).astype(F32)
    top = rng.permutation(np.setdiff1d(np.arange(N), cluster))[:nms_pre - 5]
    best[top] = np.linspace(2.0, 5.0, len(top)).astype(F32)[rng.permutation(len(top))]
    best[cluster] = F32(1.0)
    x[np.arange(N), rng.integers(0, A3D_NC, N)] = best
    return x, cluster


def a3d_set_case(n, total_cut=False):
    """x [N][nc] on a 16 x 13 x 2 grid: class 0 has exactly n candidates above the score threshold (one anchor per
    pixel; quantised logits: ties inside the set), the other classes none -- or, with total_cut, class 1 has n // 2 more,
    so that max_num = total - 1 cuts one entry of the concatenated list."""
    H, W, A = 16, 13, 2
    rng = np.random.default_rng(_seed("a3d-set", n, total_cut))
    x = np.full((H * W * A, A3D_NC), F32(-5.0), F32)
    pix = rng.permutation(H * W)
    hot = pix[:n] * A + rng.integers(0, A, n)
    x[hot, 0] = (np.round(rng.uniform(0.0, 4.0, n) * 2) / 2).astype(F32)
    if total_cut:
        hot1 = pix[n:n + n // 2] * A + rng.integers(0, A, n // 2)
        x[hot1, 1] = (np.round(rng.uniform(0.0, 4.0, n // 2) * 2) / 2).astype(F32)
    return (H, W, A), x
