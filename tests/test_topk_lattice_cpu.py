"""What tests/topk_lattice.py claims, proved without a GPU: its constants are the sources', its cases cover every digit
plan, stop depth, tie split, partition border and sort size in both forms of the probe, its restated pipeline equals the
contract on every case, and every one-line wrong version of that pipeline is caught by some case."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_lattice as L  # noqa: E402


@pytest.fixture(scope="module")
def walks():
    """walk() of every raw-key case, once."""
    return {c.id: L.walk(c.keys, c.group.K, c.group.key_bits, c.group.leave_out) for c in L.all_cases()}


def test_restated_constants_equal_the_sources():
    src = L.source_constants()
    for name, value in src.items():
        assert getattr(L, name) == value, name
    assert L.WAVES == 16 and L.SORT_BARRIER_STRIDE == 2 * src["WAVE"]
    assert L.TOPK_MAX_K == L.TOPK_THREADS          # one list entry per thread


def test_topk_key_bits_restated():
    one = L.ONE_BITS
    inf, nan = float("inf"), float("nan")
    for thr in (0.0, -0.0, -1.0, -inf, 1.0, 1.5, inf, nan, -nan):
        assert L.topk_key_bits(thr) == 30, thr        # no positive threshold below 1: every bit a score key can have
    # the fp32 thresholds either side of a digit-plan border: bits(1.0f) - bits(thr) = 2^10 - 1 | 2^10, 2^20 - 1 | 2^20
    for span, bits in ((1023, 10), (1024, 11), ((1 << 20) - 1, 20), (1 << 20, 21), (1, 1), (2, 2), (3, 2),
                       (one - 1, 30)):
        thr = L.bits_f32(one - span)
        assert 0 < thr < 1 and L.f32_bits(thr) == one - span
        assert L.topk_key_bits(thr) == bits, (span, thr)
        assert len(L.digit_plan(bits)) == (bits + 9) // 10 and sum(L.digit_plan(bits)) == bits
    assert L.topk_key_bits(0.1) == 25 and L.topk_key_bits(0.5) == 24      # (one - bits(0.5f) = 2^23)
    assert [L.digit_plan(b) for b in (9, 10, 11, 20, 21, 30)] == [(9,), (10,), (10, 1), (10, 10), (10, 10, 1),
                                                                    (10, 10, 10)]


def test_partitions_restated():
    for n, per in ((1, 64), (960, 64), (1024, 64), (1025, 128), (2048, 128), (2049, 192), (16384, 1024),
                   (16385, 1088), (107136, 6720)):
        cp = L.compact_plan(n)
        assert cp.per == per and cp.ept == -(-n // 1024), (n, cp.per, cp.ept)
        assert cp.waves[0][0] == 0 and max(i1 for _, i1 in cp.waves) == n
        assert all(a[1] == b[0] or b[0] == b[1] == n for a, b in zip(cp.waves, cp.waves[1:]))
    assert L.compact_plan(960).waves[15] == (960, 960) and L.compact_plan(961).waves[15] == (960, 961)
    assert [L.sort_plan(K) for K in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024)] == [
        (64, False), (64, False), (128, False), (128, False), (256, True), (256, True), (512, True), (512, True),
        (1024, True), (1024, True)]


def test_ids_are_unique_and_builders_are_deterministic():
    ids = [c.id for c in L.all_cases()]
    assert len(ids) == len(set(ids)) and len({g.id for g in L.GROUPS}) == len(L.GROUPS)
    g = L.GROUPS[5]
    again = L._build(g, "tie-r1", np.random.default_rng(L._seed(g.id, "tie-r1")))
    mine = next(c for c in L.group_cases(g.id) if c.family == "tie-r1")
    assert np.array_equal(again[0], mine.keys)


def test_claims_hold(walks):
    """What a family's construction guarantees is what the walk finds; every set keeps the selection's contract."""
    for c in L.all_cases():
        g, wk = c.group, walks[c.id]
        counted = L.counted_mask(c.keys, g.key_bits, g.leave_out)
        assert len(c.keys) == g.n and c.keys.dtype == np.uint32
        assert int(counted.sum()) == c.claim["counted"] > g.K, c.id
        for name in ("depth", "r", "r_class"):
            if name in c.claim:
                assert getattr(wk, name) == c.claim[name], (c.id, name, c.claim[name], getattr(wk, name))
        taken = c.keys[L.ref_select(c.keys, g.K, counted)]
        assert (c.keys[~counted].astype(np.int64) > int(taken.max())).all(), c.id  # left out: after every key taken
        plan = L.digit_plan(g.key_bits)
        if c.claim.get("first_bin"):
            assert wk.kc >> (g.key_bits - plan[0]) <= 1 and 0 in c.keys and g.values - 1 in c.keys[counted], c.id
            assert int(taken.max()) >> (g.key_bits - plan[0]) == 0, c.id
        if c.claim.get("last_bin"):
            assert int(taken.max()) >> (g.key_bits - plan[0]) == (g.values - 1) >> (g.key_bits - plan[0]), c.id
            assert g.values - 1 in c.keys[counted], c.id
        if c.family == "hot-bin":
            assert len(set((c.keys[counted] >> (g.key_bits - plan[0])).tolist())) == 1, c.id
        if c.family == "low":
            assert len(set((c.keys[counted] >> plan[-1]).tolist())) == 1, c.id
        if c.family in ("ascending", "descending"):
            d = np.diff(c.keys[counted].astype(np.int64))
            assert (d >= 0).all() if c.family == "ascending" else (d <= 0).all(), c.id


@pytest.mark.parametrize("form", L.FORMS)
def test_coverage(form, walks):
    cases = L.all_cases(form)
    groups = [g for g in L.GROUPS if form in g.forms]
    assert {g.key_bits for g in groups} == set(L.KEY_BITS)
    assert {g.K for g in groups} == set(L.KS)
    ns = {g.n for g in groups}
    assert set(L.NS) <= ns and {K for K in L.KS if K + 1 in ns} == set(L.KS)       # both sides of every n border, K + 1
    assert (set(L.NS_GLOBAL_ONLY) <= ns) == (form == 0) and max(ns) == (107136 if form == 0 else L.LDS_MAX_N)
    assert {L.sort_plan(g.K)[0] for g in groups} == {64, 128, 256, 512, 1024}
    assert {g.lo for g in groups} == {"none", "below", "above"}
    for g in groups:
        if g.lo == "below":
            assert g.leave_out < 1 << g.key_bits
        if g.lo == "above":
            assert g.leave_out >= 1 << g.key_bits
    tally = collections.Counter((walks[c.id].depth, walks[c.id].r_class) for c in cases)
    for c in cases:                                    # r = 1 of a bin of two is r = in_bin - 1 as well
        if walks[c.id].r == 1 and walks[c.id].in_bin == 2:
            tally[(walks[c.id].depth, "max")] += 1
    print(f"[topk-lattice] form {form}: {len(cases)} raw-key cases in {len(groups)} launches; (depth, r) classes "
          + ", ".join(f"{d}/{r}: {tally[(d, r)]}" for d in (1, 2, 3) for r in ("whole", "1", "max", "mid")))
    for depth in (1, 2, 3):
        for r in ("whole", "1", "max"):
            assert tally[(depth, r)] >= 3, (form, depth, r)
    # every width reaches its own last digit with r > 0 and, where it has more than one value, a whole bin there
    for B in L.KEY_BITS:
        D = len(L.digit_plan(B))
        mine = [walks[c.id] for c in cases if c.group.key_bits == B]
        assert any(w.depth == D and w.r > 0 for w in mine), B
        assert any(w.depth == D and w.r == 0 for w in mine), B
        assert {w.depth for w in mine} == set(range(1, D + 1)), B
    # ties at the cut: taken and not-taken members in different partitions of this form's compaction
    split = [L.tie_split(c, walks[c.id], form) for c in cases]
    assert sum(a for a, _ in split) >= 20 and sum(b for _, b in split) >= 10, (form, split)
    other = [L.tie_split(c, walks[c.id], 1 - form) for c in cases]          # the same keys split the other way too
    assert sum(a for a, _ in other) >= 20
    assert sum(1 for c in cases if c.claim["counted"] == c.group.K + 1) >= len(L.KS)
    assert {c.family for c in cases} == set(L.FAMILIES)
    fam = collections.Counter(c.family for c in cases)
    assert min(fam.values()) >= 20, fam
    # one launch whose sets stop at depths 1, 2 and 3
    assert any({1, 2, 3} <= {walks[c.id].depth for c in L.group_cases(g.id)} for g in groups)
    # uncounted keys on both sides of 2^key_bits appear among the sets, and 0xFFFFFFFF itself
    assert any((c.keys == np.uint32(0xFFFFFFFF)).any() for c in cases)


def test_model_equals_contract_and_every_mutant_is_caught(walks):
    """The second implementation (walk, take in index order, order by (key, index)) equals the stable argsort on every
    case; each one-line wrong version of it disagrees on at least one.

    `left-out-counted` is the exception, and the test asserts that too: under the header's contract (a key left out
    sorts after every key taken, more than K keys counted) counting the left-out value adds keys only behind rank K, in
    bins behind the cut's or in its bin behind the cut -- and a bin that holds the value is never taken whole, since kc
    would then lie above it and the compaction would take it.  So neither the selection nor (kc, r) can change: leaving
    the value out of `visit` saves histogram atomics and nothing else, and no case that keeps the contract can tell.
    The part of the sentinel convention that CAN be seen is a left-out value inside the cut's bin or before it: kc lands
    above it and the compaction takes it as well.  That breaks the contract, so it is no lattice case; the probe's guard
    sees it (tests/test_topk_lattice_gpu.py::test_broken_preconditions_are_refused_on_the_device, the `low` set)."""
    kills = {m: collections.Counter() for m in L.MUTANTS}
    for g in L.GROUPS:
        cases = L.group_cases(g.id)
        sets = [c.keys for c in cases]
        want = np.stack([L.expected(c.keys, g.K, g.key_bits, g.leave_out) for c in cases])
        assert np.array_equal(L.model(sets, g.K, g.key_bits, g.leave_out), want), g.id
        for m in L.MUTANTS:
            try:
                got = L.model(sets, g.K, g.key_bits, g.leave_out, m)
            except AssertionError:          # the wrong walk finds no bin for rank K
                got = np.full_like(want, -2)
            for c, a, b in zip(cases, got, want):
                if not np.array_equal(a, b):
                    kills[m][c.family] += 1
            if m == "left-out-counted":
                for c in cases:
                    wk = L.walk(c.keys, g.K, g.key_bits, g.leave_out, m)
                    assert (wk.kc, wk.r) == (walks[c.id].kc, walks[c.id].r), c.id
    for m in L.MUTANTS:
        print(f"[topk-lattice] mutant {m}: caught by {sum(kills[m].values())} cases of "
              f"{', '.join(sorted(kills[m])) or 'no family'}")
    for m in L.MUTANTS:
        assert (sum(kills[m].values()) == 0) == (m == "left-out-counted"), (m, kills[m])
    # the families built for a mutant catch it
    assert kills["ties-from-end"]["tie-r1"] and kills["wave-ties-not-offset"]["tie-r1"] and kills["r-minus-1"]["tie-rmax"]
    assert kills["r-plus-1"]["tie-fit"] and kills["digit-always-10"]["low"] and kills["high-keys-counted"]["sentinel"]
    assert kills["order-by-key-alone"]["equal"] and kills["every-set-reads-set-0"]["whole-1"]


# ---- the call-site cases ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def expf():
    from oracle import pyoracle as O

    return lambda x: O.libm_eval(2, x)


def test_call_site_labels(expf):
    """The labels of the cases that run through the public ops, on keys computed with the restated sigmoid: together
    they reach depth 3 with r > 0, depth <= 2 with r = 0, K + 1 candidates, and for CenterPoint (which derives its
    width from the threshold) every digit plan, with every counted key inside the derived width."""
    seen, widths = collections.Counter(), set()
    for name, pre, tname in L.CP_CASES:
        hm, masked, pre, thr, bits, span = L.cp_case(name)
        assert L.topk_key_bits(thr) == bits, name
        widths.add(bits)
        keys = L.cp_keys(hm, masked, thr, expf)
        for t, kind in enumerate(L.CP_KINDS):
            k = keys[t]
            real = k != L.KEY_OUT
            assert (k[real].astype(np.int64) < 1 << bits).all(), (name, kind)       # the derived width holds every key
            assert int(real.sum()) > pre, (name, kind)
            if thr > 0:
                assert L.KEY_OUT >= 1 << bits                                       # the sentinel is never counted
                wk = L.walk(k, pre, bits)
            else:                           # kKeyOut is below 2^30 and counted: bin 1023 of digit 1, behind every real key
                assert bits == 30 and L.KEY_OUT >> 20 == 1023 and int(k[real].max()) >> 20 <= L.ONE_BITS >> 20 == 1016
                wk = L.walk(k, pre, bits)
                assert wk.kc <= 1017 << 20 < L.KEY_OUT and (wk.kc, wk.r) == tuple(
                    (w.kc, w.r) for w in [L.walk(np.where(real, k, 0xFFFFFFFF).astype(np.uint32), pre, bits)])[0]
            want = L.ref_select(k, pre, real)
            got = L.model([k], pre, bits)[0][:pre]
            assert np.array_equal(got, want), (name, kind)
            seen[("cp", wk.depth, wk.r > 0)] += 1
            if kind == "pre-plus-1":
                assert int(real.sum()) == pre + 1, (name, kind, int(real.sum()))
                seen["cp-k+1"] += 1
            if kind == "tie-cluster":
                assert wk.r == 5 and L.tie_split(L.Case(L.Group(len(k), pre, bits, "none"), kind, k, {}), wk, 1)[0], name
    assert widths == {10, 11, 20, 21, 25, 30}
    for name in L.DECODE_CASES:
        cls, max_num = L.decode_logits(name)
        keys = L.decode_keys(cls, expf)
        assert keys.shape[1] == max_num + 1
        for k in keys:
            wk = L.walk(k, max_num, 30)
            seen[("decode", wk.depth, wk.r > 0)] += 1
            if L.DECODE_CASES[name][3] == "nan":
                assert wk.kc == L.KEY_NAN and 0 < wk.r < int((k == L.KEY_NAN).sum()), name   # the cut among the NaN keys
            if L.DECODE_CASES[name][3] == "ties":
                assert wk.r > 0 and int((k == wk.kc).sum()) == 7, name
    print("[topk-lattice] call sites:", dict(seen))
    for site in ("cp", "decode"):
        assert seen[(site, 3, True)] and any(seen[(site, d, False)] for d in (1, 2)), (site, seen)
    assert seen["cp-k+1"] == len(L.CP_CASES)


def test_bevdet_call_site_labels(expf):
    """bd_select_decode's cases: n = ncls * hw at K + 1 and at a multiple of 1024 -+ 1, the cut among the NaN keys,
    among saturated 1.0 scores tied across classes (and across a wave border of block_topk_compact), and deep."""
    seen = collections.Counter()
    for name, (ncls, h, w, K, plant) in L.BD_CASES.items():
        hm = L.bd_heatmap(name)
        n = ncls * h * w
        assert n == K + 1 or (n + 1) % 1024 == 0 or (n - 1) % 1024 == 0, name
        for b in range(2):
            k = L.score_key(L.sigmoid_f32(hm[b].reshape(-1), expf), L.BD_KEY_NAN)
            wk = L.walk(k, K, 30)
            assert np.array_equal(L.model([k], K, 30)[0][:K], L.ref_select(k, K, np.ones(n, bool))), name
            seen[(wk.depth, wk.r > 0)] += 1
            eq = np.nonzero(k == wk.kc)[0]
            if plant == "nan":
                assert wk.kc == L.BD_KEY_NAN and 0 < wk.r < len(eq), name
                seen["nan-cut"] += 1
            if plant == "saturated":
                assert wk.kc == 0 and wk.r == K and len(eq) == K + 7 + b and len(set((eq // (h * w)).tolist())) == ncls
                case = L.Case(L.Group(n, K, 30, "none"), plant, k, {})
                assert all(L.tie_split(case, wk, 0)), name      # the ties, and the taken ones alone, span wave borders
                seen["saturated"] += 1
            if n == K + 1:
                seen["k+1"] += 1
    print("[topk-lattice] bevdet call site:", dict(seen))
    assert seen[(3, True)] and seen["nan-cut"] and seen["saturated"] and seen["k+1"]


def test_ssd_call_site_labels(expf):
    """ssd_topk_kernel's cases: the sentinel below 2^key_bits and left out at a threshold <= 0, above it at a derived
    width other than 30; count == pre + 1; a tie cluster at the cut with r = 5 whose taken and not-taken members lie in
    different waves of block_topk_compact; both parities of n & 3."""
    seen = collections.Counter()
    for grid, tname, pre_kind in L.SSD_CASES:
        args, co, masks, ncls = L.ssd_setup(grid)
        cls, pre, thr, clusters = L.ssd_case(grid, tname, pre_kind)
        a = masks.shape[1]
        assert ((a & 3) == 0) == (grid == "n&3==0") and 64 < masks.sum(1).min() and masks.sum(1).max() < a // 4
        bits = L.topk_key_bits(thr)
        assert (bits == 30) == (thr <= 0)
        keys = L.ssd_keys(cls, masks, thr, expf)
        for b in range(2):
            k = keys[b]
            real = k != L.SSD_KEY_OUT
            assert int(real.sum()) == int(masks[b].sum()) > pre and (k[real].astype(np.int64) < 1 << bits).all()
            assert (L.SSD_KEY_OUT < 1 << bits) == (thr <= 0)        # left out by `visit` / never counted
            wk = L.walk(k, pre, bits, L.SSD_KEY_OUT)
            assert np.array_equal(L.model([k], pre, bits, L.SSD_KEY_OUT)[0][:pre], L.ref_select(k, pre, real))
            seen[("bits", bits)] += 1
            seen[(grid, thr <= 0)] += 1
            if int(real.sum()) == pre + 1:
                seen["k+1"] += 1
            if pre_kind == "cluster":
                eq = np.nonzero(k == wk.kc)[0]
                assert wk.depth == 3 and wk.r == 5 and np.array_equal(eq, np.sort(clusters[b])), (grid, tname, b)
                plan = L.compact_plan(a)
                assert plan.wave_of(eq[4]) != plan.wave_of(eq[5])  # the fifth tie is taken, the sixth is in the next wave
                seen["wave-split"] += 1
    print("[topk-lattice] ssd call site:", dict(seen))
    assert seen["k+1"] >= 4 and seen["wave-split"] == 8 and len([k for k in seen if k[0] == "bits"]) == 2
    assert all(seen[(g, z)] for g in L.SSD_GRIDS for z in (True, False))


def test_anchor3d_call_site_labels(expf):
    """a3d_topk_kernel's cases: nms_pre 63 / 64 / 65 / 129 / 1024 with N & 3 both ways, the cut inside a cluster of ten
    equal scores with five taken and the other five in the next wave of block_topk_compact."""
    for grid, (H, W, A) in L.A3D_GRIDS.items():
        N = H * W * A
        assert ((N & 3) == 0) == (grid == "N&3==0") and N > 1024
        for pre in L.A3D_NMS_PRE:
            x, cluster = L.a3d_select_case(grid, pre)
            s = L.sigmoid_f32(x, expf).max(1)
            k = (L.ONE_BITS - s.view(np.uint32).astype(np.int64)).astype(np.uint32)
            wk = L.walk(k, pre, 30)
            eq = np.nonzero(k == wk.kc)[0]
            assert wk.depth == 3 and wk.r == 5 and np.array_equal(eq, cluster), (grid, pre)
            plan = L.compact_plan(N)
            assert plan.wave_of(eq[4]) == 0 and plan.wave_of(eq[5]) == 1
            assert np.array_equal(L.model([k], pre, 30)[0][:pre], L.ref_select(k, pre, np.ones(N, bool)))
    for n in L.A3D_SET_SIZES:
        for total_cut in (False, True):
            (H, W, A), x = L.a3d_set_case(n, total_cut)
            s = L.sigmoid_f32(x, expf)
            assert int((s[:, 0] > 0.3).sum()) == n and int((s[:, 1] > 0.3).sum()) == (n // 2 if total_cut else 0)
            assert int((s[:, 2] > 0.3).sum()) == 0 and len(set(s[s[:, 0] > 0.3, 0].tolist())) < n     # ties in the set
    assert {L.sort_plan(n)[0] for n in L.A3D_SET_SIZES} == {64, 128, 256}
