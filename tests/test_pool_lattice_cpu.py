"""The pooling lattice's own checks (tests/pool_lattice.py), on the CPU: the restated constants equal the kernels' sources,
the case list covers every radix plan, `per = 2` and both sides of every tile border, every reference agrees with its second
implementation, and the coordinate family's planted values fall on the side of the boundary their label claims."""
import os
import sys
from collections import Counter

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_lattice as L  # noqa: E402

SORT, PREP, POOL, FRUSTUM, REFUSED = L.all_sort_cases(), L.prepare_cases(), L.all_pool_cases(), L.frustum_cases(), \
    L.refused_cases()


def test_ids_unique_and_families(capsys):
    ids = [c.id for c in SORT + PREP + POOL + tuple(FRUSTUM) + tuple(REFUSED)] + [L.big_sort_case().id]
    assert len(set(ids)) == len(ids)
    fam = Counter(c.family for c in PREP)
    assert set(fam) == {"sizes", "grids", "coord", "occupancy"} and all(v > 0 for v in fam.values())
    kinds = Counter(c.kind for c in SORT)
    assert set(kinds) == set(L.SORT_KINDS) | {"sizes", "f32", "table"}
    chain = [c for c in POOL if c.source]
    assert len(POOL) > len(chain) > 0 and len(FRUSTUM) == 4 and len(REFUSED) == len(L.REFUSED_GRIDS)
    assert {p.family for p in PREP if p.cells <= L.CHAIN_MAX_CELLS} == set(fam)     # the chain draws on every family
    with capsys.disabled():
        print("\npool lattice: sort", dict(kinds), "prepare", dict(fam), "pool", len(POOL) - len(chain), "chain", len(chain))


def test_constants_equal_the_sources():
    """A changed constant in radix_sort.hpp / scan.hpp / bev_pool.hip fails here before any coverage claim is trusted."""
    src = L.source_constants()
    for name, value in src.items():
        assert getattr(L, name) == value, (name, getattr(L, name), value)
    assert L.RS_TILE == src["RS_THREADS"] * src["RS_ROUNDS"] == 2048
    assert L.SCAN_TILE == src["SCAN_THREADS"] * src["SCAN_ITEMS"] == 4096
    assert L.BIG_N == 2048 * 4096 + 1 and L.BIG_MAX_KEY == 1023


def test_plan_switch_points():
    """Key widths 10 / 11, 20 / 21 and 30 / 31 bits: 1x10, 2x6, 2x10, 3x7, 3x10, 4x8; fp32 keys always run 4x8."""
    names = [L.plan(mk, 1).name for mk in (1023, 1024, (1 << 20) - 1, 1 << 20, (1 << 30) - 1, 1 << 30)]
    assert tuple(names) == L.PLANS
    assert L.plan(0, 1).name == L.plan(1, 1).name == "1x1" and L.plan(3, 1).name == "1x2"
    assert L.plan((1 << 31) - 1, 1).name == L.plan(0xFFFFFFFF, 1).name == "4x8"
    p = L.plan(1023, 2049)
    assert (p.tiles, p.bins, p.hist_ints, p.scan_tiles, p.per) == (2, 1024, 2048, 1, 1)
    assert all(L.plan(mk, 1).bins <= L.RS_MAX_BINS for mk in range(0, 1 << 12)) and L.plan(0xFFFFF, 5).bins == L.RS_MAX_BINS


def test_cases_cover_plans_and_borders():
    mode0 = [c for c in SORT if c.mode == 0]
    assert set(L.PLANS) <= {c.plan.name for c in mode0}
    assert {c.plan.name for c in SORT if c.mode == 1} == {"4x8"}
    assert set(L.PLANS) <= {c.plan.name for c in PREP}
    assert {c.max_key for c in mode0} >= set(L.MAX_KEYS)
    for mk in L.MAX_KEYS:     # every key family at every max_key that leaves it room
        kinds = {c.kind for c in mode0 if c.max_key == mk}
        assert kinds >= (set(L.SORT_KINDS) if mk > 1 else {"equal"}), (mk, kinds)
    borders = [t + d for t in (L.BLOCK, L.RS_TILE, L.SCAN_TILE) for d in (-1, 0, 1)] + [1, 2, 3 * L.RS_TILE + 1]
    assert set(borders) == set(L.NS)
    for mode in (0, 1):
        assert {c.n for c in SORT if c.mode == mode} >= set(borders), mode
    for mode in (0, 1, 2):
        assert {len(L.coor_of(c)) for c in PREP if c.mode == mode and c.family == "sizes"} == set(borders), mode
    # the scan over the [digit][tile] table: exactly one scan tile, two, and the first size with per = 2
    hist = {c.plan.hist_ints for c in mode0}
    assert L.SCAN_TILE in hist and any(L.SCAN_TILE < h <= 2 * L.SCAN_TILE for h in hist) and any(h < L.SCAN_TILE for h in hist)
    big = L.big_sort_case()
    assert big.plan.per == 2 and big.plan.name == "1x10" and big.plan.tiles == 4097 and big.plan.scan_tiles == 1025
    assert L.plan(big.max_key, big.n - 1).per == 1                      # one key fewer: the branch does not run
    assert all(L.plan(mk, big.n - 1).per == 1 for mk in L.MAX_KEYS)     # and no other plan reaches it at a smaller n
    assert max(c.plan.per for c in SORT + PREP) == 1


@pytest.mark.parametrize("case", SORT, ids=lambda c: c.id)
def test_ref_argsort_equals_torch(case):
    keys = L.sort_keys(case)
    got = L.ref_argsort(keys, case.mode)
    t = torch.from_numpy(keys.copy())
    want = torch.argsort(t, stable=True, descending=True) if case.mode == 1 else torch.argsort(t.long(), stable=True)
    np.testing.assert_array_equal(got, want.numpy())
    assert sorted(got.tolist()) == list(range(case.n))


def test_sort_families_are_what_they_claim():
    for c in SORT:
        if c.mode != 0 or c.kind in ("sizes", "table"):
            continue
        k, p = L.sort_keys(c).astype(np.int64), c.plan
        mask, top = (1 << p.digit_bits) - 1, (p.passes - 1) * p.digit_bits
        if c.kind == "equal":
            assert len(set(k.tolist())) == 1
        elif c.kind == "two":
            assert set(k.tolist()) == {0, c.max_key}
        elif c.kind == "top" and c.max_key > 1:
            assert len(set((k & ((1 << top) - 1)).tolist())) == 1 and len(set((k >> top).tolist())) > 1
        elif c.kind == "bottom":
            assert len(set((k >> p.digit_bits).tolist())) == 1 and len(set((k & mask).tolist())) > 1
        elif c.kind == "extremes":
            for j in range(p.passes):
                d = (k >> (j * p.digit_bits)) & mask
                assert (d == 0).any() and ((d == mask).any() or j == p.passes - 1), (c.id, j)
            assert (k == c.max_key).any() and (k == 0).any()
        elif c.kind == "maxkey":
            assert (k == c.max_key).any()
        elif c.kind == "sorted":
            assert (np.diff(k) >= 0).all() and k[0] != k[-1]
        elif c.kind == "reverse":
            assert (np.diff(k) <= 0).all() and k[0] != k[-1]


def test_f32_specials_present():
    for c in SORT:
        if c.mode == 1 and c.n >= 255:
            bits = L.sort_keys(c).view(np.uint32)
            assert set(L.F32_SPECIALS.tolist()) <= set(bits.tolist()), c.id
            assert Counter(bits.tolist())[0x7FC00000] >= 2          # planted values tie with themselves
    order = L.ref_argsort(L.F32_SPECIALS.view(np.float32), 1)
    v = L.F32_SPECIALS.view(np.float32)[order]
    nan = int(np.isnan(v).sum())
    assert nan == 8 and np.isnan(v[:nan]).all() and np.isposinf(v[nan]) and np.isneginf(v[-1])
    assert order[:nan].tolist() == sorted(order[:nan].tolist())      # NaNs of either sign and any payload: input order
    z = [int(i) for i in order if L.F32_SPECIALS[i] in (0x80000000, 0)]
    assert z == [0, 1]                                               # -0.0 before +0.0: as planted


def test_big_case_closed_form():
    """big_sort_expected at a size the host sorts at once (the same residue n % 1024 == 1, the same multiplier)."""
    for n in (1025, 1024 * 9 + 1):
        keys = (np.arange(n, dtype=np.int64) * L.BIG_MUL) % 1024
        np.testing.assert_array_equal(L.big_sort_expected(np.arange(n, dtype=np.int64), n=n), L.ref_argsort(keys, 0))
    t = torch.arange(1024 * 9 + 1)
    np.testing.assert_array_equal(L.big_sort_expected(t, n=len(t)).numpy(), L.big_sort_expected(t.numpy(), n=len(t)))


def _finite(case):
    q = L.ref_quotient(L.coor_of(case), case.lower, case.step)
    return bool(np.isfinite(q).all() and (np.abs(q) < 2.0 ** 62).all())


@pytest.mark.parametrize("case", PREP, ids=lambda c: c.id)
def test_ref_prepare(oracle, case):
    """Mode 0 equals oracle.pyoracle.voxel_pooling_prepare_v2_numpy on every finite case (and on the finite points of the
    others); modes 1 and 2 are a re-ordering of the same kept points: the same (point, cell coordinates) set, keys ascending
    under their own order, mode 2's ranks_feat the split form of mode 0; every case's claim holds."""
    coor = L.coor_of(case)
    n, b, d, hw = len(coor), case.batch, case.depth_bins, case.feat_hw
    assert n % (b * d * hw) == 0, case.id
    rb, rd, rf, st, ln = L.prep_reference(case)
    cells, kept = L.ref_cells(coor, case.lower, case.step, case.size)
    fin = coor if _finite(case) else np.where(kept[:, None], coor, np.float32(case.lower[0] - 10 * case.step[0]))
    assert _finite(case) or case.family == "coord"
    want = oracle.voxel_pooling_prepare_v2_numpy(fin.reshape(b, n // (b * d * hw), d, hw, 1, 3), case.lower, case.step, case.size)
    if case.mode == 0:
        for g, w in zip((rb, rd, rf, st, ln), want):
            np.testing.assert_array_equal(g, w)
    else:
        assert sorted(rd.tolist()) == sorted(want[1].tolist())
        full_rf = np.empty(n, np.int64)
        full_rf[want[1]] = want[2]
        np.testing.assert_array_equal(rf, rd if case.mode == 1 else full_rf[rd])
        gx, gy, gz = (int(s) for s in case.size)
        c = cells[rd]
        np.testing.assert_array_equal(rb, (((rd // (n // b)) * gz + c[:, 2]) * gx + c[:, 0]) * gy + c[:, 1])
    assert (np.diff(rb.astype(np.int64)) >= 0).all() and (rb >= 0).all()
    assert len(st) == len(ln) == len(np.unique(rb)) and int(ln.sum()) == len(rb) == int(kept.sum())
    same = rb[1:] == rb[:-1]
    assert (np.diff(rd)[same] > 0).all()                                   # stability: points of a cell in index order
    if case.c("kept") is not None:
        assert len(rb) == case.c("kept"), case.id
    if case.c("intervals") is not None:
        assert len(st) == case.c("intervals"), case.id
    if case.c("n") is not None:
        assert n == case.c("n") and (n < 255 or 0 < len(rb) < n)
    if case.c("cells") is not None:
        assert case.cells == case.c("cells") <= L.MAX_CELLS and rb[0] == 0 and int(rb[-1]) == case.cells - 1
        p = case.plan
        mask = (1 << p.digit_bits) - 1
        for j in range(p.passes):   # every digit all-zero and all-one on some kept key
            dig = (rb.astype(np.int64) >> (j * p.digit_bits)) & mask
            top = ((case.cells - 1) >> (j * p.digit_bits)) & mask if j == p.passes - 1 else mask
            assert (dig == 0).any() and (dig == top).any(), (case.id, j)


def test_occupancy_claims():
    occ = {c.id: c for c in PREP if c.family == "occupancy"}
    for mode in (0, 1, 2):
        m = f"m{mode}"
        for name, at in (("first", 0), ("last", 4096)):
            assert L.prep_reference(occ[f"occ-{name}-{m}"])[1].tolist() == [at]
        rd = L.prep_reference(occ[f"occ-lastbatch-{m}"])[1]
        assert rd.min() >= 1400 and len(rd) == 700
        rd = L.prep_reference(occ[f"occ-interleave-{m}"])[1]
        assert (rd % 2 == 0).all() and len(L.coor_of(occ[f"occ-interleave-{m}"])) == 4098
        for n in (L.SCAN_TILE, L.SCAN_TILE + 1):
            assert (L.prep_reference(occ[f"occ-distinct{n}-{m}"])[4] == 1).all()
        assert L.prep_reference(occ[f"occ-onecell-{m}"])[4].tolist() == [L.SCAN_TILE + 1]
    assert {(c.depth_bins, c.feat_hw) for c in occ.values() if c.c("dhw")} == set(L.DHW)
    for c in occ.values():      # on gx != gy != gz with B = 2 the two cell orders differ
        if c.c("dhw"):
            assert c.batch == 2 and c.size == (5.0, 3.0, 2.0)
            a = L.ref_prepare(L.coor_of(c), 2, c.depth_bins, c.feat_hw, c.lower, c.step, c.size, 0)
            b = L.ref_prepare(L.coor_of(c), 2, c.depth_bins, c.feat_hw, c.lower, c.step, c.size, 1)
            assert not np.array_equal(a[1], b[1]) and sorted(a[1].tolist()) == sorted(b[1].tolist()), c.id
            assert len(a[3]) == 60                                   # every cell of both batch entries is occupied


def test_grid_borders():
    for cells, (gx, gy, gz, b) in L.PLAN_GRIDS.items():
        assert gx * gy * gz * b == cells <= L.MAX_CELLS and len({gx, gy, gz}) > 1
    assert max(L.PLAN_GRIDS) == L.MAX_CELLS and {1023, 1024, (1 << 20) - 1, 1 << 20, 1 << 30, 2047 << 20} <= set(L.PLAN_GRIDS)
    prods = {name: g[0] * g[1] * g[2] * g[3] for name, g in L.REFUSED_GRIDS.items()}
    assert all(p > L.MAX_CELLS for p in prods.values())
    assert prods["2049x1024x1024"] == (1 << 31) + (1 << 20) < 0xFFFFFFFF       # below the former bound: was accepted
    assert {0xFFFFFFFF, 1 << 32} <= set(prods.values()) and prods["2^30x2^30x2^30"] % (1 << 64) == 0
    for c in REFUSED:
        assert all(float(np.float32(s)) == s for s in c.size)                   # the sizes are exact as fp32


@pytest.mark.parametrize("case", [c for c in PREP if c.family == "coord" and c.mode == 0], ids=lambda c: c.id)
def test_coord_plants_fall_where_they_claim(case):
    coor = L.coor_of(case)
    cells, kept = L.ref_cells(coor, case.lower, case.step, case.size)
    q = L.ref_quotient(coor, case.lower, case.step)
    seen = Counter()
    by_key = {}
    for row, axis, label, k in L.coord_plants(case):
        size = int(case.size[axis])
        others = [a for a in range(3) if a != axis]
        assert (cells[row, others] >= 0).all() or not kept[row]
        inside_others = all(0 <= np.trunc(q[row, a]) < case.size[a] for a in others)
        assert inside_others, (case.id, row)                        # the planted axis alone decides
        cell, keep, qq = int(cells[row, axis]), bool(kept[row]), float(q[row, axis])
        if label in ("lo", "hi"):
            by_key[axis, k, label] = coor[row, axis]
            seen[label, min(max(k, -1), 2) if k < size - 1 else ("last" if k == size - 1 else "size")] += 1
            if k == -1:
                assert (qq <= -1 and not keep) if label == "lo" else (-1 < qq < 0 and keep and cell == 0), (case.id, axis, qq)
            elif label == "lo":
                assert qq < k and keep and cell == max(k - 1, 0), (case.id, axis, k, qq, cell)
                assert k > 0 or (-1 < qq < 0)                       # within one step below the lower bound: cell 0, kept
            else:
                assert qq >= k and (keep and cell == k if k < size else not keep), (case.id, axis, k, qq, cell)
        elif label == "special":
            v = coor[row, axis]
            if not np.isfinite(v) or abs(v) >= 1e30 or abs(qq) > 1e18:
                assert not keep, (case.id, axis, float(v))
            else:
                assert v == 0 and keep == (0 <= np.trunc(qq) < size)
    for (axis, k, label), v in by_key.items():
        if label == "lo":
            assert np.nextafter(v, np.float32(np.inf)) == by_key[axis, k, "hi"]    # fp32 neighbours
    assert seen["lo", -1] == seen["hi", -1] == 3 and seen["lo", "size"] == seen["hi", "size"] == 3
    col = coor[[r for r, _, lab, _ in L.coord_plants(case) if lab == "special"]]
    assert np.isnan(col).any() and np.isposinf(col).any() and np.isneginf(col).any() and np.signbit(col[col == 0]).any()
    big = np.abs(L.ref_quotient(col, case.lower, case.step))
    with np.errstate(invalid="ignore"):
        assert ((big > np.float32(L.CLAMP)) & (big < 1e19)).any() and ((big <= np.float32(L.CLAMP)) & (big > 9e18)).any()
    assert kept.any() and (~kept).any()
    # "one step below or more is dropped" is a statement about the quotient: the k = -1 'lo' plant is the largest fp32 value
    # whose quotient is <= -1.  On the dyadic grid it is lower - step itself with the quotient -1.0; on the others no fp32
    # value has that quotient (BEVDet's -52.0 gives f32(-52 - f32(-51.2)) / f32(0.8) = -0.999999: cell 0, kept -- the
    # reference's rule, planted as a 'near' value)
    for row, axis, label, k in L.coord_plants(case):
        if (label, k) == ("lo", -1):
            assert q[row, axis] <= np.float32(-1.0) and not kept[row], (case.id, axis, float(q[row, axis]))
            if case.c("grid") == "lss-05":
                assert q[row, axis] == np.float32(-1.0)
                assert coor[row, axis] == np.float32(case.lower[axis]) - np.float32(case.step[axis])


@pytest.mark.parametrize("case", POOL, ids=lambda c: c.id)
def test_ref_pool_equals_port(oracle, case):
    d = L.pool_data(case)
    rd, rf, rb, ln, st = d.fwd
    got, dg, fg = L.pool_reference(case)
    want = oracle.bev_pool_v2(d.depth, d.feat, rd, rf, rb, ln, st, (d.cells, case.channels), kind="port")
    assert L.same_bits(got, want)
    named = np.zeros(d.cells, bool)
    named[rb] = True
    assert not got[~named].view(np.uint32).any()                      # cells no interval names stay zero
    rd, rf, rb, ln, st = d.bwd
    wdg, wfg = oracle.bev_pool_v2_bkwd(d.out_grad, d.depth, d.feat, rd, rf, rb, ln, st, kind="port")
    assert L.same_bits(dg, wdg) and L.same_bits(fg, wfg)


def test_pool_tables_are_what_they_claim():
    built = [c for c in POOL if not c.source]
    assert {c.channels for c in built} == set(L.POOL_CHANNELS)
    totals = {len(c.lengths) * c.channels for c in built if c.channels == 1}
    assert {L.BLOCK - 1, L.BLOCK, L.BLOCK + 1} <= totals
    u = L.POOL_U
    assert {1, 2, u - 1, u, u + 1, 2 * u - 1, 2 * u, 2 * u + 1, 3 * u, 3 * u + 1} == set(L.LENGTH_MIX)
    for c in built:
        d = L.pool_data(c)
        if len(c.lengths) > 1:
            assert set(c.lengths) == set(L.LENGTH_MIX), c.id
            total = len(c.lengths) * c.channels
            assert total > L.BLOCK - 2 and (c.channels in (1, 256) or total % L.BLOCK), c.id     # straddles a block edge
        else:
            assert c.lengths == (100,)
        for (rd, rf, rb, ln, st), group, other in ((d.fwd, 2, 1), (d.bwd, 1, 2)):
            t = (rd, rf, rb)
            heads = t[group][st]
            assert len(set(heads.tolist())) == len(st)                     # distinct per interval ...
            assert len(st) < 3 or not (np.diff(heads) > 0).all()           # ... and not monotone
            assert len(set(rd.tolist())) == len(rd)                        # a depth entry belongs to one point
            if len(st) > 20:
                owners = {}
                for iv, (s, n) in enumerate(zip(st.tolist(), ln.tolist())):
                    for r in set(t[other][s:s + n].tolist()):
                        owners.setdefault(r, set()).add(iv)
                assert max(len(v) for v in owners.values()) > 1            # rows shared between intervals
        assert np.isinf(d.feat).any() == (d.feat.size >= 256 and len(c.lengths) > 1) and d.cells > len(d.fwd[4])
        assert np.isinf(d.depth).any() == (len(c.lengths) > 1) and (len(c.lengths) == 1 or np.signbit(d.depth[d.depth == 0]).any())
        out, _, fg = L.pool_reference(c)
        for r, heads in ((out, d.fwd[2][d.fwd[4]]), (fg, d.bwd[1][d.bwd[4]])):   # inf / NaN sums stay the exception
            assert np.isfinite(r[heads]).mean() >= 0.8, (c.id, float(np.isfinite(r[heads]).mean()))
            assert len(c.lengths) == 1 or not np.isfinite(r[heads]).all(), c.id


@pytest.mark.parametrize("case", FRUSTUM, ids=lambda c: c.id)
def test_ref_frustum(case):
    """The fp32 restatement against the same chain in float64 (a sanity bound: 3 x 3 products of values below 1e5)."""
    fr, a, pt, c, tr, bda = L.frustum_data(case)
    got = L.ref_frustum_to_lidar(fr, case.cams, a, pt, c, tr, bda)
    assert got.shape == (case.batch * case.cams * case.per_cam, 3) and got.dtype == np.float32
    f64 = [x.astype(np.float64) for x in (fr, a, pt, c, tr, bda)]
    p = f64[0][None] - f64[2][:, None]
    p = np.einsum("cij,cpj->cpi", f64[1], p)
    p = np.concatenate([p[..., :2] * p[..., 2:], p[..., 2:]], -1)
    p = np.einsum("cij,cpj->cpi", f64[3], p) + f64[4][:, None]
    want = np.einsum("cij,cpj->cpi", f64[5][np.arange(len(a)) // case.cams], p).reshape(-1, 3)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    assert np.linalg.cond(a).max() < 10 and np.linalg.cond(c).max() < 10 and np.linalg.cond(bda).max() < 10
