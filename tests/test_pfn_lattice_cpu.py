"""CPU side of the pillar encoders' lattice (tests/pfn_lattice.py): the restated dispatcher against the numbers in
csrc/pfn.hip, every case's claim, the borders the cases reach, the exact class's bound, the fp64 references against the
oracle's fp32 statements, and mutated references that the cases must tell from the true one."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pfn_lattice as L  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [c for c in L.CASES if not c.seed and c.D >= 3]                      # cases that own their data (and have a net)
OWNERS = list({L._key(c).id: c for c in L.CASES if c.seed and c.M == c.base_m}.values())   # the largest of a shared set


def _shape(P, D, cd, c1, c2, M=67, vper=0):
    return L.Case("", "", M, P, D, cd, c1, c2, "real", vper=vper)


def test_ids_unique_and_counts(capsys):
    ids = [c.id for c in L.CASES] + [c.id for c in L.SCATTER_CASES] + [c.id for c in L.MEAN_CASES]
    assert len(set(ids)) == len(ids)
    counts = Counter(c.family for c in L.CASES)
    counts.update(scatter=len(L.SCATTER_CASES), mean=len(L.MEAN_CASES))
    assert set(counts) == {"dispatch", "rows", "stride", "index", "scatter", "mean"}
    with capsys.disabled():
        print("\npfn lattice cases:", dict(counts))


def test_constants_restated_from_the_source():
    with open(os.path.join(ROOT, "paddle3d_amd", "csrc", "pfn.hip")) as f:
        assert L.read_constants(f.read()) == L.CONSTANTS


def test_dispatch_borders():
    """Both sides of every border of the dispatcher, under the restatement."""
    f = lambda *a, path=0, **kw: L.form(_shape(*a, **kw), path)  # noqa: E731
    assert (f(26, 4, 2, 32, 64).nv, f(21, 5, 2, 32, 64).nv) == (13, 20)                 # P D = 104 | 105
    assert (f(19, 5, 2, 32, 64).park, f(24, 4, 2, 32, 64).park) == (False, True)        # 95 | 96
    assert (f(31, 4, 3, 64, 64).park, f(32, 4, 3, 64, 64).park) == (False, True)        # 124 | 128
    assert all(f(p, 4, 3, 64, 64).kernel == "packed64" and f(p, 4, 3, 64, 64).w2g for p in (16, 64))
    assert (f(64, 4, 3, 64, 64, path=1).kernel, f(65, 4, 3, 64, 64, path=1).kernel) == ("mfma64", "generic")
    assert f(65, 4, 3, 64, 64, path=2).status == -3
    assert (f(32, 4, 2, 64, 0).kernel, f(26, 5, 2, 64, 0).kernel) == ("single64", "generic")   # 128 | 130
    assert f(25, 5, 2, 64, 0).kernel == "single64"
    assert (f(32, 4, 2, 32, 64, path=1).kernel, f(26, 5, 2, 32, 64, path=1).kernel) == ("mfma32", "generic")
    assert (f(32, 5, 2, 32, 64).kernel, f(33, 4, 2, 32, 64).kernel) == ("packed32", "generic")   # P = 32 | 33, 8 P D = 1280
    assert f(33, 4, 2, 32, 64, path=2).status == -3
    assert (f(1, 4, 2, 32, 64).status, f(2, 5, 3, 32, 64).status, f(3, 4, 2, 32, 64).kernel) == (-3, -3, "packed32")
    assert (f(5, 4, 2, 64, 17).status, f(6, 4, 2, 64, 17).kernel) == (-3, "generic")
    assert f(9, 4, 2, 30, 17).status == -3 and f(9, 4, 2, 68, 17).status == -3 and f(9, 4, 2, 36, 65).status == -3
    assert f(9, 2, 2, 32, 64).status == -1 and f(9, 4, 2, 32, 64, path=3).status == -1
    assert f(20, 5, 2, 32, 64, M=0) == L.Form()
    def g(p, m=64, v=8, n=100, ls=100):
        return L.form(_shape(p, 5 if p <= 25 else 4, 2, 32, 64, M=m, vper=v), 0, True, n, ls)

    assert (g(24).nsl, g(25).nsl) == (3, 4)                                              # 8 P = 192 | 200
    assert g(20, v=12).status == -3 and g(20, m=60, v=16).status == -3 and g(33).status == -3
    assert g(20, n=(1 << 24) - 1, ls=(1 << 24) - 1).kernel == "packed32"
    assert g(20, n=1 << 24).status == -3 and g(20, ls=1 << 24).status == -3
    assert g(20, m=1 << 22, v=8).status == -3 and g(20, ls=0).status == -1
    w = L.WAVE_NET
    lasts = [L.generic_border(w["D"], w["cd"], w["c1"], w["c2"], k) for k in (8, 4, 2, 1)]
    assert lasts == [52, 105, 210, 421] and L.generic_border(w["D"], w["cd"], w["c1"], w["c2"], 0) == 422
    for p, k in zip(lasts, (8, 4, 2, 1)):     # worked out from the kernel's LDS: 8960 weight floats + waves * 76 P <= 40960
        assert 8960 + k * 76 * p <= 40960 < 8960 + k * 76 * (p + 1)


def test_cases_reach_every_form():
    seen, packed, idx, above = Counter(), set(), set(), set()
    for c in L.CASES:
        if c.family == "index":
            f = L.form(c, 0, True, 100, 100)
            assert f.kernel == "packed32", c.id
            idx.add((f.nv, f.nsl, f.park))
            continue
        for p in L.paths(c):
            f = L.form(c, p)
            seen[f.kernel or f.status] += 1
            if f.kernel == "generic":
                seen[("generic", f.waves)] += 1
            if f.kernel.startswith("packed"):
                packed.add((f.kernel, f.nv, f.park, f.w2g))
            if f.kernel and not c.seed and (L.pillars(c)[1] > c.P).any():
                above.add((f.kernel, f.waves, c.values))
    assert {"single64", "packed32", "packed64", "mfma32", "mfma64", "generic", -1, -3} <= set(seen)
    assert {("generic", k) for k in (8, 4, 2, 1)} <= set(seen)
    assert packed == {("packed32", 13, False, False), ("packed32", 13, True, False), ("packed32", 20, True, False),
                      ("packed64", 32, False, True), ("packed64", 32, True, True)}
    assert {(nv, nsl) for nv, nsl, _ in idx} == {(13, 3), (13, 4), (20, 3), (20, 4)}
    # every non-indexed kernel, the generic one at every wave count, sees num_points above P in both value classes
    assert above == {(k, w, v) for v in ("exact", "real") for k, w in
                     [(k, 0) for k in ("single64", "packed32", "packed64", "mfma32", "mfma64")] +
                     [("generic", w) for w in (8, 4, 2, 1)]}


@pytest.mark.parametrize("case", L.family("dispatch"), ids=lambda c: c.id)
def test_dispatch_claims(case):
    forms = [L.form(case, p) for p in (0, 1, 2)]
    if case.c("status") is not None:
        assert all(f.status == case.c("status") and not f.kernel for f in forms)
    if case.c("waves") is not None:
        assert forms[0].kernel == forms[1].kernel == "generic" and forms[0].waves == case.c("waves")
    vox, npv, co = L.pillars(case)
    assert vox.shape == (case.M, case.P, case.D) and (co[npv > 0, 0] > 0).any() and (co[npv > 0, 1] > 0).all()
    if case.M >= 9:
        live = np.flatnonzero(npv > 0)
        _, ncx, ncy, _ = L.GEOMETRY[case.values]
        assert tuple(co[live[0], 2:]) == (0, 0) and tuple(co[live[-1], 2:]) == (ncy - 1, ncx - 1)
        assert case.P == 1 or {case.P, case.P - 1, 0} <= set(npv.tolist())
    if case.shift != "plain":
        b1 = L.params(case)["b1"]
        assert (b1 < 0).all() if case.shift == "neg" else (b1 >= 64).all()


@pytest.mark.parametrize("case", L.family("rows"), ids=lambda c: c.id)
def test_rows_claims(case):
    _, npv, _ = L.pillars(case)
    R, live, notfull, masks = L.chunk_layout(npv[:L.PK], case.P)
    assert (R, live) == (case.c("R"), case.c("live"))
    if case.c("end0") is not None:
        assert (masks[0] if masks else 0) == case.c("end0")
    assert L.form(case, 2).kernel in ("packed32", "packed64")
    assert L.form(case, 2).park == (case.P * case.D >= (128 if case.c1 == 64 else 96))
    name = case.fill
    if name == "R16-ends-on-block":
        assert masks[0] >> 15 == 1 and len(masks) == 1
    if name == "straddle2":
        assert len(masks) == 2 and masks[1] == 1 << 3
    if name == "straddle3":
        assert len(masks) == 3 and masks[1] == 0 and masks[2] == 1 << 2     # rows 15 .. 34 of blocks 0, 1 and 2
    if name == "first-empty":
        assert live & 1 == 0
    if name == "R8P-then-ones":
        assert notfull == 0 and (npv[L.PK:] == 1).all()
    if name == "above-P":
        assert (npv > case.P).sum() == 3


def test_rows_patterns_cover_the_listed_totals():
    rs = {L._rows_patterns(20)[n][1]["R"] for n in L.ROWS_PATTERNS}
    assert {0, 1, 15, 16, 17, 32, 160} <= rs
    forms = {(c.fill, L.form(c, 2).kernel, L.form(c, 2).park) for c in L.family("rows")}
    assert forms == {(n, k, p) for n in L.ROWS_PATTERNS for k in ("packed32", "packed64") for p in (False, True)}


@pytest.mark.parametrize("case", [c for c in L.family("stride") + L.family("index") if c.c("cap")], ids=lambda c: c.id)
def test_stride_claims(case):
    cap = case.c("cap")
    assert case.M in (cap - 8, cap, cap + 8, 2 * cap, 2 * cap + 8)
    if case.family == "stride":
        f = L.form(case, case.c("path"))
        assert (f.kernel, f.cap) == (case.c("kernel"), cap)
    else:
        assert L.form(case, 0, True, 100, 100).cap == cap
    _, npv, _ = L.pillars(case)
    if case.family == "stride":    # a chunk of full pillars, and one-point pillars in the chunk its wave walks next
        assert (npv[:L.PK] == case.P).all() and (case.M <= cap or (npv[cap:cap + L.PK] == 1).all())


def test_stride_sizes_cover_both_sides_of_every_cap():
    for kernel, *_ in L.STRIDE_NETS:
        cs = [c for c in L.family("stride") if c.c("kernel") == kernel]
        cap = cs[0].c("cap")
        want = {cap - 8, cap, cap + 8} | (set() if kernel == "packed64" else {2 * cap, 2 * cap + 8})
        assert {c.M for c in cs if c.values == "exact"} == want == {c.M for c in cs if c.values == "real"}
    assert {c.c("cap") for c in L.family("stride")} == {24576, 16384, 8192}


@pytest.mark.parametrize("case", [c for c in L.family("index") if not c.seed or c.M == c.base_m], ids=lambda c: c.id)
def test_index_claims(case):
    """The hand-made index names exactly the case's pillars, out of order, with gaps, through a permuted cloud."""
    points, span, plist = L.index_of(case)
    vox, npv, co = L.pillars(case)
    v2, n2 = L.rows_from_index(points, span, plist, case.P)
    np.testing.assert_array_equal(v2, vox)
    np.testing.assert_array_equal(n2, npv)
    assert npv.max() <= case.P and points.shape[0] == case.c("frames") == case.M // case.vper
    assert plist.shape[1] == points.shape[1] + case.list_extra
    v = case.vper
    pad = npv == 0
    assert pad[3::v].all() and pad[v - 1::v].all() and (co[pad] == (-1, 0, 0, 0)).all() and (span[pad] == 0).all()
    if case.c("empty_frame") is not None:
        e = case.c("empty_frame")
        assert pad[e * v:(e + 1) * v].all()
    disorder = gaps = permuted = False
    for f in range(min(case.c("frames"), 16)):
        s0 = span[f * v:(f + 1) * v][~pad[f * v:(f + 1) * v]]
        if len(s0) < 2:
            continue
        disorder |= bool((np.diff(s0[:, 0]) < 0).any())                                  # not in firing order
        order = np.argsort(s0[:, 0])
        gaps |= bool(((s0[order, 0] + s0[order, 1])[:-1] < s0[order, 0][1:]).any())       # gaps between runs
        run = plist[f][s0[0, 0]:s0[0, 0] + s0[0, 1]]
        permuted |= bool((np.diff(run) != 1).any())                                       # points permuted in the cloud
    assert disorder and gaps and permuted


def test_index_cases_cover_the_listed_layouts():
    cs = L.family("index")
    assert {c.P for c in cs} == {20, 24, 25, 32} and {c.D for c in cs} == {4, 5} and {c.cd for c in cs} == {2, 3}
    assert {c.vper for c in cs} == {8, 16, 4096} and {1, 2, 5} <= {c.c("frames") for c in cs}
    assert any(c.list_extra > 0 for c in cs) and any(c.list_extra == 0 for c in cs)


def _sample(case):
    """The pillars of a case the CPU tests evaluate: all of a small case; of a large shared set its head (the chunk of full
    pillars) and both sides of its kernel's grid cap (every pillar is drawn alike, so the rest adds time, not cases)."""
    if not case.seed:
        return np.arange(case.M)
    cap = case.c("cap")
    return np.concatenate([np.arange(1024), np.arange(cap - 512, min(cap + 512, case.M))])


@pytest.mark.parametrize("case", [c for c in L.CASES if c.values == "exact"], ids=lambda c: c.id)
def test_exact_bound(case):
    assert L.exact_bound(case) < 2 ** 24


@pytest.mark.parametrize("case", [c for c in SMALL + OWNERS if c.values == "exact"], ids=lambda c: c.id)
def test_exact_limits_hold_on_the_data(case):
    """What exact_bound assumes about the values is true of the values: every measured stage lies within its limit, and
    every number of the case lies on the grid its stage is counted in."""
    limit, got = L.exact_stages(case), L.measured_stages(case, _sample(case))
    assert set(got) == set(limit) and all(got[k] <= limit[k] for k in got), (got, limit)
    vox, _, _ = L.pillars(case)
    prm = L.params(case)
    on = lambda a, step: a is None or bool((np.asarray(a, np.float64) * step % 1 == 0).all())  # noqa: E731
    assert on(vox, 4) and on(L.geometry(case)[3:], 4) and on(prm["w1"], 1) and on(prm["w2"], 1)
    assert on(prm["s1"], 2) and on(prm["s2"], 2) and on(prm["b1"], 4) and on(prm["b2"], 4)
    assert all(np.log2(v) % 1 == 0 for v in L.geometry(case)[:3])


# ---- the references against the oracle's fp32 statements ------------------------------------------------------------------
def _unit_var():
    """A BatchNorm variance whose fp32 sqrt(var + 1e-3) is exactly 1: the oracle then applies (scale, shift) as folded."""
    v = np.float32(1.0) - np.float32(1e-3)
    for _ in range(8):
        if np.sqrt(np.float32(v + np.float32(1e-3)), dtype=np.float32) == np.float32(1.0):
            return v
        v = np.nextafter(v, np.float32(2.0))
    raise AssertionError("no such variance")


def _oracle_out(oracle, case, rows):
    vox, npv, co = (a[rows] for a in L.pillars(case))
    prm = L.params(case)
    var = _unit_var()
    layers = [dict(weight=prm[f"w{i}"], gamma=prm[f"s{i}"], beta=prm[f"b{i}"], mean=np.zeros_like(prm[f"s{i}"]),
                   var=np.full_like(prm[f"s{i}"], var)) for i in (1, 2) if prm[f"w{i}"] is not None]
    vx, vy, vz, xo, yo, zo = L.geometry(case)
    live = npv > 0
    fn = oracle.hard_vfe_forward_torch if case.cd == 3 else oracle.pfn_forward_torch
    out = np.zeros((len(npv), case.cout), np.float32)
    out[live] = fn(vox[live], npv[live], co[live], layers, (vx, vy, vz), (xo - vx / 2, yo - vy / 2, zo - vz / 2)).reshape(
        int(live.sum()), case.cout)
    return out


_RATIO = {"max": 0.0, "case": ""}


@pytest.mark.parametrize("case", SMALL + OWNERS, ids=lambda c: c.id)
def test_reference_against_fp32_oracle(oracle, case):
    """The oracle's fp32 statement lies within the derived bound of the fp64 reference (with a factor 2 to spare) and equals
    it bit for bit on the exact class."""
    rows = _sample(case)
    out = _oracle_out(oracle, case, rows)
    ref, tol = L.reference_rows(case, rows)
    assert L.compare(case, out, ref, tol / 2 if case.values == "real" else tol) is None
    if case.values == "real":
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.nanmax(np.where(tol > 0, np.abs(out - ref) / tol, 0.0))
        if r > _RATIO["max"]:
            _RATIO.update(max=float(r), case=case.id)


def test_report_oracle_ratio(capsys):
    with capsys.disabled():
        print(f"\nlargest fp32-oracle error / derived bound: {_RATIO['max']:.4f} ({_RATIO['case']})")
    assert _RATIO["max"] < 0.5


# ---- mutated references: the cases tell them from the true one -----------------------------------------------------------
@pytest.mark.parametrize("mut", L.MUTATIONS)
def test_cases_catch_a_mutated_reference(mut):
    caught = []
    for case in SMALL:
        if case.family == "index" or L.form(case, 0).status:
            continue
        vox, npv, co = L.pillars(case)
        ref, tol = L.reference(case)
        wrong = L.ref_pfn(vox, npv, co, L.params(case), L.geometry(case), case.cd, mut=mut)
        if L.compare(case, wrong.astype(np.float32), ref, tol) is not None:
            caught.append(case)
    assert caught, mut
    assert {c.values for c in caught} == {"exact", "real"}, mut      # each class catches it on its own
    if mut == "z_in_2d":
        assert all(c.cd == 2 for c in caught)
    if mut == "min_div":      # told apart only where a count lies above P -- on every kernel (test_cases_reach_every_form)
        assert all((L.pillars(c)[1] > c.P).any() for c in caught)
        assert {str(L.form(c, p).kernel) for c in caught for p in (0, 1, 2)} >= {
            "single64", "packed32", "packed64", "mfma32", "mfma64", "generic"}


def test_scatter_reference(oracle):
    for c in L.SCATTER_CASES:
        feats, co = L.scatter_data(c)
        canvas, inv = L.ref_scatter(feats, co, c.batch, c.ny, c.nx)
        assert canvas.shape == (c.batch, c.C, c.ny, c.nx)
        if c.kind == "unique":
            np.testing.assert_array_equal(canvas, oracle.pillar_scatter(feats, co, c.batch, c.ny, c.nx))
            np.testing.assert_array_equal(canvas, oracle.pillar_scatter_numpy(feats, co, c.batch, c.ny, c.nx))
            assert (inv >= 0).sum() == c.M
        first, _ = L.ref_scatter(feats, co, c.batch, c.ny, c.nx, first_wins=True)
        assert (first != canvas).any() == c.kind.startswith("dup"), c.id
        if c.kind.startswith("dup"):
            n = int(c.kind[3:])
            cell = (co[-1, 0] * c.ny + co[-1, 2]) * c.nx + co[-1, 3]
            assert inv.reshape(-1)[cell] == c.M - 1 and (co[:, [0, 2, 3]] == co[-1, [0, 2, 3]]).all(1).sum() == n
        if c.kind == "invalid":
            assert (inv >= 0).sum() == c.M - 8 and set(inv[inv >= 0].tolist()).isdisjoint({20, 21, 22, 23, 44, 45, 46, 47})
    assert {(c.C % 4 == 0, (c.ny * c.nx) % 4) for c in L.SCATTER_CASES} >= {(True, 0), (False, 0), (True, 1), (True, 2)}
    assert {c.vec4 for c in L.SCATTER_CASES} == {True, False}


def test_mean_reference(oracle):
    for c in L.MEAN_CASES:
        vox, npv = L.mean_data(c)
        ref = L.ref_voxel_mean(vox, npv)
        with np.errstate(divide="ignore", invalid="ignore"):
            o = oracle.voxel_mean(vox, npv)
        if c.M > 3:
            assert np.isnan(ref[2]).all() and np.isposinf(ref[3]).all() and (npv > c.P).any()
        if c.values == "exact":
            np.testing.assert_array_equal(o, ref.astype(np.float32))
        else:
            fin = np.isfinite(ref)
            assert (np.abs(o[fin].astype(np.float64) - ref[fin]) <= (c.P + 1) * 2.0 ** -24 * np.abs(ref[fin])).all()
    assert {c.D for c in L.MEAN_CASES} == {3, 4, 5} and {c.P for c in L.MEAN_CASES} == {1, 10, 35}
    assert {m * d for m, d in ((c.M, c.D) for c in L.MEAN_CASES)} >= {255, 256, 258, 260}


def test_forward_indexed_declines_a_grid_the_cell_words_cannot_hold():
    """PillarFeatureNet.forward_indexed answers None, before it touches a tensor, where an axis has more than 65 536 cells
    (the indexed kernel carries x and y in 16 bits each); 65 536 cells (cells 0 .. 65 535) pass this check."""
    from paddle3d_amd.centerpoint import PillarFeatureNet
    from paddle3d_amd.ops.voxel_encoder import INDEXED_MAX_AXIS_CELLS

    assert INDEXED_MAX_AXIS_CELLS == 1 << L.CONSTANTS["cell_bits"]
    for nx, ny in ((131072, 8), (8, 65537)):
        net = PillarFeatureNet(4, (64, 64), voxel_size=(1, 1, 8), point_cloud_range=(0, 0, -3, nx, ny, 5))
        assert net.grid_xy == (nx, ny)
        assert net.forward_indexed(None, None, None, None) is None
    # a quotient of exactly k + 1/2 rounds away from zero in the voxelizer (std::round): 65 537 cells, not 65 536
    net = PillarFeatureNet(4, (64, 64), voxel_size=(1, 1, 8), point_cloud_range=(0, 0, -3, 65536.5, 2.5, 5))
    assert net.grid_xy == (65537, 3) and net.forward_indexed(None, None, None, None) is None
    net = PillarFeatureNet(4, (64, 64), voxel_size=(1, 1, 8), point_cloud_range=(0, 0, -3, 65536, 8, 5))
    with pytest.raises(RuntimeError):      # goes on to the op, which wants device tensors
        net.forward_indexed(None, None, None, None)
