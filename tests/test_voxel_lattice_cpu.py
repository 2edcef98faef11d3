"""The voxelizer lattice's own checks (tests/voxel_lattice.py), on the CPU: every case has the property its id claims under
the restated plans, the two references agree on every case, and the cells family would catch a wrong tolerance band."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_lattice as L  # noqa: E402

CASES = L.all_cases()


def test_ids_unique_and_counts(capsys):
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)
    counts = Counter(c.family for c in CASES)
    assert set(counts) == {"cells", "points", "groups", "slots", "voxels", "grids", "rows", "batch"}
    with capsys.disabled():
        print("\nvoxel lattice cases per family:", dict(counts), "index:", len(L.index_cases()), "total:", len(CASES))
    for c in CASES:
        assert set(c.forms) <= set(L.FAST) and c.D >= 3, c.id


def test_plan_restated_on_known_sizes():
    """The plans on sizes whose answer the kernels' own comments state."""
    nusc = 512 * 512
    pl = L.plan("wave", nusc, 270000, 20, 60000, 5, 16)
    assert (pl.ok, pl.groups, pl.cpg, pl.tile) == (True, 256, 1024, 10240)       # 27 tiles x 16 frames >= 384
    assert L.plan("wave", nusc, 270000, 20, 60000, 5, 1).tile == 4096
    assert L.plan("auto", 1440 * 1440 * 40, 270000, 10, 120000, 5, 8).kind == "wave3d"
    assert L.plan("auto", 1440 * 1440 * 40, 270000, 10, 120000, 5, 8).tile == 10240  # 27 x 8 >= 192
    assert not L.plan("wave", 1440 * 1440 * 40, 270000, 10, 120000, 5, 8).ok
    assert L.plan("auto", 1 << 29, 1000, 10, 1000, 5, 1).kind == "sort"
    assert L.plan("auto", 1 << 21, 1000, 10, 1000, 3, 1).kind == "tiled"          # the 3-D form writes D = 4 / 5 rows only
    assert L.plan("wave", 1 << 20, 1000, 10, 1000, 4, 1).ok and not L.plan("wave", (1 << 20) + 1, 1000, 10, 1000, 4, 1).ok
    assert L.plan("tiled", 1 << 22, 1000, 10, 1000, 4, 1).ok and not L.plan("tiled", (1 << 22) + 1, 1000, 10, 1000, 4, 1).ok
    assert L.plan("w3d", 1 << 28, 1000, 10, 1000, 4, 1).ok and not L.plan("w3d", (1 << 28) + 1, 1000, 10, 1000, 4, 1).ok
    assert L.plan("wave", 4096, 1000, 254, 100, 4, 1).ok and not L.plan("wave", 4096, 1000, 255, 100, 4, 1).ok
    assert L.plan("wave", 4096, 1000, 1, L.ROW_LIMIT - 1, 4, 1).ok and not L.plan("wave", 4096, 1000, 1, L.ROW_LIMIT, 4, 1).ok
    for ncells in (1, 2, 16, 2047, 2048, 4096):   # small grids: four groups, 128 threads of the assign kernel per group
        assert L.plan("wave", ncells, 1000, 3, 100, 4, 1).groups == 4
    key = np.arange(1 << 12)
    for gbits in (2, 8, 10):                       # (group, local) <-> key is a bijection
        back = np.concatenate([L.keys_of_group(g, gbits, 1 << 12) for g in range(1 << gbits)])
        assert np.array_equal(np.sort(back), key)
        assert all((L.group_of(L.keys_of_group(g, gbits, 1 << 12), gbits) == g).all() for g in range(1 << gbits))


def _tile_group_firsts(case, t, gbits, b=0):
    """{(tile, group): first points} and {tile: first points} of frame b under route tiles of t points."""
    k, pos, first = L.first_points(case, b)
    tile, grp = pos[first] // t, L.group_of(k[first], gbits)
    return Counter(zip(tile.tolist(), grp.tolist())), Counter(tile.tolist())


@pytest.mark.parametrize("case", L.family("points"), ids=lambda c: c.id)
def test_points_claims(case):
    b, n = L.sizes(case)
    assert n == case.c("N") and set(case.forms) & set(L.TILE_OF)
    for form in case.forms:
        if form in L.TILE_OF:
            pl = L.case_plan(case, form)
            assert pl.tile == L.TILE_OF[form] == case.c("T") or form in ("tiled", "gather", "w3d"), (case.id, form)
            assert pl.tiles == -(-n // pl.tile)
    k, pos, first = L.first_points(case, b - 1)
    assert pos[-1] == n - 1 and first[-1] and int((k == k[-1]).sum()) == 1, case.id   # the last point opens a cell of its own
    assert case.V > int(first.sum())                                                  # (no cell is hidden by the cap)
    assert n < 2000 or (0 < first.sum() < len(k) < n), case.id   # cells open and fill, some points lie outside


@pytest.mark.parametrize("case", L.family("groups"), ids=lambda c: c.id)
def test_groups_claims(case):
    gbits, group, t = case.c("gbits"), case.c("group"), L.GROUP_T
    pl = L.case_plan(case, "wave" if gbits == 8 else "w3d")
    assert pl.ok and pl.gbits == gbits and pl.tile == t
    k, pos, _ = L.first_points(case)
    mine = L.group_of(k, gbits) == group
    assert int(mine.sum()) == case.c("records") and len(np.unique(k[mine])) == case.c("cells")
    tiles = np.unique(pos[mine] // t).tolist()
    layout = case.c("layout")
    if layout == "one":
        assert tiles == [0]
    elif layout == "spread":
        assert set(tiles) <= {0, 2, 5} and pl.tiles == 7 and (case.c("records") < 3 or tiles == [0, 2, 5])
    else:
        run = pos[mine][pos[mine] < t]
        assert len(run) and np.array_equal(run, np.arange(t - len(run), t))   # a run ending at the tile's last point
    if gbits == 10:   # the 3-D form's borders: register steps by records, hash passes by distinct cells
        assert case.c("records") in (L.V3_REG - 1, L.V3_REG, L.V3_REG + 1) or \
            (case.c("records") > case.c("cells") and case.c("cells") in (L.V3_LOAD - 1, L.V3_LOAD, L.V3_LOAD + 1))
    last = k[mine][-min(3, case.c("cells")):]      # the group's last records open cells of their own
    assert all(int((k == c).sum()) == 1 for c in last.tolist()), case.id
    other = Counter(L.group_of(k[~mine], gbits).tolist())
    assert len(other) > (1 << gbits) // 2 and max(other.values()) < case.c("records") + 400   # shuffled background everywhere


@pytest.mark.parametrize("case", L.family("slots"), ids=lambda c: c.id)
def test_slots_claims(case):
    k, _, _ = L.first_points(case)
    mult = Counter(Counter(k.tolist()).values())
    for m in set(case.c("mults")):
        assert mult[m] >= 3 or (m == 1 and mult[m] >= 53), (case.id, m)
    assert mult[300] == 3 and case.V < len(set(k.tolist()))      # late points of a full cell, cells beyond the cap
    refused = [f for f in L.FAST if not L.case_plan(case, f).ok]
    if case.c("refused"):
        assert case.P == 255 and sorted(refused) == sorted(L.FAST) and L.case_plan(case, "auto").kind == "sort"
    else:
        assert len(refused) < len(L.FAST)


@pytest.mark.parametrize("case", L.family("voxels"), ids=lambda c: c.id)
def test_voxels_claims(case):
    k, pos, first = L.first_points(case)
    if case.c("cells"):
        assert int(first.sum()) == case.c("cells") and case.V in (1, 299, 300, 301)
    if case.c("firsts"):
        _, per_tile = _tile_group_firsts(case, case.c("T"), 2)
        want = case.c("firsts")
        assert tuple(per_tile[i] for i in range(len(want))) == want, (case.id, per_tile)
        assert case.ncells >= 16384
        after = pos[~first] > pos[first].max()    # points behind the last first point: of kept and of dropped cells
        order = {c: i for i, c in enumerate(k[first].tolist())}
        late = np.array([order[c] for c in k[~first][after].tolist()])
        assert case.V > int(first.sum()) - 50 or ((late < case.V).any() and (late >= case.V).any()), case.id
    if case.c("hold"):
        per, _ = _tile_group_firsts(case, case.c("T"), case.c("gbits"))
        pl = L.case_plan(case, "s0")
        assert pl.ok and pl.gbits == case.c("gbits") and pl.tile == case.c("T")
        tpg = max(L.ASSIGN_THREADS // pl.groups, 1)
        shares = set()
        for g, c in case.c("hold"):
            assert per[0, g] == c and per[1, g] == c, (case.id, g, per[0, g], per[1, g])
            shares |= {c * (s + 1) // tpg - c * s // tpg for s in range(tpg)}
        assert {L.HOLD, L.HOLD + 1} <= shares, (case.id, shares)
        assert min(per.values()) // tpg < L.HOLD                  # shares below kHold occur by themselves


@pytest.mark.parametrize("case", L.family("grids"), ids=lambda c: c.id)
def test_grids_claims(case):
    k, _, _ = L.first_points(case)
    assert k.min() == 0 and k.max() == case.ncells - 1 and case.grid == tuple(int(x) for x in case.pr[3:])
    kinds = {f: L.case_plan(case, f) for f in ("auto", "wave", "tiled", "w3d")}
    bits = L._bits(case.ncells)
    assert kinds["wave"].ok == (bits <= 20) and kinds["tiled"].ok == (bits <= 22)
    assert kinds["w3d"].ok == (20 < bits <= 28 and case.D in (4, 5))
    want = "wave" if bits <= 20 else ("wave3d" if bits <= 28 and case.D != 3 else ("tiled" if bits <= 22 else "sort"))
    assert kinds["auto"].kind == want, (case.id, kinds["auto"])


def test_grid_borders_present():
    bits = sorted(L._bits(g[0] * g[1] * g[2]) for g in L.GRIDS)
    assert {20, 21, 22, 23, 28, 29} <= set(bits) and bits[0] == 0


@pytest.mark.parametrize("case", L.family("rows") + L.family("batch"), ids=lambda c: c.id)
def test_rows_batch_claims(case):
    if case.family == "rows":
        assert (case.P * case.D) % 4 == case.c("rowmod")
    else:
        b, n = L.sizes(case)
        lens = L.data(case)[1]
        assert b == case.c("B") and len(lens) == b and n in lens and (b == 1 or 0 in lens)


def test_rows_cover_both_remainders():
    mods = {(c.D, c.c("rowmod") == 0) for c in L.family("rows")}
    for d in (3, 5, 6, 7):
        assert (d, True) in mods and (d, False) in mods
    assert (4, True) in mods and (8, True) in mods


@pytest.mark.parametrize("name,vs,pr,dyadic", L.CELL_GRIDS, ids=[g[0] for g in L.CELL_GRIDS])
def test_cells_family_catches_a_wrong_band(name, vs, pr, dyadic):
    """On every non-dyadic grid and axis the bare floor((p - lo) * fp32(1 / size)) differs from ref_cells on some of the
    family's points, and vt_axis_cell's tolerance band, emulated in NumPy, agrees with ref_cells on all of them."""
    grid = L.grid_of(vs, pr)
    for axis in range(3):
        vals = L.axis_values(vs, pr, axis)
        pts = np.zeros((len(vals), 3), np.float32)
        for a in range(3):
            pts[:, a] = vals if a == axis else np.float32(pr[a]) + np.float32(vs[a]) * np.float32(0.5)
        cells, inside = L.ref_cells(pts, vs, pr)
        want = np.where(inside, cells[:, axis], -1)
        band = L.axis_cell_band(vals, pr[axis], vs[axis], grid[axis])
        bare = L.axis_cell_band(vals, pr[axis], vs[axis], grid[axis], fallback=False)
        assert np.array_equal(band, want), (name, axis, int((band != want).sum()))
        share = float((bare != want).mean())
        print(f"cells {name} axis {axis}: {len(vals)} points, bare multiply differs on {int((bare != want).sum())}")
        if axis in dyadic:
            assert share == 0.0, (name, axis)
        else:
            assert share > 0.0, (name, axis)
        assert inside.any() and (~inside).any()


@pytest.mark.parametrize("case", L.family("cells"), ids=lambda c: c.id)
def test_cells_every_point_is_decisive(case):
    """No point of the family hides behind P: an inside point holds a slot below P in its cell, and the edge cell a point
    outside the range would join holds fewer than P earlier points -- a single wrong cell changes hard_voxelize's output."""
    pts = L.frame_points(case, 0)
    earlier = L.earlier_inside(pts, case.vs, case.pr)
    assert int(earlier.max()) < case.P, (case.id, int(earlier.max()), int((earlier >= case.P).sum()))
    _, inside = L.ref_cells(pts, case.vs, case.pr)
    rv, rc, rn, rnv = L.ref_hard_voxelize(pts, case.vs, case.pr, case.P, case.V)
    assert int(rn.sum()) == int(inside.sum()) and rnv < case.V      # every inside point is stored


def test_plan_follows_the_row_writer():
    """max_voxels * rowq counts the units of the writer that runs: floats, not float4s, behind a misaligned voxels tensor
    (except D = 4 / 5 on the wave form, whose slot-per-lane writer does not care)."""
    v = 1 << 21
    for form in ("tiled", "gather", "wave", "s0", "prio", "split"):
        assert L.plan(form, 4096, 1000, 1, v, 8, 1).ok and not L.plan(form, 4096, 1000, 1, v, 8, 1, aligned=False).ok, form
    assert L.plan("auto", 4096, 1000, 1, v, 8, 1, aligned=False).kind == "sort"
    assert L.plan("wave", 4096, 1000, 1, 4 * v - 8192, 4, 1, aligned=False).ok
    assert not L.plan("tiled", 4096, 1000, 1, 4 * v - 8192, 4, 1, aligned=False).ok
    assert L.plan("tiled", 4096, 1000, 1, 4 * v - 8192, 4, 1).ok


def test_cells_specials_present():
    for name, vs, pr, _ in L.CELL_GRIDS:
        for axis in range(3):
            vals = L.axis_values(vs, pr, axis)
            assert np.isnan(vals).any() and np.isposinf(vals).any() and np.isneginf(vals).any()
            assert (vals == np.float32(L.FLT_MAX)).any() and (np.abs(vals) == np.float32(1e30)).any()
            if pr[axis] == 0.0:
                tiny = vals[(np.abs(vals) < 1e-38)]
                assert np.signbit(tiny[tiny == 0]).any() and (~np.signbit(tiny[tiny == 0])).any()
                assert {1, 4, 5, 8} <= set(np.round(np.abs(tiny) / L.DENORM).astype(np.int64).tolist())
    # the single-cell z test: a negative t whose quotient rounds to -0 lies in cell 0 (size 8: -4 denormals, not -5)
    lo, hi = L.single_cell_bounds(8.0)
    assert lo == np.float32(-4 * L.DENORM) and hi == np.nextafter(np.float32(8.0), np.float32(0.0))
    pts = np.array([[0.1, 0.1, -4 * L.DENORM], [0.1, 0.1, -5 * L.DENORM], [0.1, 0.1, -0.0]], np.float32)
    _, inside = L.ref_cells(pts, (0.25, 0.25, 8.0), (-50.0, -50.0, 0.0, 50.0, 50.0, 8.0))
    assert inside.tolist() == [True, False, True]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_port_equals_restatement(oracle, case):
    """The oracle port equals ref_hard_voxelize on every frame of every case, bit for bit."""
    b, _ = L.sizes(case)
    for f in range(b):
        pts = L.frame_points(case, f)
        rv, rc, rn, rnv = L.port_reference(oracle, case, f)
        wv, wc, wn, wnv = L.ref_hard_voxelize(pts, case.vs, case.pr, case.P, case.V)
        assert rnv == wnv, (case.id, f, rnv, wnv)
        np.testing.assert_array_equal(rc, wc)
        np.testing.assert_array_equal(rn, wn)
        np.testing.assert_array_equal(rv.view(np.uint32), wv.view(np.uint32))
    if case.family == "cells":
        assert L.port_reference(oracle, case)[3] == case.c("occupied") < case.V
