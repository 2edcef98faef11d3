"""tests/sparse_lattice.py checked against itself and against dense torch, on the CPU: its NumPy index reference against the
dense occupancy oracle, its gather reference against dense conv3d, the lattice against the clauses of the dispatch it is
meant to straddle, the exact class against its representability bound, the case ids."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_lattice as L  # noqa: E402

GEMM = L.all_gemm_cases()
INDEX = L.index_cases()
SMALL = [c for c in INDEX if c.small]


def _mask(coords, batch, shape):
    ok = L.valid_rows(coords, batch, shape)
    c = np.asarray(coords, np.int64)[ok]
    m = torch.zeros(batch, 1, *shape, dtype=torch.float64)
    m[c[:, 0], 0, c[:, 1], c[:, 2], c[:, 3]] = 1
    return m


def _steps(case, plan):
    """(input rows, input shape, (kernel, stride, padding, subm), (out_coords, nbr, out_shape)) per convolution."""
    if plan:
        _, cur, sets = L.plan_reference(case)
    else:
        cur, sets = L.index_coords(case), L.chain_reference(case)
    shape = case.shape
    for spec, got in zip(case.chain, sets):
        yield cur, shape, spec, got
        cur, shape = got[0], got[2]


@pytest.mark.parametrize("plan", [False, True], ids=["indices", "plan"])
@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.id)
def test_index_reference_matches_dense_occupancy(case, plan):
    """Output set = conv3d of the occupancy mask > 0 (tests/test_sparse_conv_gpu.py::_dense_oracle), in raster order; a
    submanifold convolution keeps its input rows; nbr holds the highest row of the coordinate it names."""
    for cur, shape, (ks, st, pd, subm), (oc, nbr, oshape) in _steps(case, plan):
        ok = L.valid_rows(cur, case.batch, shape)
        mask = _mask(cur, case.batch, shape)
        if subm:
            assert oshape == tuple(shape) and np.array_equal(oc, cur)
            assert (nbr[~ok] == -1).all()
            centre = nbr[:, nbr.shape[1] // 2]
            assert (centre[ok] >= np.nonzero(ok)[0]).all()          # itself, or a later row of the same coordinate
            assert np.array_equal(np.asarray(cur)[centre[ok]], np.asarray(cur)[ok])
        else:
            active = F.conv3d(mask, torch.ones(1, 1, *ks, dtype=torch.float64), stride=st, padding=pd) > 0
            assert tuple(active.shape[2:]) == oshape
            want = active[:, 0].nonzero().numpy()                    # nonzero() lists in raster order
            assert np.array_equal(oc, want), (case.id, len(oc), len(want))
            keys = L.keys_of(oc, oshape)
            assert (np.diff(keys) > 0).all()
        assert nbr.max(initial=-1) < len(cur) and (ok[nbr[nbr >= 0]]).all()


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.id)
def test_gather_reference_matches_dense_conv3d(case):
    """gather_reference on the reference's nbr = float64 conv3d of the densified rows (the highest row of a coordinate is
    the one a dense tensor holds), read at the output coordinates."""
    g = torch.Generator().manual_seed(5)
    cin, cout = 3, 2
    for cur, shape, (ks, st, pd, subm), (oc, nbr, oshape) in _steps(case, False):
        feats = torch.randint(-4, 5, (len(cur), cin), generator=g).double()
        weight = torch.randint(-3, 4, (int(np.prod(ks)), cin, cout), generator=g).double()
        got = L.gather_reference(feats, torch.from_numpy(nbr), weight)
        ok = L.valid_rows(cur, case.batch, shape)
        dense = np.zeros((case.batch, cin) + tuple(shape))
        for i in np.nonzero(ok)[0]:                                  # ascending: the highest row stays
            b, z, y, x = (int(v) for v in cur[i])
            dense[b, :, z, y, x] = feats[i].numpy()
        w = weight.reshape(*ks, cin, cout).permute(4, 3, 0, 1, 2).contiguous()
        pad = tuple(k // 2 for k in ks) if subm else pd
        full = F.conv3d(torch.from_numpy(dense), w, stride=st, padding=pad)
        live = L.valid_rows(oc, case.batch, oshape)
        o = np.asarray(oc, np.int64)[live]
        want = full[o[:, 0], :, o[:, 1], o[:, 2], o[:, 3]]
        assert torch.equal(got[torch.from_numpy(live)], want), case.id
        assert not got[torch.from_numpy(~live)].any()               # a padding row of a submanifold set: no neighbour


def test_large_key_case_is_large():
    case = next(c for c in INDEX if c.axis == "large")
    co = L.index_coords(case)
    cells = case.batch * int(np.prod(case.shape))
    assert 1 << 31 < cells < 0xFFFFFFFE
    keys = L.keys_of(co, case.shape)
    assert 2000 <= len(keys) <= 4000 and len(np.unique(keys)) == len(keys)
    assert (keys >= 1 << 31).sum() * 3 >= len(keys)
    assert keys.min() == 0 and keys.max() == cells - 1
    (oc0, nbr0, _), (oc1, nbr1, osh1) = L.chain_reference(case)
    assert (nbr0 >= 0).sum() > 3 * len(oc0) and (nbr1 >= 0).sum() > 1.5 * len(oc1)   # neighbourhoods, not lone voxels
    # device memory: the output-cell byte map dominates
    assert case.batch * int(np.prod(osh1)) + 16 < 512 << 20
    for name, batch, shape in L.GRID_REFUSALS:
        assert batch * int(np.prod(shape)) >= 0xFFFFFFFF, name
    assert (4 * 16 * 8192 * 8192) % (1 << 32) == 0


def test_lattice_straddles_every_dispatch_clause():
    """Sets, so that an edited case list fails here: every template instance of every entry, both sides of every clause of
    the fp32 dispatch and of every refusal, every border of the row sweep."""
    run = [c for c in GEMM if not c.axis.startswith("refuse") and c.o("status") is None]
    fp32 = {c.path for c in run if c.entry == "fp32"}
    assert fp32 == ({f"rows<{nb},{t}>" for nb in (1, 2, 4, 8) for t in (4, 8)} | {f"mfma<{nb}>" for nb in (1, 2, 4, 8)}
                    | {"valu<1>", "valu<2>", "valu<1>:goto", "valu<2>:goto"})
    assert {c.path for c in run if c.entry == "x3"} == {f"x3<{n},{k}>" for n in (1, 2, 4) for k in (16, 32)}
    assert {c.path for c in run if c.entry == "f16"} == {f"f16<{n},{k}>" for n in (1, 2, 4) for k in (16, 32, 64)}
    ch = [c for c in run if c.axis == "channels"]
    shapes = {(c.cin, c.cout, c.kvol) for c in ch if c.entry == "fp32"}
    assert {s[0] for s in shapes} >= set(L.CIN_SWEEP) == {1, 3, 4, 5, 7, 16, 17, 32, 33, 48, 64, 128}
    assert {s[1] for s in shapes} >= set(L.COUT_SWEEP) == {1, 8, 16, 24, 32, 48, 64, 112, 128}
    assert {s[2] for s in shapes} >= set(L.KVOL_SWEEP) == {1, 2, 3, 8, 9, 27, 28, 36}
    for entry in ("x3", "f16"):
        assert {(c.cin, c.cout, c.kvol) for c in ch if c.entry == entry} == {
            (a, b, k) for a in (16, 32, 48, 64, 128) for b in (32, 64, 128) for k in (1, 3, 27)}
    # the clauses of pd3_sparse_conv3d_features_ordered, one pair each: (shape inside, nearest shape outside) -> other kernels
    pairs = [((16, 16, 3), (17, 16, 3)), ((16, 16, 3), (5, 16, 3)),      # cin % 16
             ((16, 16, 27), (16, 16, 28)),                                # kernel_volume <= 27
             ((16, 16, 3), (16, 24, 3)), ((16, 32, 3), (16, 48, 3)),      # cout in (16, 32, 64, 128)
             ((5, 16, 3), (5, 24, 3)), ((5, 16, 3), (5, 8, 3)),           # cout % 16
             ((5, 128, 3), (5, 112, 3)), ((16, 48, 3), (16, 64, 3)),      # cout / 16 not in (1, 2, 4, 8): the VALU kernel
             ((16, 64, 3), (16, 112, 3)), ((5, 64, 3), (5, 112, 3)),      # cout <= 64: one or two columns per lane
             ((32, 16, 3), (48, 16, 3)), ((32, 16, 3), (16, 16, 3))]      # cin % 32: eight or four channels per lane
    for a, b in pairs:
        assert a in shapes and b in shapes and L.fp32_path(*a) != L.fp32_path(*b), (a, b)
    assert (4, 16, 3) in shapes and L.fp32_path(4, 16, 3) == L.fp32_path(5, 16, 3)      # float4 rows / scalar rows, one kernel
    # alignment: each fp32 case runs another kernel than its aligned twin; the 16-bit entries answer -1
    al = [c for c in GEMM if c.axis == "align"]
    assert {(c.entry, c.o("misalign")) for c in al} == {(e, w) for e in ("fp32", "x3", "f16", "gg16")
                                                          for w in ("feats", "weight")}
    moved = {(c.cin, c.cout, c.o("misalign")): (L.fp32_path(c.cin, c.cout, c.kvol), c.path) for c in al if c.entry == "fp32"}
    assert moved[(16, 16, "feats")] == ("rows<1,4>", "valu<1>") and moved[(16, 16, "weight")] == ("rows<1,4>", "valu<1>")
    assert moved[(5, 16, "feats")] == ("mfma<1>", "mfma<1>") and moved[(5, 16, "weight")] == ("mfma<1>", "valu<1>")
    assert moved[(16, 128, "weight")] == ("rows<8,4>", "valu<2>") and moved[(32, 48, "feats")] == ("valu<1>:goto", "valu<1>")
    assert {c.cin % 16 == 0 for c in al if c.entry == "fp32"} == {True, False}
    assert all(c.o("status") == -1 for c in al if c.entry != "fp32")
    # refusals, and the accepted neighbour of each in the lattice
    ref = {(c.entry, c.axis): c for c in GEMM if c.axis.startswith("refuse")}
    assert set(ref) == ({("fp32", "refuse:cout<=128"), ("fp32", "refuse:valu-lds"), ("gg16", "refuse:out_off%4"),
                         ("gg16", "refuse:off+cout<=ld")}
                        | {(e, a) for e in ("x3", "f16", "gg16") for a in ("refuse:kvol<=27", "refuse:cin%16", "refuse:cout")}
                        | {(e, "refuse:scale-without-shift") for e in ("fp32", "x3", "f16")})
    c = ref[("fp32", "refuse:cout<=128")]
    assert (c.cout, c.path, c.o("status")) == (144, "refuse:cout", -3) and any(s[1] == 128 for s in shapes)
    c = ref[("fp32", "refuse:valu-lds")]
    assert c.path == "refuse:lds" and c.o("status") == -3
    # cin = 256, cout = 120 asks for 155776 bytes of LDS: under the 160 KiB bound, so it RUNS (valu<2>); 16 channels more do not
    assert (256, 120, 1) in shapes and L.fp32_path(256, 120, 1) == "valu<2>" and (c.cin, c.cout) == (272, 120)
    assert (256 * 120 + 32 * 256) * 4 + 128 == 155776 <= 160 * 1024 < (272 * 120 + 32 * 272) * 4 + 128
    for e in ("x3", "f16", "gg16"):
        assert ref[(e, "refuse:kvol<=27")].kvol == 28 and ref[(e, "refuse:kvol<=27")].o("status") == -3
    assert any(c.kvol == 27 for c in ch if c.entry == "x3") and any(c.kvol == 27 for c in ch if c.entry == "f16")
    assert (32, -1) in L.TILE_ORDER_REFUSALS
    assert any(c.order and c.kvol == 27 for c in ch) and not any(c.order and not 1 < c.kvol <= 31 for c in GEMM)
    assert ref[("gg16", "refuse:out_off%4")].o("off") % 4 and ref[("gg16", "refuse:out_off%4")].o("status") == -1
    assert any(c.entry == "gg16" and c.o("off") == 4 for c in run)
    # rows: every border of every kernel's tile, the 16-row block and the window, each in the four forms
    rows = [c for c in GEMM if c.axis == "rows"]
    assert {L.tile_rows(c.path) for c in rows} == {32, 64, 128, 256}
    for entry, cin, cout in L.ROW_KERNELS:
        mine = [c for c in rows if (c.entry, c.cin, c.cout) == (entry, cin, cout)]
        t = L.tile_rows(mine[0].path)
        want = {1, 15, 16, 17, t - 1, t, t + 1, 8191, 8192, 8193}
        for order in (False, True):
            for cap in (False, True):
                assert {c.rows for c in mine if c.order == order and c.cap == cap} == want, (entry, cin, order, cap)
        assert all(c.alloc_rows % 8192 == 0 and c.alloc_rows > c.rows for c in mine if c.cap)
    # epilogue: all sixteen combinations per kernel, fp32 output, channel slices
    ep = [c for c in GEMM if c.axis == "epilogue"]
    for entry, cin, cout in L.ROW_KERNELS:
        assert {c.epi for c in ep if (c.entry, c.cin, c.cout) == (entry, cin, cout) and not c.opt} == set(L.EPILOGUES)
    assert len(set(L.EPILOGUES)) == 16 and any(c.o("out_f32") for c in ep)
    assert {(c.o("ld"), c.o("off")) for c in ep if c.entry == "gg16"} == {(32, 0), (40, 0), (40, 8), (96, 64), (36, 4)}


def test_index_lattice_covers_the_listed_borders():
    by_axis = {}
    for c in INDEX:
        by_axis.setdefault(c.axis, []).append(c)
    assert {c.chain[0] for c in by_axis["geometry"]} == {g for _, g in L.GEOMETRIES} and len(L.GEOMETRIES) == 13
    assert {g for _, g in L.GEOMETRIES} == {
        ((3, 3, 3), (1, 1, 1), (1, 1, 1), True), ((1, 1, 3), (1, 1, 1), (0, 0, 1), True), ((1, 3, 3), (1, 1, 1), (0, 1, 1), True),
        ((3, 3, 3), (2, 2, 2), (1, 1, 1), False), ((3, 3, 3), (2, 2, 2), (0, 1, 1), False), ((3, 1, 1), (2, 1, 1), (0, 0, 0), False),
        ((1, 1, 1), (1, 1, 1), (0, 0, 0), False), ((1, 1, 1), (2, 2, 2), (0, 0, 0), False), ((2, 2, 2), (2, 2, 2), (0, 0, 0), False),
        ((2, 2, 2), (2, 2, 2), (1, 0, 1), False), ((2, 2, 2), (3, 3, 3), (0, 0, 0), False), ((3, 3, 3), (3, 3, 3), (0, 0, 0), False),
        ((3, 3, 3), (1, 1, 1), (2, 2, 2), False)}
    occ = {c.name: c for c in by_axis["occupancy"]}
    assert set(occ) >= {"corners", "one", "full", "line", "dups", "invalid", "allpad", "W1", "H1", "D1"}
    co = L.index_coords(occ["corners"])
    d, h, w = occ["corners"].shape
    have = {tuple(r) for r in co}
    assert all((b, z, y, x) in have for b in range(2) for z in (0, d - 1) for y in (0, h - 1) for x in (0, w - 1))
    assert (0, d // 2, 0, 0) in have and (1, d - 1, h // 2, w - 1) in have and (0, 0, h - 1, w // 2) in have
    assert len(L.index_coords(occ["one"])) == 1
    full = L.index_coords(occ["full"])
    assert len(np.unique(full, axis=0)) == len(full) == 2 * d * h * w
    # on a full grid the cell count is what caps the output set (cap = min(n * per_in, batch * cells))
    assert len(L.chain_reference(occ["full"])[1][0]) == 2 * 3 * 3 * 4 < len(full) * 8
    line = {tuple(r) for r in L.index_coords(occ["line"])}
    assert all((0, 1, 2, x) in line for x in range(w)) and not any(r[:2] == (0, 1) and r[2] in (1, 3) for r in line)
    dups = L.index_coords(occ["dups"])
    _, counts = np.unique(dups, axis=0, return_counts=True)
    assert (counts == 4).sum() == 10 and set(counts) == {1, 4}
    bad = L.index_coords(occ["invalid"])
    assert (bad[:, 0] >= 2).any() and (bad[:, 1] < 0).any() and (bad[:, 3] == w).any() and (bad[:, 0] == -1).any()
    assert L.valid_rows(bad, 2, (d, h, w)).sum() == len(bad) - 40
    assert not L.valid_rows(L.index_coords(occ["allpad"]), 2, (d, h, w)).any()
    for name, axis in (("W1", 2), ("H1", 1), ("D1", 0)):
        assert occ[name].shape[axis] == 1 and occ[name].chain[0][0][axis] == 3 and occ[name].chain[0][2][axis] == 1
    assert [len(L.index_coords(c)) for c in by_axis["n_in"]] == [511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097]
    cells = []
    for c in by_axis["out_grid"]:
        oshape = L.chain_reference(c)[0][2]
        cells.append(int(np.prod(oshape)))
        keys = L.keys_of(L.chain_reference(c)[0][0], oshape)
        assert keys[0] == 0 and keys[-1] == cells[-1] - 1 and not c.chain[0][3]
    assert cells == [16383, 16384, 16385, 16391, 32767, 32768, 32769, 32775]
    assert {cc % 16 == 0 for cc in cells} == {True, False}
    for c in INDEX:      # every case goes through plan() with shuffled rows and padding rows between them
        mixed = L.plan_input(c)
        assert (mixed[:, 0] == -1).sum() >= len(L.index_coords(c)) // 3 + 1 and len(mixed) > len(L.index_coords(c))
    assert L.CAP_CASES == [(1, -1), (1, 0), (1, 1), (2, -1), (2, 0), (2, 1)]
    assert sum(1 for s in L.CAP_CHAIN if not s[3]) == 2
    assert L.TO_DENSE_CASES == [(1, False), (1, True), (5, False), (5, True), (128, False), (128, True)]


@pytest.mark.parametrize("case", [c for c in GEMM if not c.axis.startswith("refuse") and c.o("status") is None],
                         ids=lambda c: c.id)
def test_exact_class_is_representable(case):
    d = L.gemm_data(case, "exact")
    want = L.case_reference(case, d)
    L.assert_representable(case, d, want)
    assert float(want.abs().max()) > 0
    if case.rows > 3 and not set(case.epi) & {"bias", "bn", "res"}:
        assert not want[3].any()      # a row without neighbours: the epilogue of 0
    for k in ("feats", "weight", "bias", "shift", "res"):
        if d[k] is not None:
            assert bool((d[k] == d[k].round()).all()) and float(d[k].abs().max()) <= 4
    if d["scale"] is not None:
        assert set(d["scale"].tolist()) <= {-1.0, 1.0, 2.0}
    assert int(d["nbr"].min()) >= -1 and int(d["nbr"].max()) < L.N_IN and bool((d["nbr"][3::5] == -1).all())
    if case.out_f16:     # fp16 holds every integer up to 2048; the operands are fp16 values
        assert torch.equal(want.half().double(), want)


def test_case_ids_are_unique_and_stable():
    ids = [c.id for c in GEMM] + [c.id for c in INDEX]
    assert len(set(ids)) == len(ids)
    assert ids == [c.id for c in L.all_gemm_cases()] + [c.id for c in L.index_cases()]
    assert all(" " not in i and "0x" not in i and "object" not in i for i in ids)
    assert (len(GEMM), len(INDEX)) == (495, 57)
    assert zlib.crc32("\n".join(ids).encode()) == 961223278   # (an edited case list changes it: update it with the lists)
    # the data of a case does not depend on the run either
    c = GEMM[0]
    a = L.gemm_data(c, "exact")["feats"].clone()
    L._gemm_data_of.cache_clear()
    assert torch.equal(a, L.gemm_data(c, "exact")["feats"])
