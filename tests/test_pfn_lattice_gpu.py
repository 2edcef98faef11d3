"""GPU side of the pillar encoders' lattice (tests/pfn_lattice.py): every case on every kernel form the restated dispatcher
says serves it, against the NumPy fp64 reference -- bit for bit on the exact class, within the derived per-element bound on
the real one -- and exactly the restated status where a form refuses.  Outputs are allocated pre-filled with a sentinel, so
an unwritten row shows; rows with num_points <= 0 must be all zero (the reference and its zero tolerance say so).

No case loops: a test is one launch per form.  The stride and index families' large cases share one data set and one
reference per kernel and value class (lru_cache in the lattice); the reference of the largest costs a few seconds once.

The sweep found nothing that the kernels compute wrongly.  The two holes of the indexed entry that reading had found are
closed beside it: test_indexed_grid_bound (on an 8 x 131 072 grid the raw indexed op gave every pillar with x >= 65 536 a
wrong centre) and the 2^24 refusals in tests/test_entry_status_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pfn_lattice as L  # noqa: E402

pytestmark = pytest.mark.gpu


def _run_paths(case):
    vox, npv, co = L.pillars(case)
    prm = L.params(case)
    t = L.upload(case, vox, npv, co, prm)
    served = [p for p in L.paths(case) if L.form(case, p).kernel]
    ref, tol = L.reference(case) if served else (None, None)
    for path in L.paths(case):
        f = L.form(case, path)
        rc, out = L.launch_path(case, t, path)
        if not f.kernel:
            assert rc == f.status, f"path {path}: status {rc}, the dispatcher's restatement says {f.status}"
            assert (out == L.SENTINEL).all(), f"path {path}: a refused call wrote its output"
            continue
        assert rc == 0, f"path {path} ({f}): status {rc}"
        assert not (out == L.SENTINEL).any(), f"path {path} ({f}): {int((out == L.SENTINEL).all(1).sum())} rows unwritten"
        bad = L.compare(case, out, ref, tol)
        assert bad is None, f"path {path} ({f}): {bad}"


@pytest.mark.parametrize("case", L.family("dispatch"), ids=lambda c: c.id)
def test_dispatch(case):
    _run_paths(case)


@pytest.mark.parametrize("case", L.family("rows"), ids=lambda c: c.id)
def test_rows(case):
    _run_paths(case)


@pytest.mark.parametrize("case", L.family("stride"), ids=lambda c: c.id)
def test_stride(case):
    assert L.form(case, case.c("path")).kernel == case.c("kernel")
    _run_paths(case)


@pytest.mark.parametrize("case", L.family("index"), ids=lambda c: c.id)
def test_index(case):
    """pd3_pillar_feature_net_indexed on a hand-made index against the reference on the rows the index stands for, and bit
    for bit against the padded packed form on the same rows."""
    points, span, plist = L.index_of(case)
    vox, npv, co = L.pillars(case)
    v2, n2 = L.rows_from_index(points, span, plist, case.P)
    assert np.array_equal(v2, vox) and np.array_equal(n2, npv)
    ref, tol = L.reference(case)
    f = L.form(case, 0, True, points.shape[1], plist.shape[1])
    assert f.kernel == "packed32"
    t = L.upload(case, v2, n2, co, L.params(case))
    rc, out = L.launch_indexed(case, t, points, span, plist)
    assert rc == 0
    assert not (out == L.SENTINEL).any(), f"{f}: {int((out == L.SENTINEL).all(1).sum())} rows unwritten"
    bad = L.compare(case, out, ref, tol)
    assert bad is None, f"{f}: {bad}"
    rc, packed = L.launch_path(case, t, 2)
    assert rc == 0
    assert np.array_equal(out.view(np.int32), packed.view(np.int32)), "indexed and padded packed forms differ"


def test_indexed_entry_refuses_what_form_refuses():
    """The refusals of the indexed entry that the restatement names, on a small case: no launch, nothing written."""
    case = [c for c in L.family("index") if c.vper == 8 and not c.seed][0]
    points, span, plist = L.index_of(case)
    vox, npv, co = L.pillars(case)
    t = L.upload(case, vox, npv, co, L.params(case))
    for n, ls in ((1 << 24, plist.shape[1]), (points.shape[1], 1 << 24), (points.shape[1], 0)):
        f = L.form(case, 0, True, n, ls)
        rc, out = L.launch_indexed(case, t, points, span, plist, points_per_frame=n, list_stride=ls)
        assert not f.kernel and rc == f.status and (out == L.SENTINEL).all()


# ---- pointpillars_scatter / inverse map / voxel_mean ------------------------------------------------------------------------
def _offset_view(shape, off, fill=None, src=None):
    """A contiguous tensor of `shape` that starts `off` floats past an allocation (which lies on 512 bytes)."""
    n = int(np.prod(shape))
    base = torch.full((n + 8,), L.SENTINEL if fill is None else fill, dtype=torch.float32, device="cuda")
    view = base[off:off + n].view(*shape)
    if src is not None:
        view.copy_(torch.from_numpy(src))
    assert view.data_ptr() % 16 == 4 * off % 16 and view.is_contiguous()
    return view


@pytest.mark.parametrize("case", L.SCATTER_CASES, ids=lambda c: c.id)
def test_scatter(case):
    from paddle3d_amd.ops import pointpillars_scatter as ps

    feats, co = L.scatter_data(case)
    canvas, inv = L.ref_scatter(feats, co, case.batch, case.ny, case.nx)
    f = _offset_view(feats.shape, case.feats_off, src=feats)
    c4 = torch.from_numpy(co).cuda()
    out = _offset_view(canvas.shape, case.out_off)
    res = ps.pointpillars_scatter(f, c4, case.batch, case.ny, case.nx, out=out)
    assert res.data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(out.cpu().numpy(), canvas)          # every cell written: no sentinel is left
    np.testing.assert_array_equal(ps.inverse_map(c4, case.batch, case.ny, case.nx).cpu().numpy(), inv)


@pytest.mark.parametrize("case", L.MEAN_CASES, ids=lambda c: c.id)
def test_voxel_mean(case):
    from paddle3d_amd.ops import voxel_encoder as ve

    vox, npv = L.mean_data(case)
    ref = L.ref_voxel_mean(vox, npv)
    out = ve.voxel_mean(torch.from_numpy(vox).cuda(), torch.from_numpy(npv).cuda()).cpu().numpy()
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(out[~fin], ref[~fin].astype(np.float32))     # num_points == 0: nan / +inf, as the division
    if case.values == "exact":
        np.testing.assert_array_equal(out, ref.astype(np.float32))
    else:   # P additions and a division, each within half an ulp of a running sum of positive terms
        assert (np.abs(out[fin].astype(np.float64) - ref[fin]) <= (case.P + 1) * 2.0 ** -24 * np.abs(ref[fin])).all()


# ---- the grid bound of the indexed form ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,served", [(65536, True), (131072, False)])
def test_indexed_grid_bound(nx, served):
    """A 2-D grid of 8 x nx unit cells with points across the whole x range.  Up to 65 536 cells along an axis the indexed
    form serves the grid and equals the pair of operators bit for bit (cell 65 535 is the largest its 16-bit words hold);
    above, PillarFeatureNet.forward_indexed answers None and the caller runs the pair."""
    from paddle3d_amd.centerpoint import HardVoxelizer, PillarFeatureNet

    vs, pr = (1.0, 1.0, 8.0), (0.0, 0.0, -3.0, float(nx), 8.0, 5.0)
    rng = np.random.default_rng(nx)
    cells = np.stack([rng.integers(0, nx, 700), rng.integers(0, 8, 700)], 1)
    cells[:4] = ((nx - 1, 7), (nx - 1, 0), (65535, 3), (0, 7))
    cells = np.repeat(cells, 4, 0)
    pts = np.concatenate([cells + rng.integers(1, 4, (len(cells), 2)) / 4.0, rng.uniform(-2, 4, (len(cells), 1)),
                          rng.uniform(0, 1, (len(cells), 1))], 1).astype(np.float32)
    assert (pts[:, 0] > 65536).sum() > 500 or served
    points = torch.from_numpy(pts[rng.permutation(len(pts))]).cuda()[None]
    torch.manual_seed(nx)
    vox = HardVoxelizer(vs, pr, 20, 4096).cuda().eval()
    net = PillarFeatureNet(4, (64, 64), max_num_points_in_voxel=20, voxel_size=vs, point_cloud_range=pr).cuda().eval()
    for layer in net.pfn_layers:
        layer.norm.running_mean.normal_(0, 0.2)
        layer.norm.running_var.uniform_(0.5, 1.5)
        layer.norm.weight.data.normal_(0, 1)
    idx = vox.index(points)
    assert idx is not None
    span, plist, coors, npv, nv = idx
    assert int(nv[0]) >= 600 and int(coors[0, :, 3].max()) == nx - 1
    coors = coors.view(-1, 4)
    with torch.no_grad():
        feats = net.forward_indexed(points, span, plist, coors)
        voxels, coors2, npv2, _ = vox(points)
        pair = net(voxels.view(-1, 20, 4), npv2.view(-1), coors2.view(-1, 4))
    assert torch.equal(coors, coors2.view(-1, 4))
    if served:
        assert feats is not None and torch.equal(feats.view(torch.int32), pair.view(torch.int32))
    else:
        assert feats is None
