"""pointnet2 stack ops on the device (csrc/pointnet2_stack.hip) against the NumPy restatement
(tests/golden/pointnet2_stack_numpy.py): ball_query_stack at PV-RCNN's shapes, voxel_query at Voxel R-CNN's x_conv2
shapes, grouping forward and backward, the edge rules (frame scan, boundary, NaN, fill), the layers of
paddle3d_amd/pointnet2_stack.py against the reference's recorded outputs, refusals and host synchronisation."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_pointnet2_stack_golden as mk  # noqa: E402
import pointnet2_stack_numpy as pn  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
DEV = "cuda"
MLP_TOL = dict(rtol=1e-4, atol=1e-4)  # 1x1 convolutions and BN on the device against torch on the CPU


def _ops():
    from paddle3d_amd.ops import pointnet2_ops

    return pointnet2_ops


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cloud(rng, n):
    lo, hi = np.array([0, -40, -3], F32), np.array([70.4, 40, 1], F32)
    return (lo + rng.random((n, 3), dtype=F32) * (hi - lo)).astype(F32)


def _pv_inputs():
    """Two frames of 16384 / 15000 raw points, 2048 keypoints each (points of the frame, jittered)."""
    rng = np.random.default_rng(3)
    pts = [_cloud(rng, 16384), _cloud(rng, 15000)]
    keys = [p[rng.choice(len(p), 2048, replace=False)] + rng.normal(0, 0.3, (2048, 3)).astype(F32) for p in pts]
    return (np.concatenate(keys).astype(F32), np.array([2048, 2048], np.int32), np.concatenate(pts),
            np.array([16384, 15000], np.int32))


@pytest.mark.parametrize("radius,nsample", [(0.4, 16), (0.8, 32), (2.4, 16), (4.8, 32)])
def test_ball_query_stack_pvrcnn_shapes(radius, nsample):
    q, qc, p, pc = _pv_inputs()
    got = _ops().ball_query_stack(_d(q), _d(qc), _d(p), _d(pc), radius, nsample).cpu().numpy()
    want = pn.ball_query_stack(q, qc, p, pc, radius, nsample)
    assert np.array_equal(got, want)
    assert (want[:, 0] == -1).any() or radius > 1  # small radii leave balls empty
    assert (want[:, -1] != want[:, 0]).any()  # some rows are full


def test_ball_query_stack_roi_grid():
    """RoI-grid pooling: 6 x 6 x 6 grid points of 40 RoIs per frame, radii 0.8 / 1.6."""
    rng = np.random.default_rng(5)
    _, _, p, pc = _pv_inputs()
    g = (np.stack(np.meshgrid(*[np.linspace(-1.5, 1.5, 6)] * 3, indexing="ij"), -1).reshape(-1, 3)).astype(F32)
    centres = [p[rng.integers(0, 16384, 40)], p[16384 + rng.integers(0, 15000, 40)]]
    q = np.concatenate([(c[:, None] + g[None]).reshape(-1, 3) for c in centres]).astype(F32)
    qc = np.array([40 * 216, 40 * 216], np.int32)
    for radius in (0.8, 1.6):
        got = _ops().ball_query_stack(_d(q), _d(qc), _d(p), _d(pc), radius, 16).cpu().numpy()
        assert np.array_equal(got, pn.ball_query_stack(q, qc, p, pc, radius, 16))


def _voxel_scene(seed=7):
    """Voxel R-CNN x_conv2: a 21 x 800 x 704 grid (0.1 x 0.1 x 0.2 m) per frame, ~30k occupied voxels per frame in
    clusters, 100 RoIs x 216 grid points per frame around the clusters."""
    rng = np.random.default_rng(seed)
    Z, Y, X = 21, 800, 704
    ind, rois = [], []
    for b in range(2):
        c = np.stack([rng.integers(2, Z - 2, 160), rng.integers(20, Y - 20, 160), rng.integers(20, X - 20, 160)], 1)
        cells = (c[rng.integers(0, 160, 36000)] + np.round(rng.normal(0, [2, 8, 8], (36000, 3)))).astype(np.int64)
        cells = np.clip(cells, 0, [Z - 1, Y - 1, X - 1])
        flat = np.sort(rng.permutation(np.unique((cells[:, 0] * Y + cells[:, 1]) * X + cells[:, 2]))[:30000 - 1500 * b])
        z, y, x = np.unravel_index(flat, (Z, Y, X))
        ind.append(np.stack([np.full(len(flat), b), z, y, x], 1))
        rois.append(c[:100])
    ind = np.concatenate(ind).astype(np.int32)
    vs, lo = np.array([0.1, 0.1, 0.2], F32), np.array([0.0, -40.0, -3.0], F32)
    xyz = ((ind[:, [3, 2, 1]].astype(F32) + F32(0.5)) * vs + lo).astype(F32)
    g = (np.stack(np.meshgrid(*[np.linspace(-1.2, 1.2, 6)] * 3, indexing="ij"), -1).reshape(-1, 3)).astype(F32)
    new_xyz = []
    for r in rois:
        centre = (r[:, [2, 1, 0]].astype(F32) + F32(0.5)) * vs + lo
        new_xyz.append((centre[:, None] + g[None]).reshape(-1, 3))
    new_xyz = np.concatenate(new_xyz).astype(F32)
    b = np.repeat(np.arange(2), 100 * 216)[:, None]
    cxyz = np.floor((new_xyz - lo) / vs).astype(np.int64)  # (x, y, z) cells; some grid points leave the grid
    new_coords = np.concatenate([b, cxyz[:, [2, 1, 0]]], 1).astype(np.int32)  # (b, z, y, x)
    cnt = np.bincount(ind[:, 0], minlength=2).astype(np.int32)
    return ind, xyz, cnt, new_xyz, new_coords, (2, Z, Y, X)


def test_voxel_query_voxelrcnn_shapes():
    from paddle3d_amd import pointnet2_stack as L

    ind, xyz, cnt, new_xyz, new_coords, shape = _voxel_scene()
    pinds = L.generate_voxel2pinds(list(shape) + [32], _d(ind))
    want_p = np.full(shape, -1, np.int32)
    want_p[tuple(ind.T)] = np.arange(len(ind))
    assert np.array_equal(pinds.cpu().numpy(), want_p)
    for radius in (0.4, 1.6):
        got = _ops().voxel_query_wrapper(_d(new_xyz), _d(xyz), _d(new_coords), pinds, radius, 16, 4, 4, 4)
        want = pn.voxel_query(new_xyz, xyz, new_coords, want_p, radius, 16, 4, 4, 4)
        assert np.array_equal(got.cpu().numpy(), want)
        assert (want[:, 0] >= 0).mean() > 0.3 and (want[:, 0] == -1).any()


def test_grouping_forward_bit_equal():
    rng = np.random.default_rng(8)
    B_cnt = np.array([30000, 28500], np.int32)
    idx_cnt = np.array([21600, 21600], np.int32)
    idx = rng.integers(0, 28500, (43200, 16)).astype(np.int32)
    idx[::97, 0] = -1  # the empty-ball marker: reads the previous frame's last row, or 0 in frame 0
    idx[::89, 3] = 40000  # past the frame: a row of the next frame or outside [0, N)
    for C in (32, 3, 6):
        feat = rng.standard_normal((int(B_cnt.sum()), C)).astype(F32)
        got = _ops().grouping_operation_stack(_d(feat), _d(B_cnt), _d(idx), _d(idx_cnt)).cpu().numpy()
        want = pn.group_stack(feat, B_cnt, idx, idx_cnt)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), C


def test_grouping_backward():
    P = _ops()
    rng = np.random.default_rng(9)
    fc, ic = np.array([500, 300], np.int32), np.array([70, 50], np.int32)
    idx = rng.integers(-2, 320, (120, 16)).astype(np.int32)
    for C in (32, 5):
        feat = _d(rng.standard_normal((800, C)).astype(F32)).requires_grad_(True)
        out = P.grouping_operation_stack(feat, _d(fc), _d(idx), _d(ic))
        go = rng.standard_normal(tuple(out.shape)).astype(F32)
        out.backward(_d(go))
        want = pn.group_stack_grad(go, fc, idx, ic, 800)
        np.testing.assert_allclose(feat.grad.cpu().numpy(), want, rtol=1e-5, atol=1e-5)
    # no repeated row: every gradient is one value, exact
    perm = rng.permutation(300)[:256].reshape(16, 16).astype(np.int32)
    go = rng.standard_normal((16, 8, 16)).astype(F32)
    gf = P.grouping_operation_stack_grad(_d(go), _d(np.array([500, 300], np.int32)), _d(perm),
                                         _d(np.array([0, 16], np.int32)), 800).cpu().numpy()
    assert np.array_equal(gf, pn.group_stack_grad(go, [500, 300], perm, [0, 16], 800).astype(F32))


def test_edge_rules_on_device():
    P = _ops()
    rng = np.random.default_rng(10)
    p = rng.uniform(-1, 1, (60, 3)).astype(F32)
    q = rng.uniform(-1, 1, (40, 3)).astype(F32)
    p[5] = (0.5, 0.0, 0.0)
    q[0] = (0.0, 0.0, 0.0)  # d2 == 0.25 == r2 to point 5
    p[9] = (np.nan, 0.0, 0.0)
    # zero-count frames, rows past the total, a frame longer than the rest of xyz, a negative count
    for qc, pc in (([10, 0, 20], [30, 0, 30]), ([0, 15, 5], [20, 25, 15]), ([10, 10], [50, 30]),
                   ([12, 8, 10], [20, -5, 40])):
        qc, pc = np.array(qc, np.int32), np.array(pc, np.int32)
        for nsample in (1, 7, 70):
            got = P.ball_query_stack(_d(q), _d(qc), _d(p), _d(pc), 0.5, nsample).cpu().numpy()
            assert np.array_equal(got, pn.ball_query_stack(q, qc, p, pc, 0.5, nsample)), (qc, pc, nsample)
            assert np.array_equal(P.ball_query_stack(_d(q), _d(qc), _d(p), _d(pc), -0.5, nsample).cpu().numpy(),
                                  pn.ball_query_stack(q, qc, p, pc, 0.5, nsample))
    # voxel query: surface and NaN are hits, batch indices outside [0, B), out-of-range point indices
    grid = np.full((2, 3, 4, 5), -1, np.int32)
    grid[0, 1, 1, 1], grid[0, 1, 1, 2], grid[0, 1, 2, 1], grid[1, 0, 0, 0] = 5, 9, 77, 3
    co = np.array([[0, 1, 1, 1], [0, 1, 1, 2], [1, 0, 0, 0], [2, 1, 1, 1], [-1, 0, 0, 0], [0, 2, 3, 4]], np.int32)
    qq = np.zeros((6, 3), F32)
    for rng_ in ((1, 1, 1), (0, 0, 1), (2, 0, 3), (-1, 1, 1)):
        got = P.voxel_query_wrapper(_d(qq), _d(p), _d(co), _d(grid), 0.5, 4, *rng_).cpu().numpy()
        assert np.array_equal(got, pn.voxel_query(qq, p, co, grid, 0.5, 4, *rng_)), rng_
    got = P.voxel_query_wrapper(_d(qq), _d(p), _d(co), _d(grid), 0.5, 4, 1, 1, 1).cpu().numpy()
    assert got[0].tolist() == [5, 9, 5, 5] and got[3].tolist() == [-1, 0, 0, 0]


def _load(module, state):
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    load_paddle_state_dict(module, state)
    return module.to(DEV).eval()


def test_layers_match_golden():
    from paddle3d_amd import pointnet2_stack as L

    g = mk.load()
    T = lambda k: _d(g[k])  # noqa: E731
    new_features, idx = L.QueryAndGroup(0.5, 16)(T("pv_xyz"), T("pv_xyz_cnt"), T("pv_new_xyz"), T("pv_new_cnt"),
                                                 T("pv_features"))
    assert np.array_equal(new_features.cpu().numpy(), g["qag_out"])
    assert np.array_equal(idx.cpu().numpy(), g["qag_idx"])
    config = {"mlps": [[8, 16], [8, 8]], "pool_radius": [0.5, 1.0], "nsample": [16, 32]}
    sa, c_out = L.build_local_aggregation_module(4, copy.deepcopy(config))
    assert c_out == int(g["sa_c_out"].reshape(-1)[0])
    sa = _load(sa, mk.state(g, "sa"))
    prev = torch.backends.cudnn.allow_tf32
    torch.backends.cudnn.allow_tf32 = False
    try:
        with torch.no_grad():
            _, nf = sa(T("pv_xyz"), T("pv_xyz_cnt"), T("pv_new_xyz"), T("pv_new_cnt"), T("pv_features"))
            np.testing.assert_allclose(nf.cpu().numpy(), g["sa_new_features"], **MLP_TOL)
            pinds = L.generate_voxel2pinds([2, 4, 12, 12, 4], T("vx_indices"))
            assert np.array_equal(pinds.cpu().numpy(), g["voxel2pinds"])
            bzyx = T("vx_new_coords")[:, [0, 3, 2, 1]].contiguous()
            idx, empty = L.voxel_query([2, 2, 2], 0.5, 16, T("vx_xyz"), T("vx_new_xyz"), bzyx, pinds)
            assert np.array_equal(idx.cpu().numpy(), g["vq_idx"]) and np.array_equal(empty.cpu().numpy(),
                                                                                       g["vq_empty"])
            gf, gx, empty = L.VoxelQueryAndGrouping([1, 2, 3], 1.0, 8)(
                bzyx, T("vx_xyz"), T("vx_xyz_cnt"), T("vx_new_xyz"), T("vx_new_cnt"), T("vx_features"), pinds)
            assert np.array_equal(gf.cpu().numpy(), g["vqg_features"])
            assert np.array_equal(gx.cpu().numpy(), g["vqg_xyz"])
            assert np.array_equal(empty.cpu().numpy(), g["vqg_empty"])
            nv = _load(L.NeighborVoxelSAModuleMSG(query_ranges=[[2, 2, 2], [1, 2, 3]], radii=[0.5, 1.0],
                                                  nsamples=[16, 8], mlps=[[4, 8, 8], [4, 8, 16]]),
                       mk.state(g, "nv"))
            out = nv(T("vx_xyz"), T("vx_xyz_cnt"), T("vx_new_xyz"), T("vx_new_cnt"), T("vx_new_coords"),
                     T("vx_features"), pinds)
            np.testing.assert_allclose(out.cpu().numpy(), g["nv_out"], **MLP_TOL)
    finally:
        torch.backends.cudnn.allow_tf32 = prev


def test_refusals():
    P = _ops()
    q, c1, c2 = torch.zeros((4, 3), device=DEV), torch.tensor([2, 2], dtype=torch.int32, device=DEV), \
        torch.tensor([3, 3], dtype=torch.int32, device=DEV)
    p = torch.zeros((6, 3), device=DEV)
    co, grid = torch.zeros((4, 4), dtype=torch.int32, device=DEV), torch.zeros((2, 2, 2, 2), dtype=torch.int32,
                                                                                device=DEV)
    idx, feat = torch.zeros((4, 5), dtype=torch.int32, device=DEV), torch.zeros((6, 8), device=DEV)
    none = torch.zeros((0,), dtype=torch.int32, device=DEV)
    bad = [
        lambda: P.ball_query_stack(q.cpu(), c1, p, c2, 0.5, 4),
        lambda: P.ball_query_stack(q.double(), c1, p, c2, 0.5, 4),
        lambda: P.ball_query_stack(q, c1.long(), p, c2, 0.5, 4),
        lambda: P.ball_query_stack(torch.zeros((4, 4), device=DEV), c1, p, c2, 0.5, 4),
        lambda: P.ball_query_stack(q, c1, p, c2[:1], 0.5, 4),
        lambda: P.ball_query_stack(q, c1, p, c2, 0.5, 0),
        lambda: P.ball_query_stack(q, none, p, none, 0.5, 4),
        lambda: P.voxel_query_wrapper(q, p, co.cpu(), grid, 0.5, 4, 1, 1, 1),
        lambda: P.voxel_query_wrapper(q, p, co.float(), grid, 0.5, 4, 1, 1, 1),
        lambda: P.voxel_query_wrapper(q, p, co[:, :3], grid, 0.5, 4, 1, 1, 1),
        lambda: P.voxel_query_wrapper(q, p, co, grid[0], 0.5, 4, 1, 1, 1),
        lambda: P.voxel_query_wrapper(q, p, co[:3], grid, 0.5, 4, 1, 1, 1),
        lambda: P.voxel_query_wrapper(q, p, co, grid, 0.5, 0, 1, 1, 1),
        lambda: P.voxel_query_wrapper(q, p, co, grid[:0], 0.5, 4, 1, 1, 1),
        lambda: P.grouping_operation_stack(feat.cpu(), c2, idx, c1),
        lambda: P.grouping_operation_stack(feat.double(), c2, idx, c1),
        lambda: P.grouping_operation_stack(feat[0], c2, idx, c1),
        lambda: P.grouping_operation_stack(feat, c2, idx.float(), c1),
        lambda: P.grouping_operation_stack(feat, c2[:1], idx, c1),
        lambda: P.grouping_operation_stack(feat, c2, idx[:, :0], c1),
        lambda: P.grouping_operation_stack(feat, none, idx, none),
        lambda: P.grouping_operation_stack_grad(torch.zeros((4, 8, 5), device=DEV), c2, idx[:, :4], c1, 6),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError):
            f()
            pytest.fail(f"case {i} was not refused")
    # M == 0: empty results, nothing launched
    assert P.ball_query_stack(q[:0], none, p, none, 0.5, 4).shape == (0, 4)
    assert P.voxel_query_wrapper(q[:0], p, co[:0], grid, 0.5, 4, 1, 1, 1).shape == (0, 4)
    assert P.grouping_operation_stack(feat, c2, idx[:0], c1).shape == (0, 8, 5)


def test_no_host_sync():
    from paddle3d_amd import pointnet2_stack as L

    P = _ops()
    g = mk.load()
    T = lambda k: _d(g[k])  # noqa: E731
    sa, _ = L.build_local_aggregation_module(4, {"mlps": [[8, 16]], "pool_radius": [0.5], "nsample": [16]})
    sa = sa.to(DEV).eval()
    nv = L.NeighborVoxelSAModuleMSG(query_ranges=[[2, 2, 2]], radii=[0.5], nsamples=[16],
                                    mlps=[[4, 8, 8]]).to(DEV).eval()
    ins = {k: T(k) for k in ("pv_xyz", "pv_xyz_cnt", "pv_new_xyz", "pv_new_cnt", "vx_indices", "vx_xyz",
                             "vx_xyz_cnt", "vx_new_xyz", "vx_new_cnt", "vx_new_coords", "vx_features")}
    feat = T("pv_features").requires_grad_(True)
    n_dev = torch.tensor([170], dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, idx = L.QueryAndGroup(1.0, 16)(ins["pv_xyz"], ins["pv_xyz_cnt"], ins["pv_new_xyz"], ins["pv_new_cnt"],
                                            feat)
        out.sum().backward()
        _, nf = sa(ins["pv_xyz"], ins["pv_xyz_cnt"], ins["pv_new_xyz"], ins["pv_new_cnt"], feat)
        pinds = L.generate_voxel2pinds([2, 4, 12, 12, 4], ins["vx_indices"], n_dev=n_dev)
        nvo = nv(ins["vx_xyz"], ins["vx_xyz_cnt"], ins["vx_new_xyz"], ins["vx_new_cnt"], ins["vx_new_coords"],
                 ins["vx_features"], pinds)
        vq = P.voxel_query_wrapper(ins["vx_new_xyz"], ins["vx_xyz"], ins["vx_new_coords"], pinds, 1.0, 8, 1, 1, 1)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert feat.grad is not None and nf.shape == (64, 16) and nvo.shape == (32, 8) and vq.shape == (32, 8)
    assert np.array_equal(pinds.cpu().numpy(), g["voxel2pinds"])
