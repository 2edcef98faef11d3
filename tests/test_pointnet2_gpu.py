"""pointnet2 batch ops and points_in_boxes on the device (csrc/pointnet2.hip) against the NumPy restatement
(tests/golden/pointnet2_numpy.py): FPS bit-equal on both tiers at KITTI's and Waymo's shapes, its tie, NaN and clamp
rules, ball query, gather / grouping forward and backward, points_in_boxes at box faces, the IA-SSD layer against the
reference's recorded output, refusals and host synchronisation."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_pointnet2_golden as mk  # noqa: E402
import pointnet2_numpy as pn  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
DEV = "cuda"


def _ops():
    from paddle3d_amd.ops import pointnet2_ops, roiaware_pool3d

    return pointnet2_ops, roiaware_pool3d


def _cloud(rng, b, n):
    lo, hi = np.array([0, -40, -3], F32), np.array([70.4, 40, 1], F32)
    return (lo + rng.random((b, n, 3), dtype=F32) * (hi - lo)).astype(F32)


def _fps(xyz, m, tier=0):
    P, _ = _ops()
    return P.farthest_point_sample(torch.from_numpy(xyz).to(DEV), m, tier=tier).cpu().numpy()


@pytest.mark.parametrize("tier", [1, 2])
def test_fps_kitti_shapes_both_tiers(tier):
    rng = np.random.default_rng(1)
    xyz = _cloud(rng, 2, 16384)
    idx = _fps(xyz, 4096, tier)
    assert np.array_equal(idx, pn.farthest_point_sample(xyz, 4096))
    sub = np.take_along_axis(xyz, idx[..., None].astype(np.int64), 1)
    assert np.array_equal(_fps(sub, 1024, tier), pn.farthest_point_sample(sub, 1024))


def test_fps_waymo_shape_general_tier():
    rng = np.random.default_rng(2)
    xyz = _cloud(rng, 1, 65536)
    assert np.array_equal(_fps(xyz, 16384), pn.farthest_point_sample(xyz, 16384))
    P, _ = _ops()
    with pytest.raises(RuntimeError):  # the register tier holds n <= 16384
        P.farthest_point_sample(torch.from_numpy(xyz).to(DEV), 4, tier=1)


def test_fps_workspace_part_of_general_tier():
    rng = np.random.default_rng(4)
    xyz = _cloud(rng, 2, 70001)  # minima beyond 65536 points live in the workspace
    assert np.array_equal(_fps(xyz, 300), pn.farthest_point_sample(xyz, 300))


@pytest.mark.parametrize("n", [1, 2, 3, 100, 1000, 1023, 1024, 1025])
@pytest.mark.parametrize("tier", [1, 2])
def test_fps_small_n(n, tier):
    rng = np.random.default_rng(n)
    xyz = rng.standard_normal((2, n, 3)).astype(F32)
    m = min(n, 64) + 3  # m > n repeats for the small ones
    assert np.array_equal(_fps(xyz, m, tier), pn.farthest_point_sample(xyz, m))


@pytest.mark.parametrize("n", [5, 1024, 1500, 2048, 5000, 16384, 20000])
def test_fps_ties(n):
    rng = np.random.default_rng(n + 7)
    grid = rng.integers(0, 3, (1, n, 3)).astype(F32)  # quantised grid: many equal distances
    dup = np.repeat(rng.standard_normal((1, (n + 3) // 4, 3)).astype(F32), 4, 1)[:, :n]  # duplicates
    for xyz, m in ((grid, 40), (dup, 40)):
        want = pn.farthest_point_sample(xyz, m)
        if n <= 4096:
            assert np.array_equal(want, pn.fps_reference_sim(xyz, m))
        for tier in ((1, 2) if n <= 16384 else (2,)):
            assert np.array_equal(_fps(xyz, m, tier), want), (n, tier)
    # cases where neither the smallest index nor the smallest k mod bs wins
    for a, b, w in ((3, 1025, 1025), (1, 512, 512)):
        if b < n and n >= 1024:
            xyz = np.zeros((1, n, 3), F32)
            xyz[0, a], xyz[0, b] = (1, 0, 0), (0, 1, 0)
            assert _fps(xyz, 2)[0, 1] == w


def test_fps_nan_clamp_and_m():
    xyz = np.zeros((1, 40, 3), F32)
    xyz[0, 5], xyz[0, 9], xyz[0, 17] = (1e6, 0, 0), (0, -1e6, 0), (np.nan, 1, 1)
    for m in (0, 1, 2, 10, 100):
        got = _fps(xyz, m)
        assert got.shape == (1, m)
        assert np.array_equal(got, pn.farthest_point_sample(xyz, m))
    P, _ = _ops()
    with pytest.raises(RuntimeError):
        P.farthest_point_sample(torch.zeros((1, 0, 3), device=DEV), 3)


def test_ball_query_bit_equal():
    P, _ = _ops()
    rng = np.random.default_rng(5)
    xyz = _cloud(rng, 2, 4096) / 20.0
    xyz[:, 4095] = (60, 60, 0)  # an isolated point: the query there has exactly one hit
    lone = np.tile(np.array([[[60, 60, 0]]], F32), (2, 3, 1))
    q = np.concatenate([xyz[:, :500], np.full((2, 12, 3), 99, F32), lone], 1)  # rows with no hit, one hit
    for r, s in ((0.2, 16), (0.8, 32), (0.4, 64), (1.6, 128)):
        got = P.ball_query_batch(torch.from_numpy(q).to(DEV), torch.from_numpy(xyz).to(DEV), r, s).cpu().numpy()
        want = pn.ball_query(q, xyz, r, s)
        assert np.array_equal(got, want), (r, s)
    # rows with 0, 1 and more than nsample hits (r 0.2: ~37 points per ball, nsample 16)
    want = pn.ball_query(q, xyz, 0.2, 16)
    assert (want[:, 500:512] == 0).all() and (want[:, 512:] == 4095).all()
    assert (want[:, :500, 1:] != want[:, :500, :1]).all(-1).any()


def test_gather_group_forward_bit_equal():
    P, _ = _ops()
    rng = np.random.default_rng(6)
    feats = rng.standard_normal((2, 67, 3000)).astype(F32)
    gidx = rng.integers(-2, 3002, (2, 777)).astype(np.int32)
    got = P.gather_operation(torch.from_numpy(feats).to(DEV), torch.from_numpy(gidx).to(DEV)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), pn.group(feats, gidx).view(np.uint32))
    idx = rng.integers(0, 3000, (2, 512, 32)).astype(np.int32)
    idx[0, 0, 5] = -1
    idx[1, 3, 0] = 3000
    got = P.grouping_operation_batch(torch.from_numpy(feats).to(DEV), torch.from_numpy(idx).to(DEV)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), pn.group(feats, idx).view(np.uint32))


def test_gather_group_backward():
    P, _ = _ops()
    rng = np.random.default_rng(7)
    n = 2000
    idx = np.repeat(rng.integers(-1, n + 1, (2, 300, 4)), 4, axis=2).astype(np.int32)  # first-hit repeats
    ti = torch.from_numpy(idx).to(DEV)
    go_int = rng.integers(-8, 9, (2, 16, 300, 16)).astype(F32)
    got = P.grouping_operation_batch_grad(torch.from_numpy(go_int).to(DEV), ti, n).cpu().numpy()
    assert np.array_equal(got, pn.group_grad(go_int, idx, n).astype(F32))  # every sum exact
    go = rng.standard_normal((2, 16, 300, 16)).astype(F32)
    got = P.grouping_operation_batch_grad(torch.from_numpy(go).to(DEV), ti, n).cpu().numpy().astype(np.float64)
    want = pn.group_grad(go, idx, n)
    assert np.all(np.abs(got - want) <= 1e-6 * np.maximum(np.abs(want), 1.0))
    gidx = idx[:, :, 0]
    g1 = rng.standard_normal((2, 16, 300)).astype(F32)
    got = P.gather_operation_grad(torch.from_numpy(g1).to(DEV), torch.from_numpy(gidx).to(DEV), n).cpu().numpy()
    want = pn.group_grad(g1, gidx, n)
    assert np.all(np.abs(got - want) <= 1e-6 * np.maximum(np.abs(want), 1.0))
    # autograd through the shims
    pts = torch.from_numpy(rng.standard_normal((2, 16, n)).astype(F32)).to(DEV).requires_grad_(True)
    y = P.grouping_operation_batch(pts, ti)
    z = P.gather_operation(pts, torch.from_numpy(gidx).to(DEV))
    (y * torch.from_numpy(go_int).to(DEV)).sum().backward(retain_graph=True)
    g_group = pts.grad.clone()
    pts.grad = None
    z.sum().backward()
    assert np.array_equal(g_group.cpu().numpy(), pn.group_grad(go_int, idx, n).astype(F32))
    assert np.array_equal(pts.grad.cpu().numpy(), pn.group_grad(np.ones((2, 16, 300)), gidx, n).astype(F32))


def test_points_in_boxes_bit_equal_and_faces():
    from oracle import pyoracle as O

    _, R = _ops()
    rng = np.random.default_rng(8)
    boxes = np.zeros((2, 64, 8), F32)
    boxes[..., 0:3] = rng.uniform(-20, 20, (2, 64, 3))
    boxes[..., 3:6] = rng.uniform(0.5, 6, (2, 64, 3))
    boxes[..., 6] = rng.uniform(-np.pi, np.pi, (2, 64))
    boxes[1, 60:] = 0  # padding rows
    pts = rng.uniform(-22, 22, (2, 16384, 3)).astype(F32)
    # points 1 ulp either side of box faces (rz = 0 boxes: local = x - cx exactly)
    boxes[0, 0, 6] = 0
    face = []
    cx, cy, cz, dx, dy, dz = (float(v) for v in boxes[0, 0, :6])
    for e in (np.float64(dx) / 2.0 + np.float64(F32(1e-5)),):
        x = F32(cx + e)
        for v in (np.nextafter(x, F32(-1e9)), x, np.nextafter(x, F32(1e9))):
            face.append((v, cy, cz))
    zt = F32(cz + dz / 2.0)
    for v in (np.nextafter(zt, F32(-1e9)), zt, np.nextafter(zt, F32(1e9))):
        face.append((cx, cy, v))
    pts[0, :len(face)] = np.array(face, F32)
    tb = torch.from_numpy(boxes).to(DEV)
    got = R.points_in_boxes_gpu(torch.from_numpy(pts).to(DEV), tb[:, :, 0:7]).cpu().numpy()
    want = pn.points_in_boxes(pts, boxes, O.libm_eval)
    assert np.array_equal(got, want)
    assert (want >= 0).any()
    # the [k:k+1, :, 0:7] slice read in place, and zero boxes
    for k in range(2):
        got = R.points_in_boxes_gpu(torch.from_numpy(pts[k:k + 1]).to(DEV), tb[k:k + 1, :, 0:7]).cpu().numpy()
        assert np.array_equal(got, want[k:k + 1])
    got = R.points_in_boxes_gpu(torch.from_numpy(pts).to(DEV), torch.zeros((2, 0, 7), device=DEV)).cpu().numpy()
    assert (got == -1).all()
    # more boxes than one LDS chunk
    big = np.tile(boxes[:, :, :7], (1, 5, 1))
    got = R.points_in_boxes_gpu(torch.from_numpy(pts).to(DEV), torch.from_numpy(big).to(DEV)).cpu().numpy()
    assert np.array_equal(got, pn.points_in_boxes(pts, big, O.libm_eval))


def test_iassd_layer_matches_golden():
    from paddle3d_amd import iassd

    g = mk.load()
    xyz = torch.from_numpy(g["xyz"]).to(DEV)
    feat = torch.from_numpy(g["features"]).to(DEV)
    idx, new_xyz = iassd.sample_points(xyz, 512, "D-FPS")
    assert np.array_equal(idx.cpu().numpy(), g["fps0_out"])
    assert np.array_equal(new_xyz.cpu().numpy(), g["sa1_new_xyz"])
    pooled = [iassd.QueryAndGroup(r, s)(xyz, new_xyz, feat).amax(-1) for r, s in ((0.2, 16), (0.8, 32))]
    assert np.array_equal(torch.cat(pooled, 1).cpu().numpy(), g["sa1_new_features"])
    nf = torch.from_numpy(g["sa1_new_features"]).to(DEV)
    cls = torch.from_numpy(g["sa2_cls_features"]).to(DEV)
    _, new_xyz2 = iassd.sample_points(new_xyz, 128, "ctr_aware", cls)
    assert np.array_equal(new_xyz2.cpu().numpy(), g["sa2_new_xyz"])
    out = iassd.QueryAndGroup(0.8, 16, use_xyz=True)(new_xyz, new_xyz2, nf)
    assert np.array_equal(out.cpu().numpy(), g["qag_out"])
    idx, same = iassd.sample_points(new_xyz2, 512, "D-FPS")  # N <= npoint: no downsample
    assert np.array_equal(idx.cpu().numpy(), np.arange(128)[None]) and torch.equal(same, new_xyz2)


def test_refusals():
    P, R = _ops()
    x = torch.zeros((1, 10, 3), device=DEV)
    with pytest.raises(RuntimeError):
        P.farthest_point_sample(x.double(), 4)
    with pytest.raises(RuntimeError):
        P.farthest_point_sample(torch.zeros((1, 10, 4), device=DEV), 4)
    with pytest.raises(RuntimeError):
        P.farthest_point_sample(x.cpu(), 4)
    with pytest.raises(RuntimeError):
        P.ball_query_batch(x, torch.zeros((2, 10, 3), device=DEV), 0.1, 4)
    with pytest.raises(RuntimeError):
        P.grouping_operation_batch(torch.zeros((1, 4, 10), device=DEV), torch.zeros((1, 2, 3), device=DEV))
    with pytest.raises(RuntimeError):
        P.gather_operation(torch.zeros((1, 4, 10), device=DEV), torch.zeros((1, 2, 3), dtype=torch.int32,
                                                                             device=DEV))
    with pytest.raises(RuntimeError):
        R.points_in_boxes_gpu(x, torch.zeros((1, 3, 8), device=DEV))
    with pytest.raises(RuntimeError):
        R.points_in_boxes_gpu(x, torch.zeros((1, 3, 7), device=DEV, dtype=torch.float64))
    # non-contiguous inputs are copied: same results
    t = torch.randn(1, 3, 50, device=DEV).transpose(1, 2)
    assert torch.equal(P.farthest_point_sample(t, 8), P.farthest_point_sample(t.contiguous(), 8))


def test_no_host_sync():
    from paddle3d_amd import iassd

    P, R = _ops()
    rng = np.random.default_rng(9)
    xyz = torch.from_numpy(_cloud(rng, 2, 4096)).to(DEV)
    feat = torch.randn(2, 8, 4096, device=DEV, requires_grad=True)
    boxes = torch.randn(2, 10, 7, device=DEV).abs()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        idx, new_xyz = iassd.sample_points(xyz, 1024, "D-FPS")
        out = iassd.QueryAndGroup(1.0, 16)(xyz, new_xyz, feat)
        out.sum().backward()
        g = P.gather_operation(feat, idx)
        R.points_in_boxes_gpu(xyz, boxes)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert g.shape == (2, 8, 1024) and feat.grad is not None
