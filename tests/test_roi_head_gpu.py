"""Voxel R-CNN's RoI head on the device (csrc/roi_head.hip): every entry point bit-equal to the NumPy restatement
(tests/golden/roi_head_numpy.py) at the golden shapes and at the KITTI configuration's (B = 2 and 4; 21 x 800 x 704,
11 x 400 x 352 and 5 x 200 x 176 grids with about 30k / 12k / 5k voxels per frame, 100 RoIs, 70 400 anchors); the fused
pool layer against the unfused one on the same weights within the bound of tests/test_roi_head_cpu.py;
VoxelRCNNHead.forward + post_processing against the CPU run of that file; no host synchronisation; refusals."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_roi_head_golden as mk  # noqa: E402
import roi_head_numpy as rn  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
DEV = "cuda"


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ops():
    from paddle3d_amd.ops import roi_head

    return roi_head


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def golden():
    return mk.load()


def _pool_case(xyz, q, co_bzyx, pinds, C1, S, rng_, radius, pool):
    rng = np.random.default_rng(rng_)
    f = rng.standard_normal((xyz.shape[0], C1)).astype(F32)
    w = rng.standard_normal((C1, 3)).astype(F32)
    sc, sh = rng.uniform(0.5, 1.5, C1).astype(F32), rng.normal(0, 0.3, C1).astype(F32)
    return (q, co_bzyx, xyz, pinds, f, w, sc, sh), radius, S, pool


def _check_pool(args, max_range, radius, S, pool):
    got = _ops().voxel_pool(*(_d(a) for a in args), max_range, radius, S, "avg_pool" if pool else "max_pool")
    want = rn.voxel_pool(*args, max_range, radius, S, pool)
    got = got.cpu().numpy()
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), (S, pool, np.abs(got - want).max())
    return want


@pytest.mark.parametrize("C1", (16, 32, 64))
def test_voxel_pool_golden_shapes(golden, C1):
    g = golden
    for tag, k, rng_range in (("a", 0, [2, 2, 2]), ("b", 1, [1, 2, 2])):
        xyz, q = g[f"{tag}_pool{k}_xyz"], g[f"{tag}_pool{k}_new_xyz"]
        co = np.ascontiguousarray(g[f"{tag}_pool{k}_new_coords"][:, [0, 3, 2, 1]])
        for S, pool in ((16, 0), (16, 1), (5, 1), (64, 0), (1, 1)):
            args, radius, S, pool = _pool_case(xyz, q, co, g[f"{tag}_pool{k}_v2p"], C1, S, 5 + S, 0.5 * (k + 1), pool)
            want = _check_pool(args, rng_range, radius, S, pool)
            assert (want != 0).any()
    # a row without a hit: relu(shift) in every channel
    idx = rn.pn.voxel_query(q, xyz, co, g[f"{tag}_pool{k}_v2p"], radius, S, *rng_range)
    assert (idx[:, 0] < 0).any()


@pytest.mark.parametrize("batch", (2, 4))
def test_voxel_pool_kitti_shapes(batch, oracle):
    scene, rois = rn.kitti_scene(batch)
    strides = [rn.KITTI_SCALES[n][0] for n in scene]
    xyz_q, coords = rn.roi_grid_points(oracle, rois, 6, rn.KITTI_RANGE[:3], rn.KITTI_VOXEL, strides)
    assert xyz_q.shape[0] == batch * 21600
    for k, (name, (ind, _)) in enumerate(scene.items()):
        stride, grid, n, _, radius = rn.KITTI_SCALES[name]
        assert 0.9 * n * batch < len(ind) <= n * batch
        xyz = rn.voxel_centers(ind, stride)
        pinds = rn.voxel2pinds(ind, batch, grid)
        co = np.ascontiguousarray(coords[k][:, [0, 3, 2, 1]])
        args, radius, S, pool = _pool_case(xyz, xyz_q, co, pinds, 32, 16, 40 + k, radius, 0)
        want = _check_pool(args, [4, 4, 4], radius, S, pool)
        idx = rn.pn.voxel_query(xyz_q, xyz, co, pinds, radius, 16, 4, 4, 4)
        hit = idx[:, 0] >= 0
        assert 0.2 < hit.mean() < 1.0 and (idx[hit, -1] != idx[hit, 0]).any(), (name, hit.mean())
        assert (want != 0).any()
        if batch == 2 and k == 0:
            _check_pool(args, [4, 4, 4], radius, 16, 1)


@pytest.mark.parametrize("batch", (2, 4))
def test_grid_points_and_decode(golden, oracle, batch):
    cases = [(golden[f"{t}_rois"], mk.model_cfg(t)["roi_grid_pool"]["grid_size"], mk.PCR[:3], mk.VOXEL, [1, 2])
             for t in ("a", "b")] if batch == 2 else []
    cases.append((rn.kitti_scene(batch)[1], 6, rn.KITTI_RANGE[:3], rn.KITTI_VOXEL, [2, 4, 8]))
    far = cases[-1][0].copy()
    far[0, 0, :3] = (1e12, -1e12, np.nan)  # coordinates that leave int32: saturate, a NaN is 0
    cases.append((far, 3, rn.KITTI_RANGE[:3], rn.KITTI_VOXEL, [1, 2, 4, 8]))
    rng = np.random.default_rng(5)
    for rois, G, lo, vs, strides in cases:
        xyz, coords = _ops().roi_grid_points(_d(rois), G, lo + [0, 0, 0], vs, strides)
        wx, wc = rn.roi_grid_points(oracle, rois, G, lo, vs, strides)
        if rois is far:  # a NaN's payload is not part of the contract: equal values, NaN where NaN
            np.testing.assert_array_equal(xyz.cpu().numpy(), wx)
            assert wc[0].max() == np.iinfo(np.int32).max and wc[0].min() == np.iinfo(np.int32).min
        else:
            assert np.array_equal(_bits(xyz.cpu().numpy()), _bits(wx))
        assert len(coords) == len(strides)
        for c, w in zip(coords, wc):
            assert np.array_equal(c.cpu().numpy(), w)
        if rois is far:
            continue
        enc = rng.normal(0, 0.3, rois.shape).astype(F32)
        got = _ops().rcnn_decode_boxes(_d(rois), _d(enc.reshape(-1, 7))).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(rn.rcnn_decode_boxes(oracle, rois, enc)))


def _check_nms(oracle, box, cls, sigmoid, thresh, labels, cfg):
    got = _ops().class_agnostic_nms(_d(box), _d(cls), cfg, score_thresh=thresh, apply_sigmoid=sigmoid,
                                    labels=None if labels is None else _d(labels))
    want = rn.class_agnostic_nms(oracle, box, cls, sigmoid, thresh, labels, cfg["nms_pre_maxsize"], cfg["nms_thresh"],
                                 cfg["nms_post_maxsize"])
    names = ("boxes", "scores", "labels", "count")
    for n, a, w in zip(names, got, want):
        a = a.cpu().numpy()
        assert a.dtype == w.dtype and a.shape == w.shape, n
        assert np.array_equal(a.view(np.uint32) if a.dtype == F32 else a, w.view(np.uint32) if w.dtype == F32 else w), n
    return want


@pytest.mark.parametrize("tag", ("a", "b"))
def test_nms_golden_shapes(golden, oracle, tag):
    g = golden
    nmsc = mk.model_cfg(tag)["nms_config"]["test"]
    w = _check_nms(oracle, g[f"{tag}_box_preds"], g[f"{tag}_cls_preds"], False, None, None, nmsc)
    assert np.array_equal(_bits(w[0]), _bits(g[f"{tag}_rois"]))  # and so equal to the reference's proposal layer
    post = mk.POST_CFG["nms_config"]
    K = mk.NUM_CLASS[tag]
    w = _check_nms(oracle, g[f"{tag}_syn_box"], g[f"{tag}_syn_cls"], True, mk.POST_CFG["score_thresh"],
                   g[f"{tag}_syn_labels"] if K > 1 else None, post)
    assert w[3][1] == 0 and w[1][1, 0] == -1 and w[2][1, 0] == -1  # the box_empty frame
    _check_nms(oracle, g[f"{tag}_syn_box"], g[f"{tag}_syn_cls"], False, -100.0, None, dict(post, nms_post_maxsize=64))


@pytest.mark.parametrize("batch,pre", ((2, 2048), (4, 4096)))
def test_nms_kitti_shapes(oracle, batch, pre):
    box, cls = rn.kitti_proposals(batch)
    w = _check_nms(oracle, box, cls, False, None, None,
                   {"nms_pre_maxsize": pre, "nms_post_maxsize": 100, "nms_thresh": 0.7})
    assert (w[3] == 100).all()
    w = _check_nms(oracle, box, cls, True, 0.3, None, {"nms_pre_maxsize": pre, "nms_post_maxsize": 500, "nms_thresh": 0.1})
    assert ((w[3] > 20) & (w[3] < 500)).all(), w[3]


@pytest.mark.parametrize("tag", ("a", "b"))
def test_fused_layer_against_unfused(golden, tag):
    """Same weights, same inputs: the fused forward within the stored bound of the unfused one (and of the reference)."""
    import test_roi_head_cpu as cpu

    g = golden
    for k in (0, 1):
        T = lambda name: _d(g[f"{tag}_pool{k}_{name}"])  # noqa: E731
        feats = _d(g[f"{tag}_x_conv{k + 1}_features"])
        M = g[f"{tag}_pool{k}_new_xyz"].shape[0]
        cnt = torch.full((2,), M // 2, dtype=torch.int32, device=DEV)
        bound = float(g[f"{tag}_pool{k}_bound"])
        outs = []
        for fused in (False, True):
            layer = cpu._pool_layer(g, tag, k, fused).to(DEV)
            with torch.no_grad():
                outs.append(layer(T("xyz"), T("xyz_cnt"), T("new_xyz"), cnt, T("new_coords"), feats,
                                  T("v2p")).cpu().numpy().astype(np.float64))
        e_pair = float(np.abs(outs[0] - outs[1]).max())
        e_ref = [float(np.abs(o - g[f"{tag}_pool{k}_out"]).max()) for o in outs]
        print(f"{tag} pool{k}: fused - unfused {e_pair:.3e}, against the reference {e_ref[0]:.3e} / {e_ref[1]:.3e}, "
              f"bound {bound:.3e}")
        assert e_pair <= bound and max(e_ref) <= bound


def test_fused_layer_kitti_shape(oracle):
    """x_conv2 at B = 2: the bound is formed by the issue's rule from the unfused layer's own error against an fp64
    evaluation of the same sums (4 x, one fp32 ulp of the largest output as the floor)."""
    import copy

    from paddle3d_amd import pointnet2_stack as L

    scene, rois = rn.kitti_scene(2)
    ind, feats = scene["x_conv2"]
    xyz = rn.voxel_centers(ind, 2)
    q, coords = rn.roi_grid_points(oracle, rois, 6, rn.KITTI_RANGE[:3], rn.KITTI_VOXEL, [2])
    pinds = rn.voxel2pinds(ind, 2, rn.KITTI_SCALES["x_conv2"][1])
    torch.manual_seed(3)
    layer = L.NeighborVoxelSAModuleMSG(query_ranges=[[4, 4, 4]], radii=[0.4], nsamples=[16], mlps=[[32, 32, 32]],
                                       pool_method="max_pool", fused=False).eval()
    for m in layer.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.1)
    ref64 = copy.deepcopy(layer).double()
    layer = layer.to(DEV)
    cnt = _d(np.bincount(ind[:, 0], minlength=2).astype(np.int32))
    qcnt = torch.full((2,), 21600, dtype=torch.int32, device=DEV)
    outs = []
    with torch.no_grad():
        for fused in (False, True):
            layer.fused = fused
            outs.append(layer(_d(xyz), cnt, _d(q), qcnt, _d(coords[0]), _d(feats), _d(pinds)).cpu().numpy())
        # fp64: mlps_in in double, the pool from rn.voxel_pool_f64 on fp64-rounded-to-fp32 inputs is not the same sum;
        # so the whole layer is evaluated in double on the CPU from the fp32 inputs and weights
        fin = ref64.mlps_in[0](torch.from_numpy(feats).double().t().unsqueeze(0)).squeeze(0).t()
        conv, bn = ref64.mlps_pos[0][0], ref64.mlps_pos[0][1]
        idx = rn.pn.voxel_query(q, xyz, coords[0][:, [0, 3, 2, 1]], pinds, 0.4, 16, 4, 4, 4)
        empty = idx[:, 0] < 0
        rows = torch.from_numpy(np.where(empty[:, None], 0, idx)).long()
        d = torch.from_numpy(xyz).double()[rows] - torch.from_numpy(q).double()[:, None]
        f = fin[rows]
        d[torch.from_numpy(empty)] = 0
        f[torch.from_numpy(empty)] = 0
        pos = bn(conv(d.permute(2, 0, 1).unsqueeze(0))).squeeze(0).permute(1, 2, 0)  # [M, S, C1]
        pooled = torch.relu(f + pos).max(1).values
        want = ref64.mlps_out[0](pooled.t().unsqueeze(0)).squeeze(0).t().numpy()
    err = [float(np.abs(o - want).max()) for o in outs]
    bound = max(4 * err[0], float(np.spacing(F32(np.abs(want).max()))))
    pair = float(np.abs(outs[0].astype(np.float64) - outs[1]).max())
    print(f"x_conv2 B=2: unfused error {err[0]:.3e}, fused error {err[1]:.3e}, fused - unfused {pair:.3e}, bound {bound:.3e}")
    assert err[1] <= bound and pair <= bound


def _gpu_head(g, tag, fused):
    from paddle3d_amd import roi_heads as rh
    from paddle3d_amd.checkpoint import load_paddle_state_dict
    from paddle3d_amd.sparse import SparseConvTensor

    head = rh.VoxelRCNNHead(input_channels=dict(mk.INPUT_CHANNELS), model_cfg=mk.model_cfg(tag),
                            point_cloud_range=mk.PCR, voxel_size=mk.VOXEL, num_class=1, fused_pool=fused).eval()
    assert load_paddle_state_dict(head, mk.state(g, tag)) == []
    head = head.to(DEV)

    def batch():
        feats = {}
        for n in mk.GRIDS:
            ind, f = g[f"{tag}_{n}_indices"], g[f"{tag}_{n}_features"]
            pad = 7  # rows at a remembered capacity: behind n_dev they hold nothing
            ind_p = np.concatenate([ind, np.full((pad, 4), 1, np.int32)])
            f_p = np.concatenate([f, np.full((pad, f.shape[1]), 9.0, F32)])
            feats[n] = SparseConvTensor(_d(f_p), _d(ind_p), mk.GRIDS[n], 2,
                                        n_dev=torch.tensor([len(ind)], dtype=torch.int32, device=DEV))
        return {"batch_size": 2, "batch_box_preds": _d(g[f"{tag}_box_preds"]),
                "batch_cls_preds": _d(g[f"{tag}_cls_preds"]), "multi_scale_3d_features": feats,
                "multi_scale_3d_strides": dict(mk.STRIDES)}

    return rh, head, batch


@pytest.mark.parametrize("tag", ("a", "b"))
@pytest.mark.parametrize("fused", (False, True))
def test_head_against_cpu_run(golden, oracle, monkeypatch, tag, fused):
    import test_roi_head_cpu as cpu

    g = golden
    rh, head, batch = _gpu_head(g, tag, fused)
    seen = {}
    head.reg_pred_layer.register_forward_hook(lambda m, i, o: seen.__setitem__("reg", o.detach().cpu().numpy()))
    with torch.no_grad():
        bd = head(batch())
        post = [t.cpu().numpy() for t in rh.post_processing(bd, mk.POST_CFG, mk.NUM_CLASS[tag], padded=True)]
        frames = rh.post_processing(bd, mk.POST_CFG, mk.NUM_CLASS[tag])
    cbd, creg, cpost, cframes = cpu.run_head_cpu(g, tag, oracle, monkeypatch.setattr, fused)
    for key in ("rois", "roi_scores"):
        assert np.array_equal(_bits(bd[key].cpu().numpy()), _bits(cbd[key].numpy())), key
    assert np.array_equal(bd["roi_labels"].cpu().numpy(), cbd["roi_labels"].numpy())
    for name, got, want in (("rcnn_cls", bd["batch_cls_preds"].cpu().numpy(), cbd["batch_cls_preds"].numpy()),
                            ("rcnn_reg", seen["reg"], creg)):
        err, bound = float(np.abs(got.astype(np.float64) - want).max()), float(g[f"{tag}_{name}_bound"])
        print(f"{tag} {name} fused={fused}: device - CPU {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (name, err, bound)
    np.testing.assert_allclose(bd["batch_box_preds"].cpu().numpy(), cbd["batch_box_preds"].numpy(), rtol=2e-6, atol=4e-6)
    assert np.array_equal(post[3], cpost[3].numpy()) and np.array_equal(post[2], cpost[2].numpy())
    np.testing.assert_allclose(post[1], cpost[1].numpy(), rtol=0, atol=1e-6)
    for d, c in zip(frames, cframes):
        assert np.array_equal(d["label_preds"].cpu().numpy(), c["label_preds"].numpy())
        np.testing.assert_allclose(d["box3d_lidar"].cpu().numpy(), c["box3d_lidar"].numpy(), rtol=2e-6, atol=4e-6)


@pytest.mark.parametrize("fused", (False, True))
def test_forward_has_no_host_sync(golden, fused):
    rh, head, batch = _gpu_head(golden, "a", fused)
    bd = batch()
    with torch.no_grad():
        head(batch())  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            bd = head(bd)
            padded = rh.post_processing(bd, mk.POST_CFG, 1, padded=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert bd["batch_box_preds"].shape == (2, 10, 7) and padded[0].shape == (2, 6, 7)


def test_refusals_and_empty():
    from paddle3d_amd._lib import Paddle3DAmdError

    R = _ops()
    q, co = torch.zeros((4, 3), device=DEV), torch.zeros((4, 4), dtype=torch.int32, device=DEV)
    xyz, pi = torch.zeros((5, 3), device=DEV), torch.full((1, 2, 2, 2), -1, dtype=torch.int32, device=DEV)

    def pool(C1, S, **kw):
        a = dict(new_xyz=q, new_coords=co, xyz=xyz, point_indices=pi, features_in=torch.zeros((5, C1), device=DEV),
                 w_pos=torch.zeros((C1, 3), device=DEV), pos_scale=torch.ones(C1, device=DEV),
                 pos_shift=torch.full((C1,), 0.25, device=DEV), max_range=[1, 1, 1], radius=1.0, nsample=S)
        a.update(kw)
        return R.voxel_pool(**a)

    assert not R.voxel_pool_supported(24, 16) and not R.voxel_pool_supported(32, 65) and R.voxel_pool_supported(64, 64)
    for C1, S in ((24, 16), (8, 16), (32, 65)):
        with pytest.raises(Paddle3DAmdError, match="unsupported"):
            pool(C1, S)
    out = pool(32, 16)  # no voxel anywhere: relu(shift)
    assert out.shape == (4, 32) and bool((out == 0.25).all())
    assert pool(32, 16, new_xyz=q[:0], new_coords=co[:0]).shape == (0, 32)
    with pytest.raises(RuntimeError):
        pool(32, 16, new_coords=co.long())
    with pytest.raises(RuntimeError):
        pool(32, 16, new_xyz=q.cpu())
    with pytest.raises(NotImplementedError):
        pool(32, 16, pool_method="sum_pool")
    box, cls = torch.zeros((1, 8, 7), device=DEV), torch.zeros((1, 8, 1), device=DEV)
    with pytest.raises(RuntimeError):
        R.class_agnostic_nms(box, cls, {"nms_pre_maxsize": 0, "nms_post_maxsize": 4, "nms_thresh": 0.5})
    with pytest.raises(Paddle3DAmdError, match="unsupported"):
        R.class_agnostic_nms(box, cls, {"nms_pre_maxsize": 70000, "nms_post_maxsize": 4, "nms_thresh": 0.5})
    with pytest.raises(RuntimeError):
        R.roi_grid_points(box, 6, [0, 0, 0], [1, 1, 1], [1, 2, 4, 8, 16])
    with pytest.raises(RuntimeError):
        R.rcnn_decode_boxes(box, cls)
    b, s, l, c = R.class_agnostic_nms(box[:, :0], cls[:, :0], {"nms_pre_maxsize": 4, "nms_post_maxsize": 3,
                                                                 "nms_thresh": 0.5}, score_thresh=0.1)
    assert c.tolist() == [0] and s[0].tolist() == [-1.0, 0.0, 0.0] and l[0].tolist() == [-1, 0, 0]
