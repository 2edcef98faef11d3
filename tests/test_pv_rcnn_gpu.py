"""PV-RCNN's keypoint branch and RoI head on the device: the two entry points of csrc/pvrcnn.hip against their NumPy
restatement (tests/golden/pv_rcnn_numpy.py) and against what the reference's own Python computed
(tests/golden/python_pv_rcnn.npz), and the modules of paddle3d_amd/pv_rcnn.py / roi_heads.PVRCNNHead against their CPU
runs over the restatement.

bev_interpolate is compared bit for bit.  stack_sa_pool against the recorded reference: the bound the maker stored
(4 x the reference's own fp32 error against the fp64 evaluation); against the restatement's fp32 form (the ascending-j
fmaf chain) and against itself under a permutation or another placement of its rows: bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_pv_rcnn_golden as mk  # noqa: E402
import pv_rcnn_numpy as pv  # noqa: E402
import test_pv_rcnn_cpu as cpu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32


@pytest.fixture(scope="module")
def golden():
    return mk.load()


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _ops():
    from paddle3d_amd.ops import pvrcnn
    return pvrcnn


def _pool(args):
    return _ops().stack_sa_pool(*[_t(a) for a in args[:11]], args[11], args[12]).cpu().numpy()


def kitti_bev_case(seed=3):
    rng = np.random.default_rng(seed)
    bev = rng.standard_normal((2, 256, 200, 176)).astype(F32)
    kp = np.concatenate([np.repeat(np.arange(2), 2048)[:, None], rng.uniform(-1.0, 71.4, (4096, 1)),
                         rng.uniform(-41.0, 41.0, (4096, 1)), rng.uniform(-3, 1, (4096, 1))], 1).astype(F32)
    kp[0, 1:3], kp[1, 1:3] = (70.4, 40.0), (0.0, -40.0)  # on the map's borders
    return kp, bev, [0, -40, -3, 70.4, 40, 1], [0.05, 0.05, 0.1], 8


@pytest.mark.parametrize("case", ("a", "b", "kitti"))
def test_bev_interpolate_equals_restatement(golden, case):
    g = golden
    if case == "kitti":
        kp, bev, pcr, vs, stride = kitti_bev_case()
    else:
        kp, bev, pcr, vs, stride = g[f"{case}_keypoints"], g[f"{case}_bev"], mk.PCR, mk.VOXEL, mk.BEV[case][3]
        kp = np.concatenate([kp, kp[:6]])
        kp[-6, 0], kp[-5, 0], kp[-4, 0], kp[-3, 1], kp[-2, 2], kp[-1, 1] = -1, 2, 0.5, np.nan, 1e30, -1e30
    want = pv.bev_interpolate(kp, bev, pcr, vs, stride)
    got = _ops().bev_interpolate(_t(kp), _t(bev), pcr, vs, stride).cpu().numpy()
    same = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
    assert got.shape == want.shape and same.all(), (case, int((~same).sum()))
    if case != "kitti":
        assert np.array_equal(_bits(got[:-6]), _bits(g[f"{case}_point_bev"]))  # the reference's own result
        assert not got[-6:-3].any()  # no such frame: zero rows


def test_stack_sa_pool_against_reference_at_every_golden_scale(golden):
    g = golden
    seen = set()
    for tag, name, k in cpu.all_scales(g):
        args, cols = cpu.scale_args(g, tag, name, k)
        want, bound = g[f"{tag}_{name}_out"][:, cols], float(g[f"{tag}_{name}_bound"])
        got = _pool(args)
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"{tag} {name} scale {k} (c1 {args[5].shape[0]} c2 {args[8].shape[0]} nsample {args[12]}): "
              f"err {err:.3e} bound {bound:.3e}")
        assert got.shape == want.shape and err <= bound, (tag, name, k, err, bound)
        assert np.array_equal(_bits(got), _bits(pv.stack_sa_pool(*args))), (tag, name, k)  # the fmaf chain, bit for bit
        seen.add((args[5].shape[0], args[8].shape[0]))
    assert {c for c, _ in seen} == {16, 32, 64} == {c for _, c in seen}


@pytest.mark.parametrize("name", ("sa_rawpoints", "roi_pool"))
def test_stack_sa_pool_is_placement_independent(golden, name):
    """Two runs; the queries permuted within each frame; the frames swapped: every row keeps its bits."""
    g, tag = golden, "a"
    for k in range(len(g[f"{tag}_{name}_radii"])):
        args, _ = cpu.scale_args(g, tag, name, k)
        q, qc, p, pc, fin = args[:5]
        ref = _pool(args)
        assert np.array_equal(_bits(ref), _bits(_pool(args)))
        rng = np.random.default_rng(k)
        perm = np.concatenate([rng.permutation(int(qc[0])), int(qc[0]) + rng.permutation(int(qc[1]))])
        got = _pool((q[perm], qc, p, pc, fin) + args[5:])
        assert np.array_equal(_bits(got), _bits(ref[perm])), (name, k, "permuted")
        q0, p0 = int(qc[0]), int(pc[0])
        swap = lambda a, n: None if a is None else np.concatenate([a[n:], a[:n]])  # noqa: E731
        got = _pool((swap(q, q0), qc[::-1].copy(), swap(p, p0), pc[::-1].copy(), swap(fin, p0)) + args[5:])
        assert np.array_equal(_bits(got), _bits(swap(ref, q0))), (name, k, "frames swapped")
        # more rows than one launch's waves walk once: the grid-stride loop and the tail of a block
        reps = 4096 * 4 // q0 + 1
        big = _pool((np.concatenate([np.tile(q[:q0], (reps, 1)), q[q0:]]), np.array([q0 * reps, qc[1]], np.int32), p, pc,
                     fin) + args[5:])
        assert len(big) > 4096 * 4 and np.array_equal(_bits(big[:q0 * reps]), _bits(np.tile(ref[:q0], (reps, 1))))
        assert np.array_equal(_bits(big[q0 * reps:]), _bits(ref[q0:]))


def _layer(g, tag, name, fused):
    from paddle3d_amd.checkpoint import load_paddle_state_dict
    from paddle3d_amd.pointnet2_stack import build_local_aggregation_module

    if name == "roi_pool":
        module, prefix, cfg, cin = "roi_head", "roi_grid_pool_layer.", mk.roi_head_cfg(tag)["roi_grid_pool"], 24
    else:
        e = mk.encoder_cfg(tag)
        srcs = [n for n in e["features_source"] if n not in ("bev", "raw_points")]
        module = "point_encoder"
        prefix = "sa_rawpoints." if name == "sa_rawpoints" else f"sa_layers.{srcs.index(name[3:])}."
        cfg = e["sa_layer"]["raw_points" if name == "sa_rawpoints" else name[3:]]
        cin = mk.NUM_RAWPOINT_FEATURES - 3 if name == "sa_rawpoints" else mk.CHANNELS[name[3:]]
    layer, _ = build_local_aggregation_module(cin, cfg, fused=fused)
    st = mk.state(g, tag, module)
    load_paddle_state_dict(layer, {n[len(prefix):]: v for n, v in st.items() if n.startswith(prefix)})
    return layer.eval().to(DEV)


def test_fused_against_unfused_layer(golden):
    g = golden
    for tag in mk.TAGS:
        for name in mk.layer_names(tag):
            kw = {k: _t(g.get(f"{tag}_{name}_{k}")) for k in ("xyz", "xyz_batch_cnt", "new_xyz", "new_xyz_batch_cnt",
                                                                "features")}
            want, bound = g[f"{tag}_{name}_out"], float(g[f"{tag}_{name}_bound"])
            outs = {}
            for fused in (False, True):
                layer = _layer(g, tag, name, fused)
                with torch.no_grad():
                    assert all(layer._takes_fused(k) == fused for k in range(len(layer.mlps)))
                    outs[fused] = layer(**kw)[1].cpu().numpy()
                err = float(np.abs(outs[fused].astype(np.float64) - want).max())
                print(f"{tag} {name} fused={fused}: err to the reference {err:.3e} bound {bound:.3e}")
                assert outs[fused].shape == want.shape and err <= bound, (tag, name, fused, err, bound)
            assert float(np.abs(outs[True].astype(np.float64) - outs[False]).max()) <= bound


def kitti_pool_case(seed=5):
    """B = 2, 2048 keypoints per frame with 128 features -> 64 / 64, r = 0.8, 16 RoIs x 216 grid points per frame."""
    rng = np.random.default_rng(seed)
    kps, qs = [], []
    for b in range(2):
        centres = np.stack([rng.uniform(5, 65, 16), rng.uniform(-35, 35, 16), rng.uniform(-2, 0, 16)], 1)
        near = centres[rng.integers(0, 16, 1400)] + rng.normal(0, [1.5, 0.8, 0.5], (1400, 3))
        wide = np.stack([rng.uniform(0, 70.4, 648), rng.uniform(-40, 40, 648), rng.uniform(-3, 1, 648)], 1)
        kps.append(np.concatenate([near, wide]))
        lin = (np.arange(6) + 0.5) / 6 - 0.5
        grid = np.stack(np.meshgrid(lin * 3.9, lin * 1.6, lin * 1.56, indexing="ij"), -1).reshape(-1, 3)
        qs.append((centres[:, None, :] + grid[None]).reshape(-1, 3))
    xyz, q = np.concatenate(kps).astype(F32), np.concatenate(qs).astype(F32)
    feats = rng.standard_normal((4096, 128)).astype(F32)
    w1 = (rng.standard_normal((64, 131)) / np.sqrt(131)).astype(F32)
    w2 = (rng.standard_normal((64, 64)) / 8).astype(F32)
    s1, s2 = rng.uniform(0.5, 1.5, 64).astype(F32), rng.uniform(0.5, 1.5, 64).astype(F32)
    h1, h2 = rng.normal(0, 0.3, 64).astype(F32), rng.normal(0, 0.3, 64).astype(F32)
    fin = (feats @ w1[:, 3:].T).astype(F32)
    return (q, np.array([3456, 3456], np.int32), xyz, np.array([2048, 2048], np.int32), fin,
            np.ascontiguousarray(w1[:, :3]), s1, h1, w2, s2, h2, 0.8, 16)


def test_stack_sa_pool_at_the_kitti_shape():
    """Every row bit for bit against the restatement's fmaf chain, and against the fp64 evaluation under 4 x the
    restatement's own fp32 error over the same rows."""
    args = kitti_pool_case()
    got = _pool(args)
    want = pv.stack_sa_pool(*args, chunk=1024)
    want64 = pv.stack_sa_pool(*args, dtype=np.float64)
    rows, empty = pv.stack_sa_rows(*args[:4], args[11], args[12])
    assert got.shape == (6912, 64) and empty.any() and (~empty).sum() > 1000
    assert np.array_equal(_bits(got), _bits(want))
    bound = 4 * float(np.abs(want.astype(np.float64) - want64).max())
    err = float(np.abs(got.astype(np.float64) - want64).max())
    print(f"KITTI-shaped pool: err to fp64 {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def _gpu_model(g, tag, fused):
    from paddle3d_amd import pv_rcnn as pr
    from paddle3d_amd import roi_heads as rh
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    C = mk.BEV[tag][0]
    enc = pr.VoxelSetAbstraction(mk.encoder_cfg(tag), mk.VOXEL, mk.PCR, num_bev_features=C,
                                 num_rawpoint_features=mk.NUM_RAWPOINT_FEATURES, fused=fused)
    ph = pr.PointHeadSimple(mk.NUM_CLASS, enc.num_point_features_before_fusion, mk.POINT_HEAD_CFG)
    head = rh.PVRCNNHead(enc.num_point_features, mk.roi_head_cfg(tag), num_class=1, fused=fused)
    for name, m in (("point_encoder", enc), ("point_head", ph), ("roi_head", head)):
        load_paddle_state_dict(m, mk.state(g, tag, name))
    return rh, pr.PVRCNNSecondStage(enc, ph, head).eval().to(DEV)


def _batch(g, tag):
    from paddle3d_amd.sparse import SparseConvTensor

    feats = {n: SparseConvTensor(_t(g[f"{tag}_{n}_features"]), _t(g[f"{tag}_{n}_indices"]), mk.GRIDS[n], 2)
             for n in mk.GRIDS}
    return {"batch_size": 2, "points": _t(g[f"{tag}_points"]), "points_batch_cnt": g[f"{tag}_points_cnt"].tolist(),
            "spatial_features": _t(g[f"{tag}_bev"]), "spatial_features_stride": mk.BEV[tag][3],
            "multi_scale_3d_features": feats, "batch_box_preds": _t(g[f"{tag}_box_preds"]),
            "batch_cls_preds": _t(g[f"{tag}_cls_preds"])}


@pytest.mark.parametrize("tag", mk.TAGS)
@pytest.mark.parametrize("fused", (False, True))
def test_modules_against_cpu_run(golden, oracle, monkeypatch, tag, fused):
    g = golden
    rh, model = _gpu_model(g, tag, fused)
    seen = {}
    model.roi_head.reg_layers.register_forward_hook(
        lambda m, i, o: seen.__setitem__("reg", o.detach().transpose(1, 2).squeeze(1).cpu().numpy()))
    with torch.no_grad():
        bd = rh.pv_rcnn_second_stage(_batch(g, tag), model)
        post = [t.cpu().numpy() for t in rh.post_processing(bd, mk.POST_CFG, mk.NUM_CLASS, padded=True)]
        frames = rh.post_processing(bd, mk.POST_CFG, mk.NUM_CLASS)
    cbd, creg, cframes = cpu.run_cpu(g, tag, oracle, monkeypatch.setattr, fused)
    for key in ("point_coords", "rois", "roi_scores"):
        assert np.array_equal(_bits(bd[key].cpu().numpy()), _bits(cbd[key].numpy())), key
    assert np.array_equal(bd["roi_labels"].cpu().numpy(), cbd["roi_labels"].numpy())
    for name, got, want in (
            ("point_features_before_fusion", bd["point_features_before_fusion"], cbd["point_features_before_fusion"]),
            ("point_features", bd["point_features"], cbd["point_features"]),
            ("point_cls_scores", bd["point_cls_scores"], cbd["point_cls_scores"]),
            ("rcnn_cls", bd["batch_cls_preds"], cbd["batch_cls_preds"]), ("rcnn_reg", seen["reg"], creg)):
        got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
        want = want.numpy() if isinstance(want, torch.Tensor) else want
        err, bound = float(np.abs(got.astype(np.float64) - want).max()), float(g[f"{tag}_{name}_bound"])
        print(f"{tag} {name} fused={fused}: device - CPU {err:.3e}, bound {bound:.3e}")
        assert got.shape == want.shape and err <= bound, (name, err, bound)
    np.testing.assert_allclose(bd["batch_box_preds"].cpu().numpy(), cbd["batch_box_preds"].numpy(), rtol=2e-6, atol=4e-6)
    assert [len(f["scores"]) for f in frames] == [len(f["scores"]) for f in cframes]
    assert post[0].shape[1] == mk.POST_CFG["nms_config"]["nms_post_maxsize"]
    for d, c in zip(frames, cframes):
        assert np.array_equal(d["label_preds"].cpu().numpy(), c["label_preds"].numpy())
        np.testing.assert_allclose(d["scores"].cpu().numpy(), c["scores"].numpy(), rtol=0, atol=1e-6)
        np.testing.assert_allclose(d["box3d_lidar"].cpu().numpy(), c["box3d_lidar"].numpy(), rtol=2e-6, atol=4e-6)


@pytest.mark.parametrize("fused", (False, True))
def test_forwards_have_no_host_sync(golden, fused):
    g, tag = golden, "b"  # the case with the tiled frame
    rh, model = _gpu_model(g, tag, fused)
    with torch.no_grad():
        rh.pv_rcnn_second_stage(_batch(g, tag), model)  # warm-up: code objects, allocator
    bd = _batch(g, tag)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            bd = model.point_encoder(bd)
            bd = model.point_head(bd)
            bd = model.roi_head(bd)
            padded = rh.post_processing(bd, mk.POST_CFG, mk.NUM_CLASS, padded=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert bd["batch_box_preds"].shape == (2, 12, 7) and padded[0].shape == (2, 6, 7)
    assert bd["point_features"].shape == (2 * mk.NUM_KEYPOINTS, 24)


def kitti_stage_batch(seed=9):
    """The reference configuration's shapes at B = 2: 16 384 raw points per frame, a 256 x 200 x 176 BEV map, the four
    sparse scales' grids and channels (fewer voxels than a scan has: 8000 / 6000 / 3000 / 1500 per frame), 2000
    proposals per frame."""
    from paddle3d_amd.sparse import SparseConvTensor

    rng = np.random.default_rng(seed)
    lo, hi = np.array([0, -40, -3]), np.array([70.4, 40, 1])
    centres = rng.uniform(lo + [5, 5, 0.5], hi - [5, 5, 0.5], (2, 40, 3))
    pts = [np.concatenate([np.full((16384, 1), b), centres[b][rng.integers(0, 40, 16384)] + rng.normal(0, [3, 3, 0.4], (16384, 3)),
                           rng.random((16384, 1))], 1) for b in range(2)]
    feats = {}
    for name, grid, n, ch in (("x_conv1", (41, 1600, 1408), 8000, 16), ("x_conv2", (21, 800, 704), 6000, 32),
                              ("x_conv3", (11, 400, 352), 3000, 64), ("x_conv4", (5, 200, 176), 1500, 64)):
        size = (hi - lo)[::-1] / np.array(grid)
        ind = []
        for b in range(2):
            cell = np.floor((pts[b][rng.integers(0, 16384, 2 * n), 1:4][:, ::-1] - lo[::-1]) / size).astype(np.int64)
            cell = np.unique(np.clip(cell, 0, np.array(grid) - 1), axis=0)[:n]  # unique sorts: raster order
            ind.append(np.concatenate([np.full((len(cell), 1), b), cell], 1))
        ind = np.concatenate(ind).astype(np.int32)
        feats[name] = SparseConvTensor(_t(rng.standard_normal((len(ind), ch)).astype(F32)), _t(ind), grid, 2)
    box = np.concatenate([centres[:, rng.integers(0, 40, 2000)][np.arange(2)[:, None], np.arange(2000)[None]]
                          + rng.normal(0, 1.0, (2, 2000, 3)), np.array([3.9, 1.6, 1.56]) * rng.uniform(0.8, 1.2, (2, 2000, 3)),
                          rng.uniform(-np.pi, np.pi, (2, 2000, 1))], 2).astype(F32)
    return {"batch_size": 2, "points": _t(np.concatenate(pts).astype(F32)), "points_batch_cnt": [16384, 16384],
            "spatial_features": _t(rng.standard_normal((2, 256, 200, 176)).astype(F32)), "spatial_features_stride": 8,
            "multi_scale_3d_features": feats, "batch_box_preds": _t(box),
            "batch_cls_preds": _t(rng.normal(0, 2, (2, 2000, 3)).astype(F32))}


def test_second_stage_at_the_kitti_shapes_without_a_host_sync():
    """pv_rcnn_second_stage(batch_dict) on the configuration's own model (pv_rcnn_kitti(), random weights), and on the
    fused one: 2 x 2048 keypoints, 100 RoIs x 216 grid points per frame, no host sync; fused and unfused agree."""
    from paddle3d_amd import roi_heads as rh

    torch.manual_seed(0)
    fused = rh.pv_rcnn_kitti(fused=True).to(DEV).eval()
    fused.load_state_dict(rh.pv_rcnn_kitti_stage(DEV).state_dict())
    outs = []
    for model in (None, fused):
        rh.pv_rcnn_second_stage(kitti_stage_batch(), model)  # warm-up: code objects, allocator
        bd = kitti_stage_batch()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            bd = rh.pv_rcnn_second_stage(bd, model)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        torch.cuda.synchronize()
        assert bd["point_features"].shape == (4096, 128) and bd["point_features_before_fusion"].shape == (4096, 640)
        assert bd["batch_box_preds"].shape == (2, 100, 7) and bd["batch_cls_preds"].shape == (2, 100, 1)
        assert bool(bd["sparse_rows_frame_contiguous"]) and bool(torch.isfinite(bd["batch_box_preds"]).all())
        outs.append(bd)
    assert torch.equal(outs[0]["point_coords"], outs[1]["point_coords"]) and torch.equal(outs[0]["rois"], outs[1]["rois"])
    # the two forms sum the same 131 + 64 + 640 products per output in other orders: each within K * 2^-24 of the exact
    # value relative to the sum of magnitudes, which BatchNorm scales of at most 1.5 and ReLUs keep near the largest output
    scale = float(outs[0]["point_features"].abs().max())
    assert float((outs[0]["point_features"] - outs[1]["point_features"]).abs().max()) <= 2 * 835 * 2.0 ** -24 * max(scale, 1.0)


def test_unsorted_sparse_rows_with_sort_rows(golden):
    """A producer whose rows are not frame-contiguous: sort_rows=True gives, bit for bit, what the same rows give once
    they are ordered by a stable sort on the batch column on the host."""
    from paddle3d_amd.sparse import SparseConvTensor

    g, tag = golden, "a"
    rh, model = _gpu_model(g, tag, True)
    rng = np.random.default_rng(1)
    perms = {n: rng.permutation(len(g[f"{tag}_{n}_indices"])) for n in mk.GRIDS}

    def batch(sort):
        bd = _batch(g, tag)
        for n, perm in perms.items():
            ind, feats = g[f"{tag}_{n}_indices"][perm], g[f"{tag}_{n}_features"][perm]
            if sort:
                order = np.argsort(ind[:, 0], kind="stable")
                ind, feats = ind[order], feats[order]
            assert sort or (np.diff(ind[:, 0]) < 0).any()
            bd["multi_scale_3d_features"][n] = SparseConvTensor(_t(feats), _t(ind), mk.GRIDS[n], 2)
        return bd

    with torch.no_grad():
        bd = model.point_encoder(batch(True))
        want = bd["point_features_before_fusion"].cpu().numpy()
        assert bool(bd["sparse_rows_frame_contiguous"])
        assert not bool(model.point_encoder(batch(False))["sparse_rows_frame_contiguous"])  # the check sees it
        model.point_encoder.sort_rows = True
        bd = model.point_encoder(batch(False))
        got = bd["point_features_before_fusion"].cpu().numpy()
    assert bool(bd["sparse_rows_frame_contiguous"]) and np.array_equal(_bits(got), _bits(want))


def test_refusals_and_empty(golden):
    from paddle3d_amd._lib import Paddle3DAmdError

    P = _ops()
    args, _ = cpu.scale_args(golden, "a", "sa_rawpoints", 0)
    dev = [_t(a) for a in args[:11]]

    def pool(c1=16, c2=16, S=16, B=None, m=None, features=True):
        q = dev[0] if m is None else dev[0][:m]
        qc, pc = (dev[1], dev[3]) if B is None else (torch.zeros(B, dtype=torch.int32, device=DEV),) * 2
        w = torch.zeros((c1, 3), device=DEV)
        f = torch.zeros((dev[2].shape[0], c1), device=DEV) if features else None
        v = torch.zeros(c1, device=DEV), torch.zeros(c2, device=DEV)
        return P.stack_sa_pool(q, qc, dev[2], pc, f, w, v[0], v[0], torch.zeros((c2, c1), device=DEV), v[1], v[1],
                               0.5, S)

    for kw in (dict(c1=24), dict(c2=48), dict(c1=128), dict(S=65), dict(B=257)):
        with pytest.raises(Paddle3DAmdError, match="unsupported"):
            pool(**kw)
        assert not P.stack_sa_pool_supported(kw.get("c1", 16), kw.get("c2", 16), kw.get("S", 16)) or "B" in kw
    assert P.stack_sa_pool_supported(64, 16, 64) and not P.stack_sa_pool_supported(16, 16, 0)
    with pytest.raises(RuntimeError):
        pool(S=0)
    assert pool(m=0).shape == (0, 16)
    with pytest.raises(RuntimeError):
        P.stack_sa_pool(dev[0].cpu(), *dev[1:], 0.5, 16)
    # NULL features read as zeros
    got = P.stack_sa_pool(*dev[:4], None, *dev[5:], args[11], args[12]).cpu().numpy()
    zeros = np.zeros_like(args[4])
    assert np.array_equal(_bits(got), _bits(pv.stack_sa_pool(*args[:4], zeros, *args[5:])))
    assert np.array_equal(_bits(got), _bits(P.stack_sa_pool(*dev[:4], _t(zeros), *dev[5:], args[11], args[12]).cpu().numpy()))
    # bev_interpolate: nothing to do, wrong shapes
    kp, bev = _t(golden["a_keypoints"]), _t(golden["a_bev"])
    assert P.bev_interpolate(kp[:0], bev, mk.PCR, mk.VOXEL, 4).shape == (0, 12)
    assert P.bev_interpolate(kp, bev[:, :0], mk.PCR, mk.VOXEL, 4).shape == (80, 0)
    with pytest.raises(RuntimeError):
        P.bev_interpolate(kp[:, :3], bev, mk.PCR, mk.VOXEL, 4)
    with pytest.raises(RuntimeError):
        P.bev_interpolate(kp, bev[0], mk.PCR, mk.VOXEL, 4)


def test_a_frame_with_count_zero(golden):
    """Three frames, the middle one with no queries and no points; then one with queries and no points (every row
    relu(shift))."""
    g = golden
    args, _ = cpu.scale_args(g, "a", "sa_x_conv2", 0)
    q, qc, p, pc, fin = args[:5]
    ref = _pool(args)
    mid = lambda c: np.array([c[0], 0, c[1]], np.int32)  # noqa: E731
    got = _pool((q, mid(qc), p, mid(pc), fin) + args[5:])
    assert np.array_equal(_bits(got), _bits(ref))
    # frame 1 keeps its queries and loses its points
    n0 = int(pc[0])
    got = _pool((q, qc, p[:n0], np.array([n0, 0], np.int32), fin[:n0]) + args[5:])
    want = pv.stack_sa_pool(q, qc, p[:n0], np.array([n0, 0], np.int32), fin[:n0], *args[5:])
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(got[:int(qc[0])]), _bits(ref[:int(qc[0])]))
    assert (got[int(qc[0]):] == got[int(qc[0])]).all()
    # no points at all (n = 0, NULL xyz)
    got = _pool((q, qc, p[:0], np.zeros(2, np.int32), fin[:0]) + args[5:])
    assert (got == got[0]).all() and np.array_equal(_bits(got[:1]), _bits(want[-1:]))
