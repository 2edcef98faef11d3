"""PV-RCNN's keypoint branch and RoI head on the CPU: the NumPy restatement of the two entry points
(tests/golden/pv_rcnn_numpy.py) against what the reference's own Python computed (tests/golden/python_pv_rcnn.npz),
and paddle3d_amd/pv_rcnn.py / roi_heads.PVRCNNHead run over the restatement (ops monkeypatched), fused and unfused,
against the recorded layer outputs, with the weights mapped from the recorded Paddle-named state dicts.

bev_interpolate has no matmul and is compared bit for bit.  Pooled layers and everything downstream: the bound the
maker stored, 4 x the largest error of the reference's own fp32 result against the fp64 evaluation of the same sums
(one fp32 ulp of the largest output as a floor).  Index outputs are compared exactly; decoded boxes under the
tolerances of tests/test_roi_head_cpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_pv_rcnn_golden as mk  # noqa: E402
import pv_rcnn_numpy as pv  # noqa: E402

F32 = np.float32
TAGS = mk.TAGS


@pytest.fixture(scope="module")
def golden():
    return mk.load()


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def scale_args(g, tag, name, k):
    """The arguments of stack_sa_pool for scale k of a recorded layer call (numpy), and the scale's output columns."""
    module, prefix = ("roi_head", "roi_grid_pool_layer") if name == "roi_pool" else ("point_encoder", None)
    if prefix is None:
        cfg = mk.encoder_cfg(tag)
        prefix = "sa_rawpoints" if name == "sa_rawpoints" else \
            f"sa_layers.{[n for n in cfg['features_source'] if n not in ('bev', 'raw_points')].index(name[3:])}"
    st = mk.state(g, tag, module)
    P = lambda s: st[f"{prefix}.mlps.{k}.{s}"]  # noqa: E731
    w1, w2 = P("0.weight")[:, :, 0, 0], P("3.weight")[:, :, 0, 0]

    def bn(i):
        scale = (P(f"{i}.weight") / np.sqrt(P(f"{i}._variance") + F32(1e-5))).astype(F32)
        return scale, (P(f"{i}.bias") - (P(f"{i}._mean") * scale).astype(F32)).astype(F32)

    feats = g.get(f"{tag}_{name}_features")
    fin = None if feats is None else (feats @ w1[:, 3:].T).astype(F32)
    widths = [mk.state(g, tag, module)[f"{prefix}.mlps.{j}.3.weight"].shape[0]
              for j in range(len(g[f"{tag}_{name}_radii"]))]
    lo = sum(widths[:k])
    args = (g[f"{tag}_{name}_new_xyz"], g[f"{tag}_{name}_new_xyz_batch_cnt"], g[f"{tag}_{name}_xyz"],
            g[f"{tag}_{name}_xyz_batch_cnt"], fin, np.ascontiguousarray(w1[:, :3]), *bn(1), np.ascontiguousarray(w2),
            *bn(4), float(g[f"{tag}_{name}_radii"][k]), int(g[f"{tag}_{name}_nsamples"][k]))
    return args, slice(lo, lo + widths[k])


def all_scales(g):
    return [(tag, name, k) for tag in TAGS for name in mk.layer_names(tag) for k in range(len(g[f"{tag}_{name}_radii"]))]


def test_golden_covers_every_width(golden):
    seen = set()
    for tag, name, k in all_scales(golden):
        a, _ = scale_args(golden, tag, name, k)
        seen.add((a[5].shape[0], a[8].shape[0], a[12]))
    assert {c for c, _, _ in seen} == {16, 32, 64} == {c for _, c, _ in seen} and {s for _, _, s in seen} == {16, 32}
    assert os.path.getsize(mk.OUT) <= 562338  # no larger than python_roi_head.npz


@pytest.mark.parametrize("tag", TAGS)
def test_bev_interpolate_restatement_is_exact(golden, tag):
    g = golden
    C, H, W, stride = mk.BEV[tag]
    got = pv.bev_interpolate(g[f"{tag}_keypoints"], g[f"{tag}_bev"], mk.PCR, mk.VOXEL, stride)
    assert np.array_equal(_bits(got), _bits(g[f"{tag}_point_bev"]))
    # bilinear_interpolate_paddle alone: frame 0's map at the recorded positions
    n = len(g[f"{tag}_bilinear_x"])
    assert np.array_equal(_bits(got[:n]), _bits(g[f"{tag}_bilinear_out"]))
    # both clip branches are in the data, and the departures: no frame -> zeros, NaN / huge coordinates
    xs = g[f"{tag}_keypoints"][:, 1] / F32(mk.VOXEL[0]) / F32(stride)
    assert (np.floor(xs) < 0).any() and (np.floor(xs) + 1 > W - 1).any()
    kp = g[f"{tag}_keypoints"][:6].copy()
    kp[0, 0], kp[1, 0], kp[2, 0], kp[3, 1], kp[4, 2], kp[5, 1] = -1, 2, 0.5, np.nan, 1e30, -1e30
    out = pv.bev_interpolate(kp, g[f"{tag}_bev"], mk.PCR, mk.VOXEL, stride)
    assert not out[:3].any() and out[3:].any()


def test_stack_sa_pool_restatement_within_stored_bounds(golden):
    g = golden
    for tag, name, k in all_scales(g):
        args, cols = scale_args(g, tag, name, k)
        want, bound = g[f"{tag}_{name}_out"][:, cols], float(g[f"{tag}_{name}_bound"])
        got = pv.stack_sa_pool(*args)
        got64 = pv.stack_sa_pool(*args, dtype=np.float64)
        err, err64 = float(np.abs(got.astype(np.float64) - want).max()), float(np.abs(got64 - want).max())
        print(f"{tag} {name} scale {k}: fp32 err {err:.3e}, fp64 err {err64:.3e}, bound {bound:.3e}")
        assert got.shape == want.shape and err <= bound and err64 <= bound, (tag, name, k, err, err64, bound)
        rows, empty = pv.stack_sa_rows(*args[:4], args[11], args[12])
        relu_sh = np.maximum(args[7], 0)  # a row without a hit: h = relu(shift1) in every slot
        if empty.any():
            h = relu_sh.astype(F32)
            acc = np.zeros(args[8].shape[0], F32)
            for j in range(len(h)):
                acc = pv.fmaf(h[j], args[8][:, j], acc)
            y = np.maximum((args[9] * acc).astype(F32) + args[10], 0).astype(F32)
            assert np.array_equal(_bits(got[empty]), _bits(np.broadcast_to(y, got[empty].shape)))


def test_fmaf_is_correctly_rounded():
    import ctypes

    m = ctypes.CDLL("libm.so.6")
    m.fmaf.restype, m.fmaf.argtypes = ctypes.c_float, [ctypes.c_float] * 3
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(4000).astype(F32), rng.standard_normal(4000).astype(F32)
    for c in (rng.standard_normal(4000).astype(F32), (-a.astype(np.float64) * b * (1 + 1e-6)).astype(F32)):
        want = np.array([m.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], F32)
        assert np.array_equal(_bits(pv.fmaf(a, b, c)), _bits(want))
    # a tie of the float64 sum that double rounding gets wrong: 1 + 2^-24 + 2^-60
    one, e = F32(1), F32(2.0 ** -24)
    assert pv.fmaf(F32(2.0 ** -30), F32(2.0 ** -30), (one + F32(0)).astype(F32)) == one
    assert pv.fmaf(np.array([1 + 2.0 ** -23], F32), np.array([2.0 ** -24], F32), np.array([1], F32))[0] == F32(1 + 2.0 ** -23)


def build_cpu(g, tag, oracle, setattr_, fused):
    """(roi_heads module, PVRCNNSecondStage on the CPU over the restatement, a batch_dict factory)."""
    from paddle3d_amd.checkpoint import load_paddle_state_dict
    from paddle3d_amd.sparse import SparseConvTensor

    rh, pr = pv.patch_cpu(setattr_, oracle)
    C, H, W, stride = mk.BEV[tag]
    enc = pr.VoxelSetAbstraction(mk.encoder_cfg(tag), mk.VOXEL, mk.PCR, num_bev_features=C,
                                 num_rawpoint_features=mk.NUM_RAWPOINT_FEATURES, fused=fused)
    ph = pr.PointHeadSimple(mk.NUM_CLASS, enc.num_point_features_before_fusion, mk.POINT_HEAD_CFG)
    head = rh.PVRCNNHead(enc.num_point_features, mk.roi_head_cfg(tag), num_class=1, fused=fused)
    model = pr.PVRCNNSecondStage(enc, ph, head).eval()
    for name, m in (("point_encoder", enc), ("point_head", ph), ("roi_head", head)):
        assert load_paddle_state_dict(m, mk.state(g, tag, name)) == []

    def batch(dev="cpu"):
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        feats = {n: SparseConvTensor(T(g[f"{tag}_{n}_features"]), T(g[f"{tag}_{n}_indices"]), mk.GRIDS[n], 2)
                 for n in mk.GRIDS}
        return {"batch_size": 2, "points": T(g[f"{tag}_points"]), "points_batch_cnt": g[f"{tag}_points_cnt"].tolist(),
                "spatial_features": T(g[f"{tag}_bev"]), "spatial_features_stride": stride,
                "multi_scale_3d_features": feats, "batch_box_preds": T(g[f"{tag}_box_preds"]),
                "batch_cls_preds": T(g[f"{tag}_cls_preds"])}

    return rh, model, batch


def run_cpu(g, tag, oracle, setattr_, fused):
    rh, model, batch = build_cpu(g, tag, oracle, setattr_, fused)
    seen = {}
    model.roi_head.reg_layers.register_forward_hook(
        lambda m, i, o: seen.__setitem__("reg", o.detach().transpose(1, 2).squeeze(1).numpy()))
    with torch.no_grad():
        assert all(l._takes_fused(k) == fused for l in [model.point_encoder.sa_rawpoints, model.roi_head.roi_grid_pool_layer,
                                                        *model.point_encoder.sa_layers] for k in range(len(l.mlps)))
        bd = rh.pv_rcnn_second_stage(batch(), model)
        frames = rh.post_processing(bd, mk.POST_CFG, mk.NUM_CLASS)
    return bd, seen["reg"], frames


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("fused", (False, True))
def test_modules_on_cpu_reproduce_reference(golden, oracle, monkeypatch, tag, fused):
    g = golden
    bd, reg, frames = run_cpu(g, tag, oracle, monkeypatch.setattr, fused)
    assert np.array_equal(_bits(bd["point_coords"].numpy()), _bits(g[f"{tag}_keypoints"]))  # FPS and the tiled frame
    for key in ("rois", "roi_scores"):
        assert np.array_equal(_bits(bd[key].numpy()), _bits(g[f"{tag}_{key}"])), key
    assert np.array_equal(bd["roi_labels"].numpy(), g[f"{tag}_roi_labels"])
    c_bev = mk.BEV[tag][0]
    assert np.array_equal(_bits(bd["point_features_before_fusion"].numpy()[:, :c_bev]), _bits(g[f"{tag}_point_bev"]))
    for name, got in (("point_features_before_fusion", bd["point_features_before_fusion"].numpy()),
                      ("point_features", bd["point_features"].numpy()),
                      ("point_cls_scores", bd["point_cls_scores"].numpy()),
                      ("rcnn_cls", bd["batch_cls_preds"].numpy().reshape(-1, 1)), ("rcnn_reg", reg)):
        want, bound = g[f"{tag}_{name}"], float(g[f"{tag}_{name}_bound"])
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"{tag} {name} fused={fused}: err {err:.3e} bound {bound:.3e}")
        assert got.shape == want.shape and err <= bound, (name, err, bound)
    np.testing.assert_allclose(bd["batch_box_preds"].numpy(), g[f"{tag}_batch_box_preds"], rtol=2e-6, atol=4e-6)
    assert bd["cls_preds_normalized"] is False
    for b, d in enumerate(frames):
        assert np.array_equal(d["label_preds"].numpy(), g[f"{tag}_post_labels{b}"]), b
        np.testing.assert_allclose(d["scores"].numpy(), g[f"{tag}_post_scores{b}"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(d["box3d_lidar"].numpy(), g[f"{tag}_post_boxes{b}"], rtol=2e-6, atol=4e-6)


def test_fused_flag_leaves_training_and_other_shapes_alone(golden, oracle, monkeypatch):
    from paddle3d_amd.pointnet2_stack import StackSAModuleMSG, build_local_aggregation_module

    pv.patch_cpu(monkeypatch.setattr, oracle)
    mlps = [[4, 16, 16], [4, 16, 16, 16], [4, 24, 16], [4, 16, 16]]
    layer = StackSAModuleMSG(radii=[1.0] * 4, nsamples=[16, 16, 16, 65], mlps=mlps, fused=True).eval()
    with torch.no_grad():
        assert [layer._takes_fused(k) for k in range(4)] == [True, False, False, False]
        assert not layer.train()._takes_fused(0)
    assert not layer.eval()._takes_fused(0)  # gradients on
    assert not StackSAModuleMSG(radii=[1.0], nsamples=[16], mlps=[[4, 16, 16]]).eval().fused  # the default
    avg = StackSAModuleMSG(radii=[1.0], nsamples=[16], mlps=[[4, 16, 16]], pool_method="avg_pool", fused=True).eval()
    with torch.no_grad():
        assert not avg._takes_fused(0)
    l2, c = build_local_aggregation_module(4, {"mlps": [[16, 16]], "pool_radius": [1.0], "nsample": [16]})
    assert c == 16 and l2.fused is False


def test_kitti_constructor_and_refusals():
    from paddle3d_amd import pv_rcnn as pr
    from paddle3d_amd import roi_heads as rh

    model = rh.pv_rcnn_kitti()
    enc, head = model.point_encoder, model.roi_head
    assert enc.num_point_features_before_fusion == 640 and enc.num_point_features == 128
    assert head.pre_channel == 6 ** 3 * 128 and head.shared_fc_layer[0].weight.shape == (256, 27648, 1)
    assert isinstance(head.shared_fc_layer[3], torch.nn.Identity) and isinstance(head.cls_layers[3], torch.nn.Identity)
    assert head.reg_layers[-1].out_channels == 7 and model.point_head.cls_layers[-1].out_features == 1
    layers = [enc.sa_rawpoints, *enc.sa_layers, head.roi_grid_pool_layer]
    assert len(layers) == 6 and all(l.fused == rh.FUSED_SA_DEFAULT for l in layers)
    assert all(l.fused for l in [rh.pv_rcnn_kitti(fused=True).roi_head.roi_grid_pool_layer])
    stage = rh.pv_rcnn_kitti_stage("cpu")  # what pv_rcnn_second_stage(batch_dict) runs: one per device, kept
    assert stage is rh.pv_rcnn_kitti_stage(torch.device("cpu")) and not stage.training
    assert set(stage.state_dict()) == set(model.state_dict())
    names = set(model.state_dict())
    assert {"point_encoder.sa_layers.3.mlps.1.3.weight", "point_encoder.sa_rawpoints.mlps.0.0.weight",
            "point_encoder.vsa_point_feature_fusion.0.weight", "point_head.cls_layers.6.bias",
            "roi_head.roi_grid_pool_layer.mlps.1.4.running_var", "roi_head.shared_fc_layer.4.weight",
            "roi_head.reg_layers.7.bias"} <= names
    for part in (model, enc, model.point_head, head):
        with pytest.raises(NotImplementedError):
            part.train()(dict())
    cfg = mk.encoder_cfg("a")
    for key, val in (("point_source", "voxel_centers"), ("sample_method", "SPC")):
        with pytest.raises(NotImplementedError):
            pr.VoxelSetAbstraction(dict(cfg, **{key: val}), mk.VOXEL, mk.PCR, 4, 4)
    cfg["sa_layer"]["raw_points"]["filter_neighbor_with_roi"] = True
    with pytest.raises(NotImplementedError):
        pr.VoxelSetAbstraction(cfg, mk.VOXEL, mk.PCR, 4, 4)


def test_state_dict_mapping(golden):
    """A Paddle-named state dict (Linear [in, out], _mean / _variance, Conv1D [out, in, 1]) lands on every entry."""
    from paddle3d_amd import pv_rcnn as pr
    from paddle3d_amd import roi_heads as rh
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    g, tag = golden, "a"
    enc = pr.VoxelSetAbstraction(mk.encoder_cfg(tag), mk.VOXEL, mk.PCR, mk.BEV[tag][0], mk.NUM_RAWPOINT_FEATURES)
    ph = pr.PointHeadSimple(mk.NUM_CLASS, enc.num_point_features_before_fusion, mk.POINT_HEAD_CFG)
    head = rh.PVRCNNHead(enc.num_point_features, mk.roi_head_cfg(tag), num_class=1)
    for name, m in (("point_encoder", enc), ("point_head", ph), ("roi_head", head)):
        st = mk.state(g, tag, name)
        assert load_paddle_state_dict(m, st) == []
        own = m.state_dict()
        assert len(st) == len([k for k in own if not k.endswith("num_batches_tracked")])
    st = mk.state(g, tag, "point_encoder")
    w = st["vsa_point_feature_fusion.0.weight"]  # Paddle's Linear: [in, out]
    assert w.shape[1] == 24 and np.array_equal(enc.vsa_point_feature_fusion[0].weight.detach().numpy(), w.T)
    assert np.array_equal(enc.sa_rawpoints.mlps[1][4].running_var.numpy(), st["sa_rawpoints.mlps.1.4._variance"])
    st = mk.state(g, tag, "roi_head")
    assert np.array_equal(head.shared_fc_layer[0].weight.detach().numpy(), st["shared_fc_layer.0.weight"])
    with pytest.raises(RuntimeError):
        load_paddle_state_dict(head, dict(st, **{"shared_fc_layer.9.weight": np.zeros(3, F32)}))


def test_abi_table():
    from paddle3d_amd import _lib

    L = _lib.lib()
    # refusals that need no launch
    pool = lambda c1, c2, s, batch=1, m=4: L.pd3_stack_sa_pool(*([None] * 11), batch, m, 4, c1, c2, 1.0, s, None, None)  # noqa: E731
    assert pool(24, 16, 16) == -3 and pool(16, 48, 16) == -3 and pool(16, 16, 65) == -3 and pool(16, 16, 0) == -1
    assert pool(16, 16, 16, m=0) == 0 and pool(16, 16, 16, batch=0) == -1 and pool(16, 16, 16, m=-1) == -1
    assert L.pd3_bev_interpolate(None, None, 0, 2, 8, 4, 4, 0.0, 0.0, 1.0, 1.0, 1.0, None, None) == 0
    assert L.pd3_bev_interpolate(None, None, -1, 2, 8, 4, 4, 0.0, 0.0, 1.0, 1.0, 1.0, None, None) == -1
