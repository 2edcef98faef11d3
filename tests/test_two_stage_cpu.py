"""The first stage of Voxel R-CNN / PV-RCNN and the two assembled models, without a GPU: paddle3d_amd/anchor_head.py
against what the reference's own AnchorGenerator and AnchorHeadSingle computed (tests/golden/python_two_stage.npz, made
by tests/golden/make_two_stage_golden.py), and the constructors, checkpoint names and predicates of
paddle3d_amd/two_stage.py.

Anchors are compared bit for bit.  The head's transcription path on CPU tensors stays within 4 x the reference's own
float32 error (its float32 result against its float64 result, the maximum over the tensor, stored by the maker) of the
float64 result; direction labels and the period the direction fix adds are compared exactly -- the maker asserted the margins
that make them comparable.
"""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_two_stage_golden as mk  # noqa: E402

from paddle3d_amd import anchor_head as ah  # noqa: E402
from paddle3d_amd import two_stage as ts  # noqa: E402
from paddle3d_amd._lib import Paddle3DAmdError  # noqa: E402
from paddle3d_amd.checkpoint import load_paddle_state_dict, save_pdparams  # noqa: E402

F32 = np.float32
BOX_COLUMNS = ("x", "y", "z", "dx", "dy", "dz", "r")


@pytest.fixture(scope="module")
def golden():
    return mk.load()


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def make_head(g, tag, fused, device="cpu"):
    """The head of golden case `tag` with the recorded weights."""
    cfg_name, C, H, W = mk.HEAD_CASES[tag]
    head = ah.AnchorHeadSingle(model_cfg=dict(mk.MODEL_CFG), input_channels=C, class_names=mk.CLASS_NAMES[cfg_name],
                               voxel_size=mk.VOXEL, point_cloud_range=mk.map_range(W, H), anchor_target_cfg={},
                               predict_boxes_when_training=True, anchor_generator_cfg=mk.CONFIGS[cfg_name],
                               num_dir_bins=2, loss_weights={}, fused=fused)
    load_paddle_state_dict(head, mk.state(g, tag), strict=True)
    return head.eval().to(device)


def check_head_output(g, tag, head, bd, what):
    """Logits and boxes within the 4 x bar of the float64 result, direction labels and rotation periods equal."""
    cls, box = bd["batch_cls_preds"].cpu().numpy(), bd["batch_box_preds"].cpu().numpy()
    assert cls.dtype == F32 and box.dtype == F32 and bd["cls_preds_normalized"] is False
    assert cls.shape == g[f"{tag}_cls"].shape and box.shape == g[f"{tag}_box"].shape
    err, bound = float(np.abs(cls.astype(np.float64) - g[f"{tag}_cls64"]).max()), float(g[f"{tag}_cls_bound"])
    print(f"{tag} {what}: cls err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (tag, what, "cls", err, bound)
    cols = np.abs(box.astype(np.float64) - g[f"{tag}_box64"]).reshape(-1, 7).max(0)
    err, bound = float(cols.max()), float(g[f"{tag}_box_bound"])
    print(f"{tag} {what}: box err {err:.3e} bound {bound:.3e}; per column "
          + " ".join(f"{n} {e:.2e}" for n, e in zip(BOX_COLUMNS, cols)))
    assert err <= bound, (tag, what, "box", err, bound)
    B, A = box.shape[:2]
    dirs = head.forward_ret_dict["dir_cls_preds"].reshape(B, A, -1).argmax(-1).cpu().numpy()
    assert np.array_equal(dirs, g[f"{tag}_dir_labels"]), (tag, what, "direction labels")
    # the rotation is (residual + anchor angle) + period * (label - floor): that integer, from the result
    period = 2 * np.pi / 2
    base = g[f"{tag}_box64"][..., 6] - period * (g[f"{tag}_dir_labels"] - g[f"{tag}_floor"])
    assert np.array_equal(np.round((box[..., 6] - base) / period).astype(np.int64),
                          g[f"{tag}_dir_labels"] - g[f"{tag}_floor"]), (tag, what, "rotation bin")


def _x(g, tag, device="cpu"):
    return torch.from_numpy(g[f"{tag}_x"]).to(device)


# ---- anchors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mk.CONFIGS))
@pytest.mark.parametrize("size", mk.MAPS)
def test_anchors_equal_the_reference_bit_for_bit(golden, name, size):
    nx, ny = size
    cfg = mk.CONFIGS[name]
    anchors, per_loc = ah.AnchorGenerator(mk.map_range(nx, ny), cfg).generate_anchors([np.array([nx, ny])] * len(cfg))
    assert per_loc == golden[f"anchors_{name}_{nx}x{ny}_per_location"].tolist() == [2] * len(cfg)
    for k, a in enumerate(anchors):
        want = golden[f"anchors_{name}_{nx}x{ny}_{k}"]
        assert a.dtype == torch.float32 and tuple(a.shape) == want.shape, (name, size, k)
        assert np.array_equal(_bits(a.numpy()), _bits(want)), (name, size, k)
    # a one-cell map without align_center: the reference's stride is infinite and it makes no anchor
    assert (anchors[0].numel() == 0) == (size == (1, 1))


def test_anchors_align_center_sizes_rotations_heights(golden):
    nx, ny = mk.ALIGN_MAP
    anchors, per_loc = ah.AnchorGenerator(mk.map_range(nx, ny), mk.ALIGN_CFG).generate_anchors([(nx, ny)])
    want = golden["anchors_align_0"]
    assert per_loc == golden["anchors_align_per_location"].tolist() == [12]
    assert tuple(anchors[0].shape) == want.shape == (2, ny, nx, 2, 3, 7)
    assert np.array_equal(_bits(anchors[0].numpy()), _bits(want))


@pytest.mark.parametrize("name", sorted(mk.CONFIGS))
def test_anchors_at_the_kitti_map_match_the_digest(golden, name):
    head = ah.AnchorHeadSingle(mk.MODEL_CFG, 16, mk.CLASS_NAMES[name], mk.VOXEL, mk.KITTI_RANGE, mk.CONFIGS[name], 2)
    a = head.anchors.numpy()
    assert a.shape == tuple(golden[f"anchors_{name}_kitti_shape"]) == (1, 200, 176, len(mk.CONFIGS[name]), 2, 7)
    assert hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() == str(golden[f"anchors_{name}_kitti_sha256"])
    assert head.num_anchors_per_location == 2 * len(mk.CONFIGS[name])


# ---- the head ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(mk.HEAD_CASES))
def test_head_transcription_on_cpu(golden, tag):
    g = golden
    for fused in (False, True):  # CPU tensors take the transcription either way
        head = make_head(g, tag, fused)
        assert np.array_equal(_bits(head.anchors.numpy()), _bits(g[f"{tag}_anchors"]))
        with torch.no_grad():
            bd = head({"spatial_features_2d": _x(g, tag), "batch_size": 2})
        check_head_output(g, tag, head, bd, f"cpu fused={fused}")


@pytest.mark.parametrize("tag", sorted(mk.HEAD_CASES))
def test_head_state_dict_keys_are_the_references(golden, tag):
    import json

    shapes = json.loads(str(golden[f"{tag}_state_shapes"]))
    own = make_head(golden, tag, False).state_dict()
    assert set(own) == set(shapes) == {f"conv_{n}.{p}" for n in ("cls", "box", "dir_cls") for p in ("weight", "bias")}
    assert {k: list(v.shape) for k, v in own.items()} == shapes
    assert "anchors" in dict(make_head(golden, tag, False).named_buffers())


def test_training_only_arguments_and_training_mode():
    with pytest.raises(ValueError):
        ah.AnchorHeadSingle(mk.MODEL_CFG, 16, ["Car"], mk.VOXEL, mk.map_range(4, 4), mk.CAR_CFG, 2, fused="yes")
    head = ah.AnchorHeadSingle(mk.MODEL_CFG, 16, ["Car"], mk.VOXEL, mk.map_range(4, 4), mk.CAR_CFG, 2,
                               anchor_target_cfg={"sample_size": 512}, predict_boxes_when_training=True,
                               loss_weights={"cls_weight": 1.0})
    with pytest.raises(NotImplementedError):
        head.train()({"spatial_features_2d": torch.zeros(1, 16, 4, 4), "batch_size": 1})
    with pytest.raises(RuntimeError, match="anchors"):
        head.eval()({"spatial_features_2d": torch.zeros(1, 16, 4, 8), "batch_size": 1})


def test_fused_predicate_at_its_borders(golden):
    head = make_head(golden, "b", True)
    rows = 6 * (3 + 7 + 2)
    assert head._rows() == rows
    for c, h, w, ok in ((16, 2, 2, True), (32, 3, 4, True), (256, 200, 176, True), (512, 200, 176, True),
                        (32, 1, 4, True), (24, 2, 2, False), (8, 2, 2, False), (15, 2, 2, False), (32, 3, 3, False),
                        (32, 1, 2, False), (32, 5, 5, False), (32, 2, 3, False)):
        assert head.fused_supported(c, h, w) == ok, (c, h, w)
        from paddle3d_amd.ops import conv
        assert conv.patch_supported(1, c, rows, h, w) == ok


def test_force_refuses_what_the_kernel_does_not_take(golden):
    head = make_head(golden, "b", "force")
    assert not head.fused_supported(32, 3, 3)  # h * w % 4
    with pytest.raises(Paddle3DAmdError, match="unsupported"):
        head({"spatial_features_2d": _x(golden, "b"), "batch_size": 2})
    with pytest.raises(Paddle3DAmdError, match="unsupported"):  # CPU tensors have no kernel either
        make_head(golden, "a", "force")({"spatial_features_2d": _x(golden, "a"), "batch_size": 2})


def test_stacked_weight_is_rebuilt_after_a_load(golden):
    from paddle3d_amd.ops import conv

    head = make_head(golden, "c", True)
    wp0, b0 = head._stacked()
    assert head._stacked()[0] is wp0  # kept
    st = {k: (v * 2 + 1).astype(F32) for k, v in mk.state(golden, "c").items()}
    load_paddle_state_dict(head, st, strict=True)
    wp1, b1 = head._stacked()
    raw = torch.cat([torch.from_numpy(st[f"conv_{n}.weight"]) for n in ("cls", "box", "dir_cls")])
    assert wp1 is not wp0 and torch.equal(wp1, conv.pack_patch_weight(raw, 1, False))
    assert torch.equal(b1, torch.cat([torch.from_numpy(st[f"conv_{n}.bias"]) for n in ("cls", "box", "dir_cls")]))
    assert wp1.shape == (2, 16, 16, 64)  # 72 rows padded to 128, K = 256
    # the rows of the packed matrix, in order: cls | box | dir, then zero padding
    rows = wp1.permute(0, 3, 1, 2).reshape(128, 256)
    assert torch.equal(rows[:72], raw[:, :, 0, 0]) and not rows[72:].any()
    with torch.no_grad():
        head.conv_box.weight.mul_(2)  # an in-place write: seen through the version counter
    assert head._stacked()[0] is not wp1  # the slot is not valid any more: rebuilt


# ---- the models --------------------------------------------------------------------------------------------------------
def paddle_state(model):
    """A model's state dict under the reference's names and layouts (what a `.pdparams` file of it holds)."""
    linear = {n + ".weight" for n, m in model.named_modules() if isinstance(m, torch.nn.Linear)}
    out = {}
    for k, v in model.state_dict().items():
        if k.endswith("num_batches_tracked"):
            continue
        a = v.detach().cpu().numpy()
        if k in linear:
            a = a.T
        out[k.replace(".running_mean", "._mean").replace(".running_var", "._variance")] = np.ascontiguousarray(a)
    return out


SMALL_RANGE = [0.0, -3.2, -3.0, 6.4, 3.2, 1.0]


@pytest.mark.parametrize("make", (ts.voxel_rcnn_005voxel_kitti_car, ts.pv_rcnn_005voxel_kitti))
def test_synthetic_pdparams_loads_strict(tmp_path, make):
    torch.manual_seed(1)
    src = make(point_cloud_range=SMALL_RANGE)
    for m in src.modules():  # statistics a fresh model does not have
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    torch.manual_seed(2)
    dst = make(point_cloud_range=SMALL_RANGE)
    stale = dst.dense_head._stacked()[0]
    path = str(tmp_path / "model.pdparams")
    state = paddle_state(src)
    save_pdparams(state, path)
    assert "dense_head.anchors" not in state and "dense_head.conv_dir_cls.weight" in state
    assert any(k.endswith("._variance") for k in state) and not any("second_stage" in k for k in state)
    assert load_paddle_state_dict(dst, path, strict=True) == []
    a, b = src.state_dict(), dst.state_dict()
    assert set(a) == set(b)
    assert all(torch.equal(a[k], b[k]) for k in a if not k.endswith("num_batches_tracked"))
    fresh = dst.dense_head._stacked()[0]
    assert fresh is not stale and torch.equal(fresh, src.dense_head._stacked()[0]) and not torch.equal(fresh, stale)
    with pytest.raises(RuntimeError):  # a key too many
        load_paddle_state_dict(dst, dict(state, **{"dense_head.conv_iou.weight": np.zeros(3, F32)}), strict=True)


def test_constructor_numbers_of_the_voxel_rcnn_yaml():
    m = ts.voxel_rcnn_005voxel_kitti_car()
    assert isinstance(m, ts.VoxelRCNN) and m.num_class == 1
    v = m.voxelizer
    assert (v.voxel_size, v.point_cloud_range) == ([0.05, 0.05, 0.1], [0, -40, -3, 70.4, 40, 1])
    assert (v.max_num_points_in_voxel, v.max_num_voxels) == (5, [16000, 40000])
    assert m.voxel_encoder.in_channels == 4 and m.middle_encoder.in_channels == 4
    assert m.middle_encoder.sparse_shape == (41, 1600, 1408)
    assert [b[0].in_channels for b in m.backbone.blocks] == [256, 64]
    assert [(b[0].out_channels, b[0].stride[0], len(b) // 3 - 1) for b in m.backbone.blocks] == [(64, 1, 5), (128, 2, 5)]
    assert [(type(d[0]).__name__, d[0].in_channels, d[0].out_channels, d[0].stride[0]) for d in m.neck.deblocks] == [
        ("ConvTranspose2d", 64, 128, 1), ("ConvTranspose2d", 128, 128, 2)]
    h = m.dense_head
    assert h.conv_cls.in_channels == 256 and (h.num_class, h.num_dir_bins, h.num_anchors_per_location) == (1, 2, 2)
    assert h.model_cfg == {"use_direction_classifier": True, "dir_offset": 0.78539, "dir_limit_offset": 0.0}
    assert [(c["class_name"], c["anchor_sizes"], c["anchor_rotations"], c["anchor_bottom_heights"], c["align_center"],
             c["feature_map_stride"]) for c in h.anchor_generator_cfg] == [
        ("Car", [[3.9, 1.6, 1.56]], [0, 1.57], [-1.78], False, 8)]
    assert tuple(h.anchors.shape) == (1, 200, 176, 1, 2, 7)
    assert (h.conv_cls.out_channels, h.conv_box.out_channels, h.conv_dir_cls.out_channels) == (2, 14, 4)
    assert h.fused_supported(256, 200, 176)
    r = m.roi_head
    test_nms = r.model_cfg["nms_config"]["test"]
    assert (test_nms["nms_pre_maxsize"], test_nms["nms_post_maxsize"], test_nms["nms_thresh"]) == (2048, 100, 0.7)
    assert r.pool_cfg["features_source"] == ["x_conv2", "x_conv3", "x_conv4"] and r.pool_cfg["grid_size"] == 6
    assert r.shared_fc_layer[0].in_features == 216 * 96 and r.shared_fc_layer[0].out_features == 256
    assert m.post_process_cfg == {"score_thresh": 0.3, "output_raw_score": False, "nms_config": {
        "multi_classes_nms": False, "nms_type": "nms_gpu", "nms_thresh": 0.1, "nms_pre_maxsize": 4096,
        "nms_post_maxsize": 500}}


def test_constructor_numbers_of_the_pv_rcnn_yaml():
    m = ts.pv_rcnn_005voxel_kitti()
    assert isinstance(m, ts.PVRCNN) and m.num_class == 3
    v = m.voxelizer
    assert (v.voxel_size, v.point_cloud_range) == ([0.05, 0.05, 0.1], [0, -40, -3, 70.4, 40, 1])
    assert (v.max_num_points_in_voxel, v.max_num_voxels) == (5, [16000, 40000])
    assert m.middle_encoder.sparse_shape == (41, 1600, 1408)
    assert [(b[0].in_channels, b[0].out_channels, b[0].stride[0], len(b) // 3 - 1) for b in m.backbone.blocks] == [
        (256, 128, 1, 5), (128, 256, 2, 5)]
    assert [(type(d[0]).__name__, d[0].in_channels, d[0].out_channels, d[0].stride[0]) for d in m.neck.deblocks] == [
        ("ConvTranspose2d", 128, 256, 1), ("ConvTranspose2d", 256, 256, 2)]
    h = m.dense_head
    assert h.conv_cls.in_channels == 512 and (h.num_class, h.num_dir_bins, h.num_anchors_per_location) == (3, 2, 6)
    assert h.class_names == ["Car", "Pedestrian", "Cyclist"]
    assert [(c["class_name"], c["anchor_sizes"], c["anchor_rotations"], c["anchor_bottom_heights"], c["align_center"],
             c["feature_map_stride"]) for c in h.anchor_generator_cfg] == [
        ("Car", [[3.9, 1.6, 1.56]], [0, 1.57], [-1.78], False, 8),
        ("Pedestrian", [[0.8, 0.6, 1.73]], [0, 1.57], [-0.6], False, 8),
        ("Cyclist", [[1.76, 0.6, 1.73]], [0, 1.57], [-0.6], False, 8)]
    assert tuple(h.anchors.shape) == (1, 200, 176, 3, 2, 7)
    assert (h.conv_cls.out_channels, h.conv_box.out_channels, h.conv_dir_cls.out_channels) == (18, 42, 12)
    assert h.fused_supported(512, 200, 176)
    e = m.point_encoder
    assert e.model_cfg["num_keypoints"] == 2048 and e.num_point_features == 128
    assert e.num_point_features_before_fusion == 640 == m.point_head.cls_layers[0].in_features
    assert m.point_head.num_class == 1  # class agnostic
    test_nms = m.roi_head.model_cfg["nms_config"]["test"]
    assert (test_nms["nms_pre_maxsize"], test_nms["nms_post_maxsize"], test_nms["nms_thresh"]) == (1024, 100, 0.7)
    assert m.roi_head.pre_channel == 216 * 128
    assert m.post_process_cfg["score_thresh"] == 0.1 and m.post_process_cfg["nms_config"]["nms_thresh"] == 0.1
    assert (m.post_process_cfg["nms_config"]["nms_pre_maxsize"], m.post_process_cfg["nms_config"]["nms_post_maxsize"]) == (4096, 500)
    assert m.second_stage.roi_head is m.roi_head and "second_stage" not in dict(m.named_children())


def test_shrunken_range_keeps_the_depth_chain():
    for make, anchors in ((ts.voxel_rcnn_005voxel_kitti_car, 512), (ts.pv_rcnn_005voxel_kitti, 1536)):
        m = make(point_cloud_range=SMALL_RANGE, fused=False)
        assert m.middle_encoder.sparse_shape == (41, 128, 128)
        assert m.dense_head.anchors.numel() // 7 == anchors and m.dense_head.fused is False
        assert m.roi_head.point_cloud_range == SMALL_RANGE if hasattr(m.roi_head, "point_cloud_range") else True


def test_to_kitti_detections_is_accepted_by_the_bridge():
    from paddle3d_amd.kitti_bridge import detections_to_kitti_annos

    box = torch.tensor([[10.0, 1.0, -1.0, 3.9, 1.6, 1.5, 0.3], [20.0, -3.0, -0.8, 0.8, 0.6, 1.7, -1.0]])
    preds = [{"box3d_lidar": box, "scores": torch.tensor([0.9, 0.4]), "label_preds": torch.tensor([1, 2])},
             {"box3d_lidar": torch.zeros(1, 7), "scores": torch.tensor([-1.0]), "label_preds": torch.tensor([-1])}]
    dets = ts.to_kitti_detections(preds)
    want = box.numpy().copy()
    want[:, 3:5] = want[:, [4, 3]]
    want[:, 6] = -(want[:, 6] + np.pi / 2)
    want[:, 2] -= want[:, 5] / 2
    np.testing.assert_allclose(dets[0]["box3d_lidar"], want, rtol=0, atol=1e-6)
    assert dets[0]["label_preds"].tolist() == [0, 1] and torch.equal(preds[0]["box3d_lidar"], box)
    calib = (np.eye(3, 4),) * 4 + (np.eye(3), np.eye(3, 4))
    calib = tuple(np.asarray(c, np.float64) for c in calib)
    with np.errstate(all="ignore"):
        annos = detections_to_kitti_annos(dets, [calib, calib], ["Car", "Pedestrian", "Cyclist"])
    assert annos[0]["name"].tolist() == ["Car", "Pedestrian"] and len(annos[1]["name"]) == 0
