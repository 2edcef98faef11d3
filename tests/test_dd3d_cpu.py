"""DD3D's FCOS heads and post-processing without a GPU: the NumPy restatement of csrc/dd3d.hip (tests/golden/dd3d_numpy.py)
and the module's plain-torch transcription against the reference's own Python (tests/golden/python_dd3d.npz, written by
tests/golden/make_dd3d_golden.py) within the stored per-group bounds, with classes, order and counts equal; state-dict
keys equal to the reference's and a strict load of a synthetic .pdparams; the predicate's borders; the C ABI's statuses
and pd3_dd3d_workspace, which need no GPU; locations, image preprocessing and the host-boundary helper."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import dd3d_numpy as dn  # noqa: E402

F32 = np.float32
GOLDEN = os.path.join(HERE, "golden", "python_dd3d.npz")
ROW_COLS = [0, 1, 2, 3, 4, 5, 6] + list(range(10, 20))  # the golden file's 17 columns in the kernels' 20-float row


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def build_model(tag, fused=True):
    """paddle3d_amd.dd3d.DD3D without a backbone and with the golden case's state, loaded under the reference's names."""
    from paddle3d_amd import dd3d as D
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    c, cfg = dn.CASES[tag], dn.cfg_of(tag)
    L = len(c["shapes"])
    head2 = D.FCOS2DHead(list(c["strides"]), [c["C"]] * L, num_classes=c["nc"], version=c["version"],
                         num_cls_convs=dn.NUM_CONVS, num_box_convs=dn.NUM_CONVS, norm=c["norm"])
    inf2 = D.FCOS2DInference(thresh_with_ctr=cfg["thresh_with_ctr"], pre_nms_thresh=cfg["pre_nms_thresh"],
                             pre_nms_topk=cfg["pre_nms_topk"], post_nms_topk=cfg["post_nms_topk"],
                             nms_thresh=cfg["nms_thresh"], num_classes=c["nc"])
    head3 = inf3 = None
    if not c.get("only_box2d"):
        head3 = D.FCOS3DHead(list(c["strides"]), [c["C"]] * L, num_classes=c["nc"], num_convs=dn.NUM_CONVS, norm=c["norm"],
                             use_per_level_predictors=bool(c.get("per_level")), per_level_predictors=bool(c.get("per_level")),
                             class_agnostic_box3d=bool(c.get("class_agnostic")))
        inf3 = D.FCOS3DInference(min_depth=cfg["min_depth"], max_depth=cfg["max_depth"],
                                 predict_distance=cfg["predict_distance"], num_classes=c["nc"],
                                 class_agnostic=bool(c.get("class_agnostic")))
    model = D.DD3D(None, c["offset"], None, head2, inf2, head3, inf3, do_nms=True, num_classes=c["nc"],
                   input_strides=c["strides"], fused=fused)
    s2, s3 = dn.golden_state(tag)
    state = {"fcos2d_head." + k: v for k, v in s2.items()}
    state.update({"fcos3d_head." + k: v for k, v in (s3 or {}).items()})
    state.update(pixel_mean=model.pixel_mean.numpy().copy(), pixel_std=model.pixel_std.numpy().copy())
    assert load_paddle_state_dict(model, state, strict=True) == []
    return model.eval()


def tower_outputs(tag):
    """(levels, packed) of a golden case: the dense parts (towers, cls_logits, centerness) by torch on the CPU in float32,
    the predictor arrays packed from the state dicts."""
    model = build_model(tag)
    feats = [torch.from_numpy(f) for f in dn.golden_inputs(tag)]
    with torch.no_grad():
        cls_out, box_out = model.fcos2d_head.towers(feats)
        t3 = model.fcos3d_head.tower(feats) if model.fcos3d_head is not None else None
        levels = []
        for l in range(len(feats)):
            lv = dict(logits=model.fcos2d_head.cls_logits(cls_out[l]).numpy(),
                      centerness=model.fcos2d_head.centerness(box_out[l]).numpy(), f2d=box_out[l].numpy())
            if t3 is not None:
                lv["f3d"] = t3[l].numpy()
            levels.append(lv)
    return levels, dn.pack_state(*dn.golden_state(tag), dn.CASES[tag])


def op_cfg(tag):
    return dn.cfg_of(tag)


def restated(tag):
    levels, packed = tower_outputs(tag)
    (rows, counts), _ = dn.head_forward(levels, dn.CASES[tag]["strides"], packed, dn.golden_camera(tag), dn.CANON, op_cfg(tag))
    return rows, counts


def run_model(model, tag, device="cpu", fused=None):
    feats = [torch.from_numpy(f).to(device) for f in dn.golden_inputs(tag)]
    with torch.no_grad():
        return model.head_padded(feats, torch.from_numpy(dn.golden_camera(tag)).to(device), fused=fused)


def check_against_golden(tag, rows, counts, G, what):
    """rows [B, R, 20] / counts against the reference's result: the same rows in the same order, classes equal, every
    other stored column within its group's bound; prints the largest difference per column in units of the bound."""
    rows, counts = np.asarray(rows, F32), np.asarray(counts)
    ref, bd = G[f"{tag}_rows"], G[f"{tag}_bound"]
    assert list(counts) == list(G[f"{tag}_counts"]), (what, tag, list(counts), list(G[f"{tag}_counts"]))
    R = rows.shape[1]
    assert (rows[np.arange(R)[None] >= counts[:, None]] == 0).all(), f"{what} {tag}: rows past the count"
    got = np.concatenate([np.concatenate([rows[b, :counts[b]][:, ROW_COLS], np.full((counts[b], 1), b, F32)], 1)
                          for b in range(len(counts))])
    assert got.shape == ref.shape, (what, tag, got.shape, ref.shape)
    assert np.array_equal(got[:, 6], ref[:, 6]) and np.array_equal(got[:, 17], ref[:, 17]), f"{what} {tag}: classes / order"
    err = np.abs(got[:, :17].astype(np.float64) - ref[:, :17]).max(0) if len(ref) else np.zeros(17)
    with np.errstate(all="ignore"):
        print(f"{what} {tag}: err / bound per column", np.array2string(err / bd, precision=2))
    assert (err <= bd).all(), (what, tag, err, bd)
    # the columns the reference does not carry through its NMS: the level and the location of every kept row
    for b in range(len(counts)):
        r = rows[b, :counts[b]]
        stride = np.asarray(dn.CASES[tag]["strides"], F32)[r[:, 7].astype(int)]
        half = stride // 2 if dn.CASES[tag]["offset"] == "half" else stride * 0
        assert ((r[:, 8:10] - half[:, None]) % stride[:, None] == 0).all()


@pytest.mark.parametrize("tag", dn.TAGS)
def test_restatement_within_the_references_bounds(tag, golden):
    rows, counts = restated(tag)
    check_against_golden(tag, rows, counts, golden, "restatement")


@pytest.mark.parametrize("tag", dn.TAGS)
def test_module_torch_transcription_within_the_references_bounds(tag, golden):
    rows, counts = run_model(build_model(tag), tag)
    check_against_golden(tag, rows.numpy(), counts.numpy(), golden, "torch transcription")


def test_golden_file_covers_what_the_cases_promise(golden):
    """Both cuts bite, an image has no detection, the nc = 6 case keeps no class 5, the depth clip bites at both ends."""
    assert any((golden[f"{t}_counts"] == 0).any() for t in dn.TAGS)
    assert all((golden[f"{t}_counts"] <= dn.CASES[t]["post_nms_topk"]).all() for t in dn.TAGS)
    assert golden["agn6_rows"][:, 6].max() < 5
    d = golden["v2_l5_rows"][:, 13]
    assert (d == F32(0.8)).any() and (d == F32(1.6)).any()
    assert not golden["box2d_rows"][:, 5].any() and not golden["box2d_rows"][:, 7:17].any()


@pytest.mark.parametrize("tag", dn.TAGS)
def test_state_dict_keys_equal_the_references(tag):
    """golden_state's dicts loaded strictly into the reference's own classes when the golden file was made."""
    model = build_model(tag)
    s2, s3 = dn.golden_state(tag)
    want = {"fcos2d_head." + k for k in s2} | {"fcos3d_head." + k for k in (s3 or {})} | {"pixel_mean", "pixel_std"}
    keys = {k.replace("running_mean", "_mean").replace("running_var", "_variance") for k in model.state_dict()
            if not k.endswith("num_batches_tracked")}
    assert keys == want, keys ^ want


def test_strict_load_of_a_pdparams_file(tmp_path):
    from paddle3d_amd.checkpoint import load_paddle_state_dict, save_pdparams

    model = build_model("v2_l5")
    rng = np.random.default_rng(3)
    state = {k.replace("running_mean", "_mean").replace("running_var", "_variance"):
             rng.uniform(0.5, 1.5, tuple(v.shape)).astype(F32) for k, v in model.state_dict().items()
             if not k.endswith("num_batches_tracked")}
    path = str(tmp_path / "dd3d.pdparams")
    save_pdparams(state, path)
    assert load_paddle_state_dict(model, path, strict=True) == []
    assert np.array_equal(model.fcos3d_head.offsets_depth[4].bias.detach().numpy(), state["fcos3d_head.offsets_depth.4.bias"])
    assert np.array_equal(model.fcos2d_head.cls_tower[1][3].running_var.numpy(), state["fcos2d_head.cls_tower.1.3._variance"])


def test_constructor_defaults_are_the_references():
    from paddle3d_amd import dd3d as D

    h2 = D.FCOS2DHead([8, 16, 32, 64, 128], [256] * 5, norm="FrozenBN")
    assert [float(s.scale.detach()) for s in h2.scales_box2d_reg] == [8.0, 16.0, 32.0, 64.0, 128.0] and len(h2.cls_tower) == 12
    assert h2.cls_tower[0].bias is None and isinstance(h2.cls_tower[1][0], D.FrozenBatchNorm2d)
    assert D.FCOS2DHead([8], [16], version="v1").cls_tower[0].bias is not None
    h3 = D.FCOS3DHead([8, 16, 32, 64, 128], [256] * 5)
    assert h3.box3d_depth[0].bias is None and h3.box3d_quat[0].out_channels == 20 and len(h3.box3d_quat) == 1
    assert float(h3.scales_depth[1].scale.detach()) == pytest.approx(7.139 * 0.3) and float(h3.offsets_depth[0].bias.detach()) == pytest.approx(32.594)
    assert D.FCOS3DHead([8, 16], [16] * 2, class_agnostic_box3d=True, per_level_predictors=True).box3d_size[1].out_channels == 3
    i2, i3 = D.FCOS2DInference(), D.FCOS3DInference()
    assert (i2.pre_nms_thresh, i2.pre_nms_topk, i2.post_nms_topk, i2.nms_thresh, i2.nms_categories) == (0.05, 1000, 100, 0.75, 5)
    assert (i3.min_depth, i3.max_depth, i3.scale_depth_by_focal_lengths_factor, len(i3.canon_box_sizes)) == (0.1, 80.0, 500.0, 8)
    fbn = D.FrozenBatchNorm2d(4)
    x = torch.randn(2, 4, 3, 3)
    assert torch.allclose(fbn(x), x, atol=1e-6)  # the identity at its initial buffers


def test_locations_preprocessing_and_the_host_boundary():
    from paddle3d_amd import dd3d as D

    model = build_model("v1_l3")
    loc = model.compute_features_locations(2, 3, 8, offset="half")
    assert loc.tolist() == [[4, 4], [12, 4], [20, 4], [4, 12], [12, 12], [20, 12]]
    assert model.compute_features_locations(1, 2, 16).tolist() == [[0, 0], [16, 0]]
    img = torch.full((1, 3, 5, 130), 255.0)
    out = model.preprocess_image(img, 128)
    assert tuple(out.shape) == (1, 3, 128, 256) and float(out[0, 0, 4, 129]) == pytest.approx((255 - 103.53) / 57.375)
    assert not out[:, :, 5:].any() and not out[:, :, :, 130:].any()
    rows = torch.arange(2 * 3 * 20, dtype=torch.float32).reshape(2, 3, 20)
    inst = D.rows_to_instances(rows, torch.tensor([2, 5], dtype=torch.int32))
    assert inst[0]["pred_boxes"].shape == (2, 4) and inst[1]["pred_boxes3d"].shape == (3, 10)
    assert inst[0]["pred_classes"].dtype == torch.int64 and inst[0]["scores_3d"].tolist() == [5.0, 25.0]
    # do_nms=False and nms_thresh <= 0 take the transcription: every candidate, in level order
    model.do_nms = False
    rows, counts = run_model(model, "v1_l3")
    assert rows.shape[1] == 3 * 20 and int(counts[0]) > 8 and (np.diff(rows[0, :int(counts[0]), 7].numpy()) >= 0).all()


def test_predicate_borders():
    from paddle3d_amd.ops.dd3d import dd3d_supported as ok

    s5 = [(48, 160), (24, 80), (12, 40), (6, 20), (3, 10)]
    assert ok(s5, 5, 1000, 0.75, 256) and ok(s5, 5, 1000, 0.75)
    assert ok(s5, 16, 1024, 0.75, 512) and not ok(s5, 17, 1000, 0.75, 256) and not ok(s5, 5, 1025, 0.75, 256)
    assert not ok(s5, 5, 0, 0.75, 256) and not ok(s5, 5, 1000, 0.0, 256) and not ok(s5, 5, 1000, 0.75, 513)
    assert ok([(1, 1)] * 8, 1, 1, 0.1, 1) and not ok([(1, 1)] * 9, 1, 1, 0.1, 1) and not ok([], 1, 1, 0.1, 1)
    assert ok([(16384, 16383)], 4, 50, 0.5) and not ok([(16384, 16384)], 4, 50, 0.5)


def test_statuses_and_workspace_without_a_gpu():
    from paddle3d_amd import _lib

    L = _lib.lib()
    buf = np.zeros(64, F32)
    p = C.c_void_p(buf.ctypes.data)

    def table(shapes, pitch=None, c=16):
        t = np.array([(h, w, 8, pitch or w, c * h * (pitch or w)) for h, w in shapes], np.int64)
        return t, C.c_void_p(t.ctypes.data)

    t5, p5 = table([(6, 10), (3, 5), (2, 3), (1, 2), (1, 1)])
    assert L.pd3_dd3d_workspace(2, 5, p5, 5, 20) > 0 and L.pd3_dd3d_workspace(2, 5, p5, 5, 1024) > L.pd3_dd3d_workspace(2, 5, p5, 5, 20)
    assert L.pd3_dd3d_workspace(2, 5, p5, 17, 20) == 0 and L.pd3_dd3d_workspace(2, 5, p5, 5, 1025) == 0
    assert L.pd3_dd3d_workspace(2, 9, p5, 5, 20) == 0 and L.pd3_dd3d_workspace(0, 5, p5, 5, 20) == 0
    ptrs = np.full(8, buf.ctypes.data, np.uint64)
    pp = C.c_void_p(ptrs.ctypes.data)

    def post(nc=5, levels=5, tab=p5, k=20, nms=0.6, arr=pp, ws=0, batch=2, ncp=None, flags=1, some=pp):
        return L.pd3_dd3d_post_process(arr, arr, arr, some, arr, arr, arr, arr, tab, p, p, batch, levels, nc,
                                       nc if ncp is None else ncp, k, 8, 5, flags, 0.3, nms, 0.1, 80.0, 500.0, p, p, p, ws, None)

    def head(nc=5, levels=5, tab=p5, k=20, nms=0.6, arr=pp, ws=0, batch=2, ncp=None, flags=1, c=16, wl=1):
        return L.pd3_dd3d_head_forward(arr, arr, arr, arr, tab, p, p, p, p, p, p, p, batch, levels, c, nc,
                                       nc if ncp is None else ncp, wl, k, 8, 5, flags, 0.3, nms, 0.1, 80.0, 500.0, p, p, p, ws,
                                       None)

    for f in (post, head):
        assert f(k=0) == -3 and f(k=1025) == -3 and f(nc=17) == -3 and f(nms=0.0) == -3 and f(nms=-1.0) == -3
        assert f(levels=9) == -3 and f(levels=0) == -1 and f(nc=0) == -1 and f(ncp=2) == -1 and f(flags=32) == -1
        assert f(arr=None) == -1 and f(tab=None) == -1
        assert f() == -2  # a workspace of 0 bytes
        assert f(batch=0) == 0
    big, pbig = table([(16384, 16384)])
    assert post(nc=4, levels=1, tab=pbig) == -3
    assert post(some=None) == -1  # four of the five 3D maps without the first
    assert head(c=513) == -3 and head(c=0) == -1 and head(wl=2) == -1 and head(wl=5) == -2
    short, pshort = table([(6, 10)], pitch=9)
    assert head(levels=1, tab=pshort) == -1
