"""The first stage of Voxel R-CNN / PV-RCNN and the two assembled models on the device.

The head (paddle3d_amd/anchor_head.py) in its three forms against what the reference's own Python computed
(tests/golden/python_two_stage.npz): logits and boxes within 4 x the reference's own float32 error of its float64
result, direction labels and rotation periods exactly.  The stacked GEMM is compared bit for bit with three separate
calls of the same kernel (the same K order: a difference is a bug in the stacking), counted as one launch, and run under
the device-sync guard.

The models (paddle3d_amd/two_stage.py) run on a shrunken range -- x in [0, 6.4], y in [-3.2, 3.2], 128 x 128 x 40
voxels, a 16 x 16 head map, 512 car anchors / 1536 three-class anchors -- with random weights from a fixed seed: their
first stage and proposals are torch.equal to the same stages run by hand, to the frames in the other order and to each
frame alone; so are Voxel R-CNN's detections against the hand run.  Behind the RoI heads' fully connected stacks, which
are GEMMs of the BLAS library and sum in an order that depends on the batch's row count (PV-RCNN's Conv1d form also
on the run), results are compared under a bar taken from those stacks' own float32 error (Case.bars, Case.close).
"""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_two_stage_golden as mk  # noqa: E402
import test_two_stage_cpu as cpu  # noqa: E402
from guarded import launch_ledger  # noqa: E402

from paddle3d_amd import anchor_head as ah  # noqa: E402
from paddle3d_amd import two_stage as ts  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
PATCH = ("pd3_patch_conv_bias_relu", "pd3_patch_conv_x3_bias_relu")
TAGS = sorted(mk.HEAD_CASES)


@pytest.fixture(scope="module")
def golden():
    return mk.load()


def _run(head, x):
    with torch.no_grad():
        return head({"spatial_features_2d": x, "batch_size": int(x.shape[0])})


def _takes_kernel(tag):
    _, C, H, W = mk.HEAD_CASES[tag]
    return C % 16 == 0 and (H * W) % 4 == 0


# ---- the head ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("fused", (False, None, True, "force"))
def test_head_against_the_reference(golden, tag, fused):
    from paddle3d_amd._lib import Paddle3DAmdError, lib

    g = golden
    head = cpu.make_head(g, tag, fused, DEV)
    x = cpu._x(g, tag, DEV)
    if fused == "force" and not _takes_kernel(tag):
        with pytest.raises(Paddle3DAmdError, match="unsupported"):
            _run(head, x)
        return
    with launch_ledger(lib(), PATCH) as calls:
        bd = _run(head, x)
    cpu.check_head_output(g, tag, head, bd, f"device fused={fused}")
    # one launch of the 1x1 kernel where the stacked GEMM runs, none where the transcription does (case b falls back)
    stacked = head.fused in (True, "force") and _takes_kernel(tag)
    assert calls == {PATCH[0]: int(stacked), PATCH[1]: 0}, (tag, fused, calls)
    assert _takes_kernel(tag) == (tag != "b")


@pytest.mark.parametrize("tag", TAGS)
def test_fused_and_transcription_agree(golden, tag):
    g = golden
    x = cpu._x(g, tag, DEV)
    a, b = (_run(cpu.make_head(g, tag, fused, DEV), x) for fused in (True, False))
    err = float((a["batch_cls_preds"].double() - b["batch_cls_preds"].double()).abs().max())
    assert err <= float(g[f"{tag}_cls_bound"]), ("cls", err)
    err = float((a["batch_box_preds"].double() - b["batch_box_preds"].double()).abs().max())
    print(f"{tag} box: fused - transcription {err:.3e}, bound {float(g[f'{tag}_box_bound']):.3e}")
    assert err <= float(g[f"{tag}_box_bound"]), ("box", err)
    if tag == "b":  # the fall-back IS the transcription
        assert torch.equal(a["batch_box_preds"], b["batch_box_preds"])


@pytest.mark.parametrize("tag", [t for t in TAGS if _takes_kernel(t)])
def test_stacked_rows_equal_three_separate_launches(golden, tag):
    from paddle3d_amd.ops import conv

    head = cpu.make_head(golden, tag, True, DEV)
    x = cpu._x(golden, tag, DEV)
    _run(head, x)
    got = [head.forward_ret_dict[k] for k in ("cls_preds", "box_preds", "dir_cls_preds")]
    for m, want_of in zip(got, (head.conv_cls, head.conv_box, head.conv_dir_cls)):
        cout = want_of.out_channels
        out = torch.full((x.shape[0], cout, x.shape[2], x.shape[3]), float("nan"), device=DEV)
        conv.patch_conv_bias_relu(x, conv.pack_patch_weight(want_of.weight.detach(), 1, False),
                                  want_of.bias.detach().contiguous(), 1, cout, out, 0, relu=False)
        assert torch.equal(m, out.permute(0, 2, 3, 1)), (tag, cout)
        assert not m.is_contiguous()  # a view of the one NCHW map, not a [B, H, W, C] copy
    # negative pre-activations are there: the kernel ran without its ReLU
    assert bool((got[1] < 0).any())


@pytest.mark.parametrize("fused", (False, True))
def test_head_makes_no_host_sync(golden, fused):
    head = cpu.make_head(golden, "c", fused, DEV)
    x = cpu._x(golden, "c", DEV)
    _run(head, x)  # warm-up: code objects, allocator, the packed weight
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        bd = _run(head, x)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert bd["batch_box_preds"].shape == (2, 24, 7)


def test_head_at_the_kitti_map_takes_the_stacked_gemm():
    """The shape the constructors produce: 200 x 176 x 256, B = 1, three classes."""
    from paddle3d_amd._lib import lib

    torch.manual_seed(0)
    head = ah.AnchorHeadSingle(ts.ANCHOR_HEAD_MODEL_CFG, 256, ["Car", "Pedestrian", "Cyclist"], ts.KITTI_VOXEL,
                               ts.KITTI_RANGE, ts.KITTI_ANCHOR_CFG, 2).to(DEV).eval()
    assert head.fused == ah.FUSED_HEAD_DEFAULT
    head.fused = True
    x = torch.randn(1, 256, 200, 176, device=DEV)
    with launch_ledger(lib(), PATCH) as calls:
        a = _run(head, x)
    assert calls[PATCH[0]] == 1
    b = _run(head, x)
    A = 200 * 176 * 6
    assert a["batch_cls_preds"].shape == (1, A, 3) and a["batch_box_preds"].shape == (1, A, 7)
    assert bool(torch.isfinite(a["batch_box_preds"]).all()) and bool(torch.isfinite(a["batch_cls_preds"]).all())
    assert torch.equal(a["batch_box_preds"], b["batch_box_preds"]) and torch.equal(a["batch_cls_preds"], b["batch_cls_preds"])


# ---- the models --------------------------------------------------------------------------------------------------------
def frame(seed, n=3000):
    """Seeded points of one frame inside the shrunken range: clusters (several voxels per level are occupied), a thin
    ground sheet, a few points outside the range."""
    rng = np.random.default_rng(seed)
    centres = np.stack([rng.uniform(1.0, 5.4, 6), rng.uniform(-2.2, 2.2, 6), rng.uniform(-1.6, -0.6, 6)], 1)
    near = centres[rng.integers(0, 6, n - 600)] + rng.normal(0, [0.45, 0.25, 0.25], (n - 600, 3))
    ground = np.stack([rng.uniform(0, 6.4, 560), rng.uniform(-3.2, 3.2, 560), rng.normal(-1.75, 0.02, 560)], 1)
    out = np.stack([rng.uniform(6.5, 8.0, 40), rng.uniform(-5, 5, 40), rng.uniform(-4, 2, 40)], 1)
    xyz = np.concatenate([near, ground, out])
    pts = np.concatenate([xyz, rng.random((n, 1))], 1).astype(np.float32)
    return torch.from_numpy(pts[rng.permutation(n)]).to(DEV)


def _model(kind):
    make = {"voxel": ts.voxel_rcnn_005voxel_kitti_car, "pv": ts.pv_rcnn_005voxel_kitti}[kind]
    torch.manual_seed(3)
    m = make(point_cloud_range=cpu.SMALL_RANGE)
    torch.nn.init.constant_(m.dense_head.conv_cls.bias, 0.0)  # lets proposals of every class through
    torch.nn.init.normal_(m.dense_head.conv_box.weight, std=0.02)  # proposals that move off their anchors
    last = m.roi_head.cls_pred_layer if kind == "voxel" else m.roi_head.cls_layers[-1]
    torch.nn.init.normal_(last.weight, std=0.3)  # final scores spread over (0, 1): some under the threshold, no near ties
    return m.to(DEV).eval()


class Case:
    """One model, two frames, its detections on them, and what entered and left the RoI head on the way."""

    def __init__(self, kind):
        self.kind, self.model = kind, _model(kind)
        self.frames = [frame(11), frame(12, n=2400)]
        self.dets, self.seen = self.run(self.frames)
        self.bar_cls, self.bar_reg = self.bars(self.seen["pooled"])

    def run(self, points, **kw):
        """model(points) and, cloned, the first stage's proposals, the RoIs and the RoI head's pooled features."""
        seen, head = {}, self.model.roi_head
        hooks = [
            head.register_forward_pre_hook(lambda m, a: seen.update(
                head_cls=a[0]["batch_cls_preds"].clone(), head_box=a[0]["batch_box_preds"].clone())),
            head.register_forward_hook(lambda m, a, out: seen.update(rois=out["rois"].clone(),
                                                                     roi_scores=out["roi_scores"].clone())),
            head.shared_fc_layer.register_forward_pre_hook(lambda m, a: seen.update(pooled=a[0].clone()))]
        try:
            return self.model(points, **kw), seen
        finally:
            for h in hooks:
                h.remove()

    def bars(self, pooled):
        """4 x the float32 error of the RoI head's fully connected stacks -- torch GEMMs, whose order of summation
        depends on the number of rows (and, for PV-RCNN's Conv1d form, on the run) -- against their float64 evaluation
        on the same float32 pooled features and weights; one float32 ulp of the largest output as a floor."""
        import copy

        def stacks(h, x):
            shared = h.shared_fc_layer(x)
            if self.kind == "pv":
                return h.cls_layers(shared), h.reg_layers(shared)
            return h.cls_pred_layer(h.cls_fc_layers(shared)), h.reg_pred_layer(h.reg_fc_layers(shared))

        def bar(a, b):
            return max(4 * float((a.double() - b).abs().max()), float(np.spacing(np.float32(float(b.abs().max())))))

        with torch.no_grad():
            c32, r32 = stacks(self.model.roi_head, pooled)
            c64, r64 = stacks(copy.deepcopy(self.model.roi_head).double(), pooled.double())
        return bar(c32, c64), bar(r32, r64)

    def close(self, a, b, what):
        """Two results of one frame whose RoI heads summed in different orders: equal counts and labels; scores within
        the logits' bar (the sigmoid contracts); boxes within the residuals' bar times what the decode multiplies a
        residual by (the RoI's diagonal or height for the centre, the decoded size for a size, 1 for the angle), plus
        one float32 ulp of the largest coordinate for the decode's own rounding."""
        assert a["scores"].shape == b["scores"].shape and torch.equal(a["label_preds"], b["label_preds"]), what
        ds = float((a["scores"].double() - b["scores"].double()).abs().max())
        size = b["box3d_lidar"][:, 3:6].double()
        scale = max(1.0, float(torch.sqrt(size[:, 0] ** 2 + size[:, 1] ** 2).max()), float(size.max()))
        bound = self.bar_reg * scale + float(np.spacing(np.float32(float(b["box3d_lidar"].abs().max()))))
        db = float((a["box3d_lidar"].double() - b["box3d_lidar"].double()).abs().max())
        print(f"{self.kind} {what}: scores {ds:.3e} (bar {self.bar_cls:.3e}), boxes {db:.3e} (bar {bound:.3e})")
        assert ds <= self.bar_cls and db <= bound, (what, ds, self.bar_cls, db, bound)


@pytest.fixture(scope="module", params=("voxel", "pv"))
def case(request):
    """Computed once per model, left unchanged."""
    return Case(request.param)


def by_hand(model, points):
    """The stages, one after the other, as the models' docstring lists them."""
    from paddle3d_amd import roi_heads as rh

    B = len(points)
    n = max(max(int(p.shape[0]) for p in points), 1)
    padded = torch.zeros((B, n, 4), device=DEV)
    for b, p in enumerate(points):
        padded[b, :p.shape[0]] = p
    lens = torch.tensor([int(p.shape[0]) for p in points], dtype=torch.int32, device=DEV)
    with torch.no_grad():
        voxels, coors, npv, _ = model.voxelizer(padded, lens)
        V = voxels.shape[1]
        feats = model.voxel_encoder(voxels.view(B * V, *voxels.shape[2:]), npv.view(B * V))
        bd = {"data": points, "batch_size": B, "voxel_coords": coors.view(B * V, 4),
              "points": torch.cat([torch.cat([torch.full((p.shape[0], 1), float(b), device=DEV), p], 1)
                                   for b, p in enumerate(points)])}
        bd.update(model.middle_encoder(feats, bd["voxel_coords"], B))
        bd["spatial_features_2d"] = model.neck(model.backbone(bd["spatial_features"]))
        bd = model.dense_head(bd)
        first = {"head_cls": bd["batch_cls_preds"].clone(), "head_box": bd["batch_box_preds"].clone()}
        if isinstance(model, ts.PVRCNN):
            bd = model.point_head(model.point_encoder(bd))
        pooled = []
        hook = model.roi_head.shared_fc_layer.register_forward_pre_hook(lambda m, a: pooled.append(a[0].clone()))
        try:
            bd = model.roi_head(bd)
        finally:
            hook.remove()
        first.update(rois=bd["rois"], roi_scores=bd["roi_scores"], pooled=pooled[0])
        return rh.post_processing(bd, model.post_process_cfg, model.num_class), bd, first


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("box3d_lidar", "scores", "label_preds"))


def test_model_equals_the_stages_by_hand(case):
    """torch.equal up to and including what the RoI head's fully connected stacks read, and in the end for Voxel R-CNN.
    PV-RCNN's RoI head runs those stacks as torch Conv1d layers over [B * R, 27 648, 1], and two runs of that
    convolution on the same bytes do not return the same bits on this device (measured: 97 of 100 logits differ, by
    at most 3e-8), so no two runs of PV-RCNN agree bit for bit behind it, by hand or through the model: there the end
    is compared under the bar of Case.close."""
    kind, model, frames, dets = case.kind, case.model, case.frames, case.dets
    want, bd, first = by_hand(model, frames)
    assert len(dets) == len(want) == 2
    for k in ("head_cls", "head_box", "rois", "roi_scores", "pooled"):
        assert torch.equal(case.seen[k], first[k]), k
    for b, (d, w) in enumerate(zip(dets, want)):
        if kind == "voxel":
            assert same(d, w)
        case.close(d, w, f"by hand, frame {b}")
        assert d["box3d_lidar"].shape[1] == 7 and d["scores"].shape[0] == d["label_preds"].shape[0] > 1
        assert bool((d["scores"] >= model.post_process_cfg["score_thresh"]).all())
        assert bool(torch.isfinite(d["box3d_lidar"]).all())
    anchors = {"voxel": 512, "pv": 1536}[kind]
    assert bd["spatial_features_2d"].shape == (2, {"voxel": 256, "pv": 512}[kind], 16, 16)
    assert bd["rois"].shape == (2, 100, 7) and model.dense_head.anchors.numel() == anchors * 7
    assert all(int(bd["multi_scale_3d_features"][f"x_conv{k}"].features.shape[0]) > 50 for k in (1, 2, 3, 4))
    if kind == "pv":
        assert set(dets[0]["label_preds"].tolist()) | set(dets[1]["label_preds"].tolist()) <= {1, 2, 3}
        assert bool(bd["sparse_rows_frame_contiguous"])


def test_frames_do_not_see_each_other(case):
    """The frames swapped, and each alone.  The first stage and the proposals are torch.equal per frame.  The RoI
    heads' fully connected stacks (VoxelRCNNHead's nn.Linear over [B * R, 20 736], PVRCNNHead's Conv1d over
    [B * R, 27 648, 1]) and the unfused set abstraction's torch MLPs are GEMMs of the BLAS library, which sums in
    another order for another number of rows (B = 1 against B = 2) and, for the Conv1d, from run to run: behind them
    the frames are compared under the bar, with equal labels and counts."""
    dets = case.dets
    swapped, seen = case.run(case.frames[::-1])
    for k in ("head_cls", "head_box", "rois", "roi_scores"):
        assert torch.equal(seen[k][1], case.seen[k][0]) and torch.equal(seen[k][0], case.seen[k][1]), k
    case.close(swapped[1], dets[0], "swapped, frame 0")
    case.close(swapped[0], dets[1], "swapped, frame 1")
    for b in range(2):
        alone, seen = case.run([case.frames[b]])
        for k in ("head_cls", "head_box", "rois", "roi_scores"):
            assert torch.equal(seen[k][0], case.seen[k][b]), (k, b)
        case.close(alone[0], dets[b], f"alone, frame {b}")


def test_padded_form_and_the_bridge(case):
    from paddle3d_amd.kitti_bridge import detections_to_kitti_annos

    model, dets = case.model, case.dets
    (boxes, scores, labels, count), _ = case.run(case.frames, padded=True)
    assert boxes.shape == (2, 500, 7) and count.tolist() == [len(d["scores"]) for d in dets]
    for b, d in enumerate(dets):
        n = len(d["scores"])
        case.close({"box3d_lidar": boxes[b, :n], "scores": scores[b, :n], "label_preds": labels[b, :n]}, d, "padded")
        assert not boxes[b, n:].any()
    calib = tuple(np.asarray(c, np.float64) for c in (np.eye(3, 4),) * 4 + (np.eye(3), np.eye(3, 4)))
    names = model.dense_head.class_names
    with np.errstate(all="ignore"):
        annos = detections_to_kitti_annos(ts.to_kitti_detections(dets), [calib] * 2, names)
    for a, d in zip(annos, dets):
        assert len(a["name"]) == len(d["scores"]) and set(a["name"].tolist()) <= set(names)
        assert a["dimensions"].shape == (len(d["scores"]), 3) and np.array_equal(a["score"], d["scores"].cpu().numpy())


def test_empty_and_out_of_range_frames(case):
    """A frame whose points all lie outside the range, and (Voxel R-CNN; PV-RCNN's keypoint sampling divides by the
    frame's point count, in the reference as here) a frame without a point, next to a full frame."""
    from paddle3d_amd.kitti_bridge import detections_to_kitti_annos

    kind, model, frames, dets = case.kind, case.model, case.frames, case.dets
    outside = frames[1].clone()
    outside[:, 0] += 100.0  # no voxel; PV-RCNN's keypoints far from every voxel
    others = [outside] if kind == "pv" else [outside, frames[0][:0]]
    for k, other in enumerate(others):
        got, seen = case.run([frames[0], other])
        for key in ("head_cls", "head_box", "rois", "roi_scores"):
            assert torch.equal(seen[key][0], case.seen[key][0]), key  # the neighbour does not change
        case.close(got[0], dets[0], f"next to an empty frame ({k})")
        d = got[1]
        assert d["box3d_lidar"].shape[1] == 7 and len(d["scores"]) == len(d["label_preds"]) >= 1
        assert bool(torch.isfinite(d["box3d_lidar"]).all()) and bool(torch.isfinite(d["scores"]).all())
        assert bool(((d["scores"] >= model.post_process_cfg["score_thresh"]) | (d["scores"] == -1)).all())
    # nothing above the threshold: the reference's box_empty row for every frame, which the bridge drops
    keep = model.post_process_cfg
    try:
        model.post_process_cfg = dict(keep, score_thresh=2.0)
        got = model([frames[0], others[-1]])
    finally:
        model.post_process_cfg = keep
    calib = tuple(np.asarray(c, np.float64) for c in (np.eye(3, 4),) * 4 + (np.eye(3), np.eye(3, 4)))
    for d in got:
        assert d["box3d_lidar"].shape == (1, 7) and not d["box3d_lidar"].any()
        assert d["scores"].tolist() == [-1.0] and d["label_preds"].tolist() == [-1]
    annos = detections_to_kitti_annos(ts.to_kitti_detections(got), [calib] * 2, model.dense_head.class_names)
    assert all(len(a["name"]) == 0 for a in annos)


def test_host_syncs_of_a_forward(case):
    """Two: SparseNet3D's exact plan and post_processing's read of the counts; the padded form leaves the plan's."""
    model, frames = case.model, case.frames

    def syncs(**kw):
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                model(frames, **kw)
            finally:
                torch.cuda.set_sync_debug_mode(0)
        torch.cuda.synchronize()
        return sum("synchroniz" in str(w.message).lower() for w in seen)

    assert (syncs(), syncs(padded=True)) == (2, 1)
