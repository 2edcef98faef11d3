"""Host side of BEVDet4D's CenterHead post-processing: the reference's `preds_dicts` in, its
`[[bboxes, scores, labels], ...]` out, every step on the device (ops/bevdet_postprocess.py) and one synchronisation
per call (the row counts).

Reference: CenterHeadMatch.get_bboxes (paddle3d/models/heads/dense_heads/bevdet_centerhead.py:669-783) with its
CenterPointBBoxCoder (:1049-1214); config configs/bevdet/bevdet4d_r50_depth_nuscenes.yml:205-273.  Equal scores are
ordered by ascending (class, cell) where the reference leaves ties open."""
from __future__ import annotations

from .ops import bevdet_postprocess as _bp

__all__ = ["CenterPointBBoxCoder", "get_bboxes", "get_bboxes_device", "BEVDET4D_TASKS", "BEVDET4D_BBOX_CODER",
           "BEVDET4D_TEST_CFG"]

BEVDET4D_TASKS = [dict(num_class=1, class_names=["car"]),
                  dict(num_class=2, class_names=["truck", "construction_vehicle"]),
                  dict(num_class=2, class_names=["bus", "trailer"]),
                  dict(num_class=1, class_names=["barrier"]),
                  dict(num_class=2, class_names=["motorcycle", "bicycle"]),
                  dict(num_class=2, class_names=["pedestrian", "traffic_cone"])]

BEVDET4D_BBOX_CODER = dict(pc_range=[-51.2, -51.2], post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
                           max_num=500, score_threshold=0.1, out_size_factor=8, voxel_size=[0.1, 0.1], code_size=9)

BEVDET4D_TEST_CFG = dict(
    pc_range=[-51.2, -51.2],
    post_center_limit_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
    max_per_img=500,
    max_pool_nms=False,
    min_radius=[4, 12, 10, 1, 0.85, 0.175],
    score_threshold=0.1,
    out_size_factor=8,
    voxel_size=[0.1, 0.1],
    pre_max_size=1000,
    post_max_size=83,
    nms_type=["rotate", "rotate", "rotate", "circle", "rotate", "rotate"],
    nms_thr=[0.2, 0.2, 0.2, 0.2, 0.2, 0.5],
    nms_rescale_factor=[1.0, [0.7, 0.7], [0.4, 0.55], 1.1, [1.0, 1.0], [4.5, 9.0]],
)


class CenterPointBBoxCoder:
    """The coder's configuration (bevdet_centerhead.py:1054-1069); decoding runs inside the device operator."""

    def __init__(self, pc_range, out_size_factor, voxel_size, post_center_range=None, max_num=100,
                 score_threshold=None, code_size=9):
        self.pc_range = pc_range
        self.out_size_factor = out_size_factor
        self.voxel_size = voxel_size
        self.post_center_range = post_center_range
        self.max_num = max_num
        self.score_threshold = score_threshold
        self.code_size = code_size


def _per_task(v, n):
    return list(v) if isinstance(v, (list, tuple)) else [v] * n


def get_bboxes_device(preds_dicts, test_cfg, bbox_coder, num_classes, norm_bbox=True):
    """get_bboxes without the synchronisation: padded device tensors + int32 counts [B]."""
    n = len(preds_dicts)
    if len(num_classes) != n:
        raise RuntimeError("bevdet get_bboxes: one num_classes entry per task")
    if any("vel" not in p or p["vel"] is None for p in preds_dicts):
        raise RuntimeError("bevdet get_bboxes: only the velocity form is supported "
                           "(the reference's merge builds paddle.empty((0, 9)))")
    if bbox_coder.post_center_range is None:
        raise NotImplementedError("Need to reorganize output as a batch, only support post_center_range is not None "
                                  "for now!")  # decode :1208-1211
    for p, c in zip(preds_dicts, num_classes):
        if int(p["heatmap"].shape[1]) != int(c):
            raise RuntimeError("bevdet get_bboxes: heatmap channels differ from num_classes")
    heads = [[p[k] for p in preds_dicts] for k in ("heatmap", "reg", "height", "dim", "rot", "vel")]
    nms_type = _per_task(test_cfg.get("nms_type"), n)
    factor = test_cfg.get("nms_rescale_factor", [1.0] * n)
    return _bp.bevdet_postprocess_device(
        *heads, nms_type=nms_type, nms_thr=_per_task(test_cfg["nms_thr"], n),
        min_radius=_per_task(test_cfg.get("min_radius", [0.0] * n), n), rescale_factors=factor,
        max_num=bbox_coder.max_num, pre_max_size=test_cfg["pre_max_size"], post_max_size=test_cfg["post_max_size"],
        score_threshold=bbox_coder.score_threshold, post_center_range=bbox_coder.post_center_range,
        post_center_limit_range=test_cfg.get("post_center_limit_range"), pc_range=bbox_coder.pc_range,
        voxel_size=bbox_coder.voxel_size, out_size_factor=bbox_coder.out_size_factor, norm_bbox=norm_bbox)


def get_bboxes(preds_dicts, test_cfg, bbox_coder, num_classes, norm_bbox=True):
    """preds_dicts: one dict per task with `heatmap, reg, height, dim, rot, vel` [B, c, 128, 128] GPU tensors.
    Returns [[bboxes [n, 9], scores [n], labels int32 [n]], ...] per frame (device tensors)."""
    b, s, l, cnt = get_bboxes_device(preds_dicts, test_cfg, bbox_coder, num_classes, norm_bbox)
    counts = cnt.tolist()
    return [[b[i, :k], s[i, :k], l[i, :k]] for i, k in enumerate(counts)]
