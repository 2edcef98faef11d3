"""DD3D's FCOS heads and post-processing at inference on the device (csrc/dd3d.hip, C ABI pd3_dd3d_head_forward /
pd3_dd3d_post_process, declared in include/paddle3d_amd.h); the arithmetic order and the three definitions (tie
order of the selection, no renormalisation of the egocentric quaternion, the NMS semantics) are stated in that file's
header and restated in tests/golden/dd3d_numpy.py.

Reference: paddle3d/models/heads/fcos_heads/fcos2d_head.py:160-186, :334-503 (FCOS2DHead.forward, FCOS2DInference),
fcos3d_head.py:33-108, :268-296, :519-639 (predictions_to_boxes3d, FCOS3DHead.forward, FCOS3DInference),
models/detection/dd3d/dd3d.py:144-176, :183-212 (the eval branch, compute_locations), utils/transform.py:167-246.

dd3d_head_forward(logits, centerness, box2d_feat, box3d_feat, strides, ...)
    the LAZY form: dense class logits and centerness per level, the box2d and box3d towers' outputs per level; the 4 + 11
    predictor channels of an entry (3x3 convolutions) are evaluated at the selected (pixel, class) entries only.
dd3d_post_process(logits, centerness, box2d_reg, box3d, strides, ...)
    the same selection, decode and tail from the reference's dense head outputs.
Both return (rows [B, R, 20], counts int32 [B]) on the device -- pred_boxes 4, scores, scores_3d, pred_classes,
fpn_levels, locations 2, pred_boxes3d 10, in NMS order, zero past min(counts[b], R); counts[b] is the number of rows the
reference keeps (a tie at the post-NMS cut can make it exceed R = post_nms_topk, or levels * pre_nms_topk when
post_nms_topk <= 0) -- or None when the kernels do not take the shape (`dd3d_supported`).  float32 only.  Nothing here
synchronises with the host; the kernels run on the current stream.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._common import check, gpu_tensor, lib, nchw_pitch, ptr, stream_ptr, workspace

__all__ = ["dd3d_supported", "dd3d_head_forward", "dd3d_post_process", "flags_of", "MAX_K", "MAX_LEVELS", "ROW",
           "DEFAULTS"]

_OP = "dd3d"
_UNSUPPORTED = -3
MAX_K, MAX_LEVELS, MAX_CLASSES, MAX_CHANNELS, ROW = 1024, 8, 16, 512, 20
# FCOS2DInference's and FCOS3DInference's defaults, and DD3D's feature_locations_offset
DEFAULTS = dict(thresh_with_ctr=True, pre_nms_thresh=0.05, pre_nms_topk=1000, post_nms_topk=100, nms_thresh=0.75,
                nms_categories=5, offset="none", min_depth=0.1, max_depth=80.0, predict_allocentric_rot=True,
                scale_depth_by_focal_lengths=True, scale_depth_by_focal_lengths_factor=500.0, predict_distance=False)


def dd3d_supported(shapes, num_classes, pre_nms_topk, nms_thresh, channels=None):
    """The kernels' shape predicate.  shapes: (H, W) per level; channels=None: the from-maps form."""
    if channels is not None and not 1 <= channels <= MAX_CHANNELS:
        return False
    return (1 <= len(shapes) <= MAX_LEVELS and 1 <= num_classes <= MAX_CLASSES and 1 <= pre_nms_topk <= MAX_K and
            nms_thresh > 0 and all(1 <= h <= 65535 and 1 <= w <= 65535 and num_classes * h * w < 2 ** 30
                                   for h, w in shapes))


def flags_of(cfg):
    if cfg["offset"] not in ("none", "half"):
        raise ValueError(f"{_OP}: feature_locations_offset must be 'none' or 'half', got {cfg['offset']!r}")
    return (1 * bool(cfg["thresh_with_ctr"]) | 2 * (cfg["offset"] == "half") | 4 * bool(cfg["scale_depth_by_focal_lengths"]) |
            8 * bool(cfg["predict_allocentric_rot"]) | 16 * bool(cfg["predict_distance"]))


def _pointers(tensors):
    """A host array of device pointers (kept alive by the caller's list of tensors)."""
    return np.ascontiguousarray(np.array([t.data_ptr() for t in tensors], np.uint64))


def _strided(what, t, dev, shape):
    """nchw_pitch of a checked float32 map of `shape` on `dev`."""
    gpu_tensor(_OP, what, t, dtype=None, contiguous=False)
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or t.device != dev:
        raise RuntimeError(f"{_OP}: {what} must be float32 {tuple(shape)} on {dev}, got {t.dtype} {tuple(t.shape)} on "
                           f"{t.device}")
    return nchw_pitch(t)


def _config(cfg):
    full = dict(DEFAULTS)
    unknown = set(cfg) - set(full)
    if unknown:
        raise TypeError(f"{_OP}: unknown options {sorted(unknown)}")
    full.update(cfg)
    return full


def _tail(cfg):
    return (int(cfg["pre_nms_topk"]), int(cfg["post_nms_topk"]), int(cfg["nms_categories"]), flags_of(cfg),
            C.c_float(cfg["pre_nms_thresh"]), C.c_float(cfg["nms_thresh"]), C.c_float(cfg["min_depth"]),
            C.c_float(cfg["max_depth"]), C.c_float(cfg["scale_depth_by_focal_lengths_factor"]))


def _dense(logits, centerness, strides):
    if not (len(logits) == len(centerness) == len(strides) >= 1):
        raise RuntimeError(f"{_OP}: one logits map, one centerness map and one stride per level")
    logits = [gpu_tensor(_OP, f"logits[{i}]", t) for i, t in enumerate(logits)]
    dev = logits[0].device
    b, nc = (int(s) for s in logits[0].shape[:2])
    shapes = []
    for i, t in enumerate(logits):
        if t.dim() != 4 or tuple(t.shape[:2]) != (b, nc) or t.device != dev:
            raise RuntimeError(f"{_OP}: logits[{i}] must be [{b}, {nc}, H, W] on {dev}, got {tuple(t.shape)}")
        shapes.append((int(t.shape[2]), int(t.shape[3])))
    centerness = [gpu_tensor(_OP, f"centerness[{i}]", t, dev=dev, shape=(b, 1, *shapes[i]))
                  for i, t in enumerate(centerness)]
    return logits, centerness, dev, b, nc, shapes


def _outputs(L, dev, b, table, nc, cfg):
    levels = len(table)
    cap = levels * int(cfg["pre_nms_topk"])
    r = int(cfg["post_nms_topk"]) if int(cfg["post_nms_topk"]) > 0 else cap
    rows = torch.empty((b, r, ROW), dtype=torch.float32, device=dev)
    counts = torch.empty((b,), dtype=torch.int32, device=dev)
    ws = workspace(L.pd3_dd3d_workspace(max(b, 1), levels, ptr(table), nc, int(cfg["pre_nms_topk"])), dev)
    return rows, counts, ws


def dd3d_head_forward(logits, centerness, box2d_feat, box3d_feat, strides, box2d_weight, box2d_bias, box3d_weight,
                      box3d_bias, scales, intrinsics, canon_box_sizes, **cfg):
    """logits / centerness / box2d_feat / box3d_feat: lists with one [B, nc | 1 | C | C, H, W] tensor per level (tower
    outputs may be row-padded views); box3d_feat None: only_box2d.  box2d_weight [4, C, 3, 3], box2d_bias [4];
    box3d_weight [wl, 11 * ncp, C, 3, 3], box3d_bias [wl, 11 * ncp] (rows quat, ctr, depth, size, conf; wl = 1 or the
    number of levels, ncp = nc or 1); scales [levels, 6] (box2d_reg, proj_ctr, size, conf, depth scale, depth offset);
    intrinsics [B, 3, 3]; canon_box_sizes [>= nc, 3]; options: DEFAULTS."""
    cfg = _config(cfg)
    logits, centerness, dev, b, nc, shapes = _dense(logits, centerness, strides)
    levels = len(shapes)
    c = int(box2d_weight.shape[1])
    if not dd3d_supported(shapes, nc, int(cfg["pre_nms_topk"]), cfg["nms_thresh"], c):
        return None
    has3d = box3d_feat is not None
    table = np.zeros((levels, 5), np.int64)
    f2d, f3d = [], []
    for i, (h, w) in enumerate(shapes):
        t2, sb, pitch = _strided(f"box2d_feat[{i}]", box2d_feat[i], dev, (b, c, h, w))
        if has3d:
            t3, sb3, pitch3 = _strided(f"box3d_feat[{i}]", box3d_feat[i], dev, (b, c, h, w))
            if (sb3, pitch3) != (sb, pitch):
                t2, t3, sb, pitch = t2.contiguous(), t3.contiguous(), c * h * w, w
            f3d.append(t3)
        f2d.append(t2)
        table[i] = (h, w, int(strides[i]), pitch, sb)
    w2 = gpu_tensor(_OP, "box2d_weight", box2d_weight, dev=dev, shape=(4, c, 3, 3))
    b2 = gpu_tensor(_OP, "box2d_bias", box2d_bias, dev=dev, shape=(4,))
    sc = gpu_tensor(_OP, "scales", scales, dev=dev, shape=(levels, 6))
    w3 = b3 = K = canon = None
    wl = ncp = 1
    if has3d:
        wl, rows3 = int(box3d_weight.shape[0]), int(box3d_weight.shape[1])
        ncp = rows3 // 11
        if wl not in (1, levels) or rows3 != 11 * ncp or ncp not in (1, nc):
            raise RuntimeError(f"{_OP}: box3d_weight must be [1 | levels, 11 * (1 | nc), C, 3, 3], got "
                               f"{tuple(box3d_weight.shape)}")
        w3 = gpu_tensor(_OP, "box3d_weight", box3d_weight, dev=dev, shape=(wl, rows3, c, 3, 3))
        b3 = gpu_tensor(_OP, "box3d_bias", box3d_bias, dev=dev, shape=(wl, rows3))
        K = gpu_tensor(_OP, "intrinsics", intrinsics, dev=dev, shape=(b, 3, 3))
        canon = gpu_tensor(_OP, "canon_box_sizes", canon_box_sizes[:nc], dev=dev, shape=(nc, 3))
    L = lib()
    rows, counts, ws = _outputs(L, dev, b, table, nc, cfg)
    arrays = [_pointers(x) for x in (logits, centerness, f2d)] + [_pointers(f3d) if has3d else None]
    st = L.pd3_dd3d_head_forward(*(ptr(a) for a in arrays), ptr(table), ptr(w2), ptr(b2), ptr(w3), ptr(b3), ptr(sc),
                                 ptr(K), ptr(canon), b, levels, c, nc, ncp, wl, *_tail(cfg), ptr(rows), ptr(counts),
                                 ptr(ws), ws.numel(), stream_ptr(dev))
    if st == _UNSUPPORTED:
        return None
    check(st, f"{_OP}.dd3d_head_forward")
    return rows, counts


def dd3d_post_process(logits, centerness, box2d_reg, box3d, strides, intrinsics, canon_box_sizes, **cfg):
    """logits, centerness, box2d_reg: FCOS2DHead's outputs per level; box3d: None (only_box2d) or FCOS3DHead's five
    lists (quat, ctr, depth, size, conf), each [B, k * ncp, H, W] per level with ncp = nc or 1; options: DEFAULTS."""
    cfg = _config(cfg)
    logits, centerness, dev, b, nc, shapes = _dense(logits, centerness, strides)
    levels = len(shapes)
    if not dd3d_supported(shapes, nc, int(cfg["pre_nms_topk"]), cfg["nms_thresh"]):
        return None
    reg = [gpu_tensor(_OP, f"box2d_reg[{i}]", t, dev=dev, shape=(b, 4, *shapes[i])) for i, t in enumerate(box2d_reg)]
    table = np.zeros((levels, 5), np.int64)
    for i, (h, w) in enumerate(shapes):
        table[i] = (h, w, int(strides[i]), w, 0)
    maps3d, K, canon, ncp = [None] * 5, None, None, 1
    if box3d is not None:
        ncp = int(box3d[2][0].shape[1])
        if ncp not in (1, nc):
            raise RuntimeError(f"{_OP}: the 3D maps must have 1 or {nc} class rows, got {ncp}")
        maps3d = [[gpu_tensor(_OP, f"{name}[{i}]", t, dev=dev, shape=(b, k * ncp, *shapes[i]))
                   for i, t in enumerate(m)]
                  for name, k, m in zip(("quat", "ctr", "depth", "size", "conf"), (4, 2, 1, 3, 1), box3d)]
        K = gpu_tensor(_OP, "intrinsics", intrinsics, dev=dev, shape=(b, 3, 3))
        canon = gpu_tensor(_OP, "canon_box_sizes", canon_box_sizes[:nc], dev=dev, shape=(nc, 3))
    L = lib()
    rows, counts, ws = _outputs(L, dev, b, table, nc, cfg)
    arrays = [_pointers(x) for x in (logits, centerness, reg)] + [None if m is None else _pointers(m) for m in maps3d]
    st = L.pd3_dd3d_post_process(*(ptr(a) for a in arrays), ptr(table), ptr(K), ptr(canon), b, levels, nc, ncp,
                                 *_tail(cfg), ptr(rows), ptr(counts), ptr(ws), ws.numel(), stream_ptr(dev))
    if st == _UNSUPPORTED:
        return None
    check(st, f"{_OP}.dd3d_post_process")
    return rows, counts
