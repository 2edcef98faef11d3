"""BEVDet4D CenterHead post-processing and `circle_nms` on the device.

bevdet_postprocess_device(heatmap, reg, height, dim, rot, vel, ...) -> padded (bboxes [B, T*post, 9], scores, labels
    int32) + device int32 counts [B]; no host synchronisation.
circle_nms(dets, thresh) -> list of kept indices (the signature and return of paddle3d/geometries/bbox.py:450-474).

Reference: CenterHeadMatch.get_bboxes, paddle3d/models/heads/dense_heads/bevdet_centerhead.py:669-783, with
CenterPointBBoxCoder.decode (:1119-1214), get_task_detections (:785-906), nms_bev (:939-968) and _circle_nms
(:912-921).  The host-side wrapper that takes the reference's preds_dicts is paddle3d_amd/bevdet_head.py.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._common import check, host_f32, host_i32, lib, ptr, require_gpu, stream_ptr, workspace

__all__ = ["bevdet_postprocess_device", "circle_nms", "circle_nms_device"]

_OP = "bevdet postprocess"


def _ptr_array(tensors):
    return C.cast((C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors]), C.c_void_p)


def bevdet_postprocess_device(heatmap, reg, height, dim, rot, vel, nms_type, nms_thr, min_radius, rescale_factors,
                              max_num, pre_max_size, post_max_size, score_threshold, post_center_range,
                              post_center_limit_range, pc_range, voxel_size, out_size_factor, norm_bbox=True):
    """Every head argument is a list with one [B, c, H, W] fp32 GPU tensor per task.  nms_type: list of 'rotate' /
    'circle'; nms_thr, min_radius: one value per task; rescale_factors: per task a scalar or a per-class list (the
    test_cfg's nms_rescale_factor).  score_threshold None or 0: no score mask.  post_center_limit_range None or []:
    no post-NMS mask.  Returns (bboxes [B, T * post_max_size, 9], scores [B, R], labels int32 [B, R], count int32
    [B]); rows >= count are zero."""
    if vel is None:
        raise RuntimeError("bevdet postprocess: `vel` is required (the reference's merge builds 9-column boxes)")
    groups = (heatmap, reg, height, dim, rot, vel)
    t_n = len(heatmap)
    if t_n == 0 or any(len(g) != t_n for g in groups):
        raise RuntimeError("bevdet postprocess: every head list needs one tensor per task")
    lists = [[require_gpu(t, _OP) for t in g] for g in groups]
    hm0 = lists[0][0]
    batch, h, w = int(hm0.shape[0]), int(hm0.shape[2]), int(hm0.shape[3])
    want = dict(reg=2, height=1, dim=3, rot=2, vel=2)
    for g, (name, ch) in zip(lists[1:], want.items()):
        for t in g:
            if tuple(t.shape) != (batch, ch, h, w):
                raise RuntimeError(f"bevdet postprocess: {name} must be [{batch}, {ch}, {h}, {w}], got {tuple(t.shape)}")
    for t in lists[0]:
        if t.dim() != 4 or int(t.shape[0]) != batch or tuple(t.shape[2:]) != (h, w):
            raise RuntimeError("bevdet postprocess: heatmaps of one batch and map size")
    if h * w > 1 << 24:
        raise RuntimeError(f"bevdet postprocess: H*W = {h * w} > 2^24 (the reference's float ind / W is inexact)")
    if int(max_num) > h * w:
        # paddle.topk(scores.reshape((batch, cat, -1)), K) with K > H*W raises in the reference (_topk :1088)
        raise RuntimeError(f"bevdet postprocess: max_num {max_num} > H*W = {h * w}")
    ncls = host_i32([int(t.shape[1]) for t in lists[0]])
    types = []
    for v in nms_type:
        if v not in ("rotate", "circle"):
            raise RuntimeError(f"bevdet postprocess: nms_type {v!r} (rotate / circle)")
        types.append(1 if v == "circle" else 0)
    factors = []
    for t in range(t_n):
        f = rescale_factors[t]
        per = [float(f)] * int(ncls[t]) if not isinstance(f, (list, tuple)) else \
            [float(f[k]) if k < len(f) else 1.0 for k in range(int(ncls[t]))]
        factors.extend(per)
    types = host_i32(types)
    thr = host_f32(nms_thr)
    rad = np.ascontiguousarray(np.asarray(min_radius, np.float64).reshape(-1))
    fac = host_f32(factors)
    if len(types) != t_n or thr.size != t_n or rad.size != t_n:
        raise RuntimeError("bevdet postprocess: nms_type / nms_thr / min_radius need one entry per task")
    pcr = host_f32(post_center_range, 6)
    lim = host_f32(post_center_limit_range, 6) if post_center_limit_range is not None and \
        len(post_center_limit_range) > 0 else None
    pr, vs = host_f32(pc_range)[:2].copy(), host_f32(voxel_size)[:2].copy()
    dev = hm0.device
    rows = t_n * int(post_max_size)
    out_b = torch.empty((batch, rows, 9), dtype=torch.float32, device=dev)
    out_s = torch.empty((batch, rows), dtype=torch.float32, device=dev)
    out_l = torch.empty((batch, rows), dtype=torch.int32, device=dev)
    out_n = torch.empty((batch,), dtype=torch.int32, device=dev)
    L = lib()
    ws_bytes = L.pd3_bevdet_postprocess_workspace(batch, t_n, ptr(ncls), h, w, int(max_num))
    ws = workspace(ws_bytes, dev)
    check(L.pd3_bevdet_postprocess(*[_ptr_array(g) for g in lists], batch, t_n, ptr(ncls), h, w, ptr(types),
                                   ptr(thr), ptr(rad), ptr(fac), int(max_num), int(pre_max_size),
                                   int(post_max_size), C.c_float(float(score_threshold or 0.0)),
                                   int(bool(norm_bbox)), ptr(pcr), ptr(lim), ptr(pr), ptr(vs),
                                   C.c_float(float(out_size_factor)), ptr(out_b), ptr(out_s), ptr(out_l),
                                   ptr(out_n), ptr(ws), ws.numel(), stream_ptr(dev)), _OP)
    return out_b, out_s, out_l, out_n


def circle_nms_device(dets, thresh):
    """dets [N, 3] fp32 GPU tensor (x, y, score) -> (keep int32 [N] device, num int32 [1] device), no sync."""
    dets = require_gpu(dets, "circle_nms")
    if dets.dim() != 2 or int(dets.shape[1]) != 3:
        raise RuntimeError(f"circle_nms: dets must be [N, 3], got {tuple(dets.shape)}")
    n = int(dets.shape[0])
    dev = dets.device
    keep = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
    num = torch.empty((1,), dtype=torch.int32, device=dev)
    L = lib()
    ws = workspace(L.pd3_circle_nms_workspace(n) if n else 0, dev)
    check(L.pd3_circle_nms(ptr(dets), n, C.c_double(float(thresh)), ptr(keep), ptr(num), ptr(ws), ws.numel(),
                           stream_ptr(dev)), "circle_nms")
    return keep, num


def circle_nms(dets, thresh):
    """bbox.circle_nms(dets, thresh): kept indices (a list of ints, highest score first)."""
    keep, num = circle_nms_device(dets, thresh)
    return keep[: int(num.item())].tolist()
