"""Voxel R-CNN's RoI head on the device (csrc/roi_head.hip, contract in include/paddle3d_amd.h).  Inference only.

voxel_pool_supported(c1, nsample)
    whether voxel_pool takes the shape (C1 in {16, 32, 64}, nsample <= 64).
voxel_pool(new_xyz, new_coords, xyz, point_indices, features_in, w_pos, pos_scale, pos_shift, max_range, radius,
           nsample, pool_method)
    new_xyz [M, 3], new_coords [M, 4] int32 (b, z, y, x), xyz [N, 3], point_indices [B, Z, Y, X] int32, features_in
    [N, C1], w_pos [C1, 3], pos_scale / pos_shift [C1] -> pooled [M, C1]: the inner part of
    NeighborVoxelSAModuleMSG.forward (voxel_pool_modules.py:123-155) from the voxel query to the pool.
roi_grid_points(rois, grid_size, point_cloud_range, voxel_size, strides)
    rois [B, R, 7] -> (roi_grid_xyz [B * R * G^3, 3], [coords [B * R * G^3, 4] int32 (b, x, y, z) per stride]).
rcnn_decode_boxes(rois, box_preds)
    rois [B, R, 7], box_preds [B * R, 7] or [B, R, 7] -> decoded boxes [B, R, 7] (roi_head_base.py:293-322).
class_agnostic_nms(box_preds, cls_preds, nms_config, score_thresh=None, apply_sigmoid=False, labels=None)
    box_preds [B, A, 7], cls_preds [B, A, K], labels [B, A] int64 or None -> (boxes [B, post, 7], scores [B, post],
    labels [B, post] int64, count [B] int32), zero padded (model_nms_utils.py:20-66 for every frame in one call).

float32 only, on the GPU.  Nothing here synchronises with the host.  A shape the library does not take raises.
"""
from __future__ import annotations

import math

import torch

from ._common import check, gpu_rows, gpu_tensor, host_f32, host_i32, lib, ptr, stream_ptr, workspace

__all__ = ["voxel_pool_supported", "voxel_pool", "roi_grid_points", "rcnn_decode_boxes", "class_agnostic_nms"]

POOLS = {"max_pool": 0, "avg_pool": 1}


def _same_device(op, *ts):
    dev = ts[0].device
    for t in ts[1:]:
        if t.device != dev:
            raise RuntimeError(f"{op}: tensors on {dev} and {t.device}")


def voxel_pool_supported(c1, nsample):
    return int(c1) in (16, 32, 64) and 1 <= int(nsample) <= 64


def voxel_pool(new_xyz, new_coords, xyz, point_indices, features_in, w_pos, pos_scale, pos_shift, max_range, radius,
               nsample, pool_method="max_pool"):
    op = "voxel_pool"
    if pool_method not in POOLS:
        raise NotImplementedError(pool_method)
    q = gpu_rows(op, "new_xyz", new_xyz, 3)
    co = gpu_rows(op, "new_coords", new_coords, 4, torch.int32)
    p = gpu_rows(op, "xyz", xyz, 3)
    f = gpu_rows(op, "features_in", features_in, None)
    gpu_tensor(op, "point_indices", point_indices, torch.int32, contiguous=False)
    if point_indices.dim() != 4:
        raise RuntimeError(f"{op}: point_indices must be [B, Z, Y, X], got {tuple(point_indices.shape)}")
    pi = point_indices.contiguous()
    M, N, C1 = int(q.shape[0]), int(p.shape[0]), int(f.shape[1])
    if int(co.shape[0]) != M:
        raise RuntimeError(f"{op}: new_coords has {int(co.shape[0])} rows, new_xyz {M}")
    if int(f.shape[0]) != N:
        raise RuntimeError(f"{op}: features_in has {int(f.shape[0])} rows, xyz {N}")
    w = gpu_rows(op, "w_pos", w_pos, 3)
    sc, sh = gpu_tensor(op, "pos_scale", pos_scale), gpu_tensor(op, "pos_shift", pos_shift)
    if int(w.shape[0]) != C1 or tuple(sc.shape) != (C1,) or tuple(sh.shape) != (C1,):
        raise RuntimeError(f"{op}: w_pos {tuple(w.shape)}, pos_scale {tuple(sc.shape)}, pos_shift {tuple(sh.shape)} "
                           f"for {C1} channels")
    _same_device(op, q, co, p, f, pi, w, sc, sh)
    S = int(nsample)
    if S < 1:
        raise RuntimeError(f"{op}: nsample must be >= 1, got {S}")
    B, Z, Y, X = (int(s) for s in pi.shape)
    if B == 0 and M > 0:
        raise RuntimeError(f"{op}: {M} rows but no frame")
    zr, yr, xr = (int(v) for v in max_range)
    out = torch.empty((M, C1), dtype=torch.float32, device=q.device)
    check(lib().pd3_voxel_pool(ptr(q), ptr(p), ptr(co), ptr(pi), ptr(f), ptr(w), ptr(sc), ptr(sh), M, N, B, Z, Y, X,
                               C1, float(radius), S, zr, yr, xr, POOLS[pool_method], ptr(out),
                               stream_ptr(q.device)), op)
    return out


def roi_grid_points(rois, grid_size, point_cloud_range, voxel_size, strides):
    op = "roi_grid_points"
    gpu_tensor(op, "rois", rois, contiguous=False)
    if rois.dim() != 3 or int(rois.shape[2]) != 7:
        raise RuntimeError(f"{op}: rois must be [B, R, 7], got {tuple(rois.shape)}")
    r = rois.contiguous()
    B, R, G = int(r.shape[0]), int(r.shape[1]), int(grid_size)
    strides = [int(s) for s in strides]
    if G < 1 or len(strides) > 4 or any(s < 1 for s in strides):
        raise RuntimeError(f"{op}: grid_size {G}, strides {strides} (at most 4, each >= 1)")
    lo, vs = host_f32(list(point_cloud_range)[:3], 3), host_f32(voxel_size, 3)
    st = host_i32(strides if strides else [1])
    total = B * R * G ** 3
    xyz = torch.empty((total, 3), dtype=torch.float32, device=r.device)
    coords = torch.empty((len(strides), total, 4), dtype=torch.int32, device=r.device)
    if total:
        check(lib().pd3_roi_grid_points(ptr(r), B * R, max(R, 1), G, ptr(lo), ptr(vs), ptr(st), len(strides), ptr(xyz),
                                        ptr(coords), stream_ptr(r.device)), op)
    return xyz, [coords[k] for k in range(len(strides))]


def rcnn_decode_boxes(rois, box_preds):
    op = "rcnn_decode_boxes"
    gpu_tensor(op, "rois", rois, contiguous=False)
    gpu_tensor(op, "box_preds", box_preds, contiguous=False)
    if rois.dim() != 3 or int(rois.shape[2]) != 7:
        raise RuntimeError(f"{op}: rois must be [B, R, 7], got {tuple(rois.shape)}")
    n = int(rois.shape[0]) * int(rois.shape[1])
    if box_preds.numel() != n * 7 or int(box_preds.shape[-1]) != 7:
        raise RuntimeError(f"{op}: box_preds {tuple(box_preds.shape)} for rois {tuple(rois.shape)}")
    _same_device(op, rois, box_preds)
    r, e = rois.contiguous(), box_preds.contiguous()
    out = torch.empty_like(r)
    if n:
        check(lib().pd3_rcnn_decode_boxes(ptr(r), ptr(e), n, ptr(out), stream_ptr(r.device)), op)
    return out


def class_agnostic_nms(box_preds, cls_preds, nms_config, score_thresh=None, apply_sigmoid=False, labels=None):
    op = "class_agnostic_nms"
    gpu_tensor(op, "box_preds", box_preds, contiguous=False)
    gpu_tensor(op, "cls_preds", cls_preds, contiguous=False)
    if box_preds.dim() != 3 or int(box_preds.shape[2]) != 7:
        raise RuntimeError(f"{op}: box_preds must be [B, A, 7], got {tuple(box_preds.shape)}")
    if cls_preds.dim() != 3 or tuple(cls_preds.shape[:2]) != tuple(box_preds.shape[:2]) or int(cls_preds.shape[2]) < 1:
        raise RuntimeError(f"{op}: cls_preds {tuple(cls_preds.shape)} for box_preds {tuple(box_preds.shape)}")
    bx, cl = box_preds.contiguous(), cls_preds.contiguous()
    B, A, K = (int(s) for s in cl.shape)
    lb = None
    if labels is not None:
        gpu_tensor(op, "labels", labels, torch.int64, contiguous=False)
        if tuple(labels.shape) != (B, A):
            raise RuntimeError(f"{op}: labels {tuple(labels.shape)} for {B} x {A} boxes")
        lb = labels.contiguous()
        _same_device(op, bx, lb)
    _same_device(op, bx, cl)
    pre, post = int(nms_config["nms_pre_maxsize"]), int(nms_config["nms_post_maxsize"])
    if pre < 1 or post < 1:
        raise RuntimeError(f"{op}: nms_pre_maxsize {pre}, nms_post_maxsize {post} must be >= 1")
    dev = bx.device
    boxes = torch.empty((B, post, 7), dtype=torch.float32, device=dev)
    scores = torch.empty((B, post), dtype=torch.float32, device=dev)
    out_labels = torch.empty((B, post), dtype=torch.int64, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    if B == 0:
        return boxes, scores, out_labels, count
    nbytes = lib().pd3_class_agnostic_nms_workspace(B, A, pre)
    if nbytes == 0:
        check(-3, op)
    ws = workspace(nbytes, dev)
    thresh = math.nan if score_thresh is None else float(score_thresh)
    check(lib().pd3_class_agnostic_nms(ptr(bx), ptr(cl), B, A, K, int(bool(apply_sigmoid)), thresh, ptr(lb), pre,
                                       float(nms_config["nms_thresh"]), post, ptr(boxes), ptr(scores),
                                       ptr(out_labels), ptr(count), ptr(ws), ws.numel(), stream_ptr(dev)), op)
    return boxes, scores, out_labels, count
