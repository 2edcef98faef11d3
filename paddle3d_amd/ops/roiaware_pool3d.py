"""`paddle3d.ops.roiaware_pool3d` mirror: points_in_boxes_gpu (PD_BUILD_OP(points_in_boxes_gpu),
roiaware_pool3d/box_utils.cc:65; kernel in csrc/pointnet2.hip).

points_in_boxes_gpu(pts, boxes)
    pts [B, npts, 3] float32, boxes [B, M, 7] float32 (x, y, z, dx, dy, dz, heading; z at the centre) ->
    [B, npts] int32: the first box in index order that holds the point, -1 if none.  boxes may be a view whose rows
    are strided with a unit last-axis stride, such as gt_boxes[k:k+1, :, 0:7] of an [B, M, 8] tensor: it is read in
    place.  The reference's precision is kept: cosf / sinf(-heading) with glibc's bits, the z and |local| tests in
    double, local_x / local_y in fp32.  Nothing here synchronises with the host.
"""
from __future__ import annotations

import torch

from ._common import check, lib, ptr, stream_ptr

__all__ = ["points_in_boxes_gpu"]


def points_in_boxes_gpu(pts, boxes):
    op = "points_in_boxes_gpu"
    for what, t in (("pts", pts), ("boxes", boxes)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"Unsupported device type for {op} operator.")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{op}: {what} must be float32, got {t.dtype}")
    if pts.device != boxes.device:
        raise RuntimeError(f"{op}: pts on {pts.device}, boxes on {boxes.device}")
    if pts.dim() != 3 or int(pts.shape[2]) != 3:
        raise RuntimeError(f"{op}: pts must be [B, npts, 3], got {tuple(pts.shape)}")
    if boxes.dim() != 3 or int(boxes.shape[2]) != 7:
        raise RuntimeError(f"{op}: boxes must be [B, M, 7], got {tuple(boxes.shape)}")
    B, M = int(boxes.shape[0]), int(boxes.shape[1])
    if int(pts.shape[0]) != B:
        raise RuntimeError(f"{op}: pts has batch {int(pts.shape[0])}, boxes {B}")
    p = pts.contiguous()
    bx = boxes
    if bx.stride(2) != 1 or (M > 1 and bx.stride(1) < 7) or (B > 1 and bx.stride(0) < 1):
        bx = bx.contiguous()
    npts = int(p.shape[1])
    out = torch.empty((B, npts), dtype=torch.int32, device=p.device)
    check(lib().pd3_points_in_boxes(ptr(p), ptr(bx), B, npts, M, max(int(bx.stride(1)), 7), int(bx.stride(0)),
                                    ptr(out), stream_ptr(p.device)), op)
    return out
