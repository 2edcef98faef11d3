"""PV-RCNN's keypoint branch and RoI head on the device (csrc/pvrcnn.hip, contract in include/paddle3d_amd.h).
Inference only.

stack_sa_pool_supported(c1, c2, nsample)
    whether stack_sa_pool takes the shape (c1, c2 in {16, 32, 64}, nsample <= 64).
stack_sa_pool(new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, features_in, w_pos, scale1, shift1, w2, scale2, shift2,
              radius, nsample)
    new_xyz [M, 3], xyz [N, 3], counts [B] int32, features_in [N, C1] or None (zeros), w_pos [C1, 3], scale1 / shift1
    [C1], w2 [C2, C1], scale2 / shift2 [C2] -> pooled [M, C2]: one scale of StackSAModuleMSG.forward
    (pointnet2_modules.py:31-120) from the ball query to the max pool.
bev_interpolate(keypoints, bev, point_cloud_range, voxel_size, bev_stride)
    keypoints [M, 4] as (b, x, y, z), bev [B, C, H, W] -> [M, C] (voxel_set_abstraction.py:32-67, 180-213 for every
    frame in one launch).

float32 only, on the GPU.  Nothing here synchronises with the host.  A shape the library does not take raises.
"""
from __future__ import annotations

import torch

from ._common import check, lib, ptr, stream_ptr

__all__ = ["stack_sa_pool_supported", "stack_sa_pool", "bev_interpolate"]


def _gpu(t, op, what, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"Unsupported device type for {op} operator.")
    if t.dtype != dtype:
        raise RuntimeError(f"{op}: {what} must be {dtype}, got {t.dtype}")
    return t


def _rows(t, op, what, width, dtype=torch.float32):
    _gpu(t, op, what, dtype)
    if t.dim() != 2 or (width is not None and int(t.shape[1]) != width):
        raise RuntimeError(f"{op}: {what} must be [rows, {width if width is not None else 'C'}], got {tuple(t.shape)}")
    return t.contiguous()


def _vec(t, op, what, n, dtype=torch.float32):
    _gpu(t, op, what, dtype)
    if tuple(t.shape) != (n,):
        raise RuntimeError(f"{op}: {what} must be [{n}], got {tuple(t.shape)}")
    return t.contiguous()


def _same_device(op, *ts):
    dev = ts[0].device
    for t in ts[1:]:
        if t is not None and t.device != dev:
            raise RuntimeError(f"{op}: tensors on {dev} and {t.device}")


def stack_sa_pool_supported(c1, c2, nsample):
    return int(c1) in (16, 32, 64) and int(c2) in (16, 32, 64) and 1 <= int(nsample) <= 64


def stack_sa_pool(new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, features_in, w_pos, scale1, shift1, w2, scale2,
                  shift2, radius, nsample):
    op = "stack_sa_pool"
    q = _rows(new_xyz, op, "new_xyz", 3)
    p = _rows(xyz, op, "xyz", 3)
    w = _rows(w_pos, op, "w_pos", 3)
    v = _rows(w2, op, "w2", None)
    M, N, C1, C2 = int(q.shape[0]), int(p.shape[0]), int(w.shape[0]), int(v.shape[0])
    if int(v.shape[1]) != C1:
        raise RuntimeError(f"{op}: w2 {tuple(v.shape)} for {C1} channels of w_pos")
    f = None
    if features_in is not None:
        f = _rows(features_in, op, "features_in", C1)
        if int(f.shape[0]) != N:
            raise RuntimeError(f"{op}: features_in has {int(f.shape[0])} rows, xyz {N}")
    sc1, sh1 = _vec(scale1, op, "scale1", C1), _vec(shift1, op, "shift1", C1)
    sc2, sh2 = _vec(scale2, op, "scale2", C2), _vec(shift2, op, "shift2", C2)
    _gpu(new_xyz_batch_cnt, op, "new_xyz_batch_cnt", torch.int32)
    _gpu(xyz_batch_cnt, op, "xyz_batch_cnt", torch.int32)
    qc, pc = new_xyz_batch_cnt.contiguous(), xyz_batch_cnt.contiguous()
    if qc.dim() != 1 or qc.shape != pc.shape:
        raise RuntimeError(f"{op}: batch counts {tuple(qc.shape)} and {tuple(pc.shape)}")
    _same_device(op, q, p, f, w, v, sc1, sh1, sc2, sh2, qc, pc)
    B, S = int(qc.shape[0]), int(nsample)
    if S < 1:
        raise RuntimeError(f"{op}: nsample must be >= 1, got {S}")
    if B == 0 and M > 0:
        raise RuntimeError(f"{op}: {M} rows but no frame")
    out = torch.empty((M, C2), dtype=torch.float32, device=q.device)
    check(lib().pd3_stack_sa_pool(ptr(q), ptr(qc), ptr(p), ptr(pc), ptr(f), ptr(w), ptr(sc1), ptr(sh1), ptr(v),
                                  ptr(sc2), ptr(sh2), B, M, N, C1, C2, float(radius), S, ptr(out),
                                  stream_ptr(q.device)), op)
    return out


def bev_interpolate(keypoints, bev, point_cloud_range, voxel_size, bev_stride):
    op = "bev_interpolate"
    kp = _rows(keypoints, op, "keypoints", 4)
    _gpu(bev, op, "bev")
    if bev.dim() != 4:
        raise RuntimeError(f"{op}: bev must be [B, C, H, W], got {tuple(bev.shape)}")
    im = bev.contiguous()
    _same_device(op, kp, im)
    B, C, H, W = (int(s) for s in im.shape)
    M = int(kp.shape[0])
    if B > 0 and M * C > 0 and (H == 0 or W == 0):
        raise RuntimeError(f"{op}: an empty map {tuple(im.shape)}")
    out = torch.empty((M, C), dtype=torch.float32, device=kp.device)
    check(lib().pd3_bev_interpolate(ptr(kp), ptr(im), M, B, C, H, W, float(point_cloud_range[0]),
                                    float(point_cloud_range[1]), float(voxel_size[0]), float(voxel_size[1]),
                                    float(bev_stride), ptr(out), stream_ptr(kp.device)), op)
    return out
