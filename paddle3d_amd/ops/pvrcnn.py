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

from ._common import check, gpu_rows, gpu_tensor, lib, ptr, stream_ptr

__all__ = ["stack_sa_pool_supported", "stack_sa_pool", "bev_interpolate"]


def _vec(t, op, what, n, dtype=torch.float32):
    gpu_tensor(op, what, t, dtype, contiguous=False)
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
    q = gpu_rows(op, "new_xyz", new_xyz, 3)
    p = gpu_rows(op, "xyz", xyz, 3)
    w = gpu_rows(op, "w_pos", w_pos, 3)
    v = gpu_rows(op, "w2", w2, None)
    M, N, C1, C2 = int(q.shape[0]), int(p.shape[0]), int(w.shape[0]), int(v.shape[0])
    if int(v.shape[1]) != C1:
        raise RuntimeError(f"{op}: w2 {tuple(v.shape)} for {C1} channels of w_pos")
    f = None
    if features_in is not None:
        f = gpu_rows(op, "features_in", features_in, C1)
        if int(f.shape[0]) != N:
            raise RuntimeError(f"{op}: features_in has {int(f.shape[0])} rows, xyz {N}")
    sc1, sh1 = _vec(scale1, op, "scale1", C1), _vec(shift1, op, "shift1", C1)
    sc2, sh2 = _vec(scale2, op, "scale2", C2), _vec(shift2, op, "shift2", C2)
    gpu_tensor(op, "new_xyz_batch_cnt", new_xyz_batch_cnt, torch.int32, contiguous=False)
    gpu_tensor(op, "xyz_batch_cnt", xyz_batch_cnt, torch.int32, contiguous=False)
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
    kp = gpu_rows(op, "keypoints", keypoints, 4)
    gpu_tensor(op, "bev", bev, contiguous=False)
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
