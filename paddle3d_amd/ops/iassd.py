"""IA-SSD's fused set abstraction and box decode on the device (csrc/iassd.hip, contract in include/paddle3d_amd.h).
Inference only.

sa_msg_pool_supported(c1, c2, c3, nsample)
    whether sa_msg_pool takes the shape (c1, c2, c3 each a multiple of 16 in 16 .. 256, nsample in 1 .. 64).
sa_msg_pool(new_xyz, xyz, features_in, w_pos, scale1, shift1, w2, scale2, shift2, w3, scale3, shift3, radius, nsample,
            out=None, col=0)
    new_xyz [B, M, 3], xyz [B, N, 3], features_in [B, N, C1] or None (zeros), w_pos [C1, 3], scale1 / shift1 [C1],
    w2 [C2, C1], scale2 / shift2 [C2], w3 [C3, C2], scale3 / shift3 [C3] -> pooled [B, M, C3]: one scale of
    SAModuleMSG_WithSampling.forward (iassd_modules.py:204-221) from the ball query to the max pool.  With out
    [B, M, C] (contiguous, C >= col + C3) the rows are written into out[..., col : col + C3] and out is returned: the
    scales of a layer write side by side and the reference's concat costs nothing.
iassd_decode(cls_preds, box_preds, centers, mean_size, bins)
    cls_preds [M, K], box_preds [M, 6 + 2 * bins], centers [M, 3] or a view of such columns (a row stride is taken in
    place), mean_size [K, 3] or None -> boxes [M, 7] (iassd_head.py:606-621 with iassd_coder.py:76-121).

float32 only, on the GPU.  Nothing here synchronises with the host.  A shape the library does not take raises.
"""
from __future__ import annotations

import torch

from ._common import check, gpu_tensor, lib, ptr, stream_ptr

__all__ = ["sa_msg_pool_supported", "sa_msg_pool", "iassd_decode"]

MAX_WIDTH = 256
MAX_NSAMPLE = 64


def _shaped(t, op, what, shape):
    gpu_tensor(op, what, t, contiguous=False)
    if t.dim() != len(shape) or any(s is not None and int(d) != s for d, s in zip(t.shape, shape)):
        raise RuntimeError(f"{op}: {what} must be {list(shape)}, got {tuple(t.shape)}")
    return t.contiguous()


def _same_device(op, *ts):
    dev = ts[0].device
    for t in ts[1:]:
        if t is not None and t.device != dev:
            raise RuntimeError(f"{op}: tensors on {dev} and {t.device}")


def _width_ok(c):
    c = int(c)
    return 16 <= c <= MAX_WIDTH and c % 16 == 0


def sa_msg_pool_supported(c1, c2, c3, nsample):
    return _width_ok(c1) and _width_ok(c2) and _width_ok(c3) and 1 <= int(nsample) <= MAX_NSAMPLE


def sa_msg_pool(new_xyz, xyz, features_in, w_pos, scale1, shift1, w2, scale2, shift2, w3, scale3, shift3, radius,
                nsample, out=None, col=0):
    op = "sa_msg_pool"
    q = _shaped(new_xyz, op, "new_xyz", (None, None, 3))
    p = _shaped(xyz, op, "xyz", (None, None, 3))
    B, M, N = int(q.shape[0]), int(q.shape[1]), int(p.shape[1])
    if int(p.shape[0]) != B:
        raise RuntimeError(f"{op}: new_xyz has {B} frames, xyz {int(p.shape[0])}")
    wp = _shaped(w_pos, op, "w_pos", (None, 3))
    C1 = int(wp.shape[0])
    v2 = _shaped(w2, op, "w2", (None, C1))
    C2 = int(v2.shape[0])
    v3 = _shaped(w3, op, "w3", (None, C2))
    C3 = int(v3.shape[0])
    f = None if features_in is None else _shaped(features_in, op, "features_in", (B, N, C1))
    sc1, sh1 = _shaped(scale1, op, "scale1", (C1,)), _shaped(shift1, op, "shift1", (C1,))
    sc2, sh2 = _shaped(scale2, op, "scale2", (C2,)), _shaped(shift2, op, "shift2", (C2,))
    sc3, sh3 = _shaped(scale3, op, "scale3", (C3,)), _shaped(shift3, op, "shift3", (C3,))
    S, col = int(nsample), int(col)
    if S < 1:
        raise RuntimeError(f"{op}: nsample must be >= 1, got {S}")
    if N == 0 and B * M > 0:
        raise RuntimeError(f"{op}: {B * M} rows but no point to group")
    if out is None:
        if col != 0:
            raise RuntimeError(f"{op}: a column offset needs out=")
        out = torch.empty((B, M, C3), dtype=torch.float32, device=q.device)
    else:
        gpu_tensor(op, "out", out, contiguous=False)
        if out.dim() != 3 or tuple(out.shape[:2]) != (B, M) or not out.is_contiguous():
            raise RuntimeError(f"{op}: out must be a contiguous [{B}, {M}, C], got {tuple(out.shape)}")
        if col < 0 or col + C3 > int(out.shape[2]):
            raise RuntimeError(f"{op}: columns {col} .. {col + C3} of an out with {int(out.shape[2])}")
    _same_device(op, q, p, f, wp, sc1, sh1, v2, sc2, sh2, v3, sc3, sh3, out)
    ld = int(out.shape[2])
    dst = out if col == 0 else out.reshape(-1)[col:]  # a view: the first row's slice starts col floats in
    check(lib().pd3_sa_msg_pool(ptr(q), ptr(p), ptr(f), ptr(wp), ptr(sc1), ptr(sh1), ptr(v2), ptr(sc2), ptr(sh2),
                                ptr(v3), ptr(sc3), ptr(sh3), B, M, N, C1, C2, C3, float(radius), S, ptr(dst), ld,
                                stream_ptr(q.device)), op)
    return out


def iassd_decode(cls_preds, box_preds, centers, mean_size, bins):
    op = "iassd_decode"
    bins = int(bins)
    if bins < 1:
        raise RuntimeError(f"{op}: bins must be >= 1, got {bins}")
    cl = _shaped(cls_preds, op, "cls_preds", (None, None))
    M, K = int(cl.shape[0]), int(cl.shape[1])
    if K < 1:
        raise RuntimeError(f"{op}: cls_preds {tuple(cl.shape)} has no class")
    bx = _shaped(box_preds, op, "box_preds", (M, 6 + 2 * bins))
    gpu_tensor(op, "centers", centers, contiguous=False)
    if centers.dim() != 2 or tuple(centers.shape) != (M, 3):
        raise RuntimeError(f"{op}: centers must be [{M}, 3], got {tuple(centers.shape)}")
    if M > 1 and (centers.stride(1) != 1 or centers.stride(0) < 3):
        centers = centers.contiguous()
    ld = int(centers.stride(0)) if M > 1 else 3
    ms = None if mean_size is None else _shaped(mean_size, op, "mean_size", (K, 3))
    _same_device(op, cl, bx, centers, ms)
    out = torch.empty((M, 7), dtype=torch.float32, device=cl.device)
    check(lib().pd3_iassd_decode(ptr(cl), ptr(bx), ptr(centers), ld, ptr(ms), M, K, bins, ptr(out),
                                 stream_ptr(cl.device)), op)
    return out
