"""NumPy restatement of the two entry points of PV-RCNN's keypoint branch and RoI head (csrc/pvrcnn.hip; TEST
INFRASTRUCTURE ONLY), in the kernels' operation order (include/paddle3d_amd.h states the same contract):

  bev_interpolate   xs = ((x - min_x) / voxel_x) / stride; x0 = floor(xs), x1 = x0 + 1, both clipped before the weights;
                    out = ((Ia * wa + Ib * wb) + Ic * wc) + Id * wd in float32 without FMA.  Exact.
  stack_sa_pool     pd3_ball_query_stack's row (pointnet2_stack_numpy.ball_query_stack), d = xyz[row] - new_xyz, a row
                    without a hit with features 0 and d 0; h = relu(scale1 * (f + ((w0 * dx + w1 * dy) + w2 * dz)) +
                    shift1); y = relu(scale2 * (sum_j w2[c, j] * h[j]) + shift2); max over the hits.  In float32 the sum
                    is the ascending-j fmaf chain from 0 (fmaf() below is correctly rounded), which is what the device
                    computes bit for bit; dtype float64 evaluates the same sums in float64 (the error bound's yardstick).
"""
from __future__ import annotations

import numpy as np

import pointnet2_stack_numpy as pn

F32 = np.float32
F64 = np.float64


def fmaf(a, b, c):
    """round32(a * b + c) with ONE rounding, elementwise for float32 arrays.  The product of two float32 is exact in
    float64, and rounding the float64 sum to float32 is the rounding of the exact value unless that sum sits exactly
    on the midpoint of two float32 (or in float32's subnormal range, where the midpoints are elsewhere).  Those
    elements are redone: the float64 sum is made round-to-odd from TwoSum's error term, which then rounds correctly
    (53 >= 24 + 2 bits)."""
    a, b, c = np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        p = a.astype(F64) * b.astype(F64)
        s = p + c
        bits = s.view(np.int64)
        risky = ((bits & 0x1FFFFFFF) == 0x10000000) | (np.abs(s) < 2.0 ** -126)
        out = s.astype(F32)
        if risky.any():
            pr, cr, sr = p[risky], np.broadcast_to(c, p.shape)[risky].astype(F64), s[risky]
            bb = sr - pr
            err = (pr - (sr - bb)) + (cr - bb)
            rb = sr.view(np.int64).copy()
            fix = np.isfinite(sr) & np.isfinite(err) & (err != 0) & ((rb & 1) == 0)
            rb = np.where(fix, rb + np.where((err > 0) == (sr > 0), 1, -1), rb)
            out[risky] = rb.view(F64).astype(F32)
        return out


def _to_i32(f):
    f = np.asarray(f, F32)
    out = np.zeros(f.shape, np.int64)
    ok = ~np.isnan(f)
    hi, lo = ok & (f >= F32(2147483648.0)), ok & (f <= F32(-2147483648.0))
    mid = ok & ~hi & ~lo
    out[mid] = f[mid].astype(np.int64)
    out[hi], out[lo] = np.iinfo(np.int32).max, np.iinfo(np.int32).min
    return out


def bev_interpolate(keypoints, bev, point_cloud_range, voxel_size, bev_stride):
    """keypoints [M, 4] (b, x, y, z), bev [B, C, H, W] -> [M, C] float32."""
    kp, im = np.asarray(keypoints, F32).reshape(-1, 4), np.asarray(bev, F32)
    B, C, H, W = im.shape
    out = np.zeros((kp.shape[0], C), F32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        b = _to_i32(kp[:, 0])
        ok = (b >= 0) & (b < B) & (b.astype(F32) == kp[:, 0])
        xs = (((kp[:, 1] - F32(point_cloud_range[0])).astype(F32) / F32(voxel_size[0])).astype(F32)
              / F32(bev_stride)).astype(F32)
        ys = (((kp[:, 2] - F32(point_cloud_range[1])).astype(F32) / F32(voxel_size[1])).astype(F32)
              / F32(bev_stride)).astype(F32)
        fx, fy = _to_i32(np.floor(xs)), _to_i32(np.floor(ys))
        x0, x1 = np.clip(fx, 0, W - 1), np.clip(fx + 1, 0, W - 1)
        y0, y1 = np.clip(fy, 0, H - 1), np.clip(fy + 1, 0, H - 1)
        ax, bx = (x1.astype(F32) - xs).astype(F32), (xs - x0.astype(F32)).astype(F32)
        ay, by = (y1.astype(F32) - ys).astype(F32), (ys - y0.astype(F32)).astype(F32)
        wa, wb, wc, wd = (ax * ay).astype(F32), (ax * by).astype(F32), (bx * ay).astype(F32), (bx * by).astype(F32)
        r = np.nonzero(ok)[0]
        if r.size == 0 or C == 0:
            return out
        bb = b[r]
        Ia, Ib = im[bb, :, y0[r], x0[r]], im[bb, :, y1[r], x0[r]]  # [rows, C]
        Ic, Id = im[bb, :, y0[r], x1[r]], im[bb, :, y1[r], x1[r]]
        v = ((Ia * wa[r, None]).astype(F32) + (Ib * wb[r, None]).astype(F32)).astype(F32)
        v = (v + (Ic * wc[r, None]).astype(F32)).astype(F32)
        out[r] = (v + (Id * wd[r, None]).astype(F32)).astype(F32)
    return out


def _relu(v, T):
    return np.where(np.isnan(v), v, np.where(v > 0, v, T(0))).astype(T)


def stack_sa_rows(new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, radius, nsample):
    """(global rows [M, nsample] with unused slots = slot 0 and empty rows 0, hit count [M] clipped to nsample)."""
    q, p = np.asarray(new_xyz, F32).reshape(-1, 3), np.asarray(xyz, F32).reshape(-1, 3)
    idx = pn.ball_query_stack(q, new_xyz_batch_cnt, p, xyz_batch_cnt, radius, nsample)
    empty = idx[:, 0] < 0
    f = pn.frames(q.shape[0], new_xyz_batch_cnt)
    s0, _ = pn._starts(xyz_batch_cnt, clamp=True)
    start = np.minimum(s0, p.shape[0])
    rows = np.where(empty[:, None], 0, start[f][:, None] + idx.astype(np.int64))
    return rows, empty


def stack_sa_pool(new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, features_in, w_pos, scale1, shift1, w2, scale2,
                  shift2, radius, nsample, dtype=F32, chunk=4096):
    """pooled [M, C2] in `dtype`: float32 in the kernel's order (fmaf chain), float64 from the same fp32 inputs."""
    T = dtype
    q, p = np.asarray(new_xyz, F32).reshape(-1, 3), np.asarray(xyz, F32).reshape(-1, 3)
    w, v2 = np.asarray(w_pos, F32), np.asarray(w2, F32)
    C1, C2 = w.shape[0], v2.shape[0]
    ft = None if features_in is None else np.asarray(features_in, F32)
    rows, empty = stack_sa_rows(q, new_xyz_batch_cnt, p, xyz_batch_cnt, radius, nsample)
    M, S = rows.shape
    sc1, sh1 = np.asarray(scale1, F32).astype(T), np.asarray(shift1, F32).astype(T)
    sc2, sh2 = np.asarray(scale2, F32).astype(T), np.asarray(shift2, F32).astype(T)
    out = np.zeros((M, C2), T)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(0, M, chunk):
            r, e = rows[i:i + chunk], empty[i:i + chunk]
            if p.shape[0]:
                d = (p[r].astype(T) - q[i:i + chunk, None, :].astype(T)).astype(T)  # [m, S, 3]
                f = ft[r].astype(T) if ft is not None else np.zeros(r.shape + (C1,), T)
            else:
                d, f = np.zeros(r.shape + (3,), T), np.zeros(r.shape + (C1,), T)
            d[e] = 0
            f[e] = 0
            wt = w.astype(T)
            lin = ((wt[:, 0] * d[..., 0:1]).astype(T) + (wt[:, 1] * d[..., 1:2]).astype(T)).astype(T)
            lin = (lin + (wt[:, 2] * d[..., 2:3]).astype(T)).astype(T)
            h = _relu(((sc1 * (f + lin).astype(T)).astype(T) + sh1).astype(T), T)  # [m, S, C1]
            if T is F32:
                acc = np.zeros(h.shape[:2] + (C2,), F32)
                for j in range(C1):
                    acc = fmaf(h[..., j:j + 1], v2[None, None, :, j], acc)
            else:
                acc = h @ v2.astype(T).T
            y = _relu(((sc2 * acc).astype(T) + sh2).astype(T), T)
            out[i:i + chunk] = y.max(axis=1)  # unused slots repeat slot 0: the max over all slots is over the hits
    return out


# ---- the restatement behind the op modules' signatures, for running paddle3d_amd/pv_rcnn.py on the CPU --------------
def patch_cpu(setattr_, O):
    """Put the restatements in place of the device ops with `setattr_(object, name, value)` (pytest's
    monkeypatch.setattr restores them): the two entry points of ops.pvrcnn, the RoI head's ops (roi_head_numpy), and
    the pointnet2 ops the keypoint sampling and the unfused layers call."""
    import types

    import torch

    import pointnet2_numpy as p2
    import roi_head_numpy as rn
    from paddle3d_amd import pointnet2_stack, pv_rcnn, roi_heads

    def n(t):
        return None if t is None else t.detach().numpy()

    def pool_t(new_xyz, new_cnt, xyz, cnt, features_in, w_pos, scale1, shift1, w2, scale2, shift2, radius, nsample):
        return torch.from_numpy(stack_sa_pool(n(new_xyz), n(new_cnt), n(xyz), n(cnt), n(features_in), n(w_pos),
                                              n(scale1), n(shift1), n(w2), n(scale2), n(shift2), float(radius),
                                              int(nsample)))

    ops = types.SimpleNamespace(
        stack_sa_pool=pool_t,
        bev_interpolate=lambda kp, bev, pcr, vs, stride: torch.from_numpy(bev_interpolate(n(kp), n(bev), pcr, vs, stride)),
        stack_sa_pool_supported=lambda c1, c2, s: int(c1) in (16, 32, 64) and int(c2) in (16, 32, 64) and 1 <= int(s) <= 64)
    roi, _ = rn.cpu_ops(O)
    setattr_(roi_heads, "_ops", roi)
    setattr_(pointnet2_stack, "pvrcnn", ops)
    setattr_(pv_rcnn, "pvrcnn", ops)
    p2o = pointnet2_stack.pointnet2_ops
    setattr_(p2o, "ball_query_stack", lambda q, qc, p, pc, r, s: torch.from_numpy(
        pn.ball_query_stack(n(q), n(qc), n(p), n(pc), float(r), int(s))))
    setattr_(p2o, "grouping_operation_stack", lambda f, fc, ix, ic: torch.from_numpy(
        pn.group_stack(n(f), n(fc), n(ix), n(ic))))
    setattr_(p2o, "farthest_point_sample", lambda pts, m, tier=0: torch.from_numpy(
        p2.farthest_point_sample(n(pts), int(m))))
    return roi_heads, pv_rcnn
