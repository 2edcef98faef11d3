"""NumPy restatement of the four entry points of Voxel R-CNN's RoI head (csrc/roi_head.hip; TEST INFRASTRUCTURE ONLY),
in float32 and in the kernels' operation order (include/paddle3d_amd.h states the same contract):

  voxel_pool          pd3_voxel_query's row (pointnet2_stack_numpy.voxel_query), d = xyz[idx] - new_xyz, a row without
                      a hit with features = 0 and d = 0 in every slot; v = relu(f + (scale * ((w0 * dx + w1 * dy) +
                      w2 * dz) + shift)); max over the slots, or the avg as the kernel sums it: G = 64 / C1 groups, group
                      g the slots g, g + G, ... in order, the groups by (g0 + g1) + (g2 + g3), then / nsample.
  roi_grid_points     local = ((idx + 0.5) / G) * size - size / 2, the rotation as the matmul's sums, + centre,
                      coords = floor(floor((xyz - min) / voxel) / stride) as (b, x, y, z).
  rcnn_decode_boxes   ResidualCoder.decode against the RoI with its centre zeroed, rotated by the RoI's heading,
                      + the RoI's centre.
  class_agnostic_nms  max / argmax (first maximum), optional sigmoid, >= score_thresh, stable descending order, the
                      first nms_pre_maxsize, rotated NMS on the columns as they are (oracle.nms), the first
                      nms_post_maxsize; zero padding, the box_empty row.

sinf / cosf / expf are glibc's through oracle.libm_eval(op, x) (0 sinf, 1 cosf, 2 expf).  `O` below is oracle.pyoracle.
"""
from __future__ import annotations

import numpy as np

import pointnet2_stack_numpy as pn

F32 = np.float32


def voxel_pool_terms(new_xyz, new_coords, xyz, point_indices, features_in, w_pos, pos_scale, pos_shift, max_range,
                     radius, nsample, dtype=F32):
    """([M, nsample, C1] terms relu(f + pos), idx [M, nsample]); dtype float64 gives the fp64 evaluation."""
    q, p = np.asarray(new_xyz, F32).reshape(-1, 3), np.asarray(xyz, F32).reshape(-1, 3)
    ft = np.asarray(features_in, F32)
    idx = pn.voxel_query(q, p, new_coords, point_indices, radius, nsample, *max_range)
    empty = idx[:, 0] < 0
    rows = np.where(empty[:, None], 0, idx)
    T = dtype
    with np.errstate(invalid="ignore", over="ignore"):
        if p.shape[0]:
            d = (p[rows].astype(T) - q[:, None, :].astype(T)).astype(T)  # [M, S, 3]
            f = ft[rows].astype(T)  # [M, S, C1]
        else:
            d = np.zeros(rows.shape + (3,), T)
            f = np.zeros(rows.shape + (ft.shape[1],), T)
        d[empty] = 0
        f[empty] = 0
        w = np.asarray(w_pos, F32).astype(T)
        lin = ((w[:, 0] * d[..., 0:1]).astype(T) + (w[:, 1] * d[..., 1:2]).astype(T)).astype(T)
        lin = (lin + (w[:, 2] * d[..., 2:3]).astype(T)).astype(T)
        pos = ((np.asarray(pos_scale, F32).astype(T) * lin).astype(T) + np.asarray(pos_shift, F32).astype(T)).astype(T)
        v = (f + pos).astype(T)
        v = np.where(np.isnan(v), v, np.where(v > 0, v, T(0))).astype(T)
    return v, idx


def voxel_pool(new_xyz, new_coords, xyz, point_indices, features_in, w_pos, pos_scale, pos_shift, max_range, radius,
               nsample, pool):
    """pooled [M, C1] float32 in the kernel's order; new_coords [M, 4] as (b, z, y, x); pool 0 max, 1 avg."""
    v, _ = voxel_pool_terms(new_xyz, new_coords, xyz, point_indices, features_in, w_pos, pos_scale, pos_shift,
                            max_range, radius, nsample)
    M, S, C1 = v.shape
    if pool == 0:
        return v.max(axis=1).astype(F32) if M else np.zeros((0, C1), F32)
    G = 64 // C1
    with np.errstate(invalid="ignore", over="ignore"):
        part = []
        for g in range(G):
            acc = np.zeros((M, C1), F32)
            for s in range(g, S, G):
                acc = (acc + v[:, s]).astype(F32)
            part.append(acc)
        while len(part) > 1:  # lanes g and g ^ 1 meet first, then g and g ^ 2
            part = [(part[i] + part[i + 1]).astype(F32) for i in range(0, len(part), 2)]
        return (part[0] / F32(S)).astype(F32)


def voxel_pool_f64(new_xyz, new_coords, xyz, point_indices, features_in, w_pos, pos_scale, pos_shift, max_range,
                   radius, nsample, pool):
    """The same pool evaluated in float64 from the same fp32 inputs (the error bound's yardstick)."""
    v, _ = voxel_pool_terms(new_xyz, new_coords, xyz, point_indices, features_in, w_pos, pos_scale, pos_shift,
                            max_range, radius, nsample, dtype=np.float64)
    return v.max(axis=1) if pool == 0 else v.mean(axis=1)


def _rotate(O, x, y, z, angle):
    """rotate_points_along_z as the matmul's sums; every array float32 of one shape."""
    ca, sa = O.libm_eval(1, angle).reshape(angle.shape), O.libm_eval(0, angle).reshape(angle.shape)
    zero, one = F32(0), F32(1)
    with np.errstate(invalid="ignore", over="ignore"):
        xr = (((x * ca).astype(F32) + (y * (-sa)).astype(F32)).astype(F32) + (z * zero).astype(F32)).astype(F32)
        yr = (((x * sa).astype(F32) + (y * ca).astype(F32)).astype(F32) + (z * zero).astype(F32)).astype(F32)
        zr = (((x * zero).astype(F32) + (y * zero).astype(F32)).astype(F32) + (z * one).astype(F32)).astype(F32)
    return xr, yr, zr


def _to_i32(f):
    f = np.asarray(f, F32)
    out = np.zeros(f.shape, np.int32)
    ok = ~np.isnan(f)
    hi, lo = ok & (f >= F32(2147483648.0)), ok & (f <= F32(-2147483648.0))
    mid = ok & ~hi & ~lo
    out[mid] = f[mid].astype(np.int32)
    out[hi], out[lo] = np.iinfo(np.int32).max, np.iinfo(np.int32).min
    return out


def roi_grid_points(O, rois, grid_size, range_min, voxel_size, strides):
    """rois [B, R, 7] -> (roi_grid_xyz [B * R * G^3, 3], [coords [B * R * G^3, 4] as (b, x, y, z) per stride])."""
    r = np.asarray(rois, F32)
    B, R = r.shape[0], r.shape[1]
    r = r.reshape(-1, 7)
    G = int(grid_size)
    i = np.arange(G ** 3)
    idx = np.stack([i // (G * G), i // G % G, i % G], 1).astype(F32)  # [G^3, 3]
    size = r[:, None, 3:6]
    with np.errstate(invalid="ignore", over="ignore"):
        local = ((((idx + F32(0.5)).astype(F32) / F32(G)).astype(F32)[None] * size).astype(F32)
                 - (size / F32(2)).astype(F32)).astype(F32)  # [N, G^3, 3]
        ang = np.broadcast_to(r[:, None, 6], local.shape[:2]).copy()
        x, y, z = _rotate(O, local[..., 0], local[..., 1], local[..., 2], ang)
        xyz = np.stack([(x + r[:, None, 0]).astype(F32), (y + r[:, None, 1]).astype(F32),
                        (z + r[:, None, 2]).astype(F32)], -1).reshape(-1, 3)
        c = np.floor(((xyz - np.asarray(range_min, F32)).astype(F32) / np.asarray(voxel_size, F32)).astype(F32))
        b = np.repeat(np.arange(B, dtype=np.int32), R * G ** 3)
        coords = []
        for s in strides:
            cs = _to_i32(np.floor((c / F32(s)).astype(F32)))
            coords.append(np.concatenate([b[:, None], cs], 1).astype(np.int32))
    return xyz, coords


def rcnn_decode_boxes(O, rois, box_preds):
    """rois, box_preds [..., 7] -> decoded boxes of the same shape."""
    a = np.asarray(rois, F32).reshape(-1, 7)
    e = np.asarray(box_preds, F32).reshape(-1, 7)
    zero = F32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        diag = np.sqrt(((a[:, 3] * a[:, 3]).astype(F32) + (a[:, 4] * a[:, 4]).astype(F32)).astype(F32)).astype(F32)
        xg = ((e[:, 0] * diag).astype(F32) + zero).astype(F32)
        yg = ((e[:, 1] * diag).astype(F32) + zero).astype(F32)
        zg = ((e[:, 2] * a[:, 5]).astype(F32) + zero).astype(F32)
        x, y, z = _rotate(O, xg, yg, zg, a[:, 6].copy())
        ex = O.libm_eval(2, e[:, 3:6].reshape(-1)).reshape(-1, 3)
        out = np.stack([(x + a[:, 0]).astype(F32), (y + a[:, 1]).astype(F32), (z + a[:, 2]).astype(F32),
                        (ex[:, 0] * a[:, 3]).astype(F32), (ex[:, 1] * a[:, 4]).astype(F32),
                        (ex[:, 2] * a[:, 5]).astype(F32), (e[:, 6] + a[:, 6]).astype(F32)], 1)
    return out.reshape(np.asarray(rois).shape).astype(F32)


def class_agnostic_nms(O, box_preds, cls_preds, apply_sigmoid, score_thresh, labels, nms_pre_maxsize, nms_thresh,
                       nms_post_maxsize, kind="port", trace=None):
    """box_preds [B, A, 7], cls_preds [B, A, K], labels [B, A] int64 or None, score_thresh None = no threshold ->
    (boxes [B, post, 7], scores [B, post], labels [B, post] int64, count [B] int32).  trace (a list) receives per
    frame the (order after the pre cut, keep) pair."""
    bx, cl = np.asarray(box_preds, F32), np.asarray(cls_preds, F32)
    B, A, K = cl.shape
    post = int(nms_post_maxsize)
    ob, os_ = np.zeros((B, post, 7), F32), np.zeros((B, post), F32)
    ol, oc = np.zeros((B, post), np.int64), np.zeros((B,), np.int32)
    for b in range(B):
        c = cl[b]
        if apply_sigmoid:
            with np.errstate(over="ignore"):
                e = O.libm_eval(2, (-c).reshape(-1)).reshape(c.shape)
                c = (F32(1) / (F32(1) + e).astype(F32)).astype(F32)
        best, arg = c[:, 0].copy(), np.zeros(A, np.int64)
        for k in range(1, K):
            up = c[:, k] > best
            best, arg = np.where(up, c[:, k], best), np.where(up, k, arg)
        passed = np.arange(A) if score_thresh is None else np.nonzero(best >= F32(score_thresh))[0]
        if passed.size == 0:
            if score_thresh is not None:
                os_[b, 0], ol[b, 0] = -1, -1
            continue
        s = best[passed]
        key = np.where(np.isnan(s), np.inf, np.where(s == 0, 0.0, s.astype(np.float64)))
        order = passed[np.argsort(-key, kind="stable")][:int(nms_pre_maxsize)]
        keep = O.nms(np.ascontiguousarray(bx[b][order]), float(nms_thresh), kind=kind)[:post]
        if trace is not None:
            trace.append((order.copy(), np.asarray(keep).copy()))
        sel = order[keep]
        n = len(sel)
        ob[b, :n], os_[b, :n] = bx[b][sel], best[sel]
        ol[b, :n] = arg[sel] if labels is None else np.asarray(labels)[b][sel]
        oc[b] = n
    return ob, os_, ol, oc


# ---- the restatement behind the op modules' signatures, for running paddle3d_amd/roi_heads.py on the CPU ------------
def cpu_ops(O):
    """(roi_head ops, pointnet2 ops) namespaces over torch CPU tensors: what the tests put in place of
    paddle3d_amd.ops.roi_head and of the three pointnet2 stack ops the unfused pool layer calls."""
    import types

    import torch

    def n(t):
        return t.detach().numpy()

    def voxel_pool_t(new_xyz, new_coords, xyz, point_indices, features_in, w_pos, pos_scale, pos_shift, max_range,
                     radius, nsample, pool_method="max_pool"):
        return torch.from_numpy(voxel_pool(n(new_xyz), n(new_coords), n(xyz), n(point_indices), n(features_in),
                                           n(w_pos), n(pos_scale), n(pos_shift), [int(v) for v in max_range],
                                           float(radius), int(nsample), {"max_pool": 0, "avg_pool": 1}[pool_method]))

    def grid_t(rois, grid_size, point_cloud_range, voxel_size, strides):
        xyz, coords = roi_grid_points(O, n(rois), grid_size, list(point_cloud_range)[:3], voxel_size, strides)
        return torch.from_numpy(xyz), [torch.from_numpy(c) for c in coords]

    def decode_t(rois, box_preds):
        return torch.from_numpy(rcnn_decode_boxes(O, n(rois), n(box_preds).reshape(n(rois).shape)))

    def nms_t(box_preds, cls_preds, nms_config, score_thresh=None, apply_sigmoid=False, labels=None):
        r = class_agnostic_nms(O, n(box_preds), n(cls_preds), apply_sigmoid, score_thresh,
                               None if labels is None else n(labels), nms_config["nms_pre_maxsize"],
                               nms_config["nms_thresh"], nms_config["nms_post_maxsize"])
        return tuple(torch.from_numpy(a) for a in r)

    roi = types.SimpleNamespace(voxel_pool=voxel_pool_t, roi_grid_points=grid_t, rcnn_decode_boxes=decode_t,
                                class_agnostic_nms=nms_t, POOLS={"max_pool": 0, "avg_pool": 1},
                                voxel_pool_supported=lambda c1, s: int(c1) in (16, 32, 64) and 1 <= int(s) <= 64)
    p2 = types.SimpleNamespace(
        voxel_query_wrapper=lambda q, p, co, pi, r, s, zr, yr, xr: torch.from_numpy(
            pn.voxel_query(n(q), n(p), n(co), n(pi), r, s, zr, yr, xr)),
        grouping_operation_stack=lambda f, fc, ix, ic: torch.from_numpy(pn.group_stack(n(f), n(fc), n(ix), n(ic))))
    return roi, p2


def patch_cpu(setattr_, O):
    """Put cpu_ops in place with `setattr_(object, name, value)` (pytest's monkeypatch.setattr restores them)."""
    from paddle3d_amd import pointnet2_stack, roi_heads

    roi, p2 = cpu_ops(O)
    setattr_(roi_heads, "_ops", roi)
    setattr_(pointnet2_stack, "roi_head", roi)
    setattr_(pointnet2_stack.pointnet2_ops, "voxel_query_wrapper", p2.voxel_query_wrapper)
    setattr_(pointnet2_stack.pointnet2_ops, "grouping_operation_stack", p2.grouping_operation_stack)
    return roi_heads


# ---- seeded scenes at the KITTI configuration's shapes (configs/voxel_rcnn/voxel_rcnn_005voxel_kitti_car.yml) ---------
KITTI_RANGE = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]
KITTI_VOXEL = [0.05, 0.05, 0.1]
KITTI_SCALES = {"x_conv2": (2, (21, 800, 704), 30000, 32, 0.4), "x_conv3": (4, (11, 400, 352), 12000, 64, 0.8),
                "x_conv4": (8, (5, 200, 176), 5000, 64, 1.6)}  # stride, grid (Z, Y, X), voxels per frame, channels, radius


def kitti_scene(batch, seed=7, rois_per_frame=100):
    """Clustered sparse voxels of the three pooled scales (about 30k / 12k / 5k per frame, unequal between frames, the
    way tests/test_pointnet2_stack_gpu.py builds its x_conv2 scene: 160 cluster centres per frame, cells drawn around
    them) and rois [batch, R, 7] on the clusters -> ({name: (indices [N, 4] (b, z, y, x), features [N, C])}, rois)."""
    rng = np.random.default_rng(seed)
    Z, Y, X = KITTI_SCALES["x_conv2"][1]
    cells_f, rois = [], []
    for b in range(batch):
        c = np.stack([rng.integers(2, Z - 2, 160), rng.integers(20, Y - 20, 160), rng.integers(20, X - 20, 160)], 1)
        cells = (c[rng.integers(0, 160, 40000)] + np.round(rng.normal(0, [2, 8, 8], (40000, 3)))).astype(np.int64)
        cells_f.append(np.clip(cells, 0, [Z - 1, Y - 1, X - 1]))
        centre = (c[:rois_per_frame, [2, 1, 0]].astype(F32) + F32(0.5)) * np.array([0.1, 0.1, 0.2], F32) \
            + np.array(KITTI_RANGE[:3], F32)
        size = np.array([3.9, 1.6, 1.56], F32) * rng.uniform(0.8, 1.2, (rois_per_frame, 3)).astype(F32)
        rois.append(np.concatenate([centre, size, rng.uniform(-np.pi, np.pi, (rois_per_frame, 1)).astype(F32)], 1))
    out = {}
    for name, (stride, (z, y, x), n, ch, _) in KITTI_SCALES.items():
        ind = []
        for b in range(batch):
            cc = np.minimum(cells_f[b] // (stride // 2), [z - 1, y - 1, x - 1])
            flat = np.unique((cc[:, 0] * y + cc[:, 1]) * x + cc[:, 2])
            flat = np.sort(rng.permutation(flat)[:n - (n // 20) * (b % 2)])
            zz, yy, xx = np.unravel_index(flat, (z, y, x))
            ind.append(np.stack([np.full(len(flat), b), zz, yy, xx], 1))
        ind = np.concatenate(ind).astype(np.int32)
        out[name] = (ind, rng.standard_normal((len(ind), ch)).astype(F32))
    return out, np.stack(rois).astype(F32)


def voxel_centers(indices, stride):
    """get_voxel_centers (box_utils.py:76-99) at the KITTI configuration, fp32."""
    size = (np.array(KITTI_VOXEL, F32) * F32(stride)).astype(F32)
    return ((indices[:, [3, 2, 1]].astype(F32) + F32(0.5)) * size + np.array(KITTI_RANGE[:3], F32)).astype(F32)


def voxel2pinds(indices, batch, grid):
    out = np.full((batch, *grid), -1, np.int32)
    out[tuple(indices.T)] = np.arange(len(indices), dtype=np.int32)
    return out


def kitti_proposals(batch, seed=11, A=70400):
    """box_preds [batch, A, 7], cls_preds [batch, A, 1] like a dense head's: most anchors low, a few hundred objects
    with a cloud of overlapping high-scoring anchors each."""
    rng = np.random.default_rng(seed)
    box = np.zeros((batch, A, 7), F32)
    box[..., 0] = rng.uniform(0, 70.4, (batch, A))
    box[..., 1] = rng.uniform(-40, 40, (batch, A))
    box[..., 2] = rng.uniform(-2.0, 0.0, (batch, A))
    box[..., 3:6] = np.array([3.9, 1.6, 1.56], F32) * rng.uniform(0.8, 1.2, (batch, A, 3))
    box[..., 6] = rng.uniform(-np.pi, np.pi, (batch, A))
    cls = rng.normal(-4.0, 1.5, (batch, A, 1)).astype(F32)
    for b in range(batch):
        obj = rng.integers(0, A, 150)
        for o in obj:
            near = rng.integers(0, A, 24)
            box[b, near] = box[b, o] + rng.normal(0, [0.3, 0.3, 0.1, 0.1, 0.05, 0.05, 0.05], (24, 7)).astype(F32)
            cls[b, near, 0] = rng.normal(2.0, 1.5, 24)
    return box, cls
