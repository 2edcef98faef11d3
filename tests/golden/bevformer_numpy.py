"""NumPy restatement of csrc/bevformer.hip, operation for operation in float32 (the order is the one in that file's
header), and the reference's module-level algorithm for spatial cross-attention, the rebatch / scatter form of
SpatialCrossAttention.forward (spatial_cross_attention.py:147-209), on the same per-point arithmetic.

point_sampling(ref_3d, lidar2img, pc_range, img_h, img_w) -> (reference_points_cam, bev_mask, hit_bits, hit_count)
softmax(x, expf)                                          the max, expf(x - max), the sum in index order, e / sum
sca(value, offsets, logits, ref_cam, hit_bits, shapes, starts, cams, expf)   pd3_bevformer_sca
tsa(value, offsets, logits, ref_2d, shapes, starts, expf)                    pd3_bevformer_tsa
sca_rebatch(value, offsets, logits, ref_cam, bev_mask, shapes, starts, cams, expf)
    per camera the queries it sees, gathered into zero-padded rows of the longest such list, sampled by
    ms_deform_attn, scattered back onto zeros camera by camera and divided by clip(count, 1).  `offsets` / `logits`
    are the Linear rows of the BEV queries: a rebatched query row is the BEV query row itself (query_pos is None),
    so its Linear rows are these.  Each frame uses its own mask (the reference takes frame 0's for every frame).

`expf` is a float32 array function with glibc's bits (oracle.pyoracle.libm_eval(2, x)).  The sampled point itself is
tests/golden/ms_deform_attn_numpy.py's forward().
"""
import numpy as np

import ms_deform_attn_numpy as md

F32 = np.float32
EPS = F32(1e-5)


def get_reference_points(H, W, Z=8, D=4, dim="3d"):
    """encoders.py:69-117 for one frame in float32: '3d' -> [D, Q, 3] (x, y, z in [0, 1]), '2d' -> [Q, 1, 2]."""
    import torch

    if dim == "3d":
        zs = (torch.linspace(0.5, Z - 0.5, D, dtype=torch.float32).reshape(-1, 1, 1).expand(D, H, W) / Z)
        xs = (torch.linspace(0.5, W - 0.5, W, dtype=torch.float32).reshape(1, 1, W).expand(D, H, W) / W)
        ys = (torch.linspace(0.5, H - 0.5, H, dtype=torch.float32).reshape(1, H, 1).expand(D, H, W) / H)
        return torch.stack((xs, ys, zs), -1).reshape(D, H * W, 3).numpy().copy()
    ys, xs = torch.meshgrid(torch.linspace(0.5, H - 0.5, H, dtype=torch.float32),
                            torch.linspace(0.5, W - 0.5, W, dtype=torch.float32), indexing="ij")
    return torch.stack((xs.reshape(-1) / W, ys.reshape(-1) / H), -1).unsqueeze(1).numpy().copy()


def point_sampling(ref_3d, lidar2img, pc_range, img_h, img_w):
    ref_3d, a = np.asarray(ref_3d, F32), np.asarray(lidar2img, F32)
    pc = np.asarray(pc_range, F32)
    D, Q, _ = ref_3d.shape
    B, cams = a.shape[:2]
    x = ref_3d[..., 0] * F32(pc[3] - pc[0]) + pc[0]  # [D, Q]
    y = ref_3d[..., 1] * F32(pc[4] - pc[1]) + pc[1]
    z = ref_3d[..., 2] * F32(pc[5] - pc[2]) + pc[2]
    x, y, z = (t.T[None, None] for t in (x, y, z))  # [1, 1, Q, D]
    m = a.transpose(1, 0, 2, 3)[:, :, None, None]  # [cams, B, 1, 1, 4, 4]
    with np.errstate(all="ignore"):
        c = [((m[..., k, 0] * x + m[..., k, 1] * y) + m[..., k, 2] * z) + m[..., k, 3] for k in range(3)]
        zc = np.where((c[2] > EPS) | np.isnan(c[2]), c[2], EPS).astype(F32)
        u = ((c[0] / zc) / F32(img_w)).astype(F32)
        v = ((c[1] / zc) / F32(img_h)).astype(F32)
        mask = (c[2] > EPS) & (v > 0) & (v < 1) & (u < 1) & (u > 0)
    hit = mask.any(-1)  # [cams, B, Q]
    bits = (hit.astype(np.int64) << np.arange(cams)[:, None, None]).sum(0).astype(np.uint8)
    return np.stack([u, v], -1), mask.astype(np.uint8), bits, hit.sum(0).astype(np.uint8)


def softmax(x, expf):
    x = np.asarray(x, F32)
    e = expf((x - x.max(-1, keepdims=True)).astype(F32)).reshape(x.shape).astype(F32)
    s = e[..., 0]
    for i in range(1, x.shape[-1]):
        s = (s + e[..., i]).astype(F32)
    return (e / s[..., None]).astype(F32)


def _normalizer(shapes):
    """(W_l, H_l) as float32 [L, 1, 2]."""
    sh = np.asarray(shapes, np.int64)
    return np.stack([sh[:, 1], sh[:, 0]], -1).astype(F32)[:, None, :]


def sca_locations(offsets, ref, shapes):
    """offsets [N, Q, M, L, P, 2], ref [N, Q, D, 2] -> [N, Q, M, L, P, 2]: anchors innermost (point p takes p % D)."""
    P, D = offsets.shape[4], ref.shape[2]
    with np.errstate(all="ignore"):
        o = (offsets / _normalizer(shapes)).astype(F32)
        r = ref[:, :, np.arange(P) % D]  # [N, Q, P, 2]
        return (r[:, :, None, None] + o).astype(F32)


def sca(value, offsets, logits, ref_cam, hit_bits, shapes, starts, cams, expf):
    B, Q, M, L, P, _ = offsets.shape
    C = value.shape[-1]
    a = softmax(logits, expf).reshape(B, Q, M, L, P)
    slot = np.zeros((B, Q, M * C), F32)
    v = value.reshape(B, cams, *value.shape[1:])
    for cam in range(cams):
        col = md.forward(np.ascontiguousarray(v[:, cam]), sca_locations(offsets, ref_cam[cam], shapes), a, shapes, starts)
        hit = ((hit_bits >> cam) & 1).astype(bool)[..., None]
        slot = np.where(hit, slot + col, slot).astype(F32)
    count = np.zeros((B, Q), np.int64)
    for cam in range(cams):
        count += (hit_bits >> cam) & 1
    return (slot / np.maximum(count, 1).astype(F32)[..., None]).astype(F32)


def tsa(value, offsets, logits, ref_2d, shapes, starts, expf):
    B, Q, M, _, L, P, _ = offsets.shape
    v = value.reshape(B, 2, *value.shape[1:])
    r = ref_2d.reshape(B, 2, Q, L, 2)
    cols = []
    for j in range(2):
        a = softmax(logits[:, :, :, j], expf).reshape(B, Q, M, L, P)
        with np.errstate(all="ignore"):
            loc = (r[:, j][:, :, None, :, None, :] + (offsets[:, :, :, j] / _normalizer(shapes)).astype(F32)).astype(F32)
        cols.append(md.forward(np.ascontiguousarray(v[:, j]), loc, a, shapes, starts))
    return ((cols[0] + cols[1]).astype(F32) * F32(0.5)).astype(F32)


def sca_rebatch(value, offsets, logits, ref_cam, bev_mask, shapes, starts, cams, expf):
    B, Q, M, L, P, _ = offsets.shape
    C, D = value.shape[-1], ref_cam.shape[3]
    slots = np.zeros((B, Q, M * C), F32)
    for b in range(B):  # the reference's batch is one frame
        idx = [np.nonzero(bev_mask[cam, b].sum(-1))[0] for cam in range(cams)]
        max_len = max(len(i) for i in idx)
        if max_len == 0:
            continue
        off_r = np.zeros((cams, max_len, M, L, P, 2), F32)
        log_r = np.zeros((cams, max_len, M, L * P), F32)
        ref_r = np.zeros((cams, max_len, D, 2), F32)
        for cam, i in enumerate(idx):
            off_r[cam, :len(i)], log_r[cam, :len(i)], ref_r[cam, :len(i)] = offsets[b, i], logits[b, i], ref_cam[cam, b, i]
        a = softmax(log_r, expf).reshape(cams, max_len, M, L, P)
        queries = md.forward(np.ascontiguousarray(value[b * cams:(b + 1) * cams]), sca_locations(off_r, ref_r, shapes), a,
                             shapes, starts)
        for cam, i in enumerate(idx):
            slots[b, i] = slots[b, i] + queries[cam, :len(i)]
    count = np.maximum((bev_mask.sum(-1) > 0).transpose(1, 2, 0).sum(-1), 1).astype(F32)
    return (slots / count[..., None]).astype(F32)
