"""NumPy restatement of csrc/squeezeseg.hip, operation for operation (the order is the one in that file's header).

sac_isk(xyz, feature, w, s_a, t_a, v, s_m, t_m, expf)    pd3_sac_isk_forward with the UNPACKED weights: w [9C, 3, 7, 7],
    v [C, 9C] -> Y [N, C, H, W] float32
range_project(points, offsets, H, W, fov_up, fov_down, mean, std)    pd3_range_project -> dict(image, proj_idx,
    proj_mask, proj_y, proj_x, fx, fy): fx, fy are the float64 pixel coordinates before the floor (NaN for a point
    that takes no pixel)

`expf` is a float32 array function with glibc's bits (oracle.pyoracle.libm_eval(2, x)); fmaf is pv_rcnn_numpy's
correctly rounded one.
"""
import numpy as np

from pv_rcnn_numpy import fmaf

F32 = np.float32
F64 = np.float64


def _shifted(x, dy, dx):
    """x[..., y + dy, x + dx] with +0 outside the image."""
    H, W = x.shape[-2:]
    out = np.zeros_like(x)
    ys, ye = max(0, -dy), min(H, H - dy)
    xs, xe = max(0, -dx), min(W, W - dx)
    if ys < ye and xs < xe:
        out[..., ys:ye, xs:xe] = x[..., ys + dy:ye + dy, xs + dx:xe + dx]
    return out


def sac_attention(xyz, w):
    """a [N, 9C, H, W]: the ascending fmaf chain over the 147 taps from +0."""
    xyz, w = np.asarray(xyz, F32), np.asarray(w, F32)
    N, _, H, W = xyz.shape
    J = w.shape[0]
    with np.errstate(all="ignore"):
        a = np.zeros((N, J, H, W), F32)
        for ci in range(3):
            for ky in range(7):
                for kx in range(7):
                    X = _shifted(xyz[:, ci], ky - 3, kx - 3)
                    a = fmaf(X[:, None], w[None, :, ci, ky, kx, None, None], a)
    return a


def sac_gate(a, s_a, t_a, expf):
    with np.errstate(all="ignore"):
        z = ((a * np.asarray(s_a, F32)[None, :, None, None]).astype(F32) + np.asarray(t_a, F32)[None, :, None, None]).astype(F32)
        e = expf((-z).astype(F32)).reshape(z.shape).astype(F32)
        return (F32(1) / (F32(1) + e).astype(F32)).astype(F32)


def sac_isk(xyz, feature, w, s_a, t_a, v, s_m, t_m, expf):
    feature, v = np.asarray(feature, F32), np.asarray(v, F32)
    N, C, H, W = feature.shape
    gate = sac_gate(sac_attention(xyz, w), s_a, t_a, expf)
    with np.errstate(all="ignore"):
        y = np.zeros((N, C, H, W), F32)
        for j in range(9 * C):
            c, k9 = divmod(j, 9)
            ky, kx = divmod(k9, 3)
            p = (_shifted(feature[:, c], ky - 1, kx - 1) * gate[:, j]).astype(F32)
            y = fmaf(p[:, None], v[None, :, j, None, None], y)
        r = ((y * np.asarray(s_m, F32)[None, :, None, None]).astype(F32) + np.asarray(t_m, F32)[None, :, None, None]).astype(F32)
        return np.where(r > 0, r, np.where(np.isnan(r), r, F32(0))).astype(F32)


def range_project(points, offsets, H, W, fov_up=3.0, fov_down=-25.0, mean=(0,) * 5, std=(1,) * 5):
    pts = np.asarray(points, F32).reshape(-1, 4)
    off = np.asarray(offsets, np.int64)
    P, B = pts.shape[0], off.size - 1
    upper, lower = fov_up / 180.0 * np.pi, fov_down / 180.0 * np.pi
    fov = upper - lower
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(all="ignore"):
        depth = np.sqrt(((x * x).astype(F32) + (y * y).astype(F32)).astype(F32) + (z * z).astype(F32)).astype(F32)
        frame = np.full(P, -1, np.int64)
        for b in range(B):
            frame[off[b]:off[b + 1]] = b
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (depth > 0) & (frame >= 0)
        fx = -np.arctan2(y.astype(F64), x.astype(F64)) / np.pi
        fx = fx + 1.0
        fx = 0.5 * fx
        fx = fx * float(W)
        q = np.clip(z.astype(F64) / depth.astype(F64), -1.0, 1.0)
        fy = (np.arcsin(q) + abs(lower)) / fov
        fy = 1.0 - fy
        fy = fy * float(H)
    fx, fy = np.where(ok, fx, np.nan), np.where(ok, fy, np.nan)
    px = np.where(ok, np.clip(np.floor(np.where(ok, fx, 0)), 0, W - 1), -1).astype(np.int32)
    py = np.where(ok, np.clip(np.floor(np.where(ok, fy, 0)), 0, H - 1), -1).astype(np.int32)
    raw = np.full((B, 5, H, W), -1, F32)
    proj_idx = np.full((B, H, W), -1, np.int32)
    best = np.full((B, H, W), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    for p in np.nonzero(ok)[0]:
        b = frame[p]
        key = (np.uint64(depth[p:p + 1].view(np.uint32)[0]) << np.uint64(32)) | np.uint64(p - off[b])
        if key < best[b, py[p], px[p]]:
            best[b, py[p], px[p]] = key
            proj_idx[b, py[p], px[p]] = p - off[b]
            raw[b, :, py[p], px[p]] = (depth[p], pts[p, 0], pts[p, 1], pts[p, 2], pts[p, 3])
    m = np.asarray(mean, F64).reshape(1, 5, 1, 1)
    s = np.asarray(std, F64).reshape(1, 5, 1, 1)
    with np.errstate(all="ignore"):
        image = ((raw.astype(F64) - m).astype(F32).astype(F64) / s).astype(F32)
    return dict(image=image, raw=raw, proj_idx=proj_idx, proj_mask=proj_idx > 0, proj_y=py, proj_x=px, fx=fx, fy=fy)
