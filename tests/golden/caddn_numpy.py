"""NumPy restatement of the three entry points of CaDDN's frustum-to-voxel and map-to-BEV stage (csrc/caddn.hip; TEST
INFRASTRUCTURE ONLY), in the kernels' operation order (the header comment of csrc/caddn.hip states the same contract):

  frustum_grid      trans = lidar_to_cam @ grid_to_lidar with the translation column summed left to right, voxel centres
                    index + 0.5, both homogeneous divides as scale = |w| > 1e-8 ? 1 / (w + 1e-8) : 1, the bin index of
                    utils/depth.py with its constants rounded to float32 once (SID's log of 1 + depth is the float64 log
                    rounded to float32), ((c / (n - 1)) * 2) + -1, a non-finite component = -2.  float32, no FMA.
  softmax_probs     m = max, e_i = expf(x_i - m) (glibc's expf through `expf`, oracle.pyoracle.libm_eval(2, .)),
                    s = e_0 + e_1 + ... ascending, p_i = e_i / s, the last bin dropped; [B, h, w, D].
  sample_geo        per voxel the four g_j = (wx_j * wy_j) * (wz0 * p[z0] + wz1 * p[z0 + 1]) and pixel indices (-1 = out of
                    range), corners in the order (y0,x0), (y0,x1), (y1,x0), (y1,x1).
  frustum_to_voxel  sample[c] = ((g_0 f_0[c] + g_1 f_1[c]) + g_2 f_2[c]) + g_3 f_3[c] -> [B, C, Z, Y, X].
  frustum_to_bev    relu(scale * acc + shift), acc the float32 fmaf chain from 0 over z = 0 .. Z - 1 outer and,
                    within a z, c = 16 q + 4 k + j with q outermost, then j, k innermost (chain_order), of
                    fmaf(sample_z[c], weight[o, c * Z + z], acc) (pv_rcnn_numpy.fmaf is
                    correctly rounded): what the device's MFMA chain computes bit for bit.
"""
from __future__ import annotations

import math

import numpy as np

from pv_rcnn_numpy import fmaf

F32 = np.float32
F64 = np.float64


def grid_size(pc_range, voxel_size):
    r = np.asarray(pc_range, F64)
    return tuple(int(v) for v in np.round((r[3:] - r[:3]) / np.asarray(voxel_size, F64)).astype(np.int64))


def disc_consts(disc_cfg):
    mode, D = disc_cfg["mode"], int(disc_cfg["num_bins"])
    d0, d1 = float(disc_cfg["depth_min"]), float(disc_cfg["depth_max"])
    if mode == "UD":
        return F32(d0), F32((d1 - d0) / D)
    if mode == "LID":
        return F32(d0), F32(2.0 * (d1 - d0) / (float(D) * (1.0 + D)))
    if mode == "SID":
        return F32(math.log(1.0 + d0)), F32(math.log(1.0 + d1) - math.log(1.0 + d0))
    raise NotImplementedError(mode)


def _finite_or_out(v):
    return np.where(np.isfinite(v), v, F32(-2)).astype(F32)


def frustum_grid(lidar_to_cam, cam_to_img, image_shape, grid, pc_min, voxel_size, disc_cfg):
    """[B, X, Y, Z, 3] float32."""
    l2c, c2i = np.asarray(lidar_to_cam, F32).reshape(-1, 4, 4), np.asarray(cam_to_img, F32).reshape(-1, 3, 4)
    shp = np.asarray(image_shape).astype(np.int64).reshape(-1, 2)
    X, Y, Z = grid
    mn, vs = np.asarray(pc_min, F32), np.asarray(voxel_size, F32)
    D = int(disc_cfg["num_bins"])
    c0, c1 = disc_consts(disc_cfg)
    B = l2c.shape[0]
    with np.errstate(all="ignore"):
        t = np.zeros((B, 4, 4), F32)
        t[:, :, :3] = l2c[:, :, :3] * vs[None, None, :]
        t[:, :, 3] = ((l2c[:, :, 0] * mn[0] + l2c[:, :, 1] * mn[1]) + l2c[:, :, 2] * mn[2]) + l2c[:, :, 3]
        px = (np.arange(X, dtype=F32) + F32(0.5))[None, :, None, None]
        py = (np.arange(Y, dtype=F32) + F32(0.5))[None, None, :, None]
        pz = (np.arange(Z, dtype=F32) + F32(0.5))[None, None, None, :]
        e = lambda a: a[:, None, None, None]  # noqa: E731
        ch = [((px * e(t[:, i, 0]) + py * e(t[:, i, 1])) + pz * e(t[:, i, 2])) + e(t[:, i, 3]) for i in range(4)]
        s1 = np.where(np.abs(ch[3]) > F32(1e-8), F32(1) / (ch[3] + F32(1e-8)), F32(1)).astype(F32)
        cx, cy, cz = s1 * ch[0], s1 * ch[1], s1 * ch[2]
        im = [((e(c2i[:, i, 0]) * cx + e(c2i[:, i, 1]) * cy) + e(c2i[:, i, 2]) * cz) + e(c2i[:, i, 3]) for i in range(3)]
        s2 = np.where(np.abs(im[2]) > F32(1e-8), F32(1) / (im[2] + F32(1e-8)), F32(1)).astype(F32)
        u, v = s2 * im[0], s2 * im[1]
        depth = im[2] - e(c2i[:, 2, 3])
        mode = disc_cfg["mode"]
        if mode == "UD":
            b = (depth - c0) / c1
        elif mode == "LID":
            b = F32(-0.5) + F32(0.5) * np.sqrt(F32(1) + (F32(8) * (depth - c0)) / c1)
        else:
            b = (F32(D) * (np.log((F32(1) + depth).astype(F64)).astype(F32) - c0)) / c1
        nx, ny, nz = F32(shp[:, 1].max() - 1), F32(shp[:, 0].max() - 1), F32(D - 1)
        out = np.stack([_finite_or_out((u / nx) * F32(2) + F32(-1)), _finite_or_out((v / ny) * F32(2) + F32(-1)),
                        _finite_or_out((b / nz) * F32(2) + F32(-1))], -1)
    assert out.dtype == F32 and out.shape == (B, X, Y, Z, 3)
    return out


def softmax_probs(depth_logits, expf):
    """[B, D + 1, h, w] -> [B, h * w, D] float32."""
    x = np.asarray(depth_logits, F32)
    B, D1, h, w = x.shape
    with np.errstate(all="ignore"):
        m = x.max(axis=1, keepdims=True)
        ex = expf((x - m).reshape(-1)).reshape(x.shape).astype(F32)
        s = np.zeros((B, h, w), F32)
        for i in range(D1):
            s = s + ex[:, i]
        p = ex[:, :D1 - 1] / s[:, None]
    return np.ascontiguousarray(p.transpose(0, 2, 3, 1).reshape(B, h * w, D1 - 1)).astype(F32)


def _axis(g, n):
    f = ((g + F32(1)) * F32(n) - F32(1)) * F32(0.5)
    f0 = np.floor(f)
    ok = (f0 >= -1) & (f0 <= n - 1)
    return np.where(ok, f0, 0).astype(np.int64), ((f0 + F32(1)) - f).astype(F32), (f - f0).astype(F32), ok


def sample_geo(grid, probs, h, w):
    """grid [B, X, Y, Z, 3], probs [B, h * w, D] -> g [B, X, Y, Z, 4] float32, pixel [B, X, Y, Z, 4] int64 (-1 = out)."""
    D = probs.shape[2]
    bi = np.arange(grid.shape[0])[:, None, None, None]
    with np.errstate(all="ignore"):
        x0, wx0, wx1, okx = _axis(grid[..., 0], w)
        y0, wy0, wy1, oky = _axis(grid[..., 1], h)
        z0, wz0, wz1, okz = _axis(grid[..., 2], D)
        any_ = okx & oky & okz
        gs, os_ = [], []
        for j in range(4):
            x, y = x0 + (j & 1), y0 + (j >> 1)
            v = any_ & (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= h - 1)
            pix = np.where(v, y * w + x, 0)
            vz0, vz1 = v & (z0 >= 0), v & (z0 + 1 <= D - 1)
            t0 = np.where(vz0, wz0 * probs[bi, pix, np.clip(z0, 0, D - 1)], F32(0)).astype(F32)
            t1 = np.where(vz1, wz1 * probs[bi, pix, np.clip(z0 + 1, 0, D - 1)], F32(0)).astype(F32)
            wxy = ((wx1 if j & 1 else wx0) * (wy1 if j >> 1 else wy0)).astype(F32)
            gs.append(np.where(v, wxy * (t0 + t1), F32(0)).astype(F32))
            os_.append(np.where(v, pix, -1))
    return np.stack(gs, -1), np.stack(os_, -1)


def _samples(image_features, depth_logits, lidar_to_cam, cam_to_img, image_shape, grid, pc_min, voxel_size, disc_cfg,
             expf):
    """sample [B, X, Y, Z, C] float32."""
    f = np.asarray(image_features, F32)
    B, C, h, w = f.shape
    rows = np.ascontiguousarray(f.transpose(0, 2, 3, 1).reshape(B, h * w, C))
    g = frustum_grid(lidar_to_cam, cam_to_img, image_shape, grid, pc_min, voxel_size, disc_cfg)
    gj, oj = sample_geo(g, softmax_probs(depth_logits, expf), h, w)
    bi = np.arange(B)[:, None, None, None]
    with np.errstate(all="ignore"):
        term = []
        for j in range(4):
            fj = np.where((oj[..., j] >= 0)[..., None], rows[bi, np.maximum(oj[..., j], 0)], F32(0)).astype(F32)
            term.append((gj[..., j][..., None] * fj).astype(F32))
        return ((term[0] + term[1]) + term[2]) + term[3]


def frustum_to_voxel(image_features, depth_logits, lidar_to_cam, cam_to_img, image_shape, grid, pc_min, voxel_size,
                     disc_cfg, expf):
    """[B, C, Z, Y, X] float32."""
    s = _samples(image_features, depth_logits, lidar_to_cam, cam_to_img, image_shape, grid, pc_min, voxel_size, disc_cfg,
                 expf)
    return np.ascontiguousarray(s.transpose(0, 4, 3, 2, 1))


def frustum_to_bev(image_features, depth_logits, lidar_to_cam, cam_to_img, image_shape, grid, pc_min, voxel_size,
                   disc_cfg, weight, scale, shift, expf):
    """[B, C_out, Y, X] float32."""
    s = _samples(image_features, depth_logits, lidar_to_cam, cam_to_img, image_shape, grid, pc_min, voxel_size, disc_cfg,
                 expf)  # [B, X, Y, Z, C]
    B, X, Y, Z, C = s.shape
    wt = np.asarray(weight, F32).reshape(-1, C, Z)
    acc = np.zeros((B, X, Y, wt.shape[0]), F32)
    for z in range(Z):
        for c in chain_order(C):
            acc = fmaf(s[:, :, :, z, c][..., None], wt[None, None, None, :, c, z], acc)
    with np.errstate(all="ignore"):
        v = ((np.asarray(scale, F32) * acc).astype(F32) + np.asarray(shift, F32)).astype(F32)
        v = np.where(np.isnan(v), v, np.where(v > 0, v, F32(0))).astype(F32)
    return np.ascontiguousarray(v.transpose(0, 3, 2, 1))


def chain_order(C):
    """The channels of one z in the order the chain takes them: 16 q + 4 k + j, q outermost, then j, k innermost."""
    return [16 * q + 4 * k + j for q in range(C // 16) for j in range(4) for k in range(4)]


def fold_bn(state, prefix="", eps=1e-5):
    """(weight [C_out, C_in], scale, shift) of a 1x1 ConvBNReLU without a convolution bias from its Paddle-named state."""
    P = lambda k: np.asarray(state[prefix + k], F32)  # noqa: E731
    scale = (P("_batch_norm.weight") / np.sqrt(P("_batch_norm._variance") + F32(eps))).astype(F32)
    shift = (P("_batch_norm.bias") - (P("_batch_norm._mean") * scale).astype(F32)).astype(F32)
    w = P("_conv.weight")
    return np.ascontiguousarray(w.reshape(w.shape[0], -1)), scale, shift
