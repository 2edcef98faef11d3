"""NumPy restatement of csrc/petr.hip, operation for operation in float32 (the order is the one in that file's header).

mha_stream(q, k, v, num_heads, expf, key_mask=None)    pd3_mha_stream_forward: q [B, Nq, E], k, v [B, Nk, E], key_mask
    [B, Nk] (non-zero: padded) -> [B, Nq, E]
coords3d_ratio(img2lidars, H, W, D, pad_h, pad_w, depth_start, position_range, LID, token_mask=None)
    pd3_petr_coords3d up to the ratio: (ratio [BN, 3 * D, H, W] float32, coords_mask [BN, H, W] bool, normalised -- the
    coordinates before the clip, same layout)
coords3d(...)                                          (float32(log(float64(ratio))), coords_mask): the kernel's output to
    within the one float32 ulp a double logarithm rounded once can differ by

`expf` is a float32 array function with glibc's bits (oracle.pyoracle.libm_eval(2, x)); fmaf is pv_rcnn_numpy's
correctly rounded one.
"""
import numpy as np

from pv_rcnn_numpy import fmaf

F32 = np.float32
TILE_ORDER = (0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15)  # the keys of a 16-key tile, in P V's order
WAVES = 4
MASK_ADD = F32(-1e9)
EPS = F32(1e-5)


def mha_stream(q, k, v, num_heads, expf, key_mask=None):
    q, k, v = (np.asarray(t, F32) for t in (q, k, v))
    B, Nq, E = q.shape
    Nk, M = k.shape[1], num_heads
    d = E // M
    with np.errstate(all="ignore"):
        qs = (q.reshape(B, Nq, M, d) * F32(float(d) ** -0.5)).astype(F32).transpose(0, 2, 1, 3)  # [B, M, Nq, d]
        kh = k.reshape(B, Nk, M, d).transpose(0, 2, 1, 3)  # [B, M, Nk, d]
        vh = v.reshape(B, Nk, M, d).transpose(0, 2, 1, 3)
        s = np.zeros((B, M, Nq, Nk), F32)
        for c in range(d):
            s = fmaf(qs[..., :, None, c], kh[..., None, :, c], s)
        if key_mask is not None:
            pad = np.asarray(key_mask).reshape(B, Nk) != 0
            s = np.where(pad[:, None, None, :], (s + MASK_ADD).astype(F32), s)
        nan = np.isnan(s)
        mx = np.where(nan, -np.inf, s).max(-1).astype(F32)
        mx = np.where(nan[..., 0], s[..., 0], mx)
        e = expf((s - mx[..., None]).astype(F32)).reshape(s.shape).astype(F32)
        NT = -(-Nk // 16)
        lanes = np.zeros(s.shape[:-1] + (-(-Nk // 64) * 64,), F32)
        lanes[..., :Nk] = e
        lanes = lanes.reshape(s.shape[:-1] + (-1, 64))
        p = np.zeros(s.shape[:-1] + (64,), F32)
        for step in range(lanes.shape[-2]):
            p = (p + lanes[..., step, :]).astype(F32)
        h = 32
        while h >= 1:
            p = (p[..., :h] + p[..., h:2 * h]).astype(F32)
            h //= 2
        ep = np.zeros(s.shape[:-1] + (NT * 16,), F32)
        ep[..., :Nk] = e
        vp = np.zeros((B, M, NT * 16, d), F32)
        vp[:, :, :Nk] = vh
        parts = []
        for w in range(WAVES):
            acc = np.zeros((B, M, Nq, d), F32)
            for t in range(w, NT, WAVES):
                for o in TILE_ORDER:
                    j = 16 * t + o
                    acc = fmaf(ep[..., j:j + 1], vp[:, :, None, j, :], acc)
            parts.append(acc)
        a = (((parts[0] + parts[1]).astype(F32) + parts[2]).astype(F32) + parts[3]).astype(F32)
        out = (a / p).astype(F32)
    return np.ascontiguousarray(out.transpose(0, 2, 1, 3)).reshape(B, Nq, E)


def host_constants(D, depth_start, position_range, LID):
    """(bin, ds, r[3], den[3]) as pd3_petr_coords3d's host code rounds them; position_range arrives as float32."""
    r = np.asarray(position_range, F32).astype(np.float64)
    span = r[3] - float(depth_start)
    bin_size = F32(span / (float(D) * (1.0 + float(D)))) if LID else F32(span / float(D))
    return bin_size, F32(depth_start), r[:3].astype(F32), (r[3:] - r[:3]).astype(F32)


def coords3d_ratio(img2lidars, H, W, D, pad_h, pad_w, depth_start, position_range, LID, token_mask=None):
    m = np.asarray(img2lidars, F32).reshape(-1, 4, 4)
    BN = m.shape[0]
    bin_size, ds, r, den = host_constants(D, depth_start, position_range, LID)
    with np.errstate(all="ignore"):
        ch = ((np.arange(H, dtype=F32) * F32(pad_h)).astype(F32) / F32(H)).astype(F32)[None, :, None]  # [1, H, 1]
        cw = ((np.arange(W, dtype=F32) * F32(pad_w)).astype(F32) / F32(W)).astype(F32)[None, None, :]  # [1, 1, W]
        i = np.arange(D, dtype=F32)
        if LID:
            cd = (((bin_size * i).astype(F32) * (i + F32(1)).astype(F32)).astype(F32) + ds).astype(F32)
        else:
            cd = ((bin_size * i).astype(F32) + ds).astype(F32)
        cd = cd[:, None, None]  # [D, 1, 1]
        s = np.where(cd < EPS, EPS, cd).astype(F32)
        x = (cw * s).astype(F32) + np.zeros((D, H, W), F32)
        y = (ch * s).astype(F32) + np.zeros((D, H, W), F32)
        normalised = np.empty((BN, D, 3, H, W), F32)
        for c in range(3):
            mc = m[:, c, :, None, None, None]  # [BN, 4, 1, 1, 1]
            val = ((mc[:, 0] * x).astype(F32) + (mc[:, 1] * y).astype(F32)).astype(F32)
            val = (val + (mc[:, 2] * cd).astype(F32)).astype(F32)
            val = (val + mc[:, 3]).astype(F32)
            normalised[:, :, c] = ((val - r[c]).astype(F32) / den[c]).astype(F32)
        outside = (normalised > 1) | (normalised < 0)
        mask = 2 * outside.sum((1, 2)) > D
        if token_mask is not None:
            mask = mask | (np.asarray(token_mask).reshape(BN, H, W) != 0)
        n = np.where(normalised < 0, F32(0), np.where(normalised > 1, F32(1), normalised)).astype(F32)
        x1 = np.where(n < EPS, EPS, n).astype(F32)
        u = (F32(1) - n).astype(F32)
        x2 = np.where(u < EPS, EPS, u).astype(F32)
        ratio = (x1 / x2).astype(F32)
    return ratio.reshape(BN, 3 * D, H, W), mask, normalised.reshape(BN, 3 * D, H, W)


def coords3d(*args, **kwargs):
    ratio, mask, _ = coords3d_ratio(*args, **kwargs)
    with np.errstate(all="ignore"):
        return np.log(ratio.astype(np.float64)).astype(F32), mask
