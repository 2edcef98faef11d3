"""NumPy restatement of the reference's ms_deform_attn op (paddle3d/ops/ms_deform_attn), forward and backward, in
float32 or float64, in the reference kernel's operation order:

  ms_deform_attn_cuda_kernel.h:220-274  forward loop: levels outer, points inner; h = loc_y * H - 0.5,
                                        w = loc_x * W - 0.5; range test h > -1 && w > -1 && h < H && w < W;
                                        col += bilinear * weight
  ms_deform_attn_cuda_kernel.h:37-84    bilinear: h_low = floorf(h) (a float floor also for double), lh = h - h_low,
                                        hh = 1 - lh; corners outside the map are 0;
                                        ((w1*v1 + w2*v2) + w3*v3) + w4*v4, w1 = hh*hw, w2 = hh*lw, w3 = lh*hw,
                                        w4 = lh*lw
  ms_deform_attn_cuda_kernel.h:86-151   gradient: grad_value += w_k * (grad_out * weight) at the corners,
                                        grad_attn = sum_c grad_out * val, grad_loc = sum_c (W * gw, H * gh) * tg

Rules the reference leaves open: a corner whose value row level_start + y*W + x falls outside [0, S) counts as 0
(the reference would read outside value), and a level with H or W outside [1, 2^31 - 1] or |level_start| > 2^62
contributes nothing (its row arithmetic could overflow).  csrc/ms_deform_attn.hip follows the same text; its fp32 /
fp64 forward equals forward() bit for bit.  grid_sample_attn() is an independent torch formulation (F.grid_sample per level and
head) used to check this restatement.
"""
import numpy as np


def _point(shapes, starts, S, l, lx, ly, T):
    """Range test, corner rows (or -1) and weights of one (level, point) for every (b, q, m)."""
    H, W, s0 = int(shapes[l, 0]), int(shapes[l, 1]), int(starts[l])
    level_ok = 1 <= H <= 2**31 - 1 and 1 <= W <= 2**31 - 1 and abs(s0) <= 2**62
    if not level_ok:
        H = W = s0 = 0
    with np.errstate(invalid="ignore", over="ignore"):
        h = ly * T(H) - T(0.5)
        w = lx * T(W) - T(0.5)
        ok = (h > T(-1)) & (w > T(-1)) & (h < T(H)) & (w < T(W)) & level_ok
    h = np.where(ok, h, T(0)).astype(T)
    w = np.where(ok, w, T(0)).astype(T)
    h0 = np.floor(h.astype(np.float32)).astype(np.int64)
    w0 = np.floor(w.astype(np.float32)).astype(np.int64)
    lh = (h - h0.astype(T)).astype(T)
    lw = (w - w0.astype(T)).astype(T)
    hh = (T(1) - lh).astype(T)
    hw = (T(1) - lw).astype(T)
    wts = [hh * hw, hh * lw, lh * hw, lh * lw]
    rows = []
    for k in range(4):
        y, x = h0 + (k >> 1), w0 + (k & 1)
        r = s0 + y * W + x
        valid = ok & (y >= 0) & (y < H) & (x >= 0) & (x < W) & (r >= 0) & (r < S)
        rows.append(np.where(valid, r, -1))
    return dict(ok=ok, rows=rows, w=wts, hh=hh, hw=hw, lh=lh, lw=lw, H=H, W=W)


def _gather(vrows, rows, b_off, m_idx, T):
    valid = rows >= 0
    idx = np.where(valid, rows + b_off, 0)
    v = vrows[idx, m_idx]  # [B, Q, M, C]
    return np.where(valid[..., None], v, T(0)).astype(T), valid


def forward(value, loc, attn, shapes, starts):
    """value [B, S, M, C], loc [B, Q, M, L, P, 2], attn [B, Q, M, L, P], shapes [L, 2], starts [L] -> [B, Q, M*C]
    in value's dtype."""
    T = value.dtype.type
    B, S, M, C = value.shape
    _, Q, _, L, P, _ = loc.shape
    vrows = value.reshape(B * S, M, C)
    b_off = (np.arange(B, dtype=np.int64) * S)[:, None, None]
    m_idx = np.arange(M)[None, None, :]
    col = np.zeros((B, Q, M, C), T)
    for l in range(L):
        for p in range(P):
            t = _point(shapes, starts, S, l, loc[:, :, :, l, p, 0], loc[:, :, :, l, p, 1], T)
            v = [_gather(vrows, r, b_off, m_idx, T)[0] for r in t["rows"]]
            w = [x[..., None] for x in t["w"]]
            val = ((w[0] * v[0] + w[1] * v[1]) + w[2] * v[2]) + w[3] * v[3]
            col = np.where(t["ok"][..., None], col + val * attn[:, :, :, l, p][..., None], col).astype(T)
    return col.reshape(B, Q, M * C)


def backward(grad_out, value, loc, attn, shapes, starts):
    """-> (grad_value, grad_loc, grad_attn) in value's dtype (channel sums in channel order, grad_value summed in
    (level, point, corner) order)."""
    T = value.dtype.type
    B, S, M, C = value.shape
    _, Q, _, L, P, _ = loc.shape
    vrows = value.reshape(B * S, M, C)
    b_off = (np.arange(B, dtype=np.int64) * S)[:, None, None]
    m_idx = np.broadcast_to(np.arange(M)[None, None, :], (B, Q, M))
    go = grad_out.reshape(B, Q, M, C)
    gv = np.zeros((B * S * M, C), T)
    gl = np.zeros(loc.shape, T)
    ga = np.zeros(attn.shape, T)
    for l in range(L):
        for p in range(P):
            t = _point(shapes, starts, S, l, loc[:, :, :, l, p, 0], loc[:, :, :, l, p, 1], T)
            a = attn[:, :, :, l, p][..., None]
            tg = go * a
            gh = np.zeros((B, Q, M, C), T)
            gw = np.zeros((B, Q, M, C), T)
            vs = []
            ex = lambda x: x[..., None]  # noqa: E731
            signs = [(-ex(t["hw"]), -ex(t["hh"])), (-ex(t["lw"]), ex(t["hh"])), (ex(t["hw"]), -ex(t["lh"])),
                     (ex(t["lw"]), ex(t["lh"]))]
            for k in range(4):
                v, valid = _gather(vrows, t["rows"][k], b_off, m_idx, T)
                vs.append(v)
                sh, sw = signs[k]
                gh = np.where(valid[..., None], gh + sh * v, gh)
                gw = np.where(valid[..., None], gw + sw * v, gw)
                upd = ex(t["w"][k]) * tg
                sel = valid
                dst = ((t["rows"][k] + b_off) * M + m_idx)[sel]
                np.add.at(gv, dst, upd[sel])
            w = [ex(x) for x in t["w"]]
            val = ((w[0] * vs[0] + w[1] * vs[1]) + w[2] * vs[2]) + w[3] * vs[3]
            ok = t["ok"]
            ga[:, :, :, l, p] = np.where(ok, (go * val).sum(-1), T(0))
            gl[:, :, :, l, p, 0] = np.where(ok, ((T(t["W"]) * gw) * tg).sum(-1), T(0))
            gl[:, :, :, l, p, 1] = np.where(ok, ((T(t["H"]) * gh) * tg).sum(-1), T(0))
    return gv.reshape(B, S, M, C), gl, ga


def level_layout(shapes):
    """spatial_shapes [[H, W], ...] -> (shapes int64 [L, 2], level_start_index int64 [L], S)."""
    shapes = np.asarray(shapes, np.int64).reshape(-1, 2)
    sizes = shapes[:, 0] * shapes[:, 1]
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    return shapes, starts, int(sizes.sum())


def random_case(rng, B, Q, M, C, shapes, P, dtype=np.float32, lo=-0.1, hi=1.1):
    """value N(0, 1), locations uniform in [lo, hi] (a margin outside [0, 1]), softmax-like positive weights."""
    shapes, starts, S = level_layout(shapes)
    L = shapes.shape[0]
    value = rng.standard_normal((B, S, M, C)).astype(dtype)
    loc = rng.uniform(lo, hi, (B, Q, M, L, P, 2)).astype(dtype)
    attn = rng.uniform(0.0, 1.0, (B, Q, M, L, P)).astype(dtype)
    attn = (attn / attn.sum(axis=(-1, -2), keepdims=True)).astype(dtype)
    return value, loc, attn, shapes, starts


def grid_sample_attn(value, loc, attn, shapes, starts):
    """Independent torch formulation (CPU tensors, any float dtype): per level, F.grid_sample(bilinear, zeros,
    align_corners=False) of each head's [C, H, W] map at 2*loc - 1, weighted and summed over levels and points."""
    import torch
    import torch.nn.functional as F

    B, S, M, C = value.shape
    _, Q, _, L, P, _ = loc.shape
    out = None
    for l in range(L):
        H, W, s0 = int(shapes[l, 0]), int(shapes[l, 1]), int(starts[l])
        v = value[:, s0:s0 + H * W].reshape(B, H, W, M, C).permute(0, 3, 4, 1, 2).reshape(B * M, C, H, W)
        g = (2 * loc[:, :, :, l] - 1).permute(0, 2, 1, 3, 4).reshape(B * M, Q, P, 2)
        s = F.grid_sample(v, g, mode="bilinear", padding_mode="zeros", align_corners=False)  # [B*M, C, Q, P]
        a = attn[:, :, :, l].permute(0, 2, 1, 3).reshape(B * M, 1, Q, P)
        term = (s * a).sum(-1)  # [B*M, C, Q]
        out = term if out is None else out + term
    return out.reshape(B, M, C, Q).permute(0, 3, 1, 2).reshape(B, Q, M * C)
