"""NumPy restatement of csrc/cape.hip, operation for operation in float32 (the order is the one in that file's header).

cva(q_a, q_g, k_a, k_g, v, scale_a, scale_g, num_heads, expf, mask=None)    pd3_cape_cva_forward: q_a [B, Q, E], q_g [B,
    N, Q, E], k_a, k_g, v [B, N, K, E], mask [B, N, K] (non-zero: masked), scale_a / scale_g [M] -> [B, Q, E]
posemb3d(points, dim_t, sinf, cosf, bound=None, rot=None, trans=None)        pd3_cape_posemb3d: points [B, Q, 3] -> [B,
    N, Q, 3 F] with rot [B, N, 3, 3] and trans [B, N, 3], [B, Q, 3 F] without
dim_t(num_feats, temperature=10000)    the reference's own expression for pos2posemb3d's divisors (torch on the CPU, as
    paddle3d_amd.ops.cape.dim_t computes it)

`expf`, `sinf`, `cosf` are float32 array functions with glibc's bits (oracle.pyoracle.libm_eval(2 / 0 / 1, x)); fmaf is
pv_rcnn_numpy's correctly rounded one.
"""
import numpy as np

from petr_numpy import TILE_ORDER, WAVES
from pv_rcnn_numpy import fmaf

F32 = np.float32
TWO_PI = F32(2.0 * np.pi)


def _chain(q, k):
    """q [..., Q, d], k [..., K, d] -> [..., Q, K]: the ascending-channel fmaf chain from +0."""
    s = np.zeros(q.shape[:-1] + (k.shape[-2],), F32)
    for c in range(q.shape[-1]):
        s = fmaf(q[..., :, None, c], k[..., None, :, c], s)
    return s


def cva(q_a, q_g, k_a, k_g, v, scale_a, scale_g, num_heads, expf, mask=None):
    q_a, q_g, k_a, k_g, v = (np.asarray(t, F32) for t in (q_a, q_g, k_a, k_g, v))
    B, N, K, E = k_a.shape
    Q, M = q_a.shape[1], num_heads
    d = E // M
    KT = -(-K // 16)
    KP = KT * 16          # keys of a camera with its padding
    NT = N * KT           # tiles of the padded list
    sa = np.asarray(scale_a, F32).reshape(1, M, 1, 1, 1)
    sg = np.asarray(scale_g, F32).reshape(1, M, 1, 1, 1)
    with np.errstate(all="ignore"):
        qa = q_a.reshape(B, Q, M, d).transpose(0, 2, 1, 3)[:, :, None]          # [B, M, 1, Q, d]
        qg = q_g.reshape(B, N, Q, M, d).transpose(0, 3, 1, 2, 4)                # [B, M, N, Q, d]
        ka, kg, vh = (t.reshape(B, N, K, M, d).transpose(0, 3, 1, 2, 4) for t in (k_a, k_g, v))  # [B, M, N, K, d]
        a = _chain(np.broadcast_to(qa, qg.shape), ka)                           # [B, M, N, Q, K]
        g = _chain(qg, kg)
        t = ((a * sa).astype(F32) + (g * sg).astype(F32)).astype(F32)
        if mask is not None:
            msk = np.asarray(mask).reshape(B, 1, N, 1, K) != 0
            t = np.where(msk, F32(-np.inf), t).astype(F32)
        # the padded key list: [B, M, Q, N * KP], padding keys invalid
        tp = np.zeros((B, M, N, Q, KP), F32)
        tp[..., :K] = t
        tp = tp.transpose(0, 1, 3, 2, 4).reshape(B, M, Q, N * KP)
        valid = np.tile(np.arange(KP) < K, N)
        nan = np.isnan(tp) & valid
        mx = np.where(nan | ~valid, -np.inf, tp).max(-1).astype(F32)
        mx = np.where(nan[..., 0], tp[..., 0], mx)
        e = expf((tp - mx[..., None]).astype(F32)).reshape(tp.shape).astype(F32)
        e = np.where(valid, e, F32(0)).astype(F32)
        lanes = np.zeros(e.shape[:-1] + (-(-NT // WAVES) * 64,), F32)
        lanes[..., :N * KP] = e
        lanes = lanes.reshape(e.shape[:-1] + (-1, 64))
        p = np.zeros(e.shape[:-1] + (64,), F32)
        for step in range(lanes.shape[-2]):
            p = (p + lanes[..., step, :]).astype(F32)
        h = 32
        while h >= 1:
            p = (p[..., :h] + p[..., h:2 * h]).astype(F32)
            h //= 2
        vp = np.zeros((B, M, N, KP, d), F32)
        vp[:, :, :, :K] = vh
        vp = vp.reshape(B, M, N * KP, d)
        parts = []
        for w in range(WAVES):
            acc = np.zeros((B, M, Q, d), F32)
            for T in range(w, NT, WAVES):
                for o in TILE_ORDER:
                    j = 16 * T + o
                    acc = fmaf(e[..., j:j + 1], vp[:, :, None, j, :], acc)
            parts.append(acc)
        s = (((parts[0] + parts[1]).astype(F32) + parts[2]).astype(F32) + parts[3]).astype(F32)
        out = (s / p).astype(F32)
    return np.ascontiguousarray(out.transpose(0, 2, 1, 3)).reshape(B, Q, E)


def dim_t(num_feats, temperature=10000):
    import torch

    t = torch.arange(num_feats, dtype=torch.int32)
    return (temperature ** (2 * (t // 2) / num_feats)).numpy().astype(F32)


def posemb3d(points, dim_t, sinf, cosf, bound=None, rot=None, trans=None):
    p = np.asarray(points, F32)
    dt = np.asarray(dim_t, F32)
    F = dt.size
    with np.errstate(all="ignore"):
        if bound is not None:
            b = np.asarray(bound, F32).reshape(2, 3)
            span = (b[1] - b[0]).astype(F32)
            p = ((p * span).astype(F32) + b[0]).astype(F32)
        if rot is not None:
            R, t = np.asarray(rot, F32), np.asarray(trans, F32)
            w = (p[:, None] + t[:, :, None]).astype(F32)                                    # [B, N, Q, 3]
            x = [(((R[:, :, None, r, 0] * w[..., 0]).astype(F32) + (R[:, :, None, r, 1] * w[..., 1]).astype(F32)).astype(F32)
                  + (R[:, :, None, r, 2] * w[..., 2]).astype(F32)).astype(F32) for r in range(3)]
            p = np.stack(x, -1)
        s = (p * TWO_PI).astype(F32)
        y = (s[..., None] / dt).astype(F32)                                                 # [..., 3, F]
        flat = np.ascontiguousarray(y).reshape(-1)
        e = np.where(np.arange(F) % 2 == 0, sinf(flat).reshape(y.shape), cosf(flat).reshape(y.shape)).astype(F32)
    return np.ascontiguousarray(np.concatenate([e[..., 1, :], e[..., 0, :], e[..., 2, :]], -1))
