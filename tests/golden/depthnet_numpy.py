"""NumPy restatement of csrc/depthnet.hip, operation for operation (the order is the one in that file's header).

channel_sums(x, dtype=F32)
    [N, C]: lane l adds the elements l, l + 64, ... of a plane in ascending order, then the 64 partial sums are folded
    32, 16, 8, 4, 2, 1
aspp_bias(x, p, dtype=F32)
    the pooled branch as the per-image bias [N, Cmid] behind conv1, bn1's scale applied
aspp_branches(x, p, dilations=(6, 12, 18), dtype=F32, count=None)
    [N, 4 Cmid, H, W]: per branch one chain over the taps that lie inside the image ONLY, in ascending (ky, kx), and per
    tap over the input channels in ascending order; folded BatchNorm, relu.  `count` (a list) receives the number of
    (pixel, tap) pairs each branch multiplied
aspp_forward(x, p, dilations=(6, 12, 18), dtype=F32)
    pd3_aspp_forward -> [N, Cmid, H, W]
depth_softmax_split(x, D, expf=None, dtype=F32)
    pd3_depth_softmax_split -> (depth [N, D, H, W], tran_feat [N, H, W, C])

`p` is a dict of UNPACKED arrays: w (the four atrous weights), scale / shift [4 Cmid] (their folded BatchNorms), wg
[Cmid, Cin] with gs / gb [Cmid] (the pooled branch), w1 [Cmid, 5 Cmid] with s1 / b1 [Cmid] (conv1 and the folded bn1).
dtype=F64 evaluates the same formulas in float64 with a plain multiply-add: what the float32 form is an evaluation of.
`expf` is a float32 array function with glibc's bits (oracle.pyoracle.libm_eval(2, x)); fmaf is pv_rcnn_numpy's correctly
rounded one.
"""
import numpy as np

from pv_rcnn_numpy import fmaf

F32 = np.float32
F64 = np.float64


def _fma(a, b, c, dtype):
    if dtype == F32:
        return fmaf(a, b, c)
    return np.asarray(a, F64) * np.asarray(b, F64) + c


def relu(r):
    return np.where(r > 0, r, np.where(np.isnan(r), r, r.dtype.type(0))).astype(r.dtype)


def fold(gamma, beta, mean, var, eps=1e-5, dtype=F32):
    """A BatchNorm's (scale, shift) as ops.squeezeseg.fold_batch_norm computes them: in float64, rounded to `dtype`."""
    g, b, m, v = (np.asarray(t, F64) for t in (gamma, beta, mean, var))
    scale = g / np.sqrt(v + float(eps))
    return scale.astype(dtype), (-m * scale + b).astype(dtype)


def aspp_params(state, dtype=F32, prefix=""):
    """The dict `p` of the functions below from an ASPP's state under the reference's keys."""
    def bn(name):
        return fold(*(state[f"{prefix}{name}.{k}"] for k in ("weight", "bias", "_mean", "_variance")), dtype=dtype)

    folds = [bn(f"aspp{i}.bn") for i in (1, 2, 3, 4)]
    gs, gb = bn("global_avg_pool.2")
    s1, b1 = bn("bn1")
    w1 = np.asarray(state[f"{prefix}conv1.weight"], dtype)
    return dict(w=[np.asarray(state[f"{prefix}aspp{i}.atrous_conv.weight"], dtype) for i in (1, 2, 3, 4)],
                scale=np.concatenate([s for s, _ in folds]), shift=np.concatenate([b for _, b in folds]),
                wg=np.asarray(state[f"{prefix}global_avg_pool.1.weight"], dtype).reshape(w1.shape[0], -1), gs=gs, gb=gb,
                w1=w1.reshape(w1.shape[0], -1), s1=s1, b1=b1)


def channel_sums(x, dtype=F32):
    x = np.asarray(x, dtype)
    N, C, H, W = x.shape
    flat = x.reshape(N, C, H * W)
    if dtype == F64:
        return flat.sum(-1)
    rows = -(-H * W // 64)
    padded = np.zeros((N, C, rows * 64), F32)  # + (+0) changes no partial sum: none of them is ever -0
    padded[..., :H * W] = flat
    padded = padded.reshape(N, C, rows, 64)
    with np.errstate(all="ignore"):
        part = np.zeros((N, C, 64), F32)
        for r in range(rows):
            part = (part + padded[:, :, r]).astype(F32)
        for s in (32, 16, 8, 4, 2, 1):
            part = (part[..., :s] + part[..., s:2 * s]).astype(F32)
    return part[..., 0]


def aspp_bias(x, p, dtype=F32):
    x = np.asarray(x, dtype)
    N, C, H, W = x.shape
    wg, w1 = np.asarray(p["wg"], dtype), np.asarray(p["w1"], dtype)
    cm = wg.shape[0]
    with np.errstate(all="ignore"):
        mean = (channel_sums(x, dtype) / dtype(H * W)).astype(dtype)
        g = np.zeros((N, cm), dtype)
        for c in range(C):
            g = _fma(mean[:, c, None], wg[None, :, c], g, dtype)
        g = (g * np.asarray(p["gs"], dtype)[None]).astype(dtype)
        g = relu((g + np.asarray(p["gb"], dtype)[None]).astype(dtype))
        b = np.zeros((N, cm), dtype)
        for m in range(cm):
            b = _fma(g[:, m, None], w1[None, :, 4 * cm + m], b, dtype)
        return (b * np.asarray(p["s1"], dtype)[None]).astype(dtype)


def aspp_branches(x, p, dilations=(6, 12, 18), dtype=F32, count=None):
    x = np.asarray(x, dtype)
    N, C, H, W = x.shape
    cm = p["w"][0].shape[0]
    out = np.zeros((N, 4 * cm, H, W), dtype)
    with np.errstate(all="ignore"):
        for b, w in enumerate(p["w"]):
            w = np.asarray(w, dtype)
            d = 0 if b == 0 else int(dilations[b - 1])
            acc = np.zeros((N, cm, H, W), dtype)
            pairs = 0
            for ky in range(w.shape[2]):
                for kx in range(w.shape[3]):
                    dy, dx = (ky - 1) * d, (kx - 1) * d
                    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
                    if y0 >= y1 or x0 >= x1:
                        continue  # no pixel has this tap inside the image
                    pairs += (y1 - y0) * (x1 - x0)
                    sub = acc[:, :, y0:y1, x0:x1]
                    for c in range(C):
                        sub = _fma(x[:, c, None, y0 + dy:y1 + dy, x0 + dx:x1 + dx], w[None, :, c, ky, kx, None, None], sub,
                                   dtype)
                    acc[:, :, y0:y1, x0:x1] = sub
            if count is not None:
                count.append(pairs)
            sc = np.asarray(p["scale"], dtype)[b * cm:(b + 1) * cm, None, None]
            sh = np.asarray(p["shift"], dtype)[b * cm:(b + 1) * cm, None, None]
            out[:, b * cm:(b + 1) * cm] = relu(((acc * sc).astype(dtype) + sh).astype(dtype))
    return out


def aspp_forward(x, p, dilations=(6, 12, 18), dtype=F32):
    ws = aspp_branches(x, p, dilations, dtype)
    bias = aspp_bias(x, p, dtype)
    w1 = np.asarray(p["w1"], dtype)
    N, c4, H, W = ws.shape
    cm = c4 // 4
    with np.errstate(all="ignore"):
        acc = np.zeros((N, cm, H, W), dtype)
        for j in range(c4):
            acc = _fma(ws[:, j, None], w1[None, :, j, None, None], acc, dtype)
        r = (acc * np.asarray(p["s1"], dtype)[None, :, None, None]).astype(dtype)
        r = (r + bias[:, :, None, None]).astype(dtype)
        r = (r + np.asarray(p["b1"], dtype)[None, :, None, None]).astype(dtype)
        return relu(r)


def depth_softmax_split(x, D, expf=None, dtype=F32):
    x = np.asarray(x, dtype)
    with np.errstate(all="ignore"):
        m = x[:, 0].copy()
        for d in range(1, D):
            m = np.where(x[:, d] > m, x[:, d], m)
        z = (x[:, :D] - m[:, None]).astype(dtype)
        if dtype == F32:
            e = expf(np.ascontiguousarray(z).reshape(-1)).reshape(z.shape).astype(F32)
        else:
            e = np.exp(z)
        s = np.zeros_like(m)
        for d in range(D):
            s = (s + e[:, d]).astype(dtype)
        depth = (e / s[:, None]).astype(dtype)
    return depth, np.ascontiguousarray(x[:, D:].transpose(0, 2, 3, 1))
