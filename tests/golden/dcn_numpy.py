"""NumPy restatement of csrc/deform_conv.hip, operation for operation (the order is the one in that file's header), in
the gather form: for every tap the four corners are indexed straight out of x.

sample_columns(x, offset, mask, stride, padding, dilation, dtype=F32, mask_is_logit=False, expf=None)
    p [N, Cin, 9, Ho, Wo]: the bilinear sample of every (channel, tap) times the tap's modulation, every operation
    rounded to `dtype`
deform_conv2d(x, offset, mask, weight, scale=None, shift=None, relu=False, mask_is_logit=False, stride=1, padding=0,
              dilation=1, expf=None)
    pd3_deform_conv2d_forward with the UNPACKED weight [Cout, Cin, 3, 3] -> y [N, Cout, Ho, Wo] float32: ONE fmaf chain
    over ascending j = c * 9 + k per output
deform_conv2d_f64(x, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1, mask_is_logit=False)
    the same formulas in float64 with a plain sum: what the float32 form is an evaluation of

`expf` is a float32 array function with glibc's bits (oracle.pyoracle.libm_eval(2, x)); fmaf is pv_rcnn_numpy's
correctly rounded one.
"""
import numpy as np

from pv_rcnn_numpy import fmaf

F32 = np.float32
F64 = np.float64


def output_size(size, stride, padding, dilation):
    return (size + 2 * padding - 2 * dilation - 1) // stride + 1


def modulation(mask, shape, dtype, mask_is_logit=False, expf=None):
    """m [N, 9, Ho, Wo]: ones without a mask, the mask, or 1 / (1 + expf(-mask))."""
    if mask is None:
        return np.ones(shape, dtype)
    m = np.asarray(mask, dtype)
    if not mask_is_logit:
        return m
    with np.errstate(all="ignore"):
        if dtype == F32:
            e = expf(np.ascontiguousarray(-m).reshape(-1)).reshape(m.shape).astype(F32)
        else:
            e = np.exp(-m)
        return (dtype(1) / (dtype(1) + e).astype(dtype)).astype(dtype)


def sample_columns(x, offset, mask, stride, padding, dilation, dtype=F32, mask_is_logit=False, expf=None):
    x, offset = np.asarray(x, dtype), np.asarray(offset, dtype)
    N, C, H, W = x.shape
    Ho, Wo = output_size(H, stride, padding, dilation), output_size(W, stride, padding, dilation)
    assert offset.shape == (N, 18, Ho, Wo), (offset.shape, (N, 18, Ho, Wo))
    m = modulation(mask, (N, 9, Ho, Wo), dtype, mask_is_logit, expf)
    p = np.zeros((N, C, 9, Ho, Wo), dtype)
    n_idx = np.arange(N)[:, None, None]
    ho = np.arange(Ho)[None, :, None]
    wo = np.arange(Wo)[None, None, :]
    with np.errstate(all="ignore"):
        for k in range(9):
            ky, kx = divmod(k, 3)
            h = ((ho * stride - padding + ky * dilation).astype(dtype) + offset[:, 2 * k]).astype(dtype)
            w = ((wo * stride - padding + kx * dilation).astype(dtype) + offset[:, 2 * k + 1]).astype(dtype)
            inside = (h > -1) & (w > -1) & (h < H) & (w < W)  # a NaN fails every comparison
            h, w = np.where(inside, h, dtype(0)), np.where(inside, w, dtype(0))  # before any float -> int conversion
            hl, wl = np.floor(h), np.floor(w)
            lh, lw = (h - hl).astype(dtype), (w - wl).astype(dtype)
            hh, hw = (dtype(1) - lh).astype(dtype), (dtype(1) - lw).astype(dtype)
            ih, iw = hl.astype(np.int64), wl.astype(np.int64)

            def corner(yy, xx):
                ok = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
                v = x[n_idx, :, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]  # [N, Ho, Wo, C]
                return np.where(ok[..., None], v, dtype(0)).transpose(0, 3, 1, 2)

            v1, v2, v3, v4 = corner(ih, iw), corner(ih, iw + 1), corner(ih + 1, iw), corner(ih + 1, iw + 1)
            c1, c2 = (hh * hw).astype(dtype)[:, None], (hh * lw).astype(dtype)[:, None]
            c3, c4 = (lh * hw).astype(dtype)[:, None], (lh * lw).astype(dtype)[:, None]
            val = (c1 * v1).astype(dtype)
            val = (val + (c2 * v2).astype(dtype)).astype(dtype)
            val = (val + (c3 * v3).astype(dtype)).astype(dtype)
            val = (val + (c4 * v4).astype(dtype)).astype(dtype)
            val = np.where(inside[:, None], val, dtype(0))
            p[:, :, k] = (val * m[:, k][:, None]).astype(dtype)
    return p


def deform_conv2d(x, offset, mask, weight, scale=None, shift=None, relu=False, mask_is_logit=False, stride=1, padding=0,
                  dilation=1, expf=None):
    weight = np.asarray(weight, F32)
    Co, C = weight.shape[:2]
    p = sample_columns(x, offset, mask, stride, padding, dilation, F32, mask_is_logit, expf)
    N, _, _, Ho, Wo = p.shape
    with np.errstate(all="ignore"):
        y = np.zeros((N, Co, Ho, Wo), F32)
        for c in range(C):
            for k in range(9):
                y = fmaf(p[:, c, k][:, None], weight[None, :, c, k // 3, k % 3, None, None], y)
        if scale is not None:
            y = (y * np.asarray(scale, F32)[None, :, None, None]).astype(F32)
        if shift is not None:
            y = (y + np.asarray(shift, F32)[None, :, None, None]).astype(F32)
        if relu:
            y = np.where(y > 0, y, np.where(np.isnan(y), y, F32(0))).astype(F32)
    return y


def deform_conv2d_f64(x, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1, mask_is_logit=False):
    p = sample_columns(x, offset, mask, stride, padding, dilation, F64, mask_is_logit)
    N, C, _, Ho, Wo = p.shape
    w = np.asarray(weight, F64).reshape(weight.shape[0], C * 9)
    y = np.einsum("oj,njhw->nohw", w, p.reshape(N, C * 9, Ho, Wo))
    if bias is not None:
        y = y + np.asarray(bias, F64)[None, :, None, None]
    return y
