"""NumPy restatement of the two entry points of csrc/iassd.hip (IA-SSD at inference; TEST INFRASTRUCTURE ONLY), in the
kernels' operation order (include/paddle3d_amd.h states the same contract):

  sa_msg_pool    pd3_ball_query_batch's row (pointnet2_numpy.ball_query: unused slots repeat the first hit, a row
                 without a hit is point 0 of the frame), d = xyz[b, idx] - new_xyz;
                 h1 = relu(scale1 * (f + ((w0 * dx + w1 * dy) + w2 * dz)) + shift1);
                 h2 = relu(scale2 * (sum_j w2[c, j] * h1[j]) + shift2); h3 likewise from h2 and w3; max over the slots
                 (= over the hits: the other slots repeat one).  In float32 each sum is the ascending-j fmaf chain
                 from 0 (pv_rcnn_numpy.fmaf is correctly rounded), which is what the device computes bit for bit;
                 dtype float64 evaluates the same sums in float64 (the error bound's yardstick).
                 w1_full / features give the materialised first layer instead: W1 @ [d; f] as the reference's
                 convolution over the concatenated tensor (a matrix product in `dtype`).
  iassd_decode   the class is the first maximum of the raw logits (a NaN counts as the maximum); with mean_size
                 diagonal = sqrt(dxa * dxa + dya * dya), x = xt * diagonal + xa, ..., dx = expf(dxt) * dxa, ...; without
                 x = xt + xa, dx = expf(dxt); the bin by the same argmax, its residual selected;
                 heading = ((float(bin) * bin_inter - pi) + half) + res * half.  float32 without FMA, glibc's expf
                 (oracle.pyoracle.libm_eval).  Exact.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pointnet2_numpy as pn  # noqa: E402
from pv_rcnn_numpy import fmaf  # noqa: E402

F32 = np.float32
F64 = np.float64


def expf(x):
    from oracle import pyoracle as O

    x = np.ascontiguousarray(x, F32)
    return O.libm_eval(2, x.reshape(-1)).reshape(x.shape)


def _relu(v, T):
    return np.where(np.isnan(v), v, np.where(v > 0, v, T(0))).astype(T)


def _layer(h, w, scale, shift, T):
    """h [..., cin] -> relu(scale * (h @ w^T) + shift) [..., cout]; float32: the fmaf chain."""
    w = np.asarray(w, F32)
    sc, sh = np.asarray(scale, F32).astype(T), np.asarray(shift, F32).astype(T)
    if T is F32:
        acc = np.zeros(h.shape[:-1] + (w.shape[0],), F32)
        for j in range(w.shape[1]):
            acc = fmaf(h[..., j:j + 1], w[:, j], acc)
    else:
        acc = h @ w.astype(T).T
    return _relu(((sc * acc).astype(T) + sh).astype(T), T)


def sa_msg_pool(new_xyz, xyz, features_in, w_pos, scale1, shift1, w2, scale2, shift2, w3, scale3, shift3, radius,
                nsample, dtype=F32, w1_full=None, features=None, chunk=512):
    """pooled [B, M, C3] in `dtype`.  features_in [B, N, C1] or None; with w1_full [C1, 3 + C] and features [B, N, C]
    (or None when C == 0) the first layer is the materialised W1 @ [d; f] instead of the factorised form."""
    T = dtype
    q, p = np.asarray(new_xyz, F32), np.asarray(xyz, F32)
    B, M, _ = q.shape
    idx = pn.ball_query(q, p, radius, nsample).astype(np.int64)  # [B, M, S]
    C3 = np.asarray(w3).shape[0]
    out = np.zeros((B, M, C3), T)
    sc1, sh1 = np.asarray(scale1, F32).astype(T), np.asarray(shift1, F32).astype(T)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            for i in range(0, M, chunk):
                r = idx[b, i:i + chunk]  # [m, S]
                d = (p[b][r].astype(T) - q[b, i:i + chunk, None, :].astype(T)).astype(T)  # [m, S, 3]
                if w1_full is not None:
                    w1 = np.asarray(w1_full, F32).astype(T)
                    x = d if features is None else np.concatenate([d, np.asarray(features, F32)[b][r].astype(T)], -1)
                    lin = (x @ w1.T).astype(T)
                else:
                    wt = np.asarray(w_pos, F32).astype(T)
                    lin = ((wt[:, 0] * d[..., 0:1]).astype(T) + (wt[:, 1] * d[..., 1:2]).astype(T)).astype(T)
                    lin = (lin + (wt[:, 2] * d[..., 2:3]).astype(T)).astype(T)
                    if features_in is not None:
                        lin = (np.asarray(features_in, F32)[b][r].astype(T) + lin).astype(T)
                    else:
                        lin = (T(0) + lin).astype(T)
                h = _relu(((sc1 * lin).astype(T) + sh1).astype(T), T)  # [m, S, C1]
                h = _layer(h, w2, scale2, shift2, T)
                h = _layer(h, w3, scale3, shift3, T)
                nan = np.isnan(h).any(axis=1)
                out[b, i:i + chunk] = np.where(nan, T(np.nan), np.nanmax(np.where(np.isnan(h), T(0), h), axis=1))
    return out


def argmax_first(v):
    """The first maximum along the last axis with a NaN counting as the maximum (torch.argmax)."""
    v = np.asarray(v, F32)
    best = np.zeros(v.shape[:-1], np.int64)
    bv = v[..., 0].copy()
    with np.errstate(invalid="ignore"):
        for i in range(1, v.shape[-1]):
            x = v[..., i]
            take = ~np.isnan(bv) & ((x > bv) | np.isnan(x))
            best = np.where(take, i, best)
            bv = np.where(take, x, bv)
    return best


def iassd_decode(cls_preds, box_preds, centers, mean_size, bins):
    """cls_preds [M, K], box_preds [M, 6 + 2 * bins], centers [M, 3], mean_size [K, 3] or None -> boxes [M, 7]."""
    cl, e, c = np.asarray(cls_preds, F32), np.asarray(box_preds, F32), np.asarray(centers, F32)
    M = e.shape[0]
    out = np.zeros((M, 7), F32)
    bin_inter = 2 * np.pi / bins
    bi, pi, half = F32(bin_inter), F32(np.pi), F32(bin_inter / 2)
    with np.errstate(all="ignore"):
        ex = expf(e[:, 3:6])
        if mean_size is not None:
            a = np.asarray(mean_size, F32)[argmax_first(cl)]
            dxa, dya, dza = a[:, 0], a[:, 1], a[:, 2]
            diagonal = np.sqrt(((dxa * dxa).astype(F32) + (dya * dya).astype(F32)).astype(F32)).astype(F32)
            out[:, 0] = ((e[:, 0] * diagonal).astype(F32) + c[:, 0]).astype(F32)
            out[:, 1] = ((e[:, 1] * diagonal).astype(F32) + c[:, 1]).astype(F32)
            out[:, 2] = ((e[:, 2] * dza).astype(F32) + c[:, 2]).astype(F32)
            out[:, 3:6] = (ex * a).astype(F32)
        else:
            out[:, 0:3] = (e[:, 0:3] + c).astype(F32)
            out[:, 3:6] = ex
        b = argmax_first(e[:, 6:6 + bins])
        res = e[np.arange(M), 6 + bins + b]
        rg = (((b.astype(F32) * bi).astype(F32) - pi).astype(F32) + half).astype(F32)
        out[:, 6] = (rg + (res * half).astype(F32)).astype(F32)
    return out


def fold_bn(state, prefix, eps=1e-5):
    """(scale, shift) of the eval BatchNorm at `prefix` of a Paddle-named state dict, in float32."""
    g, b = np.asarray(state[prefix + ".weight"], F32), np.asarray(state[prefix + ".bias"], F32)
    mean, var = np.asarray(state[prefix + "._mean"], F32), np.asarray(state[prefix + "._variance"], F32)
    scale = (g / np.sqrt((var + F32(eps)).astype(F32)).astype(F32)).astype(F32)
    return scale, (b - (mean * scale).astype(F32)).astype(F32)


def scale_params(state, prefix, i):
    """Scale i of the SA layer at `prefix` in sa_msg_pool's form: (w_pos, w_feat, [scale1, shift1, w2, ..., shift3])."""
    w1 = np.asarray(state[f"{prefix}.mlps.{i}.0.weight"], F32).reshape(-1, state[f"{prefix}.mlps.{i}.0.weight"].shape[1])
    rest = list(fold_bn(state, f"{prefix}.mlps.{i}.1"))
    for k in (3, 6):
        w = np.asarray(state[f"{prefix}.mlps.{i}.{k}.weight"], F32)
        rest += [w.reshape(w.shape[0], -1), *fold_bn(state, f"{prefix}.mlps.{i}.{k + 1}")]
    return np.ascontiguousarray(w1[:, :3]), np.ascontiguousarray(w1[:, 3:]), rest
