"""SMOKE's head and post-processing at inference on the device (csrc/smoke.hip, C ABI pd3_smoke_head_forward /
pd3_smoke_post_process); the arithmetic order is stated in that file's header and restated in
tests/golden/smoke_numpy.py.

Reference: paddle3d/models/detection/smoke/smoke_predictor.py:78-97 (SMOKEPredictor.forward), processor.py:45-194
(PostProcessor.forward / export_forward), smoke_coder.py:103-347, :350-383 (the decoders), models/layers/
layer_libs.py:36-116, :181-207 (sigmoid_hm, nms_hm, select_topk, select_point_of_interest), layers/layer_norm.py:20-33
(group_norm).

smoke_head_forward(cls_feat, reg_feat, ...)
    the LAZY head from the two branches' 3x3 convolution outputs: the class branch runs densely down to the clipped
    heat map; the regression branch (norm, ReLU, 1x1 convolution, activations) is evaluated at the max_detection
    selected pixels only.
smoke_post_process(heat, regression, ...)
    the same selection and decode from SMOKEPredictor's two outputs.
group_norm_tables(feat, groups)
    the (mean, rstd) tables [B, 2, G] the kernels normalise with, on the host or the device, in float64 and rounded
    once (what pd3_smoke_head_forward computes itself when no tables are given); batch_norm_tables for norm_type="bn".
Both ops return (rows [B, max_detection, 14], counts int32 [B]) on the device, rows in descending score and zero past
counts[b], or None when the kernels do not take the shape (`smoke_supported`).  float32 only.  Nothing here
synchronises with the host; the kernels run on the current stream.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._common import check, gpu_tensor, lib, nchw_pitch, ptr, stream_ptr, workspace

__all__ = ["smoke_supported", "smoke_head_forward", "smoke_post_process", "group_norm_tables", "batch_norm_tables",
           "REG_CHANNELS", "MAX_K", "FORWARD", "EXPORT"]

_OP = "smoke"
_UNSUPPORTED = -3
REG_CHANNELS = (1, 2, 3, 2, 2)
MAX_K = 1024
FORWARD, EXPORT = 0, 1


def smoke_supported(channels, groups, num_classes, feat_h, feat_w, max_detection, reg_channels=REG_CHANNELS,
                    pred_2d=True):
    """The kernels' shape predicate.  channels=None: the from-maps form, which has no channel condition."""
    if channels is not None and not (1 <= channels <= 512 and groups >= 1 and channels % groups == 0 and
                                     channels * feat_h * (feat_w + 3) < 2 ** 31):
        return False
    hw = feat_h * feat_w
    return (bool(pred_2d) and tuple(reg_channels) == REG_CHANNELS and 1 <= num_classes <= 16 and
            1 <= max_detection <= min(MAX_K, hw) and num_classes * hw < 2 ** 30)


def group_norm_tables(feat, groups, eps=1e-5):
    """feat [B, C, H, W] -> float32 [B, 2, G]: per (frame, group) the mean and 1 / sqrt(biased variance + eps),
    computed in float64 and rounded once."""
    b, c = feat.shape[:2]
    x = feat.double().reshape(b, groups, -1)
    mean = x.mean(-1)
    var = ((x - mean[..., None]) ** 2).mean(-1)
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], 1).float()


def batch_norm_tables(running_mean, running_var, batch, eps=1e-5):
    """BatchNorm's running statistics as tables with G = C: float32 [B, 2, C] (mean, 1 / sqrt(var + eps) in float64,
    rounded once)."""
    t = torch.stack([running_mean.double(), 1.0 / torch.sqrt(running_var.double() + eps)]).float()
    return t[None].expand(int(batch), 2, t.shape[1]).contiguous()


def _camera(Ks, trans, image_size, depth_ref, dim_ref, b, nc, mode, dev):
    Ks = gpu_tensor(_OP, "Ks", Ks, dev=dev, shape=(b, 3, 3))
    if mode == FORWARD:
        trans = gpu_tensor(_OP, "trans_mat", trans, dev=dev, shape=(b, 3, 3))
        image_size = gpu_tensor(_OP, "image_size", image_size.reshape(-1)[:2], dev=dev, shape=(2,))
    else:
        trans = gpu_tensor(_OP, "down_ratios", trans.reshape(-1)[:2], dev=dev, shape=(2,))
        image_size = None
    return (Ks, trans, image_size, gpu_tensor(_OP, "depth_ref", depth_ref, dev=dev, shape=(2,)),
            gpu_tensor(_OP, "dim_ref", dim_ref, dev=dev, shape=(nc, 3)))


def _tail(reg_channels, max_detection, det_threshold, mode, pred_2d):
    reg = np.ascontiguousarray(np.asarray(tuple(reg_channels) + (0,) * 5, np.int32)[:5])
    return reg, (ptr(reg), int(max_detection), C.c_float(det_threshold), int(mode), int(bool(pred_2d)))


def _strided(what, t, dev):
    """nchw_pitch of a checked float32 [B, C, H, W] map."""
    gpu_tensor(_OP, what, t, dtype=None, contiguous=False)
    if t.dtype != torch.float32 or t.dim() != 4:
        raise RuntimeError(f"{_OP}: {what} must be float32 [B, C, H, W], got {t.dtype} {tuple(t.shape)}")
    if dev is not None and t.device != dev:
        raise RuntimeError(f"{_OP}: {what} is on {t.device}, expected {dev}")
    return nchw_pitch(t)


def smoke_head_forward(cls_feat, reg_feat, cls_norm, reg_norm, cls_weight, cls_bias, reg_weight, reg_bias, Ks, trans,
                       image_size, depth_ref, dim_ref, groups, max_detection, det_threshold, mode=FORWARD,
                       cls_tables=None, reg_tables=None, reg_channels=REG_CHANNELS, pred_2d=True):
    """cls_feat / reg_feat [B, C, H, W]: the two 3x3 convolutions' outputs (views of one stacked, row-padded map are
    read in place); cls_norm / reg_norm = (gamma, beta) [C]; cls_weight [nc, C(, 1, 1)], reg_weight [10, C(, 1, 1)];
    tables None (GroupNorm with `groups` groups, computed on the device) or [B, 2, groups] (batch_norm_tables);
    trans = trans_mat [B, 3, 3] with image_size [2] (mode FORWARD) or down_ratios [.., 2] (mode EXPORT)."""
    cls_feat, bstride, pitch = _strided("cls_feat", cls_feat, None)
    dev = cls_feat.device
    b, c, h, w = (int(s) for s in cls_feat.shape)
    reg_feat, rb, rp = _strided("reg_feat", reg_feat, dev)
    if tuple(reg_feat.shape) != (b, c, h, w):
        raise RuntimeError(f"{_OP}: reg_feat must be {(b, c, h, w)}, got {tuple(reg_feat.shape)}")
    if (rb, rp) != (bstride, pitch):
        cls_feat, reg_feat, bstride, pitch = cls_feat.contiguous(), reg_feat.contiguous(), c * h * w, w
    nc, g = int(cls_weight.shape[0]), int(groups)
    if not smoke_supported(c, g, nc, h, w, int(max_detection), reg_channels, pred_2d):
        return None
    cw = gpu_tensor(_OP, "cls_weight", cls_weight.reshape(nc, -1), dev=dev, shape=(nc, c))
    cb = gpu_tensor(_OP, "cls_bias", cls_bias, dev=dev, shape=(nc,))
    rw = gpu_tensor(_OP, "reg_weight", reg_weight.reshape(reg_weight.shape[0], -1), dev=dev, shape=(10, c))
    rbias = gpu_tensor(_OP, "reg_bias", reg_bias, dev=dev, shape=(10,))
    norms = [gpu_tensor(_OP, n, t, dev=dev, shape=(c,))
             for n, t in zip(("cls_gamma", "cls_beta", "reg_gamma", "reg_beta"), (*cls_norm, *reg_norm))]
    tabs = [None if t is None else gpu_tensor(_OP, "tables", t, dev=dev, shape=(b, 2, g))
            for t in (cls_tables, reg_tables)]
    cam = _camera(Ks, trans, image_size, depth_ref, dim_ref, b, nc, mode, dev)
    L = lib()
    rows = torch.empty((b, int(max_detection), 14), dtype=torch.float32, device=dev)
    counts = torch.empty((b,), dtype=torch.int32, device=dev)
    ws = workspace(L.pd3_smoke_head_workspace(b, h, w, nc, int(max_detection)), dev)
    reg, tail = _tail(reg_channels, max_detection, det_threshold, mode, pred_2d)
    st = L.pd3_smoke_head_forward(ptr(cls_feat), ptr(reg_feat), bstride, pitch, *(ptr(t) for t in norms),
                                  ptr(tabs[0]), ptr(tabs[1]), ptr(cw), ptr(cb), ptr(rw), ptr(rbias),
                                  *(ptr(t) for t in cam), b, c, g, h, w, nc, *tail, ptr(rows), ptr(counts), ptr(ws),
                                  ws.numel(), stream_ptr(dev))
    if st == _UNSUPPORTED:
        return None
    check(st, f"{_OP}.smoke_head_forward")
    return rows, counts


def smoke_post_process(heat, regression, Ks, trans, image_size, depth_ref, dim_ref, max_detection, det_threshold,
                       mode=FORWARD, reg_channels=REG_CHANNELS, pred_2d=True):
    """heat [B, nc, H, W] (the clipped sigmoid heat map), regression [B, 10, H, W] (activations applied):
    SMOKEPredictor's outputs."""
    heat = gpu_tensor(_OP, "heat", heat)
    dev = heat.device
    if heat.dim() != 4:
        raise RuntimeError(f"{_OP}: heat must be [B, nc, H, W], got {tuple(heat.shape)}")
    b, nc, h, w = (int(s) for s in heat.shape)
    if not smoke_supported(None, None, nc, h, w, int(max_detection), reg_channels, pred_2d):
        return None
    regression = gpu_tensor(_OP, "regression", regression, dev=dev, shape=(b, 10, h, w))
    cam = _camera(Ks, trans, image_size, depth_ref, dim_ref, b, nc, mode, dev)
    L = lib()
    rows = torch.empty((b, int(max_detection), 14), dtype=torch.float32, device=dev)
    counts = torch.empty((b,), dtype=torch.int32, device=dev)
    ws = workspace(L.pd3_smoke_head_workspace(b, h, w, nc, int(max_detection)), dev)
    reg, tail = _tail(reg_channels, max_detection, det_threshold, mode, pred_2d)
    st = L.pd3_smoke_post_process(ptr(heat), ptr(regression), *(ptr(t) for t in cam), b, h, w, nc, *tail, ptr(rows),
                                  ptr(counts), ptr(ws), ws.numel(), stream_ptr(dev))
    if st == _UNSUPPORTED:
        return None
    check(st, f"{_OP}.smoke_post_process")
    return rows, counts
