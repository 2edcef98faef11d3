"""BEV-LaneDet's lane head tail and lane post-processing at inference on the device (csrc/lanedet.hip, C ABI
pd3_lanedet_head_forward / pd3_lanedet_post_process, include/paddle3d_amd_lanedet.h); the arithmetic order is stated in
that file's header and restated in tests/golden/lanedet_numpy.py.

Reference: paddle3d/models/detection/bev_lanedet/bev_lanedet.py:50-108 (InstanceEmbeddingOffsetYZ), :419-430
(test_forward), paddle3d/datasets/apollo/cluster.py:44-140 (embedding_post), post_process.py:26-75
(bev_instance2points_with_offset_z), apollo_lane_metric.py:355-383 (the cubic fit and its 40 samples).

lanedet_head_forward(seg_feat, emb_feat, offset_feat, z_feat, ...)
    the LAZY form from the four branches' 64-channel maps: the seg final convolution runs densely; the emb, offset
    (with its sigmoid) and z final convolutions are evaluated at the selected pixels only.
lanedet_post_process(seg, emb, offset, z, ...)
    the same selection, clustering, canvas, lane points and fit from the four maps test_forward saves.
Both return a LanePack of device tensors (see include/paddle3d_amd_lanedet.h for the layout), or None when the
kernels do not take the shape (`lanedet_supported`).  float32 only.  Nothing here synchronises with the host; the
kernels run on the current stream.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch

from ._common import check, gpu_tensor, lib, nchw_pitch, ptr, stream_ptr, workspace

__all__ = ["lanedet_supported", "lanedet_head_forward", "lanedet_post_process", "LanePack", "MAX_CENTRES", "MAX_LANES",
           "FIT_SAMPLES"]

_OP = "lanedet"
_UNSUPPORTED = -3
MAX_CENTRES = 128   # centres per frame; one more sets flag bit 0
MAX_LANES = 32      # canvas ids per frame; one more sets flag bit 1
FIT_SAMPLES = 40

LanePack = namedtuple("LanePack", "labels num_lanes lane_id lane_rows fit_ok points fit flags num_selected")


def lanedet_supported(h, w, nd, channels=None, pitch=None, batch=1):
    """The kernels' shape predicate, the same conditions as the entry points'.  channels=None: the from-maps form,
    which has no channel condition; pitch: floats per row of the branch maps (default: w rounded up to a multiple of
    4, what a stacked convolution output has)."""
    pitch = (w + 3) // 4 * 4 if pitch is None else pitch
    if channels is not None and not (1 <= channels <= 128 and channels * h * pitch < 2 ** 31):
        return False
    return 1 <= nd <= 4 and 1 <= h <= 1024 and w >= 1 and h * w <= 2 ** 20 and 0 <= batch <= 65535


def _outputs(b, h, w, dev):
    i32 = dict(dtype=torch.int32, device=dev)
    return LanePack(torch.empty((b, h, w), dtype=torch.uint8, device=dev), torch.empty((b,), **i32),
                    torch.empty((b, MAX_LANES), **i32), torch.empty((b, MAX_LANES), **i32),
                    torch.empty((b, MAX_LANES), **i32), torch.empty((b, MAX_LANES, h, 3), dtype=torch.float32, device=dev),
                    torch.empty((b, MAX_LANES, FIT_SAMPLES, 3), dtype=torch.float32, device=dev),
                    torch.empty((b,), **i32), torch.empty((b,), **i32))


def _tail(b, h, w, nd, conf, emb_margin, min_cluster_size, max_x, meter_per_pixel, out, ws, dev):
    mx, my = (meter_per_pixel if isinstance(meter_per_pixel, (tuple, list)) else (meter_per_pixel, meter_per_pixel))
    return (b, h, w, nd, C.c_float(conf), C.c_float(emb_margin), int(min_cluster_size), C.c_double(max_x),
            C.c_double(mx), C.c_double(my), *(ptr(t) for t in out), ptr(ws), ws.numel(), stream_ptr(dev))


def _strided(what, t, dev):
    """nchw_pitch of a checked float32 [B, C, H, W] map."""
    gpu_tensor(_OP, what, t, dtype=None, contiguous=False)
    if t.dtype != torch.float32 or t.dim() != 4:
        raise RuntimeError(f"{_OP}: {what} must be float32 [B, C, H, W], got {t.dtype} {tuple(t.shape)}")
    if dev is not None and t.device != dev:
        raise RuntimeError(f"{_OP}: {what} is on {t.device}, expected {dev}")
    return nchw_pitch(t)


def lanedet_post_process(seg, emb, offset, z, conf=0.9, emb_margin=6.0, min_cluster_size=15, max_x=103.0,
                         meter_per_pixel=0.5, offset_is_logit=False):
    """seg [B, 1, H, W] (logits), emb [B, nd, H, W], offset [B, 1, H, W] (sigmoid applied unless offset_is_logit),
    z [B, 1, H, W]: the channels of the [B, 5, H, W] tensor BEVLaneDet.test_forward saves."""
    seg = gpu_tensor(_OP, "seg", seg)
    dev = seg.device
    if seg.dim() != 4 or seg.shape[1] != 1:
        raise RuntimeError(f"{_OP}: seg must be [B, 1, H, W], got {tuple(seg.shape)}")
    b, _, h, w = (int(s) for s in seg.shape)
    gpu_tensor(_OP, "emb", emb, dev=dev, contiguous=False)
    if emb.dim() != 4 or (int(emb.shape[0]), int(emb.shape[2]), int(emb.shape[3])) != (b, h, w):
        raise RuntimeError(f"{_OP}: emb must be {(b, 'nd', h, w)}, got {tuple(emb.shape)}")
    nd = int(emb.shape[1])
    if not lanedet_supported(h, w, nd, batch=b):
        return None
    emb = emb.contiguous()
    offset = gpu_tensor(_OP, "offset", offset, dev=dev, shape=(b, 1, h, w))
    z = gpu_tensor(_OP, "z", z, dev=dev, shape=(b, 1, h, w))
    L = lib()
    out = _outputs(b, h, w, dev)
    ws = workspace(L.pd3_lanedet_workspace(b, h, w, nd), dev)
    st = L.pd3_lanedet_post_process(ptr(seg), ptr(emb), ptr(offset), ptr(z), int(bool(offset_is_logit)),
                                    *_tail(b, h, w, nd, conf, emb_margin, min_cluster_size, max_x, meter_per_pixel,
                                           out, ws, dev))
    if st == _UNSUPPORTED:
        return None
    check(st, f"{_OP}.lanedet_post_process")
    return out


def lanedet_head_forward(seg_feat, emb_feat, offset_feat, z_feat, seg_weight, seg_bias, emb_weight, emb_bias,
                         offset_weight, offset_bias, z_weight, z_bias, conf=0.9, emb_margin=6.0, min_cluster_size=15,
                         max_x=103.0, meter_per_pixel=0.5):
    """The four branches' maps after their second convolution, BatchNorm and ReLU [B, C, H, W] (views of one stacked,
    row-padded map are read in place); the final 3x3 weights [1 | nd | 1 | 1, C, 3, 3] and their biases."""
    seg_feat, bstride, pitch = _strided("seg_feat", seg_feat, None)
    dev = seg_feat.device
    b, c, h, w = (int(s) for s in seg_feat.shape)
    feats = [seg_feat]
    same = True
    for what, t in (("emb_feat", emb_feat), ("offset_feat", offset_feat), ("z_feat", z_feat)):
        t, tb, tp = _strided(what, t, dev)
        if tuple(t.shape) != (b, c, h, w):
            raise RuntimeError(f"{_OP}: {what} must be {(b, c, h, w)}, got {tuple(t.shape)}")
        same = same and (tb, tp) == (bstride, pitch)
        feats.append(t)
    if not same:
        feats, bstride, pitch = [t.contiguous() for t in feats], c * h * w, w
    gpu_tensor(_OP, "emb_weight", emb_weight, dev=dev, contiguous=False)
    nd = int(emb_weight.shape[0])
    if not lanedet_supported(h, w, nd, c, pitch, b):
        return None
    weights = []
    for what, wt, bs, rows in (("seg", seg_weight, seg_bias, 1), ("emb", emb_weight, emb_bias, nd),
                               ("offset", offset_weight, offset_bias, 1), ("z", z_weight, z_bias, 1)):
        weights.append(gpu_tensor(_OP, what + "_weight", wt, dev=dev, shape=(rows, c, 3, 3)))
        weights.append(gpu_tensor(_OP, what + "_bias", bs, dev=dev, shape=(rows,)))
    L = lib()
    out = _outputs(b, h, w, dev)
    ws = workspace(L.pd3_lanedet_workspace(b, h, w, nd), dev)
    st = L.pd3_lanedet_head_forward(*(ptr(t) for t in feats), bstride, pitch, c, *(ptr(t) for t in weights),
                                    *_tail(b, h, w, nd, conf, emb_margin, min_cluster_size, max_x, meter_per_pixel,
                                           out, ws, dev))
    if st == _UNSUPPORTED:
        return None
    check(st, f"{_OP}.lanedet_head_forward")
    return out
