"""SqueezeSegV3's spatially-adaptive convolution block and range projection on the device (csrc/squeezeseg.hip, C ABI
pd3_sac_isk_forward / pd3_range_project); the arithmetic order is stated in that file's header and restated in
tests/golden/squeezeseg_numpy.py.

sac_isk_supported(channels, height=1, width=1, batch=1)
    the kernel's shape predicate: channels % 16 == 0, 16 <= channels <= 256, any height, width >= 1.
fold_batch_norm(gamma, beta, mean, var, eps=1e-5, bias=None)
    (scale, shift) float32 of an inference BatchNorm behind a convolution with `bias` (None: without one): scale =
    gamma / sqrt(var + eps), shift = (bias - mean) * scale + beta, computed in float64 and rounded once.
pack_sac_attention_weight(w) / unpack_sac_attention_weight(packed, channels)
    the 7x7 attention convolution's [9C, 3, 7, 7] weight <-> the kernel's [9C / 16, 37, 64] order.
pack_sac_mlp_weight(v) / unpack_sac_mlp_weight(packed, channels)
    the 1x1 convolution's [C, 9C] (or [C, 9C, 1, 1]) weight <-> the kernel's [9C / 16, 4, C / 16, 64] order.
sac_isk_forward(xyz, feature, attn_packed, attn_scale, attn_shift, mlp_packed, mlp_scale, mlp_shift)
    xyz [N, 3, H, W], feature [N, C, H, W] -> relu(BN(conv1x1(unfold3x3(feature) * sigmoid(BN(conv7x7(xyz)))))) [N, C,
    H, W] in one launch; None when the kernel does not take the shape.
range_project(points, offsets, height=64, width=1024, fov_up=3.0, fov_down=-25.0, mean=RANGE_MEAN, std=RANGE_STD)
    points [P, 4] (the frames concatenated), offsets int32 [B + 1] on the device -> (image [B, 5, H, W] normalised,
    proj_idx int32 [B, H, W], proj_mask bool [B, H, W], proj_y int32 [P], proj_x int32 [P]): LoadSemanticKITTIRange and
    NormalizeRangeImage for the whole batch.

float32 only.  Nothing here synchronises with the host; the kernels run on the current stream.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ._common import check, gpu_tensor, lib, ptr, stream_ptr

__all__ = ["sac_isk_supported", "fold_batch_norm", "pack_sac_attention_weight", "unpack_sac_attention_weight",
           "pack_sac_mlp_weight", "unpack_sac_mlp_weight", "sac_isk_forward", "range_project", "MAX_CHANNELS",
           "RANGE_MEAN", "RANGE_STD"]

_OP = "squeezeseg"
MAX_CHANNELS = 256
_TAPS = 147   # 3 * 7 * 7
_STEPS = 37   # the taps padded to 148, four per MFMA step
_UNSUPPORTED = -3
RANGE_MEAN = (12.12, 10.88, 0.23, -1.04, 0.21)  # range, x, y, z, remission (configs/_base_/semantickitti.yml)
RANGE_STD = (12.32, 11.47, 6.91, 0.86, 0.16)


def sac_isk_supported(channels, height=1, width=1, batch=1):
    """The kernel's shape predicate; partial 16-pixel tiles are masked, so every height and width >= 1 is taken."""
    C, H, W, N = int(channels), int(height), int(width), int(batch)
    if C < 16 or C > MAX_CHANNELS or C % 16 != 0 or H < 1 or W < 1 or N < 0:
        return False
    return N * H * ((W + 15) // 16) < 2 ** 30


def fold_batch_norm(gamma, beta, mean, var, eps=1e-5, bias=None):
    g, b, m, v = (t.detach().double() for t in (gamma, beta, mean, var))
    scale = g / torch.sqrt(v + float(eps))
    shift = ((bias.detach().double() - m) if bias is not None else -m) * scale + b
    return scale.float().contiguous(), shift.float().contiguous()


def _attention_index(channels, device):
    """(j [T, 64], tap [37, 64]): what lane l of step s of tile T holds."""
    lane = torch.arange(64, device=device)
    m, k = lane & 15, lane >> 4
    tiles = torch.arange(9 * channels // 16, device=device)
    j = 16 * tiles[:, None] + (4 * (m & 3) + (m >> 2))[None, :]
    tap = 4 * torch.arange(_STEPS, device=device)[:, None] + k[None, :]
    return j, tap


def _mlp_index(channels, device):
    """(o [C / 16, 64], j [T, 4, 64]): lane l of step r of tile T, output tile ot holds v[o[ot, l], j[T, r, l]]."""
    lane = torch.arange(64, device=device)
    col, k = lane & 15, lane >> 4
    o = 16 * torch.arange(channels // 16, device=device)[:, None] + col[None, :]
    tiles = torch.arange(9 * channels // 16, device=device)
    j = 16 * tiles[:, None, None] + 4 * torch.arange(4, device=device)[None, :, None] + k[None, None, :]
    return o, j


def _channels_of(rows, what):
    if rows % 9 != 0 or (rows // 9) % 16 != 0 or rows == 0:
        raise RuntimeError(f"{_OP}: {what} must have 9 * C rows with C a multiple of 16, got {rows}")
    return rows // 9


def pack_sac_attention_weight(w):
    if w.dim() != 4 or tuple(w.shape[1:]) != (3, 7, 7):
        raise RuntimeError(f"{_OP}: the attention weight must be [9C, 3, 7, 7], got {tuple(w.shape)}")
    C = _channels_of(int(w.shape[0]), "the attention weight")
    flat = torch.nn.functional.pad(w.detach().float().reshape(9 * C, _TAPS), (0, 4 * _STEPS - _TAPS))
    j, tap = _attention_index(C, w.device)
    return flat[j[:, None, :], tap[None, :, :]].contiguous()


def unpack_sac_attention_weight(packed, channels):
    C = int(channels)
    j, tap = _attention_index(C, packed.device)
    flat = packed.new_zeros((9 * C, 4 * _STEPS))
    flat[j[:, None, :].expand(-1, _STEPS, -1), tap[None, :, :].expand(j.shape[0], -1, -1)] = packed
    return flat[:, :_TAPS].reshape(9 * C, 3, 7, 7).contiguous()


def pack_sac_mlp_weight(v):
    if v.dim() == 4 and tuple(v.shape[2:]) == (1, 1):
        v = v.reshape(v.shape[0], v.shape[1])
    if v.dim() != 2 or v.shape[1] != 9 * v.shape[0]:
        raise RuntimeError(f"{_OP}: the 1x1 weight must be [C, 9C], got {tuple(v.shape)}")
    C = _channels_of(int(v.shape[1]), "the 1x1 weight")
    o, j = _mlp_index(C, v.device)
    return v.detach().float()[o[None, None, :, :], j[:, :, None, :]].contiguous()


def unpack_sac_mlp_weight(packed, channels):
    C = int(channels)
    o, j = _mlp_index(C, packed.device)
    v = packed.new_zeros((C, 9 * C))
    shape = (j.shape[0], 4, C // 16, 64)
    v[o[None, None, :, :].expand(shape), j[:, :, None, :].expand(shape)] = packed
    return v


def sac_isk_forward(xyz, feature, attn_packed, attn_scale, attn_shift, mlp_packed, mlp_scale, mlp_shift):
    xyz = gpu_tensor(_OP, "xyz", xyz, torch.float32)
    dev = xyz.device
    feature = gpu_tensor(_OP, "feature", feature, torch.float32, dev)
    if feature.dim() != 4 or xyz.dim() != 4 or xyz.shape[1] != 3 or xyz.shape[0] != feature.shape[0] or \
            tuple(xyz.shape[2:]) != tuple(feature.shape[2:]):
        raise RuntimeError(f"{_OP}: xyz must be [N, 3, H, W] and feature [N, C, H, W], got {tuple(xyz.shape)} and "
                           f"{tuple(feature.shape)}")
    N, C, H, W = (int(s) for s in feature.shape)
    if max(N, C, H, W) >= 2 ** 31:
        raise RuntimeError(f"{_OP}: bad sizes {(N, C, H, W)}")
    if not sac_isk_supported(C, H, W, N):
        return None
    shapes = ((9 * C // 16, _STEPS, 64), (9 * C,), (9 * C,), (9 * C // 16, 4, C // 16, 64), (C,), (C,))
    names = ("attn_packed", "attn_scale", "attn_shift", "mlp_packed", "mlp_scale", "mlp_shift")
    params = []
    for name, t, shape in zip(names, (attn_packed, attn_scale, attn_shift, mlp_packed, mlp_scale, mlp_shift), shapes):
        t = gpu_tensor(_OP, name, t, torch.float32, dev)
        if tuple(t.shape) != shape:
            raise RuntimeError(f"{_OP}: {name} must be {shape}, got {tuple(t.shape)}")
        params.append(t)
    out = torch.empty((N, C, H, W), dtype=torch.float32, device=dev)
    st = lib().pd3_sac_isk_forward(ptr(xyz), ptr(feature), *(ptr(t) for t in params), N, C, H, W, ptr(out),
                                   stream_ptr(dev))
    if st == _UNSUPPORTED:
        return None
    check(st, f"{_OP}.sac_isk_forward")
    return out


def _host_f64(values, what):
    a = np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(-1))
    if a.size != 5 or not np.isfinite(a).all():
        raise RuntimeError(f"{_OP}: {what} must be 5 finite numbers")
    return a


def range_project(points, offsets, height=64, width=1024, fov_up=3.0, fov_down=-25.0, mean=RANGE_MEAN, std=RANGE_STD):
    points = gpu_tensor(_OP, "points", points, torch.float32)
    dev = points.device
    offsets = gpu_tensor(_OP, "offsets", offsets, torch.int32, dev)
    if points.dim() != 2 or points.shape[1] != 4 or offsets.dim() != 1 or offsets.numel() < 1:
        raise RuntimeError(f"{_OP}: points must be [P, 4] and offsets [B + 1], got {tuple(points.shape)} and "
                           f"{tuple(offsets.shape)}")
    P, B, H, W = int(points.shape[0]), int(offsets.numel()) - 1, int(height), int(width)
    up, down = float(fov_up), float(fov_down)
    if H < 1 or W < 1 or P >= 2 ** 31 or not (math.isfinite(up) and math.isfinite(down) and up > down):
        raise RuntimeError(f"{_OP}: bad sizes or inclinations {(P, B, H, W, up, down)}")
    mean64, std64 = _host_f64(mean, "mean"), _host_f64(std, "std")
    if (std64 == 0).any():
        raise RuntimeError(f"{_OP}: std is invalid")
    image = torch.empty((B, 5, H, W), dtype=torch.float32, device=dev)
    proj_idx = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    proj_mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    proj_y = torch.empty((P,), dtype=torch.int32, device=dev)
    proj_x = torch.empty((P,), dtype=torch.int32, device=dev)
    ws = torch.empty((B, H, W), dtype=torch.int64, device=dev)  # the kernel's uint64 keys
    st = lib().pd3_range_project(ptr(points), P, ptr(offsets), B, H, W, up, down, ptr(mean64), ptr(std64), ptr(image),
                                 ptr(proj_idx), ptr(proj_mask), ptr(proj_y), ptr(proj_x), ptr(ws), ws.numel() * 8,
                                 stream_ptr(dev))
    check(st, f"{_OP}.range_project")
    return image, proj_idx, proj_mask.view(torch.bool), proj_y, proj_x
