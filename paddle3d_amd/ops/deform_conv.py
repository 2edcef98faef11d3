"""Modulated deformable convolution on the device (csrc/deform_conv.hip, C ABI pd3_deform_conv2d_forward, declared in
include/paddle3d_amd_dcn.h); the arithmetic order is stated in that file's header and restated in
tests/golden/dcn_numpy.py.

deform_conv2d_supported(in_channels, out_channels, height=1, width=1, batch=1, stride=1, padding=0, dilation=1,
                        kernel_size=3, groups=1, deformable_groups=1)
    the kernel's shape predicate: 3 x 3, one group, channels multiples of 16 from 16 to 512, stride 1 or 2.
pack_deform_conv_weight(w) / unpack_deform_conv_weight(packed, in_channels)
    [Cout, Cin, 3, 3] <-> the kernel's [9 Cin / 16, Cout / 16, 64, 4] order.
deform_conv2d(x, offset, weight, bias=None, stride=1, padding=0, dilation=1, deformable_groups=1, groups=1, mask=None)
    paddle.vision.ops.deform_conv2d's forward, its argument order; raises where the kernel does not take the shape.
deform_conv2d_packed(x, offset, mask, packed, scale=None, shift=None, relu=False, mask_is_logit=False, stride=1,
                     padding=0, dilation=1)
    the entry point itself with every epilogue it has: y * scale + shift (a folded BatchNorm, or a bias as shift), relu,
    the sigmoid of a mask given as logits; None where the kernel does not take the shape.  offset and mask may be views
    of one 27-channel map (ops/_common.nchw_pitch): no copy is made.

float32 only.  Nothing here synchronises with the host; the kernel runs on the current stream.
"""
from __future__ import annotations

import torch

from ._common import check, gpu_tensor, lib, nchw_pitch, ptr, stream_ptr

__all__ = ["deform_conv2d_supported", "pack_deform_conv_weight", "unpack_deform_conv_weight", "deform_conv2d",
           "deform_conv2d_packed", "output_size", "tiles_per_wave", "fused_by_default", "MAX_CHANNELS", "PIXEL_TILE",
           "DCN_FUSED_MIN_PIXELS"]

_OP = "deform_conv"
MAX_CHANNELS = 512
PIXEL_TILE = 64  # output pixels of the whole batch per workgroup
_UNSUPPORTED = -3
# Module default (mm_resnet.DeformableConvV2(fused=True)): the kernel runs from this many output pixels of the whole
# batch on, the torch composition below it.  Measured on the MI355X against the module's own composition
# (tools/prof/dcn.py --sweep; DESIGN.md 4.5zi has the table): the layer with the kernel is 3.6 x / 1.5 x the composition
# at CAPE's stages 3 / 4, 2.8 x / 1.6 x at CAPE-T's, and still 4.0 x at 88 pixels of 256 channels and 1.9 x at 44 pixels
# of 512 -- it lost at no measured shape, so the border is the smallest output there is.
DCN_FUSED_MIN_PIXELS = 1


def fused_by_default(in_channels, out_channels, pixels):
    """Whether a layer with `pixels` output pixels in the whole batch runs the kernel under fused=True."""
    return int(pixels) >= DCN_FUSED_MIN_PIXELS


def tiles_per_wave(pixels, out_channels):
    """The form the entry point launches for `pixels` output pixels of the whole batch: 4, 2 or 1 channel tiles of 16
    per wave (dcn_tiles_per_wave in csrc/deform_conv.hip, restated for the tests and tools that have to reach every
    form).  An output's arithmetic is the same in all three."""
    tiles, ct = (int(pixels) + PIXEL_TILE - 1) // PIXEL_TILE, int(out_channels) // 16
    for ntw in (4, 2):
        if ct >= 4 * ntw and tiles * ((ct + 4 * ntw - 1) // (4 * ntw)) >= 512:
            return ntw
    return 1


def output_size(size, stride=1, padding=0, dilation=1):
    """Output rows (or columns) of a 3-tap convolution over `size` input rows; < 1: the image is too small."""
    return (int(size) + 2 * int(padding) - 2 * int(dilation) - 1) // int(stride) + 1


def deform_conv2d_supported(in_channels, out_channels, height=1, width=1, batch=1, stride=1, padding=0, dilation=1,
                            kernel_size=3, groups=1, deformable_groups=1):
    """The kernel's shape predicate.  A partial pixel tile is masked, so every output size >= 1 is taken; an image
    smaller than the dilated kernel has no output and is refused."""
    ks = tuple(kernel_size) if isinstance(kernel_size, (tuple, list)) else (kernel_size, kernel_size)
    if tuple(int(k) for k in ks) != (3, 3) or int(groups) != 1 or int(deformable_groups) != 1:
        return False
    ci, co, H, W, N = int(in_channels), int(out_channels), int(height), int(width), int(batch)
    s, p, d = int(stride), int(padding), int(dilation)
    if ci < 16 or co < 16 or ci > MAX_CHANNELS or co > MAX_CHANNELS or ci % 16 != 0 or co % 16 != 0:
        return False
    if s not in (1, 2) or d < 1 or p < 0 or max(p, d) >= 2 ** 31 or H < 1 or W < 1 or N < 0 or H * W >= 2 ** 31:
        return False
    Ho, Wo = output_size(H, s, p, d), output_size(W, s, p, d)
    if Ho < 1 or Wo < 1 or Ho >= 2 ** 31 or Wo >= 2 ** 31:
        return False
    return (N * Ho * Wo + PIXEL_TILE - 1) // PIXEL_TILE < 2 ** 30


def _index(in_channels, out_channels, device):
    """(o [Cout / 16, 64], j [9 Cin / 16, 64, 4]): element ks of lane l of chunk t, channel tile nt holds
    w[o[nt, l], j[t, l, ks]]."""
    lane = torch.arange(64, device=device)
    col, kk = lane & 15, lane >> 4
    o = 16 * torch.arange(out_channels // 16, device=device)[:, None] + col[None, :]
    t = torch.arange(9 * in_channels // 16, device=device)
    j = 16 * t[:, None, None] + 4 * torch.arange(4, device=device)[None, None, :] + kk[None, :, None]
    return o, j


def pack_deform_conv_weight(w):
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.shape[0] % 16 != 0 or w.shape[1] % 16 != 0 or w.numel() == 0:
        raise RuntimeError(f"{_OP}: the weight must be [Cout, Cin, 3, 3] with Cout and Cin multiples of 16, got "
                           f"{tuple(w.shape)}")
    co, ci = int(w.shape[0]), int(w.shape[1])
    o, j = _index(ci, co, w.device)
    flat = w.detach().float().reshape(co, 9 * ci)
    return flat[o[None, :, :, None], j[:, None, :, :]].contiguous()


def unpack_deform_conv_weight(packed, in_channels):
    ci = int(in_channels)
    if packed.dim() != 4 or tuple(packed.shape[2:]) != (64, 4) or packed.shape[0] * 16 != 9 * ci:
        raise RuntimeError(f"{_OP}: the packed weight must be [9 Cin / 16, Cout / 16, 64, 4], got {tuple(packed.shape)}")
    co = 16 * int(packed.shape[1])
    o, j = _index(ci, co, packed.device)
    flat = packed.new_zeros((co, 9 * ci))
    shape = tuple(packed.shape)
    flat[o[None, :, :, None].expand(shape), j[:, None, :, :].expand(shape)] = packed
    return flat.reshape(co, ci, 3, 3)


def _vector(name, t, n, dev):
    if t is None:
        return None
    return gpu_tensor(_OP, name, t, torch.float32, dev, (n,))


def deform_conv2d_packed(x, offset, mask, packed, scale=None, shift=None, relu=False, mask_is_logit=False, stride=1,
                         padding=0, dilation=1):
    x = gpu_tensor(_OP, "x", x, torch.float32)
    dev = x.device
    if x.dim() != 4:
        raise RuntimeError(f"{_OP}: x must be [N, Cin, H, W], got {tuple(x.shape)}")
    N, ci, H, W = (int(v) for v in x.shape)
    packed = gpu_tensor(_OP, "packed", packed, torch.float32, dev)
    if packed.dim() != 4 or tuple(packed.shape[2:]) != (64, 4) or packed.shape[0] * 16 != 9 * ci:
        raise RuntimeError(f"{_OP}: the packed weight must be [9 * {ci} / 16, Cout / 16, 64, 4], got {tuple(packed.shape)}")
    co = 16 * int(packed.shape[1])
    s, p, d = int(stride), int(padding), int(dilation)
    if not deform_conv2d_supported(ci, co, H, W, N, s, p, d):
        return None
    Ho, Wo = output_size(H, s, p, d), output_size(W, s, p, d)
    offset = gpu_tensor(_OP, "offset", offset, torch.float32, dev, (N, 18, Ho, Wo), contiguous=False)
    offset, ob, op = nchw_pitch(offset)
    mb = mp = 0
    if mask is not None:
        mask = gpu_tensor(_OP, "mask", mask, torch.float32, dev, (N, 9, Ho, Wo), contiguous=False)
        mask, mb, mp = nchw_pitch(mask)
    scale, shift = _vector("scale", scale, co, dev), _vector("shift", shift, co, dev)
    y = torch.empty((N, co, Ho, Wo), dtype=torch.float32, device=dev)
    st = lib().pd3_deform_conv2d_forward(ptr(x), ptr(offset), ob, op, ptr(mask), mb, mp, int(bool(mask_is_logit)),
                                         ptr(packed), ptr(scale), ptr(shift), int(bool(relu)), N, ci, co, H, W, s, p, d,
                                         ptr(y), stream_ptr(dev))
    if st == _UNSUPPORTED:
        return None
    check(st, f"{_OP}.deform_conv2d")
    return y


def _one(v, what):
    if isinstance(v, (tuple, list)):
        if len(v) != 2 or v[0] != v[1]:
            raise RuntimeError(f"{_OP}: {what} must be the same in both directions, got {tuple(v)}")
        v = v[0]
    return int(v)


def deform_conv2d(x, offset, weight, bias=None, stride=1, padding=0, dilation=1, deformable_groups=1, groups=1,
                  mask=None):
    x = gpu_tensor(_OP, "x", x, torch.float32)
    weight = gpu_tensor(_OP, "weight", weight, torch.float32, x.device)
    if x.dim() != 4 or weight.dim() != 4 or weight.shape[1] * int(groups) != x.shape[1]:
        raise RuntimeError(f"{_OP}: x must be [N, Cin, H, W] and weight [Cout, Cin / groups, kh, kw], got "
                           f"{tuple(x.shape)} and {tuple(weight.shape)}")
    s, p, d = _one(stride, "stride"), _one(padding, "padding"), _one(dilation, "dilation")
    N, ci, H, W = (int(v) for v in x.shape)
    if not deform_conv2d_supported(ci, int(weight.shape[0]), H, W, N, s, p, d, tuple(weight.shape[2:]), groups,
                                   deformable_groups):
        raise RuntimeError(f"{_OP}: unsupported configuration: x {tuple(x.shape)}, weight {tuple(weight.shape)}, stride "
                           f"{s}, padding {p}, dilation {d}, groups {groups}, deformable_groups {deformable_groups} "
                           "(deform_conv2d_supported)")
    y = deform_conv2d_packed(x, offset, mask, pack_deform_conv_weight(weight), None, bias, False, False, s, p, d)
    if y is None:
        raise RuntimeError(f"{_OP}: the kernel refused a shape its predicate accepts")
    return y
