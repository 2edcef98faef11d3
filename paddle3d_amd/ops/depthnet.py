"""BEVDepth's DepthNet kernels on the device (csrc/depthnet.hip, C ABI pd3_aspp_workspace / pd3_aspp_forward /
pd3_depth_softmax_split, declared in include/paddle3d_amd_depthnet.h); the arithmetic order is stated in that file's
header and restated in tests/golden/depthnet_numpy.py.

aspp_supported(cin, cmid, h=1, w=1, n=1, dilations=(6, 12, 18))
    the ASPP kernels' shape predicate: channels multiples of 16 from 16 to 512, dilations 1 .. 65535.
pack_aspp_branches(w1x1, w3a, w3b, w3c) / pack_aspp_projection(conv1_weight)
    the four atrous weights -> the branch kernel's [28, Cin / 16, Cmid / 16, 64, 4] order; conv1's [Cmid, 5 Cmid, 1, 1]
    -> (the projection kernel's [1, 4 Cmid / 16, Cmid / 16, 64, 4], the pooled columns transposed [Cmid, Cmid]).
aspp_forward(x, packed, dilations=(6, 12, 18))
    the entry point: `packed` is the dict pack_aspp(...) builds; None where the kernels do not take the shape.
depth_softmax_split(x, depth_channels)
    x [BN, D + C, H, W] -> (softmax(x[:, :D], 1) [BN, D, H, W], x[:, D:] channels last [BN, H, W, C]) in one launch;
    None where the kernel does not take the shape.
fused_by_default(kind, ...)
    whether fused=True takes a kernel: set from tools/prof/depthnet.py's measurement (DESIGN.md 4.5zj has the table).

float32 only.  Nothing here synchronises with the host; the kernels run on the current stream.
"""
from __future__ import annotations

import torch

from ._common import check, gpu_tensor, lib, ptr, stream_ptr, workspace

__all__ = ["aspp_supported", "tail_supported", "pack_aspp_branches", "pack_aspp_projection", "pack_aspp",
           "aspp_forward", "depth_softmax_split", "fused_by_default", "tiles_per_wave", "in_range_taps", "MAX_CHANNELS",
           "MAX_DILATION", "PIXEL_TILE", "ASPP_FUSED_MIN_PIXELS", "TAIL_FUSED_MAX_PIXELS"]

_OP = "depthnet"
MAX_CHANNELS = 512
MAX_DILATION = 65535
PIXEL_TILE = 64  # pixels of the whole batch per workgroup
_UNSUPPORTED = -3
# Module defaults under fused=True, from the measurement on the MI355X against the modules' own torch compositions
# (tools/prof/depthnet.py at 512 channels on 16 x 44 maps; DESIGN.md 4.5zj has the table).  Two batch sizes were timed.
# ASPP: 1.51 x the composition at 54 maps (38016 pixels), 0.94 x at 6 maps (4224 pixels): the kernel runs from the
# larger measured size on and stays behind fused="force" below it.  Tail: 1.28 x at 6 maps, 0.93 x at 54: the kernel runs
# up to the smaller measured size.  Between the two sizes nothing was measured, so the composition runs there.
ASPP_FUSED_MIN_PIXELS = 54 * 16 * 44
TAIL_FUSED_MAX_PIXELS = 6 * 16 * 44


def fused_by_default(kind, *shape):
    """Whether the module default (fused=True) runs the kernel of `kind` at `shape`: "aspp" with (N, Cin, Cmid, H, W),
    "tail" with (N, D, C, H, W)."""
    if kind not in ("aspp", "tail"):
        raise ValueError(f"kind must be 'aspp' or 'tail', got {kind!r}")
    if len(shape) != 5:
        raise ValueError(f"{kind}: the shape is five integers, got {shape!r}")
    pixels = int(shape[0]) * int(shape[3]) * int(shape[4])
    return pixels >= ASPP_FUSED_MIN_PIXELS if kind == "aspp" else 1 <= pixels <= TAIL_FUSED_MAX_PIXELS


def tiles_per_wave(pixels, out_channels):
    """The form the GEMM kernels launch for `pixels` pixels of the whole batch: 4, 2 or 1 channel tiles of 16 per wave
    (gemm_tiles_per_wave in csrc/depthnet.hip).  An output's arithmetic is the same in all three."""
    tiles, ct = (int(pixels) + PIXEL_TILE - 1) // PIXEL_TILE, int(out_channels) // 16
    for ntw in (4, 2):
        if ct >= 4 * ntw and tiles * ((ct + 4 * ntw - 1) // (4 * ntw)) >= 512:
            return ntw
    return 1


def in_range_taps(h, w, dilations=(6, 12, 18)):
    """Taps x pixels inside an h x w image, per branch (the 1 x 1 branch first), as exact integers: per direction a
    dilation d contributes size + 2 max(size - d, 0) in-range (pixel, tap) pairs."""
    def line(size, d):
        return size + 2 * max(size - d, 0)
    return [h * w] + [line(h, d) * line(w, d) for d in dilations]


def aspp_supported(cin, cmid, h=1, w=1, n=1, dilations=(6, 12, 18)):
    ci, cm, H, W, N = int(cin), int(cmid), int(h), int(w), int(n)
    if ci < 16 or cm < 16 or ci > MAX_CHANNELS or cm > MAX_CHANNELS or ci % 16 != 0 or cm % 16 != 0:
        return False
    if len(dilations) != 3 or any(int(d) < 1 or int(d) > MAX_DILATION for d in dilations):
        return False
    if H < 1 or W < 1 or N < 0 or H * W >= 2 ** 31 or N * H * W > 2 ** 36:
        return False
    return (N * H * W + PIXEL_TILE - 1) // PIXEL_TILE < 2 ** 30


def tail_supported(n, depth_channels, context_channels, h, w):
    return (0 <= int(n) <= 65535 and int(depth_channels) >= 1 and int(context_channels) >= 0 and int(h) >= 1 and
            int(w) >= 1 and int(h) * int(w) < 2 ** 31)


def _pack(flat):
    """[P, Cout, K] -> [P, K / 16, Cout / 16, 64, 4]: element ks of lane (col, kk) of chunk t, channel tile nt holds
    flat[p, 16 nt + col, 16 t + 4 ks + kk]."""
    P, co, K = (int(v) for v in flat.shape)
    lane = torch.arange(64, device=flat.device)
    col, kk = lane & 15, lane >> 4
    o = 16 * torch.arange(co // 16, device=flat.device)[:, None] + col[None, :]                      # [CT, 64]
    j = (16 * torch.arange(K // 16, device=flat.device)[:, None, None] +
         4 * torch.arange(4, device=flat.device)[None, None, :] + kk[None, :, None])                 # [NT, 64, 4]
    return flat[:, o[None, :, :, None], j[:, None, :, :]].contiguous()


def pack_aspp_branches(w1x1, w3a, w3b, w3c):
    co, ci = int(w1x1.shape[0]), int(w1x1.shape[1])
    if tuple(w1x1.shape) != (co, ci, 1, 1) or any(tuple(w.shape) != (co, ci, 3, 3) for w in (w3a, w3b, w3c)) or \
            co % 16 != 0 or ci % 16 != 0 or co == 0 or ci == 0:
        raise RuntimeError(f"{_OP}: the branch weights must be [Cmid, Cin, 1, 1] and three [Cmid, Cin, 3, 3] with Cmid "
                           f"and Cin multiples of 16, got {[tuple(w.shape) for w in (w1x1, w3a, w3b, w3c)]}")
    pairs = [w1x1.detach().float().reshape(1, co, ci)]
    pairs += [w.detach().float().reshape(co, ci, 9).permute(2, 0, 1) for w in (w3a, w3b, w3c)]
    return _pack(torch.cat(pairs, 0))


def pack_aspp_projection(conv1_weight):
    co = int(conv1_weight.shape[0])
    if tuple(conv1_weight.shape) != (co, 5 * co, 1, 1) or co % 16 != 0 or co == 0:
        raise RuntimeError(f"{_OP}: conv1's weight must be [Cmid, 5 Cmid, 1, 1] with Cmid a multiple of 16, got "
                           f"{tuple(conv1_weight.shape)}")
    w = conv1_weight.detach().float().reshape(co, 5 * co)
    return _pack(w[None, :, :4 * co]), w[:, 4 * co:].t().contiguous()


def pack_aspp(branch_weights, branch_norms, pool_weight, pool_norm, conv1_weight, norm1):
    """Everything pd3_aspp_forward reads, from the four atrous weights, their (scale, shift) pairs, the pooled branch's
    1 x 1 weight and (scale, shift), conv1's weight and bn1's (scale, shift)."""
    proj, proj_pool_t = pack_aspp_projection(conv1_weight)
    co, ci = int(pool_weight.shape[0]), int(pool_weight.shape[1])
    return dict(branches=pack_aspp_branches(*branch_weights),
                branch_scale=torch.cat([s for s, _ in branch_norms]).float().contiguous(),
                branch_shift=torch.cat([b for _, b in branch_norms]).float().contiguous(),
                pool_t=pool_weight.detach().float().reshape(co, ci).t().contiguous(),
                pool_scale=pool_norm[0].float().contiguous(), pool_shift=pool_norm[1].float().contiguous(),
                proj=proj, proj_pool_t=proj_pool_t, proj_scale=norm1[0].float().contiguous(),
                proj_shift=norm1[1].float().contiguous())


def aspp_forward(x, packed, dilations=(6, 12, 18)):
    x = gpu_tensor(_OP, "x", x, torch.float32)
    dev = x.device
    if x.dim() != 4:
        raise RuntimeError(f"{_OP}: x must be [N, Cin, H, W], got {tuple(x.shape)}")
    N, ci, H, W = (int(v) for v in x.shape)
    br = gpu_tensor(_OP, "branches", packed["branches"], torch.float32, dev)
    if br.dim() != 5 or tuple(br.shape[3:]) != (64, 4) or br.shape[0] != 28 or br.shape[1] * 16 != ci:
        raise RuntimeError(f"{_OP}: the packed branch weights must be [28, {ci} / 16, Cmid / 16, 64, 4], got "
                           f"{tuple(br.shape)}")
    cm = 16 * int(br.shape[2])
    if not aspp_supported(ci, cm, H, W, N, dilations):
        return None
    t = {k: gpu_tensor(_OP, k, packed[k], torch.float32, dev, shape)
         for k, shape in (("branch_scale", (4 * cm,)), ("branch_shift", (4 * cm,)), ("pool_t", (ci, cm)),
                          ("pool_scale", (cm,)), ("pool_shift", (cm,)), ("proj", (1, 4 * cm // 16, cm // 16, 64, 4)),
                          ("proj_pool_t", (cm, cm)), ("proj_scale", (cm,)), ("proj_shift", (cm,)))}
    L = lib()
    nbytes = int(L.pd3_aspp_workspace(N, ci, cm, H, W))
    ws = workspace(nbytes, dev)
    y = torch.empty((N, cm, H, W), dtype=torch.float32, device=dev)
    d = [int(v) for v in dilations]
    st = L.pd3_aspp_forward(ptr(x), ptr(br), ptr(t["branch_scale"]), ptr(t["branch_shift"]), ptr(t["pool_t"]),
                            ptr(t["pool_scale"]), ptr(t["pool_shift"]), ptr(t["proj"]), ptr(t["proj_pool_t"]),
                            ptr(t["proj_scale"]), ptr(t["proj_shift"]), N, ci, cm, H, W, d[0], d[1], d[2], ptr(y),
                            ptr(ws), ws.numel(), stream_ptr(dev))
    if st == _UNSUPPORTED:
        return None
    check(st, f"{_OP}.aspp_forward")
    return y


def depth_softmax_split(x, depth_channels):
    x = gpu_tensor(_OP, "x", x, torch.float32)
    D = int(depth_channels)
    if x.dim() != 4 or not 1 <= D <= x.shape[1]:
        raise RuntimeError(f"{_OP}: x must be [BN, D + C, H, W] with 1 <= D <= D + C, got {tuple(x.shape)} and D = {D}")
    N, DC, H, W = (int(v) for v in x.shape)
    if not tail_supported(N, D, DC - D, H, W):
        return None
    depth = torch.empty((N, D, H, W), dtype=torch.float32, device=x.device)
    feat = torch.empty((N, H, W, DC - D), dtype=torch.float32, device=x.device)
    st = lib().pd3_depth_softmax_split(ptr(x), N, D, DC - D, H, W, ptr(depth), ptr(feat), stream_ptr(x.device))
    if st == _UNSUPPORTED:
        return None
    check(st, f"{_OP}.depth_softmax_split")
    return depth, feat
