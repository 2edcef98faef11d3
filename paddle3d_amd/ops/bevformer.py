"""BEVFormer's encoder attention on the device (csrc/bevformer.hip, C ABI pd3_bevformer_point_sampling /
pd3_bevformer_sca / pd3_bevformer_tsa); the arithmetic order is stated in that file's header and restated in
tests/golden/bevformer_numpy.py.

point_sampling(ref_3d, lidar2img, pc_range, img_h, img_w)
    ref_3d [D, Q, 3] in [0, 1], lidar2img [B, cams, 4, 4] -> (reference_points_cam [cams, B, Q, D, 2],
    bev_mask [cams, B, Q, D] uint8, hit_bits [B, Q] uint8, hit_count [B, Q] uint8): BEVFormerEncoder.point_sampling
    (encoders.py:120-176) plus, per query, which cameras see any of its anchors.
spatial_cross_attention_sample(value, sampling_offsets, attention_logits, reference_points_cam, hit_bits,
                               spatial_shapes, level_start_index, num_cams)
    value [B*cams, S, M, C] (projected), sampling_offsets [B, Q, M, L, P, 2] and attention_logits [B, Q, M, L*P] (the
    raw Linear outputs on the BEV queries) -> [B, Q, M*C]: softmax, sampling of every hit camera, sum in camera
    order, division by max(hit count, 1).  None when the kernel does not take the shape (`sca_supported`).
temporal_self_attention_sample(value, sampling_offsets, attention_logits, reference_points, spatial_shapes,
                               level_start_index)
    value [B*2, S, M, C], sampling_offsets [B, Q, M, 2, L, P, 2], attention_logits [B, Q, M, 2, L*P] (the Linear's own
    layout), reference_points [B*2, Q, L, 2] -> [B, Q, M*C], the mean over the two queue entries.  None when the
    kernel does not take the shape (`tsa_supported`).

float32 only.  Nothing here synchronises with the host; the kernels run on the current stream.
"""
from __future__ import annotations

import torch

from ._common import check, gpu_tensor, host_f32, lib, ptr, stream_ptr

__all__ = ["point_sampling", "spatial_cross_attention_sample", "temporal_self_attention_sample", "sca_supported",
           "tsa_supported", "MAX_CAMS", "MAX_LEVEL_POINTS"]

_OP = "bevformer"
MAX_CAMS = 8
MAX_LEVEL_POINTS = 32
_UNSUPPORTED = -3


def sca_supported(channels, num_levels, num_points, num_cams, num_anchors):
    """The kernel's shape predicate (it also wants 16-byte aligned tensors, which torch's allocations are)."""
    return (channels % 4 == 0 and num_levels * num_points <= MAX_LEVEL_POINTS and num_cams <= MAX_CAMS
            and num_anchors >= 1 and num_points % num_anchors == 0)


def tsa_supported(channels, num_levels, num_points):
    return channels % 4 == 0 and num_levels * num_points <= MAX_LEVEL_POINTS


def point_sampling(ref_3d, lidar2img, pc_range, img_h, img_w):
    ref_3d = gpu_tensor(_OP, "ref_3d", ref_3d, torch.float32)
    dev = ref_3d.device
    lidar2img = gpu_tensor(_OP, "lidar2img", lidar2img, torch.float32, dev)
    if ref_3d.dim() != 3 or int(ref_3d.shape[2]) != 3:
        raise RuntimeError(f"{_OP}: ref_3d must be [D, Q, 3], got {tuple(ref_3d.shape)}")
    if lidar2img.dim() != 4 or tuple(lidar2img.shape[2:]) != (4, 4):
        raise RuntimeError(f"{_OP}: lidar2img must be [B, cams, 4, 4], got {tuple(lidar2img.shape)}")
    D, Q = int(ref_3d.shape[0]), int(ref_3d.shape[1])
    B, cams = int(lidar2img.shape[0]), int(lidar2img.shape[1])
    if D < 1 or cams < 1 or cams > MAX_CAMS:
        raise RuntimeError(f"{_OP}: 1 <= cameras <= {MAX_CAMS} and D >= 1, got cams {cams}, D {D}")
    if int(img_h) < 1 or int(img_w) < 1:
        raise RuntimeError(f"{_OP}: the image size must be positive, got {(img_h, img_w)}")
    pc = host_f32(pc_range, 6)
    ref_cam = torch.empty((cams, B, Q, D, 2), dtype=torch.float32, device=dev)
    mask = torch.empty((cams, B, Q, D), dtype=torch.uint8, device=dev)
    bits = torch.empty((B, Q), dtype=torch.uint8, device=dev)
    count = torch.empty((B, Q), dtype=torch.uint8, device=dev)
    if B > 0 and Q > 0:
        check(lib().pd3_bevformer_point_sampling(ptr(ref_3d), ptr(lidar2img), ptr(pc), int(img_h), int(img_w), B, cams,
                                                 Q, D, ptr(ref_cam), ptr(mask), ptr(bits), ptr(count),
                                                 stream_ptr(dev)), f"{_OP}.point_sampling")
    return ref_cam, mask, bits, count


def _levels(spatial_shapes, level_start_index, L, dev):
    ss = gpu_tensor(_OP, "spatial_shapes", spatial_shapes, torch.int64, dev)
    lsi = gpu_tensor(_OP, "level_start_index", level_start_index, torch.int64, dev)
    if tuple(ss.shape) != (L, 2) or tuple(lsi.shape) != (L,):
        raise RuntimeError(f"{_OP}: spatial_shapes must be [{L}, 2] and level_start_index [{L}], got "
                           f"{tuple(ss.shape)} and {tuple(lsi.shape)}")
    return ss, lsi


def spatial_cross_attention_sample(value, sampling_offsets, attention_logits, reference_points_cam, hit_bits,
                                   spatial_shapes, level_start_index, num_cams):
    value = gpu_tensor(_OP, "value", value, torch.float32)
    dev = value.device
    off = gpu_tensor(_OP, "sampling_offsets", sampling_offsets, torch.float32, dev)
    logits = gpu_tensor(_OP, "attention_logits", attention_logits, torch.float32, dev)
    ref = gpu_tensor(_OP, "reference_points_cam", reference_points_cam, torch.float32, dev)
    bits = gpu_tensor(_OP, "hit_bits", hit_bits, torch.uint8, dev)
    if value.dim() != 4 or off.dim() != 6 or int(off.shape[-1]) != 2:
        raise RuntimeError(f"{_OP}: value must be [B*cams, S, M, C] and sampling_offsets [B, Q, M, L, P, 2], got "
                           f"{tuple(value.shape)} and {tuple(off.shape)}")
    rows, S, M, Ch = (int(s) for s in value.shape)
    B, Q, _, L, P, _ = (int(s) for s in off.shape)
    cams = int(num_cams)
    if cams < 1 or rows != B * cams or int(off.shape[2]) != M:
        raise RuntimeError(f"{_OP}: value has {rows} rows and {M} heads, sampling_offsets {tuple(off.shape)}, "
                           f"num_cams {cams}")
    if tuple(logits.shape) != (B, Q, M, L * P):
        raise RuntimeError(f"{_OP}: attention_logits must be {(B, Q, M, L * P)}, got {tuple(logits.shape)}")
    if ref.dim() != 5 or tuple(ref.shape[:3]) != (cams, B, Q) or int(ref.shape[4]) != 2 or int(ref.shape[3]) < 1:
        raise RuntimeError(f"{_OP}: reference_points_cam must be [{cams}, {B}, {Q}, D, 2], got {tuple(ref.shape)}")
    D = int(ref.shape[3])
    if tuple(bits.shape) != (B, Q):
        raise RuntimeError(f"{_OP}: hit_bits must be {(B, Q)}, got {tuple(bits.shape)}")
    if S < 1 or M < 1 or Ch < 1 or L < 1 or P < 1 or max(rows, S, Q) >= 2 ** 31:
        raise RuntimeError(f"{_OP}: bad sizes {(rows, S, M, Ch, L, Q, P)}")
    ss, lsi = _levels(spatial_shapes, level_start_index, L, dev)
    out = torch.empty((B, Q, M * Ch), dtype=torch.float32, device=dev)
    st = lib().pd3_bevformer_sca(ptr(value), ptr(ss), ptr(lsi), ptr(off), ptr(logits), ptr(ref), ptr(bits), B, cams, S,
                                 M, Ch, L, Q, P, D, ptr(out), stream_ptr(dev))
    if st == _UNSUPPORTED:
        return None
    check(st, f"{_OP}.spatial_cross_attention_sample")
    return out


def temporal_self_attention_sample(value, sampling_offsets, attention_logits, reference_points, spatial_shapes,
                                   level_start_index):
    value = gpu_tensor(_OP, "value", value, torch.float32)
    dev = value.device
    off = gpu_tensor(_OP, "sampling_offsets", sampling_offsets, torch.float32, dev)
    logits = gpu_tensor(_OP, "attention_logits", attention_logits, torch.float32, dev)
    ref = gpu_tensor(_OP, "reference_points", reference_points, torch.float32, dev)
    if value.dim() != 4 or off.dim() != 7 or int(off.shape[-1]) != 2 or int(off.shape[3]) != 2:
        raise RuntimeError(f"{_OP}: value must be [B*2, S, M, C] and sampling_offsets [B, Q, M, 2, L, P, 2], got "
                           f"{tuple(value.shape)} and {tuple(off.shape)}")
    rows, S, M, Ch = (int(s) for s in value.shape)
    B, Q, _, _, L, P, _ = (int(s) for s in off.shape)
    if rows != 2 * B or int(off.shape[2]) != M:
        raise RuntimeError(f"{_OP}: value has {rows} rows and {M} heads, sampling_offsets {tuple(off.shape)}")
    if tuple(logits.shape) != (B, Q, M, 2, L * P):
        raise RuntimeError(f"{_OP}: attention_logits must be {(B, Q, M, 2, L * P)}, got {tuple(logits.shape)}")
    if tuple(ref.shape) != (2 * B, Q, L, 2):
        raise RuntimeError(f"{_OP}: reference_points must be {(2 * B, Q, L, 2)}, got {tuple(ref.shape)}")
    if S < 1 or M < 1 or Ch < 1 or L < 1 or P < 1 or max(rows, S, Q) >= 2 ** 31:
        raise RuntimeError(f"{_OP}: bad sizes {(rows, S, M, Ch, L, Q, P)}")
    ss, lsi = _levels(spatial_shapes, level_start_index, L, dev)
    out = torch.empty((B, Q, M * Ch), dtype=torch.float32, device=dev)
    st = lib().pd3_bevformer_tsa(ptr(value), ptr(ss), ptr(lsi), ptr(off), ptr(logits), ptr(ref), B, S, M, Ch, L, Q, P,
                                 ptr(out), stream_ptr(dev))
    if st == _UNSUPPORTED:
        return None
    check(st, f"{_OP}.temporal_self_attention_sample")
    return out
