"""BEVFormer's decoder attention and NMS-free decode on the device (csrc/bevformer_decoder.hip, C ABI pd3_mha_forward /
pd3_bevformer_dec_ca / pd3_nms_free_decode); the arithmetic order is stated in that file's header and restated in
tests/golden/bevformer_decoder_numpy.py.

multihead_attention(q, k, v, num_heads)
    q [B, Nq, E], k and v [B, Nk, E] (the projected Linear outputs, E = num_heads * d) -> [B, Nq, E]:
    softmax((q * d ** -0.5) k^T) v per head, paddle.nn.MultiHeadAttention's core without masks or dropout.  None when
    the kernel does not take the shape (`mha_supported`).
decoder_cross_attention_sample(value, sampling_offsets, attention_logits, reference_points, spatial_shapes,
                               level_start_index)
    value [B, S, M, C] (projected), sampling_offsets [B, Q, M, L, P, 2], attention_logits [B, Q, M, L*P] (the raw Linear
    outputs), reference_points [B, Q, 1 or L, 2] -> [B, Q, M*C].  None when the kernel does not take the shape
    (`dec_ca_supported`).
nms_free_decode(cls_scores, bbox_preds, post_center_range, max_num, score_threshold=None, bottom_center=False)
    cls_scores [B, Q, K] logits, bbox_preds [B, Q, 8 or 10] -> (boxes [B, max_num, code - 1], scores [B, max_num],
    labels [B, max_num] int32, count [B] int32): NMSFreeCoder.decode for the whole batch; rows at and after count are
    zeros with label -1.

float32 only.  Nothing here synchronises with the host; the kernels run on the current stream.
"""
from __future__ import annotations

import math

import torch

from ._common import check, gpu_tensor, host_f32, lib, ptr, stream_ptr

__all__ = ["multihead_attention", "decoder_cross_attention_sample", "nms_free_decode", "mha_supported",
           "dec_ca_supported", "MAX_HEAD_DIM", "MAX_KEYS", "MAX_LEVEL_POINTS", "MAX_NUM"]

_OP = "bevformer_decoder"
MAX_HEAD_DIM = 128
MAX_KEYS = 2048
MAX_LEVEL_POINTS = 32
MAX_NUM = 1024
_UNSUPPORTED = -3


def mha_supported(head_dim, num_key):
    """The kernel's shape predicate (it also wants 16-byte aligned tensors, which torch's allocations are)."""
    return head_dim >= 16 and head_dim % 16 == 0 and head_dim <= MAX_HEAD_DIM and num_key <= MAX_KEYS


def dec_ca_supported(channels, num_levels, num_points):
    return channels % 4 == 0 and num_levels * num_points <= MAX_LEVEL_POINTS


def multihead_attention(q, k, v, num_heads):
    q = gpu_tensor(_OP, "q", q, torch.float32)
    dev = q.device
    k = gpu_tensor(_OP, "k", k, torch.float32, dev)
    v = gpu_tensor(_OP, "v", v, torch.float32, dev)
    M = int(num_heads)
    if q.dim() != 3 or k.dim() != 3 or tuple(v.shape) != tuple(k.shape) or k.shape[0] != q.shape[0] or \
            k.shape[2] != q.shape[2]:
        raise RuntimeError(f"{_OP}: q must be [B, Nq, E] and k, v [B, Nk, E], got {tuple(q.shape)}, {tuple(k.shape)} "
                           f"and {tuple(v.shape)}")
    B, Nq, E = (int(s) for s in q.shape)
    Nk = int(k.shape[1])
    if M < 1 or E < 1 or E % M != 0:
        raise RuntimeError(f"{_OP}: embed_dims {E} must be a positive multiple of num_heads {M}")
    if Nk < 1 or max(B, Nq, Nk) >= 2 ** 31:
        raise RuntimeError(f"{_OP}: bad sizes {(B, Nq, Nk, M, E)}")
    d = E // M
    out = torch.empty((B, Nq, E), dtype=torch.float32, device=dev)
    st = lib().pd3_mha_forward(ptr(q), ptr(k), ptr(v), B, Nq, Nk, M, d, float(d) ** -0.5, ptr(out), stream_ptr(dev))
    if st == _UNSUPPORTED:
        return None
    check(st, f"{_OP}.multihead_attention")
    return out


def decoder_cross_attention_sample(value, sampling_offsets, attention_logits, reference_points, spatial_shapes,
                                   level_start_index):
    value = gpu_tensor(_OP, "value", value, torch.float32)
    dev = value.device
    off = gpu_tensor(_OP, "sampling_offsets", sampling_offsets, torch.float32, dev)
    logits = gpu_tensor(_OP, "attention_logits", attention_logits, torch.float32, dev)
    ref = gpu_tensor(_OP, "reference_points", reference_points, torch.float32, dev)
    if value.dim() != 4 or off.dim() != 6 or int(off.shape[-1]) != 2:
        raise RuntimeError(f"{_OP}: value must be [B, S, M, C] and sampling_offsets [B, Q, M, L, P, 2], got "
                           f"{tuple(value.shape)} and {tuple(off.shape)}")
    rows, S, M, Ch = (int(s) for s in value.shape)
    B, Q, _, L, P, _ = (int(s) for s in off.shape)
    if rows != B or int(off.shape[2]) != M:
        raise RuntimeError(f"{_OP}: value has {rows} rows and {M} heads, sampling_offsets {tuple(off.shape)}")
    if tuple(logits.shape) != (B, Q, M, L * P):
        raise RuntimeError(f"{_OP}: attention_logits must be {(B, Q, M, L * P)}, got {tuple(logits.shape)}")
    if ref.dim() != 4 or tuple(ref.shape[:2]) != (B, Q) or int(ref.shape[3]) != 2 or int(ref.shape[2]) not in (1, L):
        raise RuntimeError(f"{_OP}: reference_points must be [{B}, {Q}, 1 or {L}, 2], got {tuple(ref.shape)}")
    if S < 1 or M < 1 or Ch < 1 or L < 1 or P < 1 or max(rows, S, Q) >= 2 ** 31:
        raise RuntimeError(f"{_OP}: bad sizes {(rows, S, M, Ch, L, Q, P)}")
    ss = gpu_tensor(_OP, "spatial_shapes", spatial_shapes, torch.int64, dev)
    lsi = gpu_tensor(_OP, "level_start_index", level_start_index, torch.int64, dev)
    if tuple(ss.shape) != (L, 2) or tuple(lsi.shape) != (L,):
        raise RuntimeError(f"{_OP}: spatial_shapes must be [{L}, 2] and level_start_index [{L}], got "
                           f"{tuple(ss.shape)} and {tuple(lsi.shape)}")
    out = torch.empty((B, Q, M * Ch), dtype=torch.float32, device=dev)
    st = lib().pd3_bevformer_dec_ca(ptr(value), ptr(ss), ptr(lsi), ptr(off), ptr(logits), ptr(ref), B, S, M, Ch, L, Q,
                                    P, int(ref.shape[2]), ptr(out), stream_ptr(dev))
    if st == _UNSUPPORTED:
        return None
    check(st, f"{_OP}.decoder_cross_attention_sample")
    return out


def nms_free_decode(cls_scores, bbox_preds, post_center_range, max_num, score_threshold=None, bottom_center=False):
    cls = gpu_tensor(_OP, "cls_scores", cls_scores, torch.float32)
    dev = cls.device
    bbox = gpu_tensor(_OP, "bbox_preds", bbox_preds, torch.float32, dev)
    if cls.dim() != 3 or bbox.dim() != 3 or tuple(bbox.shape[:2]) != tuple(cls.shape[:2]):
        raise RuntimeError(f"{_OP}: cls_scores must be [B, Q, K] and bbox_preds [B, Q, code], got {tuple(cls.shape)} "
                           f"and {tuple(bbox.shape)}")
    B, Q, K = (int(s) for s in cls.shape)
    code = int(bbox.shape[2])
    if code not in (8, 10):
        raise RuntimeError(f"{_OP}: a code size of 8 or 10, got {code}")
    max_num = int(max_num)
    if Q < 1 or K < 1 or Q * K >= 2 ** 31:
        raise RuntimeError(f"{_OP}: bad sizes {(B, Q, K)}")
    if max_num < 1 or max_num > MAX_NUM or max_num > Q * K:
        raise RuntimeError(f"{_OP}: 1 <= max_num <= min({MAX_NUM}, Q * K = {Q * K}), got {max_num}")
    thr = -1.0 if score_threshold is None else float(score_threshold)
    if score_threshold is not None and (thr < 0 or not math.isfinite(thr)):
        raise RuntimeError(f"{_OP}: score_threshold must be None or a finite number >= 0, got {score_threshold}")
    rng = host_f32(post_center_range, 6)
    boxes = torch.empty((B, max_num, code - 1), dtype=torch.float32, device=dev)
    scores = torch.empty((B, max_num), dtype=torch.float32, device=dev)
    labels = torch.empty((B, max_num), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    if B > 0:
        check(lib().pd3_nms_free_decode(ptr(cls), ptr(bbox), ptr(rng), B, Q, K, code, max_num, thr,
                                        1 if bottom_center else 0, ptr(boxes), ptr(scores), ptr(labels), ptr(count),
                                        stream_ptr(dev)), f"{_OP}.nms_free_decode")
    return boxes, scores, labels, count
