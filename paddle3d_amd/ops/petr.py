"""PETR / PETRv2's streamed attention and 3D position coordinates on the device (csrc/petr.hip, C ABI
pd3_mha_stream_forward / pd3_petr_coords3d); the arithmetic order is stated in that file's header and restated in
tests/golden/petr_numpy.py.

multihead_attention_stream(q, k, v, num_heads, key_padding_mask=None)
    q [B, Nq, E], k and v [B, Nk, E] (the projected Linear outputs, E = num_heads * d), key_padding_mask bool or uint8
    [B, Nk] or [B, 1, Nk] (true: padded) -> [B, Nq, E]: softmax((q * d ** -0.5) k^T + mask) v per head for any number
    of keys; a padded key has -1e9f added to its score, as paddle.nn.MultiHeadAttention does with the inverted mask
    PETRMultiheadAttention hands it.  None when the kernel does not take the shape (`mha_stream_supported`).
petr_coords3d(img2lidars, feat_hw, pad_hw, depth_num, depth_start, position_range, LID, token_mask=None,
              want_mask=False)
    img2lidars [B, N, 4, 4] or [BN, 4, 4] -> coords [BN, 3 * depth_num, H, W], PETRHead.position_embeding's input to
    position_encoder (inverse_sigmoid included); with want_mask also coords_mask bool [BN, H, W], OR-ed with token_mask
    (bool or uint8 [BN, H, W] or [B, N, H, W]).  position_range is rounded to float32 first.

float32 only.  Nothing here synchronises with the host; the kernels run on the current stream.
"""
from __future__ import annotations

import math

import torch

from ._common import check, gpu_tensor, host_f32, lib, ptr, stream_ptr

__all__ = ["multihead_attention_stream", "petr_coords3d", "mha_stream_supported", "coords3d_supported", "MAX_HEAD_DIM"]

_OP = "petr"
MAX_HEAD_DIM = 128
_UNSUPPORTED = -3


def _mask_u8(what, t, dev):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"Unsupported device type for {_OP} operator.")
    if t.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f"{_OP}: {what} must be torch.bool or torch.uint8, got {t.dtype}")
    if t.device != dev:
        raise RuntimeError(f"{_OP}: {what} is on {t.device}, expected {dev}")
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def mha_stream_supported(head_dim, num_key=None):
    """The kernel's shape predicate (it also wants 16-byte aligned tensors, which torch's allocations are); every
    num_key >= 1 is taken."""
    return head_dim >= 16 and head_dim % 16 == 0 and head_dim <= MAX_HEAD_DIM


def coords3d_supported(num_views, feat_h, feat_w, depth_num=None):
    return num_views * feat_h * ((feat_w + 63) // 64) < 2 ** 31


def multihead_attention_stream(q, k, v, num_heads, key_padding_mask=None):
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
    mask = None
    if key_padding_mask is not None:
        mask = _mask_u8("key_padding_mask", key_padding_mask, dev)
        if tuple(mask.shape) not in ((B, Nk), (B, 1, Nk)):
            raise RuntimeError(f"{_OP}: key_padding_mask must be {(B, Nk)} or {(B, 1, Nk)}, got {tuple(mask.shape)}")
    d = E // M
    out = torch.empty((B, Nq, E), dtype=torch.float32, device=dev)
    st = lib().pd3_mha_stream_forward(ptr(q), ptr(k), ptr(v), ptr(mask), B, Nq, Nk, M, d, float(d) ** -0.5, ptr(out),
                                      stream_ptr(dev))
    if st == _UNSUPPORTED:
        return None
    check(st, f"{_OP}.multihead_attention_stream")
    return out


def petr_coords3d(img2lidars, feat_hw, pad_hw, depth_num, depth_start, position_range, LID, token_mask=None,
                  want_mask=False):
    m = gpu_tensor(_OP, "img2lidars", img2lidars, torch.float32)
    dev = m.device
    if m.dim() not in (3, 4) or tuple(m.shape[-2:]) != (4, 4):
        raise RuntimeError(f"{_OP}: img2lidars must be [B, N, 4, 4] or [BN, 4, 4], got {tuple(m.shape)}")
    BN = int(m.numel() // 16)
    H, W = (int(s) for s in feat_hw)
    pad_h, pad_w = (int(s) for s in pad_hw)
    D = int(depth_num)
    ds = float(depth_start)
    if min(H, W, D) < 0 or max(BN, H, W, D) >= 2 ** 31 or not math.isfinite(ds) or not 0 <= min(pad_h, pad_w) or \
            max(pad_h, pad_w) >= 2 ** 31:
        raise RuntimeError(f"{_OP}: bad sizes {(BN, H, W, D, pad_h, pad_w, ds)}")
    rng = host_f32(position_range, 6)
    tm = None
    if token_mask is not None:
        tm = _mask_u8("token_mask", token_mask, dev)
        if int(tm.numel()) != BN * H * W or tuple(tm.shape[-2:]) != (H, W):
            raise RuntimeError(f"{_OP}: token_mask must be [{BN}, {H}, {W}], got {tuple(tm.shape)}")
    coords = torch.empty((BN, 3 * D, H, W), dtype=torch.float32, device=dev)
    cmask = torch.empty((BN, H, W), dtype=torch.uint8, device=dev) if want_mask else None
    st = lib().pd3_petr_coords3d(ptr(m), BN, H, W, D, pad_h, pad_w, ds, ptr(rng), 1 if LID else 0, ptr(tm), ptr(coords),
                                 ptr(cmask), stream_ptr(dev))
    if st == _UNSUPPORTED:
        return None
    check(st, f"{_OP}.petr_coords3d")
    if want_mask:
        if D == 0 and BN * H * W > 0:  # no launch: the mask is the token mask
            cmask = tm.reshape(BN, H, W).clone() if tm is not None else torch.zeros_like(cmask)
        return coords, cmask.view(torch.bool)
    return coords
