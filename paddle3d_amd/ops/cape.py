"""CAPE / CAPE-T's cross-view attention core and 3D sine position embedding on the device (csrc/cape.hip, C ABI
pd3_cape_cva_forward / pd3_cape_posemb3d, declared in include/paddle3d_amd_cape.h); the arithmetic order is stated in
that file's header and restated in tests/golden/cape_numpy.py.

cross_view_attention(q_a, q_g, k_a, k_g, v, scale_a, scale_g, num_heads, mask=None)
    q_a [B, Q, E], q_g [B, N, Q, E], k_a, k_g and v [B, N, K, E] (the projected Linear outputs, E = num_heads * d),
    scale_a and scale_g float32 [num_heads] ON THE DEVICE (they are parameters), mask bool or uint8 [B, N, K] (true:
    masked) -> [B, Q, E]: softmax over the N * K keys of scale_a * (q_a . k_a) + scale_g * (q_g[n] . k_g), masked keys
    at -inf, times v -- what CrossAttention.proj receives.  A query whose keys are all masked gets a NaN row, as in the
    reference.  None when the kernel does not take the shape (`cva_supported`).
posemb3d(points, num_feats, bound=None, rot=None, trans=None, temperature=10000)
    points [B, Q, 3] -> pos2posemb3d of them [B, Q, 3 * num_feats]; with bound (6 floats) un-normalised first; with rot
    [B, N, 3, 3] and trans [B, N, 3] of rot @ (p + trans) per view, [B, N, Q, 3 * num_feats].  None when the kernel does
    not take the shape (`posemb3d_supported`).
dim_t(num_feats, temperature=10000)
    pos2posemb3d's divisors, computed once per (num_feats, temperature) on the host in the reference's own order.

float32 only.  Nothing here synchronises with the host; the kernels run on the current stream.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import torch

from ._common import check, gpu_tensor, host_f32, lib, ptr, stream_ptr

__all__ = ["cross_view_attention", "posemb3d", "cva_supported", "posemb3d_supported", "dim_t", "MAX_HEAD_DIM",
           "MAX_POS_FEATS"]

_OP = "cape"
MAX_HEAD_DIM = 128
MAX_POS_FEATS = 128
_UNSUPPORTED = -3


def _mask_u8(t, dev, shape):
    gpu_tensor(_OP, "mask", t, None, dev, shape, contiguous=False)
    if t.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f"{_OP}: mask must be torch.bool or torch.uint8, got {t.dtype}")
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def cva_supported(head_dim, num_cams=None, num_key=None, num_query=None):
    """The kernel's shape predicate (it also wants 16-byte aligned tensors, which torch's allocations are); every
    num_cams, num_key, num_query >= 1 is taken."""
    return head_dim >= 16 and head_dim % 16 == 0 and head_dim <= MAX_HEAD_DIM


def posemb3d_supported(num_feats):
    return num_feats >= 2 and num_feats % 2 == 0 and num_feats <= MAX_POS_FEATS


@lru_cache(maxsize=None)
def _dim_t(num_feats, temperature):
    t = torch.arange(num_feats, dtype=torch.int32)  # cape_transformer.py:79-80, the same expression
    return np.ascontiguousarray((temperature ** (2 * (t // 2) / num_feats)).numpy().astype(np.float32))


def dim_t(num_feats, temperature=10000):
    return _dim_t(int(num_feats), temperature).copy()


def cross_view_attention(q_a, q_g, k_a, k_g, v, scale_a, scale_g, num_heads, mask=None):
    q_a = gpu_tensor(_OP, "q_a", q_a, torch.float32)
    dev = q_a.device
    q_g = gpu_tensor(_OP, "q_g", q_g, torch.float32, dev)
    k_a = gpu_tensor(_OP, "k_a", k_a, torch.float32, dev)
    if q_a.dim() != 3 or q_g.dim() != 4 or k_a.dim() != 4:
        raise RuntimeError(f"{_OP}: q_a must be [B, Q, E], q_g [B, N, Q, E] and k_a [B, N, K, E], got "
                           f"{tuple(q_a.shape)}, {tuple(q_g.shape)} and {tuple(k_a.shape)}")
    B, Q, E = (int(s) for s in q_a.shape)
    N, K = int(k_a.shape[1]), int(k_a.shape[2])
    gpu_tensor(_OP, "q_g", q_g, torch.float32, dev, (B, N, Q, E), contiguous=False)
    gpu_tensor(_OP, "k_a", k_a, torch.float32, dev, (B, N, K, E), contiguous=False)
    k_g = gpu_tensor(_OP, "k_g", k_g, torch.float32, dev, (B, N, K, E))
    v = gpu_tensor(_OP, "v", v, torch.float32, dev, (B, N, K, E))
    M = int(num_heads)
    if M < 1 or E < 1 or E % M != 0:
        raise RuntimeError(f"{_OP}: embed_dims {E} must be a positive multiple of num_heads {M}")
    if N < 1 or K < 1 or max(B, N, Q, K) >= 2 ** 31:
        raise RuntimeError(f"{_OP}: bad sizes {(B, N, Q, K, M, E)}")
    scale_a = gpu_tensor(_OP, "scale_a", scale_a, torch.float32, dev, (M,))
    scale_g = gpu_tensor(_OP, "scale_g", scale_g, torch.float32, dev, (M,))
    m8 = None
    if mask is not None:
        m8 = _mask_u8(mask, dev, (B, N, K))
    out = torch.empty((B, Q, E), dtype=torch.float32, device=dev)
    st = lib().pd3_cape_cva_forward(ptr(q_a), ptr(q_g), ptr(k_a), ptr(k_g), ptr(v), ptr(m8), ptr(scale_a), ptr(scale_g),
                                    B, N, Q, K, M, E // M, ptr(out), stream_ptr(dev))
    if st == _UNSUPPORTED:
        return None
    check(st, f"{_OP}.cross_view_attention")
    return out


def posemb3d(points, num_feats, bound=None, rot=None, trans=None, temperature=10000):
    p = gpu_tensor(_OP, "points", points, torch.float32)
    dev = p.device
    if p.dim() != 3 or int(p.shape[2]) != 3:
        raise RuntimeError(f"{_OP}: points must be [B, Q, 3], got {tuple(p.shape)}")
    B, Q = int(p.shape[0]), int(p.shape[1])
    F = int(num_feats)
    if F < 1 or max(B, Q, F) >= 2 ** 31:
        raise RuntimeError(f"{_OP}: bad sizes {(B, Q, F)}")
    if (rot is None) != (trans is None):
        raise RuntimeError(f"{_OP}: rot and trans come together")
    N = 0
    if rot is not None:
        rot = gpu_tensor(_OP, "rot", rot, torch.float32, dev)
        if rot.dim() != 4 or tuple(rot.shape[2:]) != (3, 3) or int(rot.shape[0]) != B or int(rot.shape[1]) < 1:
            raise RuntimeError(f"{_OP}: rot must be [{B}, N, 3, 3], got {tuple(rot.shape)}")
        N = int(rot.shape[1])
        trans = gpu_tensor(_OP, "trans", trans, torch.float32, dev, (B, N, 3))
    bnd = None if bound is None else host_f32(bound, 6)
    if not posemb3d_supported(F):
        return None
    out = torch.empty((B, N, Q, 3 * F) if N else (B, Q, 3 * F), dtype=torch.float32, device=dev)
    st = lib().pd3_cape_posemb3d(ptr(p), ptr(bnd), ptr(rot), ptr(trans), ptr(_dim_t(F, temperature)), B, N, Q, F,
                                 ptr(out), stream_ptr(dev))
    if st == _UNSUPPORTED:
        return None
    check(st, f"{_OP}.posemb3d")
    return out
