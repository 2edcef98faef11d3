"""`paddle3d.ops.ms_deform_attn` mirror (PD_BUILD_OP(ms_deform_attn) + PD_BUILD_GRAD_OP, ms_deform_attn.cc:85-101):
multi-scale deformable attention on the device (csrc/ms_deform_attn.hip, C ABI pd3_ms_deform_attn_forward /
pd3_ms_deform_attn_backward).

ms_deform_attn(value, sampling_locations, attention_weights, spatial_shapes, level_start_index, im2col_step)
    value [B, S, M, C], sampling_locations [B, Q, M, L, P, 2] (x, y in [0, 1]), attention_weights [B, Q, M, L, P],
    spatial_shapes [L, 2] int64 (H, W), level_start_index [L] int64, all on the GPU -> [B, Q, M*C].
    Differentiable: a torch.autograd.Function fills the gradients of value, sampling_locations and
    attention_weights.
ms_deform_attn_backward(grad_out, value, sampling_locations, attention_weights, spatial_shapes, level_start_index,
                        im2col_step) -> (grad_value, grad_sampling_locations, grad_attention_weights)

float32 or float64 (all floating-point inputs the same).  im2col_step is checked as the reference checks it
(batch % min(batch, im2col_step) == 0) and otherwise ignored: one launch covers the batch, so the result does not
depend on it.  Nothing here synchronises with the host; spatial_shapes and level_start_index are read on the device.
"""
from __future__ import annotations

import torch

from ._common import check, gpu_tensor, lib, ptr, stream_ptr

__all__ = ["ms_deform_attn", "ms_deform_attn_backward", "MSDeformAttnFunction"]

_OP = "ms_deform_attn"
_DTYPES = {torch.float32: 0, torch.float64: 1}


def _check(value, sampling_locations, attention_weights, spatial_shapes, level_start_index, im2col_step,
           grad_out=None):
    """Validated contiguous inputs and the dims (B, S, M, C, L, Q, P)."""
    named = [("value", value), ("sampling_locations", sampling_locations), ("attention_weights", attention_weights),
             ("spatial_shapes", spatial_shapes), ("level_start_index", level_start_index)]
    if grad_out is not None:
        named.append(("grad_out", grad_out))
    for what, t in named:
        gpu_tensor(_OP, what, t, dtype=None, contiguous=False)
    dt = value.dtype
    if dt not in _DTYPES:
        raise RuntimeError(f"{_OP}: value must be float32 or float64, got {dt}")
    for what, t in named[1:3] + named[5:]:
        if t.dtype != dt:
            raise RuntimeError(f"{_OP}: {what} must have value's dtype {dt}, got {t.dtype}")
    for what, t in named[3:5]:
        if t.dtype != torch.int64:
            raise RuntimeError(f"{_OP}: {what} must be int64, got {t.dtype}")
    dev = value.device
    for what, t in named:
        if t.device != dev:
            raise RuntimeError(f"{_OP}: {what} is on {t.device}, value on {dev}")
    if value.dim() != 4:
        raise RuntimeError(f"{_OP}: value must be [B, S, M, C], got {tuple(value.shape)}")
    B, S, M, Ch = (int(s) for s in value.shape)
    if sampling_locations.dim() != 6 or int(sampling_locations.shape[-1]) != 2:
        raise RuntimeError(f"{_OP}: sampling_locations must be [B, Q, M, L, P, 2], got "
                           f"{tuple(sampling_locations.shape)}")
    _, Q, _, L, P, _ = (int(s) for s in sampling_locations.shape)
    if tuple(sampling_locations.shape) != (B, Q, M, L, P, 2):
        raise RuntimeError(f"{_OP}: sampling_locations must be {(B, Q, M, L, P, 2)}, got "
                           f"{tuple(sampling_locations.shape)}")
    if tuple(attention_weights.shape) != (B, Q, M, L, P):
        raise RuntimeError(f"{_OP}: attention_weights must be {(B, Q, M, L, P)}, got "
                           f"{tuple(attention_weights.shape)}")
    if tuple(spatial_shapes.shape) != (L, 2) or tuple(level_start_index.shape) != (L,):
        raise RuntimeError(f"{_OP}: spatial_shapes must be [{L}, 2] and level_start_index [{L}], got "
                           f"{tuple(spatial_shapes.shape)} and {tuple(level_start_index.shape)}")
    if grad_out is not None and tuple(grad_out.shape) != (B, Q, M * Ch):
        raise RuntimeError(f"{_OP}: grad_out must be {(B, Q, M * Ch)}, got {tuple(grad_out.shape)}")
    if S < 1 or M < 1 or Ch < 1 or L < 1 or P < 1:
        raise RuntimeError(f"{_OP}: S, M, C, L and P must be >= 1, got {(S, M, Ch, L, P)}")
    if max(B * S * M * Ch, B * Q * M * L * P * 2) >= 2 ** 62 or max(B, S, Q) >= 2 ** 31:
        raise RuntimeError(f"{_OP}: tensor too large")
    if B > 0:
        step = min(B, int(im2col_step))
        if step < 1 or B % step != 0:
            raise RuntimeError(f"batch({B}) must divide im2col_step({step})")
    return B, S, M, Ch, L, Q, P


def _forward(value, sampling_locations, attention_weights, spatial_shapes, level_start_index, im2col_step):
    B, S, M, Ch, L, Q, P = _check(value, sampling_locations, attention_weights, spatial_shapes, level_start_index,
                                  im2col_step)
    v, loc, w = value.contiguous(), sampling_locations.contiguous(), attention_weights.contiguous()
    ss, lsi = spatial_shapes.contiguous(), level_start_index.contiguous()
    out = torch.empty((B, Q, M * Ch), dtype=value.dtype, device=value.device)
    if B == 0 or Q == 0:
        return out
    check(lib().pd3_ms_deform_attn_forward(_DTYPES[value.dtype], ptr(v), ptr(ss), ptr(lsi), ptr(loc), ptr(w), B, S,
                                           M, Ch, L, Q, P, ptr(out), stream_ptr(value.device)), _OP)
    return out


def ms_deform_attn_backward(grad_out, value, sampling_locations, attention_weights, spatial_shapes,
                            level_start_index, im2col_step):
    """The grad op (input order of ms_deform_attn.cc:97-99) -> (grad_value, grad_sampling_locations,
    grad_attention_weights).  grad_value is summed with float atomics (last bits may vary from run to run); the
    other two are reduced in a fixed order."""
    B, S, M, Ch, L, Q, P = _check(value, sampling_locations, attention_weights, spatial_shapes, level_start_index,
                                  im2col_step, grad_out)
    v, loc, w = value.contiguous(), sampling_locations.contiguous(), attention_weights.contiguous()
    ss, lsi, go = spatial_shapes.contiguous(), level_start_index.contiguous(), grad_out.contiguous()
    gv = torch.empty_like(v)
    gl = torch.empty_like(loc)
    ga = torch.empty_like(w)
    if B == 0:
        return gv, gl, ga
    check(lib().pd3_ms_deform_attn_backward(_DTYPES[value.dtype], ptr(v), ptr(ss), ptr(lsi), ptr(loc), ptr(w),
                                            ptr(go), B, S, M, Ch, L, Q, P, ptr(gv), ptr(gl), ptr(ga),
                                            stream_ptr(value.device)), _OP)
    return gv, gl, ga


class MSDeformAttnFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, value, sampling_locations, attention_weights, spatial_shapes, level_start_index, im2col_step):
        ctx.im2col_step = im2col_step
        ctx.save_for_backward(value, sampling_locations, attention_weights, spatial_shapes, level_start_index)
        return _forward(value, sampling_locations, attention_weights, spatial_shapes, level_start_index, im2col_step)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        value, loc, w, ss, lsi = ctx.saved_tensors
        gv, gl, ga = ms_deform_attn_backward(grad_out, value, loc, w, ss, lsi, ctx.im2col_step)
        need = ctx.needs_input_grad
        return (gv if need[0] else None, gl if need[1] else None, ga if need[2] else None, None, None, None)


def ms_deform_attn(value, sampling_locations, attention_weights, spatial_shapes, level_start_index, im2col_step):
    """out [B, Q, M*C] (the reference's op; differentiable in value, sampling_locations and attention_weights)."""
    for t in (value, sampling_locations, attention_weights, spatial_shapes, level_start_index):
        gpu_tensor(_OP, None, t, dtype=None, contiguous=False)  # the device check alone
    return MSDeformAttnFunction.apply(value, sampling_locations, attention_weights, spatial_shapes,
                                      level_start_index, im2col_step)
