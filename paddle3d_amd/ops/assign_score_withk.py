"""`paddle3d.ops.assign_score_withk` mirror (PD_BUILD_OP(assign_score_withk) + PD_BUILD_GRAD_OP,
assign_score_withk_cuda.cc:265-274): PAConv's assembly of weight-bank features with ScoreNet scores on the device
(csrc/assign_score_withk.hip, C ABI pd3_assign_score_withk_forward / pd3_assign_score_withk_backward).

assign_score_withk(scores, points, centers, knn_idx)
    scores [B, N, K, M], points [B, N, M, O], centers [B, N, M, O] float32, knn_idx [B, N, K] int64, all on the GPU
    -> output [B, O, N].  Differentiable: a torch.autograd.Function fills the gradients of scores, points and centers
    (only those autograd asks for are computed).
assign_score_withk_backward(grad_out, scores, points, centers, knn_idx, need=(True, True, True))
    -> (grad_scores, grad_points, grad_centers); an output not in `need` is None and is not computed.

float32 only.  Every result is bitwise reproducible (no float atomics).  A knn_idx entry outside [0, N) reads points
as 0 (the reference reads out of bounds there).  Nothing here synchronises with the host.
"""
from __future__ import annotations

import torch

from ._common import check, gpu_tensor, lib, ptr, stream_ptr, workspace

__all__ = ["assign_score_withk", "assign_score_withk_backward", "AssignScoreWithKFunction"]

_OP = "assign_score_withk"


def _check(scores, points, centers, knn_idx, grad_out=None):
    """Validated inputs and the dims (B, N, K, M, O)."""
    named = [("scores", scores), ("points", points), ("centers", centers), ("knn_idx", knn_idx)]
    if grad_out is not None:
        named.append(("grad_out", grad_out))
    for what, t in named:
        gpu_tensor(_OP, what, t, dtype=None, contiguous=False)
    for what, t in named[:3] + named[4:]:
        if t.dtype != torch.float32:
            raise RuntimeError(f"{_OP}: {what} must be float32, got {t.dtype}")
    if knn_idx.dtype != torch.int64:
        raise RuntimeError(f"{_OP}: knn_idx must be int64, got {knn_idx.dtype}")
    dev = scores.device
    for what, t in named:
        if t.device != dev:
            raise RuntimeError(f"{_OP}: {what} is on {t.device}, scores on {dev}")
    if points.dim() != 4:
        raise RuntimeError(f"{_OP}: points must be [B, N, M, O], got {tuple(points.shape)}")
    B, N, M, O = (int(s) for s in points.shape)
    if tuple(centers.shape) != (B, N, M, O):
        raise RuntimeError(f"{_OP}: centers must be {(B, N, M, O)}, got {tuple(centers.shape)}")
    if scores.dim() != 4 or (int(scores.shape[0]), int(scores.shape[1]), int(scores.shape[3])) != (B, N, M):
        raise RuntimeError(f"{_OP}: scores must be [{B}, {N}, K, {M}], got {tuple(scores.shape)}")
    K = int(scores.shape[2])
    if tuple(knn_idx.shape) != (B, N, K):
        raise RuntimeError(f"{_OP}: knn_idx must be {(B, N, K)}, got {tuple(knn_idx.shape)}")
    if grad_out is not None and tuple(grad_out.shape) != (B, O, N):
        raise RuntimeError(f"{_OP}: grad_out must be {(B, O, N)}, got {tuple(grad_out.shape)}")
    if B * N * K >= 2 ** 31 or max(B * N * M * O, B * N * K * M) >= 2 ** 62 or max(B, N, M, O) >= 2 ** 31:
        raise RuntimeError(f"{_OP}: tensor too large (B*N*K must stay below 2^31)")
    return B, N, K, M, O


def _forward(scores, points, centers, knn_idx):
    B, N, K, M, O = _check(scores, points, centers, knn_idx)
    s, p, c, idx = scores.contiguous(), points.contiguous(), centers.contiguous(), knn_idx.contiguous()
    out = torch.empty((B, O, N), dtype=torch.float32, device=scores.device)
    if out.numel() == 0:
        return out
    check(lib().pd3_assign_score_withk_forward(ptr(s), ptr(p), ptr(c), ptr(idx), B, N, K, M, O, ptr(out),
                                               stream_ptr(scores.device)), _OP)
    return out


def assign_score_withk_backward(grad_out, scores, points, centers, knn_idx, need=(True, True, True)):
    """The grad op -> (grad_scores, grad_points, grad_centers) in the shapes of their inputs; the outputs whose
    `need` entry is false are None and are not computed."""
    B, N, K, M, O = _check(scores, points, centers, knn_idx, grad_out)
    s, p, c, idx, go = (scores.contiguous(), points.contiguous(), centers.contiguous(), knn_idx.contiguous(),
                        grad_out.contiguous())
    gs = torch.empty_like(s) if need[0] else None
    gp = torch.empty_like(p) if need[1] else None
    gc = torch.empty_like(c) if need[2] else None
    if not any(need) or B * N * M == 0:
        return gs, gp, gc
    L = lib()
    ws = workspace(L.pd3_assign_score_withk_backward_workspace(B, N, K, O), scores.device)
    check(L.pd3_assign_score_withk_backward(ptr(go), ptr(s), ptr(p), ptr(c), ptr(idx), B, N, K, M, O, ptr(gs),
                                            ptr(gp), ptr(gc), ptr(ws), ws.numel(), stream_ptr(scores.device)), _OP)
    return gs, gp, gc


class AssignScoreWithKFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, points, centers, knn_idx):
        ctx.save_for_backward(scores, points, centers, knn_idx)
        return _forward(scores, points, centers, knn_idx)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        scores, points, centers, knn_idx = ctx.saved_tensors
        need = ctx.needs_input_grad[:3]
        gs, gp, gc = assign_score_withk_backward(grad_out, scores, points, centers, knn_idx, need)
        return gs, gp, gc, None


def assign_score_withk(scores, points, centers, knn_idx):
    """output [B, O, N] (the reference's op; differentiable in scores, points and centers)."""
    for t in (scores, points, centers, knn_idx):
        gpu_tensor(_OP, None, t, dtype=None, contiguous=False)  # the device check alone
    return AssignScoreWithKFunction.apply(scores, points, centers, knn_idx)
