"""`paddle3d.ops.pointnet2_ops` mirror: the batch ops (csrc/pointnet2.hip) IA-SSD's SA layers call and the stack ops
(csrc/pointnet2_stack.hip) PV-RCNN's and Voxel R-CNN's set abstractions call.

farthest_point_sample(points, npoints)
    points [B, N, 3] float32 -> idx [B, npoints] int32 (PD_BUILD_OP(farthest_point_sample), sampling.cc:62).
    Ties among equal maximum distances follow the reference's thread layout (include/paddle3d_amd.h).
gather_operation(points, idx)
    points [B, C, N], idx [B, M] int32 -> [B, C, M] (gather_points.cc:100-110); differentiable in points.
ball_query_batch(new_xyz, xyz, radius, nsample)
    new_xyz [B, M, 3], xyz [B, N, 3] -> idx [B, M, nsample] int32 (ball_query_batch.cc:61); a row with no point
    inside the ball is 0 (the reference leaves it undefined).
grouping_operation_batch(points, idx)
    points [B, C, N], idx [B, M, nsample] int32 -> [B, C, M, nsample] (group_points_batch.cc:95-106);
    differentiable in points.

Stack ops: frames are stacked along the rows and told apart by int32 counts [B] that stay on the device; a row's
frame is the reference's scan (the first k < B - 1 whose running count exceeds the row, else B - 1).
ball_query_stack(new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, radius, nsample)
    new_xyz [M, 3], xyz [N, 3] -> idx [M, nsample] int32 (ball_query_stack.cc:73): frame-local indices of the
    first nsample points of the row's frame with d2 < radius^2; unused slots repeat the first hit; a row without
    a hit is [-1, 0, 0, ...].
voxel_query_wrapper(new_xyz, xyz, new_coords, point_indices, radius, nsample, z_range, y_range, x_range)
    new_coords [M, 4] int32 (b, z, y, x), point_indices [B, Z, Y, X] int32 -> idx [M, nsample] int32
    (voxel_query.cc:78): rows of xyz found in the (2z_range+1)(2y_range+1)(2x_range+1) window in dz, dy, dx order
    with !(d2 > radius^2) (the surface and a NaN distance are hits); fill and empty rows as the ball query.
grouping_operation_stack(features, features_batch_cnt, idx, idx_batch_cnt)
    features [N, C], idx [M, nsample] int32 (frame-local) -> [M, C, nsample] (group_points_stack.cc:117-130);
    differentiable in features.

float32 only, int32 indices, on the GPU.  Indices outside [0, N) (for the stack grouping: the frame's start plus
the index) read as 0 and add nothing to a gradient.  The gradients are summed with float atomics: their last bits
may vary from run to run, as the reference's do.  Nothing here synchronises with the host; M == 0 launches nothing.
"""
from __future__ import annotations

import torch

from ._common import check, gpu_tensor, lib, ptr, stream_ptr, workspace

__all__ = ["farthest_point_sample", "gather_operation", "ball_query_batch", "grouping_operation_batch",
           "gather_operation_grad", "grouping_operation_batch_grad", "GatherOperation", "GroupingOperationBatch",
           "ball_query_stack", "voxel_query_wrapper", "grouping_operation_stack", "grouping_operation_stack_grad",
           "GroupingOperationStack"]


def _same_device(op, *ts):
    dev = ts[0].device
    for t in ts[1:]:
        if t.device != dev:
            raise RuntimeError(f"{op}: tensors on {dev} and {t.device}")


def _xyz(t, op, what):
    gpu_tensor(op, what, t, torch.float32, contiguous=False)
    if t.dim() != 3 or int(t.shape[2]) != 3:
        raise RuntimeError(f"{op}: {what} must be [B, N, 3], got {tuple(t.shape)}")
    return t.contiguous()


def farthest_point_sample(points, npoints, tier: int = 0):
    """idx [B, npoints] int32.  tier 0 picks the kernel (register tier for N <= 16384); 1 / 2 force the register /
    general tier (tests and measurements)."""
    op = "farthest_point_sample"
    xyz = _xyz(points, op, "points")
    B, N = int(xyz.shape[0]), int(xyz.shape[1])
    m = int(npoints)
    idx = torch.empty((B, max(m, 0)), dtype=torch.int32, device=xyz.device)
    if B == 0 or m <= 0:
        return idx
    if N == 0:
        raise RuntimeError(f"{op}: no points to sample {m} from")
    nbytes = int(lib().pd3_farthest_point_sample_workspace(B, N, int(tier)))
    ws = workspace(nbytes, xyz.device) if nbytes else None
    check(lib().pd3_farthest_point_sample(ptr(xyz), B, N, m, int(tier), ptr(ws), nbytes, ptr(idx),
                                          stream_ptr(xyz.device)), op)
    return idx


def _features(points, op):
    gpu_tensor(op, "points", points, torch.float32, contiguous=False)
    if points.dim() != 3:
        raise RuntimeError(f"{op}: points must be [B, C, N], got {tuple(points.shape)}")
    return points.contiguous()


def _gather_fwd(points, idx):
    op = "gather_operation"
    pts = _features(points, op)
    gpu_tensor(op, "idx", idx, torch.int32, contiguous=False)
    _same_device(op, pts, idx)
    B, C, N = (int(s) for s in pts.shape)
    if idx.dim() != 2 or int(idx.shape[0]) != B:
        raise RuntimeError(f"{op}: idx must be [{B}, M], got {tuple(idx.shape)}")
    M = int(idx.shape[1])
    ix = idx.contiguous()
    out = torch.empty((B, C, M), dtype=torch.float32, device=pts.device)
    check(lib().pd3_gather_points(ptr(pts), ptr(ix), B, C, N, M, ptr(out), stream_ptr(pts.device)), op)
    return out


def gather_operation_grad(grad_out, idx, n):
    """The grad op (gather_points.cc:108-110): grad_out [B, C, M], idx [B, M] -> grad_points [B, C, n]."""
    op = "gather_operation_grad"
    go = _features(grad_out, op)
    gpu_tensor(op, "idx", idx, torch.int32, contiguous=False)
    _same_device(op, go, idx)
    B, C, M = (int(s) for s in go.shape)
    if tuple(idx.shape) != (B, M):
        raise RuntimeError(f"{op}: idx must be {(B, M)}, got {tuple(idx.shape)}")
    gp = torch.empty((B, C, int(n)), dtype=torch.float32, device=go.device)
    check(lib().pd3_gather_points_grad(ptr(go), ptr(idx.contiguous()), B, C, int(n), M, ptr(gp),
                                       stream_ptr(go.device)), op)
    return gp


def _group_fwd(points, idx):
    op = "grouping_operation_batch"
    pts = _features(points, op)
    gpu_tensor(op, "idx", idx, torch.int32, contiguous=False)
    _same_device(op, pts, idx)
    B, C, N = (int(s) for s in pts.shape)
    if idx.dim() != 3 or int(idx.shape[0]) != B:
        raise RuntimeError(f"{op}: idx must be [{B}, npoints, nsample], got {tuple(idx.shape)}")
    P, S = int(idx.shape[1]), int(idx.shape[2])
    out = torch.empty((B, C, P, S), dtype=torch.float32, device=pts.device)
    check(lib().pd3_group_points_batch(ptr(pts), ptr(idx.contiguous()), B, C, N, P, S, ptr(out),
                                       stream_ptr(pts.device)), op)
    return out


def grouping_operation_batch_grad(grad_out, idx, n):
    """The grad op (group_points_batch.cc:103-106): grad_out [B, C, P, S], idx [B, P, S] -> grad_points [B, C, n]."""
    op = "grouping_operation_batch_grad"
    gpu_tensor(op, "grad_out", grad_out, torch.float32, contiguous=False)
    if grad_out.dim() != 4:
        raise RuntimeError(f"{op}: grad_out must be [B, C, npoints, nsample], got {tuple(grad_out.shape)}")
    go = grad_out.contiguous()
    gpu_tensor(op, "idx", idx, torch.int32, contiguous=False)
    _same_device(op, go, idx)
    B, C, P, S = (int(s) for s in go.shape)
    if tuple(idx.shape) != (B, P, S):
        raise RuntimeError(f"{op}: idx must be {(B, P, S)}, got {tuple(idx.shape)}")
    gp = torch.empty((B, C, int(n)), dtype=torch.float32, device=go.device)
    check(lib().pd3_group_points_batch_grad(ptr(go), ptr(idx.contiguous()), B, C, int(n), P, S, ptr(gp),
                                            stream_ptr(go.device)), op)
    return gp


class GatherOperation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, idx):
        ctx.n = int(points.shape[2])
        ctx.save_for_backward(idx)
        ctx.mark_non_differentiable(idx)
        return _gather_fwd(points, idx)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        return gather_operation_grad(grad_out, idx, ctx.n), None


class GroupingOperationBatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, idx):
        ctx.n = int(points.shape[2])
        ctx.save_for_backward(idx)
        return _group_fwd(points, idx)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        return grouping_operation_batch_grad(grad_out, idx, ctx.n), None


def gather_operation(points, idx):
    """[B, C, M] = points[b, c, idx[b, m]] (differentiable in points)."""
    _features(points, "gather_operation")
    gpu_tensor("gather_operation", "idx", idx, torch.int32, contiguous=False)
    return GatherOperation.apply(points, idx)


def grouping_operation_batch(points, idx):
    """[B, C, npoints, nsample] = points[b, c, idx[b, p, s]] (differentiable in points)."""
    _features(points, "grouping_operation_batch")
    gpu_tensor("grouping_operation_batch", "idx", idx, torch.int32, contiguous=False)
    return GroupingOperationBatch.apply(points, idx)


def ball_query_batch(new_xyz, xyz, radius, nsample):
    """idx [B, M, nsample] int32: the first nsample points of xyz, in index order, strictly inside the ball of
    radius around each new_xyz row; unused slots repeat the first hit; rows without a hit are 0."""
    op = "ball_query_batch"
    q = _xyz(new_xyz, op, "new_xyz")
    p = _xyz(xyz, op, "xyz")
    _same_device(op, q, p)
    B, M = int(q.shape[0]), int(q.shape[1])
    if int(p.shape[0]) != B:
        raise RuntimeError(f"{op}: new_xyz has batch {B}, xyz {int(p.shape[0])}")
    N, S = int(p.shape[1]), int(nsample)
    if S < 0:
        raise RuntimeError(f"{op}: nsample must be >= 0, got {S}")
    idx = torch.empty((B, M, S), dtype=torch.int32, device=q.device)
    check(lib().pd3_ball_query_batch(ptr(q), ptr(p), B, N, M, float(radius), S, ptr(idx), stream_ptr(q.device)),
          op)
    return idx


# ---- stack ops ------------------------------------------------------------------------------------------------------
def _rows(t, op, what, width, dtype=torch.float32):
    gpu_tensor(op, what, t, dtype, contiguous=False)
    if t.dim() != 2 or (width is not None and int(t.shape[1]) != width):
        raise RuntimeError(f"{op}: {what} must be [rows, {width if width is not None else 'C'}], got {tuple(t.shape)}")
    return t.contiguous()


def _counts(t, op, what):
    gpu_tensor(op, what, t, torch.int32, contiguous=False)
    if t.dim() != 1:
        raise RuntimeError(f"{op}: {what} must be [B], got {tuple(t.shape)}")
    return t.contiguous()


def _nsample(nsample, op):
    S = int(nsample)
    if S < 1:
        raise RuntimeError(f"{op}: nsample must be >= 1, got {S}")
    return S


def _batch(op, B, M, *cnts):
    for c in cnts:
        if int(c.shape[0]) != B:
            raise RuntimeError(f"{op}: batch counts of {B} and {int(c.shape[0])} frames")
    if B == 0 and M > 0:
        raise RuntimeError(f"{op}: {M} rows but no frame")


def ball_query_stack(new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, radius, nsample):
    """idx [M, nsample] int32, frame-local: the first nsample points of the row's frame, in index order, strictly
    inside the ball; unused slots repeat the first hit; a row without a hit is [-1, 0, 0, ...]."""
    op = "ball_query_stack"
    q = _rows(new_xyz, op, "new_xyz", 3)
    qc = _counts(new_xyz_batch_cnt, op, "new_xyz_batch_cnt")
    p = _rows(xyz, op, "xyz", 3)
    pc = _counts(xyz_batch_cnt, op, "xyz_batch_cnt")
    _same_device(op, q, qc, p, pc)
    S = _nsample(nsample, op)
    M, N, B = int(q.shape[0]), int(p.shape[0]), int(pc.shape[0])
    _batch(op, B, M, qc)
    idx = torch.empty((M, S), dtype=torch.int32, device=q.device)
    if M == 0:
        return idx
    check(lib().pd3_ball_query_stack(ptr(q), ptr(qc), ptr(p), ptr(pc), B, M, N, float(radius), S, ptr(idx),
                                     stream_ptr(q.device)), op)
    return idx


def voxel_query_wrapper(new_xyz, xyz, new_coords, point_indices, radius, nsample, z_range, y_range, x_range):
    """idx [M, nsample] int32 of rows of xyz: the first nsample points of the window's cells (dz, then dy, then dx)
    with !(d2 > radius^2); unused slots repeat the first hit; a row without a hit is [-1, 0, 0, ...]."""
    op = "voxel_query_wrapper"
    q = _rows(new_xyz, op, "new_xyz", 3)
    p = _rows(xyz, op, "xyz", 3)
    co = _rows(new_coords, op, "new_coords", 4, torch.int32)
    gpu_tensor(op, "point_indices", point_indices, torch.int32, contiguous=False)
    if point_indices.dim() != 4:
        raise RuntimeError(f"{op}: point_indices must be [B, Z, Y, X], got {tuple(point_indices.shape)}")
    pi = point_indices.contiguous()
    _same_device(op, q, p, co, pi)
    S = _nsample(nsample, op)
    M, N = int(q.shape[0]), int(p.shape[0])
    if int(co.shape[0]) != M:
        raise RuntimeError(f"{op}: new_coords has {int(co.shape[0])} rows, new_xyz {M}")
    B, Z, Y, X = (int(s) for s in pi.shape)
    _batch(op, B, M)
    idx = torch.empty((M, S), dtype=torch.int32, device=q.device)
    if M == 0:
        return idx
    check(lib().pd3_voxel_query(ptr(q), ptr(p), ptr(co), ptr(pi), M, N, B, Z, Y, X, float(radius), S, int(z_range),
                                int(y_range), int(x_range), ptr(idx), stream_ptr(q.device)), op)
    return idx


def _group_stack_fwd(features, features_batch_cnt, idx, idx_batch_cnt):
    op = "grouping_operation_stack"
    f = _rows(features, op, "features", None)
    fc = _counts(features_batch_cnt, op, "features_batch_cnt")
    ix = _rows(idx, op, "idx", None, torch.int32)
    ic = _counts(idx_batch_cnt, op, "idx_batch_cnt")
    _same_device(op, f, fc, ix, ic)
    N, C = int(f.shape[0]), int(f.shape[1])
    M, S = int(ix.shape[0]), int(ix.shape[1])
    _nsample(S, op)
    B = int(ic.shape[0])
    _batch(op, B, M, fc)
    out = torch.empty((M, C, S), dtype=torch.float32, device=f.device)
    if M == 0:
        return out
    check(lib().pd3_group_points_stack(ptr(f), ptr(fc), ptr(ix), ptr(ic), B, N, C, M, S, ptr(out),
                                       stream_ptr(f.device)), op)
    return out


def grouping_operation_stack_grad(grad_out, features_batch_cnt, idx, idx_batch_cnt, n):
    """The grad op (group_points_stack.cc:126-130): grad_out [M, C, nsample] -> grad_features [n, C]."""
    op = "grouping_operation_stack_grad"
    gpu_tensor(op, "grad_out", grad_out, torch.float32, contiguous=False)
    if grad_out.dim() != 3:
        raise RuntimeError(f"{op}: grad_out must be [M, C, nsample], got {tuple(grad_out.shape)}")
    go = grad_out.contiguous()
    fc = _counts(features_batch_cnt, op, "features_batch_cnt")
    ix = _rows(idx, op, "idx", None, torch.int32)
    ic = _counts(idx_batch_cnt, op, "idx_batch_cnt")
    _same_device(op, go, fc, ix, ic)
    M, C, S = (int(s) for s in go.shape)
    if tuple(ix.shape) != (M, S):
        raise RuntimeError(f"{op}: idx must be {(M, S)}, got {tuple(ix.shape)}")
    _nsample(S, op)
    B = int(ic.shape[0])
    _batch(op, B, M, fc)
    gf = torch.empty((int(n), C), dtype=torch.float32, device=go.device)
    check(lib().pd3_group_points_stack_grad(ptr(go), ptr(ix), ptr(ic), ptr(fc), B, int(n), C, M, S, ptr(gf),
                                            stream_ptr(go.device)), op)
    return gf


class GroupingOperationStack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, features_batch_cnt, idx, idx_batch_cnt):
        ctx.n = int(features.shape[0])
        ctx.save_for_backward(features_batch_cnt, idx, idx_batch_cnt)
        return _group_stack_fwd(features, features_batch_cnt, idx, idx_batch_cnt)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        fc, idx, ic = ctx.saved_tensors
        return grouping_operation_stack_grad(grad_out, fc, idx, ic, ctx.n), None, None, None


def grouping_operation_stack(features, features_batch_cnt, idx, idx_batch_cnt):
    """[M, C, nsample] = features[start(frame(m)) + idx[m, s], c] (differentiable in features)."""
    op = "grouping_operation_stack"
    _rows(features, op, "features", None)
    gpu_tensor(op, "idx", idx, torch.int32, contiguous=False)
    return GroupingOperationStack.apply(features, features_batch_cnt, idx, idx_batch_cnt)
