"""NumPy restatement of the reference's pointnet2 stack ops, in float32 and in the reference kernels' operation order
(csrc/pointnet2_stack.hip states the same contract):

  ball_query_gpu_stack.cu:26-81     ball_query_stack: a row's frame is the first k < B - 1 with row < cnt[0] + ... +
                                    cnt[k], else B - 1.  The frame's points (negative counts read as 0, the range
                                    clamped into [0, N)) are scanned in index order; a hit is ((new_x - x)^2 +
                                    (new_y - y)^2) + (new_z - z)^2 < r2, r2 = radius * radius in fp32.  The first
                                    nsample hits, frame-local; unused slots = the first hit; no hit: [-1, 0, 0, ...].
  voxel_query_gpu.cu:11-93          voxel_query: cells in (dz, dy, dx) order from -range to +range, cells outside the
                                    grid, a batch index outside [0, B), point_indices < 0 and >= N skipped; a hit is
                                    !(((x - new_x)^2 + (y - new_y)^2) + (z - new_z)^2 > r2) (surface and NaN are hits);
                                    indices are rows of xyz; fill and no-hit rows as the ball query.
  group_points_gpu_stack.cu:26-131  grouping_operation_stack: out[m, c, s] = features[start(frame(m)) + idx[m, s], c],
                                    start = the sum of the earlier frames' feature counts; a global row outside
                                    [0, N) reads as 0 and adds nothing to the gradient (a float64 sum here).
"""
import numpy as np

F32 = np.float32
CHUNK = 1 << 22  # distance-matrix elements per step


def frames(m, cnt):
    """Frame of each of m rows by the reference's scan over the counts cnt [B] (raw, 64-bit sums)."""
    cnt = np.asarray(cnt, np.int64).reshape(-1)
    B = cnt.size
    rows = np.arange(m, dtype=np.int64)
    f = np.full(m, B - 1, np.int64)
    if B > 1:
        below = rows[:, None] < np.cumsum(cnt)[None, :B - 1]
        f = np.where(below.any(1), below.argmax(1), B - 1)
    return f


def _starts(cnt, clamp):
    cnt = np.asarray(cnt, np.int64).reshape(-1)
    if clamp:
        cnt = np.maximum(cnt, 0)
    incl = np.cumsum(cnt)
    return incl - cnt, incl


def _d2(ax, ay, az, bx, by, bz):
    """((ax - bx)^2 + (ay - by)^2) + (az - bz)^2 in fp32."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (ax - bx).astype(F32), (ay - by).astype(F32), (az - bz).astype(F32)
        return ((dx * dx + dy * dy) + dz * dz).astype(F32)


def _select(hit, vals, nsample):
    """First nsample hits of each row (in column order) -> [rows, nsample] with the fill and no-hit rules."""
    R = hit.shape[0]
    out = np.zeros((R, nsample), np.int32)
    cnt = hit.sum(1)
    pos = np.cumsum(hit, 1) - 1
    r, c = np.nonzero(hit & (pos < nsample))
    out[r, pos[r, c]] = vals[r, c]
    first = np.where(cnt > 0, vals[np.arange(R), hit.argmax(1)] if hit.shape[1] else 0, 0)
    slot = np.arange(nsample)[None, :]
    out = np.where(slot < cnt[:, None], out, first[:, None]).astype(np.int32)
    out[cnt == 0, 0] = -1
    return out


def _r2(radius):
    r = F32(radius)
    return F32(r * r)


def ball_query_stack(new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, radius, nsample):
    """new_xyz [M, 3], xyz [N, 3], counts [B] -> idx [M, nsample] int32 (frame-local)."""
    q, p = np.asarray(new_xyz, F32).reshape(-1, 3), np.asarray(xyz, F32).reshape(-1, 3)
    M, N, S = q.shape[0], p.shape[0], int(nsample)
    r2 = _r2(radius)
    out = np.zeros((M, S), np.int32)
    f = frames(M, new_xyz_batch_cnt)
    s0, e0 = _starts(xyz_batch_cnt, clamp=True)
    start, end = np.minimum(s0, N), np.minimum(e0, N)
    for b in np.unique(f):
        rows = np.nonzero(f == b)[0]
        pts = p[start[b]:end[b]]
        L = pts.shape[0]
        step = max(1, CHUNK // max(L, 1))
        for i in range(0, rows.size, step):
            r = rows[i:i + step]
            d2 = _d2(q[r, 0:1], q[r, 1:2], q[r, 2:3], pts[None, :, 0], pts[None, :, 1], pts[None, :, 2])
            hit = d2 < r2
            out[r] = _select(hit, np.broadcast_to(np.arange(L, dtype=np.int32), hit.shape), S)
    return out


def window(z_range, y_range, x_range):
    """(dz, dy, dx) offsets of the window in the reference's visiting order."""
    if min(z_range, y_range, x_range) < 0:
        return np.zeros((0, 3), np.int64)
    dz, dy, dx = np.meshgrid(np.arange(-z_range, z_range + 1), np.arange(-y_range, y_range + 1),
                             np.arange(-x_range, x_range + 1), indexing="ij")
    return np.stack([dz.ravel(), dy.ravel(), dx.ravel()], 1).astype(np.int64)


def voxel_query(new_xyz, xyz, new_coords, point_indices, radius, nsample, z_range, y_range, x_range):
    """new_coords [M, 4] (b, z, y, x), point_indices [B, Z, Y, X] -> idx [M, nsample] int32 (rows of xyz)."""
    q, p = np.asarray(new_xyz, F32).reshape(-1, 3), np.asarray(xyz, F32).reshape(-1, 3)
    co = np.asarray(new_coords, np.int64).reshape(-1, 4)
    pi = np.asarray(point_indices, np.int32)
    B, Z, Y, X = pi.shape
    M, N, S = q.shape[0], p.shape[0], int(nsample)
    r2 = _r2(radius)
    w = window(int(z_range), int(y_range), int(x_range))
    out = np.zeros((M, S), np.int32)
    step = max(1, CHUNK // max(len(w), 1))
    for i in range(0, M, step):
        c = co[i:i + step]
        b = c[:, :1]
        z, y, x = c[:, 1:2] + w[None, :, 0], c[:, 2:3] + w[None, :, 1], c[:, 3:4] + w[None, :, 2]
        ok = (b >= 0) & (b < B) & (z >= 0) & (z < Z) & (y >= 0) & (y < Y) & (x >= 0) & (x < X)
        ni = np.where(ok, pi[np.where(ok, b, 0), np.where(ok, z, 0), np.where(ok, y, 0), np.where(ok, x, 0)], -1)
        ok &= (ni >= 0) & (ni < N)
        pt = p[np.where(ok, ni, 0)]
        qq = q[i:i + step]
        d2 = _d2(pt[..., 0], pt[..., 1], pt[..., 2], qq[:, 0:1], qq[:, 1:2], qq[:, 2:3])
        hit = ok & ~(d2 > r2)
        out[i:i + step] = _select(hit, ni.astype(np.int32), S)
    return out


def _global_rows(features_batch_cnt, idx, idx_batch_cnt, n):
    ix = np.asarray(idx, np.int64)
    f = frames(ix.shape[0], idx_batch_cnt)
    start, _ = _starts(features_batch_cnt, clamp=False)
    g = start[f][:, None] + ix
    return g, (g >= 0) & (g < n)


def group_stack(features, features_batch_cnt, idx, idx_batch_cnt):
    """features [N, C], idx [M, nsample] -> [M, C, nsample]."""
    ft = np.asarray(features, F32)
    N = ft.shape[0]
    g, ok = _global_rows(features_batch_cnt, idx, idx_batch_cnt, N)
    vals = ft[np.where(ok, g, 0)] if N else np.zeros(g.shape + (ft.shape[1],), F32)
    return np.where(ok[..., None], vals, F32(0)).transpose(0, 2, 1).astype(F32)


def group_stack_grad(grad_out, features_batch_cnt, idx, idx_batch_cnt, n):
    """grad_out [M, C, nsample] -> grad_features [n, C] (float64 sums)."""
    go = np.asarray(grad_out, np.float64)
    M, C, S = go.shape
    g, ok = _global_rows(features_batch_cnt, idx, idx_batch_cnt, n)
    out = np.zeros((n, C), np.float64)
    np.add.at(out, g[ok], go.transpose(0, 2, 1)[ok])
    return out
