"""NumPy restatement of the reference's pointnet2 batch ops and roiaware_pool3d.points_in_boxes_gpu, in float32 and
in the reference kernels' operation order (csrc/pointnet2.hip states the same contract):

  sampling_gpu.cu:37-149            farthest_point_sample: temp starts at 1e10, d = ((dx*dx + dy*dy) + dz*dz) with
                                    dx = x - x_centre, temp = fminf(d, temp), next centre = argmax temp; idx[0] = 0.
                                    Ties: the smallest (bitreverse_L(k mod bs), k), bs = 2^L = min(2^floor(log2 n),
                                    1024) -- what the reference's per-thread strict > scan and its left-biased tree
                                    pick (fps_reference_sim runs that scan and tree literally).
  ball_query_gpu_batch.cu:20-61     ball_query: the first nsample k in index order with ((new_x - x)^2 + (new_y - y)^2)
                                    + (new_z - z)^2 < radius * radius (fp32), unused slots = the first hit; a row
                                    with no hit is 0 (the reference leaves it undefined).
  group_points_gpu_batch.cu:25, 74  grouping / gather: out[b, c, p, s] = points[b, c, idx[b, p, s]]; indices outside
  gather_points_gpu.cu:25, 69       [0, N) read as 0 and add nothing to the gradient (a float64 sum here).
  box_utils_gpu.cu:28-78            points_in_boxes: the first box k with |z - cz| <= dz / 2.0 (double) and
                                    |local| < d / 2.0 + 1e-5f (double), local_x = sx * cosa + sy * (-sina),
                                    local_y = sx * sina + sy * cosa in fp32, cosa / sina = glibc cosf / sinf(-rz).
"""
import numpy as np

F32 = np.float32


def fps_bs_log2(n):
    """floor(log2 n) of opt_n_threads (sampling_gpu.cu:13-16), capped at 10 (1024 threads)."""
    return min(int(n).bit_length() - 1, 10)


def fps_order(n):
    """Tie order of point k: smaller wins among equal distances."""
    L = fps_bs_log2(n)
    k = np.arange(n, dtype=np.int64)
    t = k & ((1 << L) - 1)
    rank = np.zeros_like(t)
    for i in range(L):
        rank |= ((t >> i) & 1) << (L - 1 - i)
    return (rank << 22) | (k >> L)


def _dist(cx, cy, cz, x, y, z):
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = x - cx, y - cy, z - cz
        return ((dx * dx + dy * dy) + dz * dz).astype(F32)


def farthest_point_sample(xyz, m):
    """xyz [B, N, 3] float32 -> idx [B, m] int32."""
    xyz = np.asarray(xyz, F32)
    B, N, _ = xyz.shape
    m = int(m)
    out = np.zeros((B, max(m, 0)), np.int32)
    if m <= 0:
        return out
    order = fps_order(N)
    for b in range(B):
        x, y, z = xyz[b, :, 0], xyz[b, :, 1], xyz[b, :, 2]
        temp = np.full(N, 1e10, F32)
        old = 0
        for j in range(1, m):
            temp = np.fmin(_dist(x[old], y[old], z[old], x, y, z), temp)  # fminf: a NaN distance keeps temp
            best = temp.max()
            cand = np.flatnonzero(temp == best)
            old = int(cand[np.argmin(order[cand])])
            out[b, j] = old
    return out


def fps_reference_sim(xyz, m):
    """The reference kernel's selection run literally: bs threads, each a strict > scan over k = t, t + bs, ...
    (best = -1, besti = 0), then the tree __update(t, t + s) for s = bs/2 .. 1 keeping the left slot unless the right
    value is strictly greater."""
    xyz = np.asarray(xyz, F32)
    B, N, _ = xyz.shape
    bs = 1 << fps_bs_log2(N)
    out = np.zeros((B, max(int(m), 0)), np.int32)
    rows = -(-N // bs)
    for b in range(B):
        x, y, z = xyz[b, :, 0], xyz[b, :, 1], xyz[b, :, 2]
        temp = np.full(N, 1e10, F32)
        old = 0
        for j in range(1, int(m)):
            temp = np.fmin(_dist(x[old], y[old], z[old], x, y, z), temp)
            grid = np.full(rows * bs, -2.0, F32)  # padding below best = -1: never taken
            grid[:N] = temp
            grid = grid.reshape(rows, bs)
            r = np.argmax(grid, axis=0)  # first maximum of each thread's scan
            dists = np.maximum(grid[r, np.arange(bs)], F32(-1))
            idx = np.where(grid[r, np.arange(bs)] > F32(-1), r * bs + np.arange(bs), 0)
            s = bs // 2
            while s >= 1:
                v1, v2, i1, i2 = dists[:s].copy(), dists[s:2 * s], idx[:s].copy(), idx[s:2 * s]
                dists[:s] = np.maximum(v1, v2)
                idx[:s] = np.where(v2 > v1, i2, i1)
                s //= 2
            old = int(idx[0])
            out[b, j] = old
    return out


def ball_query(new_xyz, xyz, radius, nsample):
    """new_xyz [B, M, 3], xyz [B, N, 3] -> idx [B, M, nsample] int32."""
    new_xyz, xyz = np.asarray(new_xyz, F32), np.asarray(xyz, F32)
    B, M, _ = new_xyz.shape
    r2 = F32(radius) * F32(radius)
    out = np.zeros((B, M, nsample), np.int32)
    for b in range(B):
        q = new_xyz[b][:, None, :]
        p = xyz[b][None, :, :]
        d2 = _dist(p[..., 0], p[..., 1], p[..., 2], q[..., 0], q[..., 1], q[..., 2])  # (new - x) order
        hit = d2 < r2
        for i in range(M):
            k = np.flatnonzero(hit[i])[:nsample]
            if k.size:
                out[b, i, :] = k[0]
                out[b, i, :k.size] = k
    return out


def group(points, idx):
    """points [B, C, N], idx [B, ...] -> [B, C, ...]; indices outside [0, N) read as 0."""
    points = np.asarray(points, F32)
    idx = np.asarray(idx)
    B, C, N = points.shape
    ok = (idx >= 0) & (idx < N)
    safe = np.where(ok, idx, 0).reshape(B, -1)
    g = np.take_along_axis(points, np.broadcast_to(safe[:, None, :], (B, C, safe.shape[1])), axis=2)
    g = np.where(ok.reshape(B, 1, -1), g, F32(0))
    return g.reshape((B, C) + idx.shape[1:]).astype(F32)


def group_grad(grad_out, idx, n):
    """float64 sums of grad_out into [B, C, n]; indices outside [0, n) add nothing."""
    go = np.asarray(grad_out, np.float64)
    idx = np.asarray(idx)
    B, C = go.shape[:2]
    flat_i = idx.reshape(B, -1)
    flat_g = go.reshape(B, C, -1)
    out = np.zeros((B, C, n), np.float64)
    for b in range(B):
        ok = (flat_i[b] >= 0) & (flat_i[b] < n)
        for c in range(C):
            np.add.at(out[b, c], flat_i[b][ok], flat_g[b, c][ok])
    return out


def points_in_boxes(pts, boxes, libm):
    """pts [B, P, 3], boxes [B, M, >=7] -> [B, P] int32.  libm(op, x): glibc's float sinf (op 0) / cosf (op 1)."""
    pts = np.asarray(pts, F32)
    boxes = np.asarray(boxes, F32)[..., :7]
    B, P, _ = pts.shape
    out = np.full((B, P), -1, np.int32)
    margin = np.float64(F32(1e-5))
    for b in range(B):
        bx = boxes[b]
        if bx.shape[0] == 0:
            continue
        neg = (-bx[:, 6]).astype(F32)
        cosa = np.asarray(libm(1, neg), F32)[None, :]
        sina = np.asarray(libm(0, neg), F32)[None, :]
        x, y, z = (pts[b, :, i][:, None] for i in range(3))
        with np.errstate(invalid="ignore", over="ignore"):
            zin = ~(np.abs(z - bx[None, :, 2]).astype(np.float64) > bx[None, :, 5].astype(np.float64) / 2.0)
            sx, sy = (x - bx[None, :, 0]).astype(F32), (y - bx[None, :, 1]).astype(F32)
            lx = (sx * cosa + sy * (-sina)).astype(F32)
            ly = (sx * sina + sy * cosa).astype(F32)
            inx = np.abs(lx).astype(np.float64) < bx[None, :, 3].astype(np.float64) / 2.0 + margin
            iny = np.abs(ly).astype(np.float64) < bx[None, :, 4].astype(np.float64) / 2.0 + margin
        inside = zin & inx & iny
        anyin = inside.any(axis=1)
        out[b] = np.where(anyin, inside.argmax(axis=1), -1)
    return out
