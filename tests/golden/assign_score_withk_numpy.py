"""NumPy restatement of the reference's assign_score_withk and its gradient (assign_score_withk_cuda.cc:32-158, the
CPU kernels), vectorised in float32 in the kernels' operation order (csrc/assign_score_withk.hip states the same
contract).  kn = knn_idx[b, n, k]; an index outside [0, N) reads points as 0 and adds nothing to grad_points.

  forward       acc = +0; for k, for m: acc = acc + points[b, kn, m, o] * s; acc = acc - centers[b, n, m, o] * s
  grad_scores   acc = +0; for o: acc = acc + (points[b, kn, m, o] - centers[b, n, m, o]) * grad_out[b, o, n]
  grad_points   acc = +0; for every (n, k) with kn == j in ascending (n, k) order: acc = acc + s * grad_out[b, o, n]
                (done by rank within the segment of j: every rank step adds to distinct rows)
  grad_centers  acc = +0; for k: acc = acc - scores[b, n, k, m] * grad_out[b, o, n]

Every product and every sum is a float32 operation rounded on its own (NumPy does not contract a * b + c).
"""
import numpy as np

F32 = np.float32


def _valid(knn_idx, N):
    kn = np.asarray(knn_idx, np.int64)
    ok = (kn >= 0) & (kn < N)
    return np.where(ok, kn, 0), ok


def _gather(points, kn, ok, m):
    """points[b, kn[b, n, k], m, :] as [B, N, K, O], rows of out-of-range indices 0."""
    B = points.shape[0]
    rows = points[np.arange(B)[:, None, None], kn, m]
    return np.where(ok[..., None], rows, F32(0))


def forward(scores, points, centers, knn_idx):
    scores, points, centers = (np.asarray(a, F32) for a in (scores, points, centers))
    B, N, M, O = points.shape
    K = scores.shape[2]
    kn, ok = _valid(knn_idx, N)
    acc = np.zeros((B, N, O), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        rows = [_gather(points, kn, ok, m) for m in range(M)]  # [B, N, K, O] per m
        for k in range(K):
            for m in range(M):
                s = scores[:, :, k, m, None]
                acc = (acc + rows[m][:, :, k] * s).astype(F32)
                acc = (acc - centers[:, :, m] * s).astype(F32)
    return np.ascontiguousarray(acc.transpose(0, 2, 1))


def grad_scores(grad_out, scores, points, centers, knn_idx):
    points, centers = np.asarray(points, F32), np.asarray(centers, F32)
    g = np.asarray(grad_out, F32)
    B, N, M, O = points.shape
    K = np.asarray(scores).shape[2]
    kn, ok = _valid(knn_idx, N)
    acc = np.zeros((B, N, K, M), F32)
    bi = np.arange(B)[:, None, None]
    with np.errstate(invalid="ignore", over="ignore"):
        for o in range(O):
            p = np.where(ok[..., None], points[bi, kn, :, o], F32(0))  # [B, N, K, M]
            d = (p - centers[:, :, None, :, o]).astype(F32)
            acc = (acc + (d * g[:, o, :, None, None]).astype(F32)).astype(F32)
    return acc


def grad_points(grad_out, scores, knn_idx, M, O):
    scores, g = np.asarray(scores, F32), np.asarray(grad_out, F32)
    B, N, K, _ = scores.shape
    kn, ok = _valid(knn_idx, N)
    acc = np.zeros((B, N, M, O), F32)
    if K == 0:
        return acc
    gT = g.transpose(0, 2, 1)  # [B, N, O]
    b, n, k = (a.reshape(-1) for a in np.meshgrid(np.arange(B), np.arange(N), np.arange(K), indexing="ij"))
    j, v = kn.reshape(-1), ok.reshape(-1)
    b, n, k, j = b[v], n[v], k[v], j[v]
    # (b, j) segments in ascending (n, k): entries are already in (b, n, k) order, the sort is stable
    order = np.lexsort((np.arange(b.size), j, b))
    b, n, k, j = b[order], n[order], k[order], j[order]
    key = b * N + j
    start = np.r_[0, np.flatnonzero(key[1:] != key[:-1]) + 1] if key.size else np.zeros(0, np.int64)
    first = np.repeat(start, np.diff(np.r_[start, key.size]))
    rank = np.arange(key.size) - first
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(int(rank.max()) + 1 if rank.size else 0):
            e = rank == r
            term = (scores[b[e], n[e], k[e], :, None] * gT[b[e], n[e], None, :]).astype(F32)
            acc[b[e], j[e]] = (acc[b[e], j[e]] + term).astype(F32)
    return acc


def grad_centers(grad_out, scores, M, O):
    scores, g = np.asarray(scores, F32), np.asarray(grad_out, F32)
    B, N, K, _ = scores.shape
    gT = g.transpose(0, 2, 1)  # [B, N, O]
    acc = np.zeros((B, N, M, O), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            acc = (acc - (scores[:, :, k, :, None] * gT[:, :, None, :]).astype(F32)).astype(F32)
    return acc


def backward(grad_out, scores, points, centers, knn_idx):
    """(grad_scores, grad_points, grad_centers)."""
    M, O = np.asarray(points).shape[2:]
    return (grad_scores(grad_out, scores, points, centers, knn_idx), grad_points(grad_out, scores, knn_idx, M, O),
            grad_centers(grad_out, scores, M, O))


def forward_f64(scores, points, centers, knn_idx):
    """The op in float64 as an einsum over gathered rows: sum_{k, m} (p - c) * s."""
    s, p, c = (np.asarray(a, np.float64) for a in (scores, points, centers))
    N = p.shape[1]
    kn, ok = _valid(knn_idx, N)
    P = np.where(ok[..., None, None], p[np.arange(p.shape[0])[:, None, None], kn], 0.0)  # [B, N, K, M, O]
    return np.einsum("bnkmo,bnkm->bon", P - c[:, :, None], s)


def forward_magnitude(scores, points, centers, knn_idx):
    """sum_{k, m} |p * s| + |c * s| in float64, [B, O, N]: the scale of the forward's rounding error."""
    s, p, c = (np.abs(np.asarray(a, np.float64)) for a in (scores, points, centers))
    N = p.shape[1]
    kn, ok = _valid(knn_idx, N)
    P = np.where(ok[..., None, None], p[np.arange(p.shape[0])[:, None, None], kn], 0.0)
    return np.einsum("bnkmo,bnkm->bon", P + c[:, :, None], s)


def backward_f64(grad_out, scores, points, centers, knn_idx):
    s, p, c, g = (np.asarray(a, np.float64) for a in (scores, points, centers, grad_out))
    B, N, M, O = p.shape
    kn, ok = _valid(knn_idx, N)
    P = np.where(ok[..., None, None], p[np.arange(B)[:, None, None], kn], 0.0)
    gs = np.einsum("bnkmo,bon->bnkm", P - c[:, :, None], g)
    terms = np.einsum("bnkm,bon->bnkmo", s, g) * ok[..., None, None]
    gp = np.zeros_like(p)
    np.add.at(gp, (np.arange(B)[:, None, None], kn), terms)
    gc = -np.einsum("bnkm,bon->bnmo", s, g)
    return gs, gp, gc
