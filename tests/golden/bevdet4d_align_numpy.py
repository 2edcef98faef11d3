"""NumPy restatement of BEVDet4D's temporal BEV alignment as the device computes it (csrc/bev_shift.hip): the
reference's shift_feature (paddle3d/models/detection/bevdet/bevdet4d.py:90-159) for every adjacent frame plus the
channel concat of its callers (:205-216, :291-298).

    tf     per (frame, batch) entry from camera 0's poses, bda and feat2bev, composed in double with the operation
           order written out in `transform` (closed-form affine inverse), rounded to fp32 once
    grid   gx = (tf00*x + tf01*y) + tf02; nx = (gx / (W-1)) * 2 - 1           (fp32, x = w index, y = h index)
    sample ix = ((nx + 1) / 2) * (W-1); corners floor(ix), floor(ix) + 1; weights nw, ne, sw, se; acc = 0, then
           acc += v * w over the in-range corners in the order nw, ne, sw, se (fp32, zero padding)
    concat [current, shifted adj 1 .. F-1] along channels

The GPU tests require the device output and grid to equal this bit for bit; tests/test_bevdet4d_align_cpu.py pins
it to the reference's own output (python_bevdet4d_align.npz, made by make_bevdet4d_align_golden.py).  Also the
seeded pose / feature generators both use.
"""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
# BEVDet4D-R50's view transformer grid (configs/bevdet/bevdet4d_r50_depth_nuscenes.yml): x, y in [-51.2, 51.2) at 0.8
GRID_INTERVAL = np.array([0.8, 0.8], np.float32)
GRID_LOWER = np.array([-51.2, -51.2], np.float32)


def _affine(D, R, t):
    A = [[(D[i][0] * R[0][j] + D[i][1] * R[1][j]) + D[i][2] * R[2][j] for j in range(3)] for i in range(3)]
    a = [(D[i][0] * t[0] + D[i][1] * t[1]) + D[i][2] * t[2] for i in range(3)]
    return A, a


def transform(R0, t0, R1, t1, D, Da, interval=GRID_INTERVAL, lower=GRID_LOWER):
    """Rows 0 and 1 of tf = inv(feat2bev) @ (bda4 @ c0 @ inverse(bda4' @ c1))[[0,1,3]][:, [0,1,3]] @ feat2bev as
    fp32 [6], composed in double in the device's order."""
    m = lambda x: [[float(v) for v in row] for row in np.asarray(x, np.float32)]  # noqa: E731
    v = lambda x: [float(e) for e in np.asarray(x, np.float32)]  # noqa: E731
    R0, R1, D, Da, t0, t1 = m(R0), m(R1), m(D), m(Da), v(t0), v(t1)
    A0, a0 = _affine(D, R0, t0)
    A, a1 = _affine(Da, R1, t1)
    c00 = A[1][1] * A[2][2] - A[1][2] * A[2][1]
    c01 = A[1][2] * A[2][0] - A[1][0] * A[2][2]
    c02 = A[1][0] * A[2][1] - A[1][1] * A[2][0]
    det = (A[0][0] * c00 + A[0][1] * c01) + A[0][2] * c02
    B = [[c00 / det, (A[0][2] * A[2][1] - A[0][1] * A[2][2]) / det, (A[0][1] * A[1][2] - A[0][2] * A[1][1]) / det],
         [c01 / det, (A[0][0] * A[2][2] - A[0][2] * A[2][0]) / det, (A[0][2] * A[1][0] - A[0][0] * A[1][2]) / det],
         [c02 / det, (A[0][1] * A[2][0] - A[0][0] * A[2][1]) / det, (A[0][0] * A[1][1] - A[0][1] * A[1][0]) / det]]
    b = [-((B[i][0] * a1[0] + B[i][1] * a1[1]) + B[i][2] * a1[2]) for i in range(3)]
    T = [[(A0[i][0] * B[0][j] + A0[i][1] * B[1][j]) + A0[i][2] * B[2][j] for j in range(2)]
         + [((A0[i][0] * b[0] + A0[i][1] * b[1]) + A0[i][2] * b[2]) + a0[i]] for i in range(2)]
    sx, sy = float(interval[0]), float(interval[1])
    lx, ly = float(lower[0]), float(lower[1])
    s, l = (sx, sy), (lx, ly)
    tf = []
    for i in range(2):
        tf += [(T[i][0] * sx) / s[i], (T[i][1] * sy) / s[i], (((T[i][0] * lx + T[i][1] * ly) + T[i][2]) - l[i]) / s[i]]
    return np.array(tf, np.float64).astype(np.float32)


def grid(tf, H, W):
    """Normalised sampling grid [H, W, 2] (fp32) of one entry."""
    tf = np.asarray(tf, np.float32)
    x = np.broadcast_to(np.arange(W, dtype=F32)[None, :], (H, W))
    y = np.broadcast_to(np.arange(H, dtype=F32)[:, None], (H, W))
    gx = (tf[0] * x + tf[1] * y) + tf[2]
    gy = (tf[3] * x + tf[4] * y) + tf[5]
    nx = (gx / F32(W - 1)) * F32(2) - F32(1)
    ny = (gy / F32(H - 1)) * F32(2) - F32(1)
    return np.stack([nx, ny], -1).astype(F32)


def sample(src, g):
    """grid_sample(src [C, H, W], g [H, W, 2], bilinear, zeros, align_corners=True) in the device's order."""
    src = np.asarray(src, F32)
    C, H, W = src.shape
    nx, ny = g[..., 0], g[..., 1]
    with np.errstate(invalid="ignore", over="ignore"):
        ix = ((nx + F32(1)) / F32(2)) * F32(W - 1)
        iy = ((ny + F32(1)) / F32(2)) * F32(H - 1)
        inside = (ix >= F32(-1)) & (ix < F32(W)) & (iy >= F32(-1)) & (iy < F32(H))  # NaN: False
    ix = np.where(inside, ix, F32(0))
    iy = np.where(inside, iy, F32(0))
    ix0, iy0 = np.floor(ix), np.floor(iy)
    ix1, iy1 = ix0 + F32(1), iy0 + F32(1)
    x0, y0 = ix0.astype(np.int64), iy0.astype(np.int64)
    w = [(ix1 - ix) * (iy1 - iy), (ix - ix0) * (iy1 - iy), (ix1 - ix) * (iy - iy0), (ix - ix0) * (iy - iy0)]
    corners = [(x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)]
    acc = np.zeros((C, H, W), F32)
    for (cx, cy), wk in zip(corners, w):
        ok = inside & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
        v = src[:, np.clip(cy, 0, H - 1), np.clip(cx, 0, W - 1)]
        acc = np.where(ok[None], acc + v * wk[None], acc)
    return acc.astype(F32)


def align_concat(feats, rots_cur, trans_cur, rots_adj, trans_adj, bda, bda_adj=None, interval=GRID_INTERVAL,
                 lower=GRID_LOWER):
    """feats: list of F arrays [B, C, H, W] (current first).  rots_* / trans_* / bda / bda_adj: lists of F-1 arrays,
    one per adjacent frame: [B, N, 3, 3] / [B, N, 3] / [B, 3, 3] (bda_adj None: bda).  Returns
    (out [B, F*C, H, W], grids [(F-1)*B, H, W, 2])."""
    F = len(feats)
    B, C, H, W = feats[0].shape
    out = np.zeros((B, F * C, H, W), F32)
    grids = np.zeros(((F - 1) * B, H, W, 2), F32)
    out[:, :C] = feats[0]
    for f in range(1, F):
        for b in range(B):
            Da = bda[f - 1][b] if bda_adj is None else bda_adj[f - 1][b]
            tf = transform(rots_cur[f - 1][b, 0], trans_cur[f - 1][b, 0], rots_adj[f - 1][b, 0],
                           trans_adj[f - 1][b, 0], bda[f - 1][b], Da, interval, lower)
            g = grid(tf, H, W)
            grids[(f - 1) * B + b] = g
            out[b, f * C:(f + 1) * C] = sample(feats[f][b], g)
    return out, grids


# ---- seeded inputs ----------------------------------------------------------------------------------------------

def rot_z(yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


# camera 0 (front) to ego: camera z forward = ego x, camera x right = ego -y, camera y down = ego -z
_CAM0 = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])


def poses(rng, B, num_adj, ncam=6, yaw_max_deg=10.0, trans_max=5.0, far=None):
    """Camera poses of the BEVDet4D input: rots [num_adj + 1] x [B, ncam, 3, 3], trans [num_adj + 1] x [B, ncam, 3]
    (frame 0 the current one).  Adjacent frame k's cameras are the current rig moved by a random ego motion (yaw up
    to yaw_max_deg, translation up to trans_max m; `far` adds that many metres in x).  Cameras 1.. are random rigid
    poses: only camera 0 enters the alignment."""
    rig_r = np.empty((B, ncam, 3, 3))
    rig_t = np.empty((B, ncam, 3))
    for b in range(B):
        for c in range(ncam):
            rig_r[b, c] = rot_z(rng.uniform(-0.05, 0.05) + 2 * math.pi * c / ncam) @ _CAM0
            rig_t[b, c] = rng.uniform(-1.0, 1.0, 3) + np.array([1.0, 0.0, 1.6])
    rots, trans = [rig_r.astype(F32)], [rig_t.astype(F32)]
    for _ in range(num_adj):
        r = np.empty_like(rig_r)
        t = np.empty_like(rig_t)
        for b in range(B):
            m = rot_z(math.radians(rng.uniform(-yaw_max_deg, yaw_max_deg)))
            d = np.array([rng.uniform(-trans_max, trans_max), rng.uniform(-trans_max, trans_max) * 0.3,
                          rng.uniform(-0.05, 0.05)])
            if far is not None:
                d[0] += far
            r[b] = m @ rig_r[b]
            t[b] = (m @ rig_t[b].T).T + d
        rots.append(r.astype(F32))
        trans.append(t.astype(F32))
    return rots, trans


def bda_matrix(rot_deg=0.0, flip_x=False, flip_y=False, scale=1.0):
    """BEV data augmentation matrix as the reference's bev_transform builds it: flips @ scale * rot_z."""
    m = scale * rot_z(math.radians(rot_deg))
    f = np.diag([-1.0 if flip_x else 1.0, -1.0 if flip_y else 1.0, 1.0])
    return (f @ m).astype(F32)


def features(rng, shape):
    return rng.uniform(-1.0, 1.0, shape).astype(F32)


# ---- the golden cases (tests/golden/make_bevdet4d_align_golden.py) ----------------------------------------------
# one shift_feature call each: (name, seed, yaw_max_deg, trans_max, far, bda, bda_adj); C = 4, H = W = 128, n = 1
GOLDEN_C, GOLDEN_H, GOLDEN_W, GOLDEN_N = 4, 128, 128, 1
GOLDEN_CASES = [
    ("small", 11, 2.0, 1.0, None, dict(), None),
    ("yaw10_5m", 12, 10.0, 5.0, None, dict(), None),
    ("bda_flip_rot", 13, 6.0, 3.0, None, dict(rot_deg=17.0, flip_x=True, scale=1.05), None),
    ("bda_adj", 14, 6.0, 3.0, None, dict(rot_deg=-9.0, flip_y=True), dict(rot_deg=4.0, scale=0.95)),
    ("partly_out", 15, 5.0, 2.0, 40.0, dict(), None),
]


# the golden file keeps a fixed sample of each case's output pixels (the reference runs at the full 128 x 128)
GOLDEN_PIXELS = 1024


def golden_pixels(i):
    """Flat H*W indices (sorted, int64) of the pixels golden case i records."""
    rng = np.random.default_rng(1000 + i)
    return np.sort(rng.choice(GOLDEN_H * GOLDEN_W, GOLDEN_PIXELS, replace=False))


def at_pixels(out, grid, pix):
    """(out [n, C, H, W], grid [n, H, W, 2]) -> (out [n, C, P], grid [n, P, 2]) at the flat pixel indices `pix`."""
    out, grid = np.asarray(out), np.asarray(grid)
    n, c = out.shape[:2]
    return out.reshape(n, c, -1)[:, :, pix], grid.reshape(n, -1, 2)[:, pix]


def golden_case(i):
    """Inputs of golden case i: dict(input [n, C, H, W], trans [cur, adj], rots [cur, adj], bda, bda_adj or None)."""
    name, seed, yaw, tmax, far, bda_kw, adj_kw = GOLDEN_CASES[i]
    rng = np.random.default_rng(seed)
    rots, trans = poses(rng, GOLDEN_N, 1, yaw_max_deg=yaw, trans_max=tmax, far=far)
    n = GOLDEN_N
    bda = np.broadcast_to(bda_matrix(**bda_kw), (n, 3, 3)).copy()
    bda_adj = None if adj_kw is None else np.broadcast_to(bda_matrix(**adj_kw), (n, 3, 3)).copy()
    x = features(rng, (n, GOLDEN_C, GOLDEN_H, GOLDEN_W))
    return dict(name=name, input=x, trans=trans, rots=rots, bda=bda, bda_adj=bda_adj)


def shift_feature(x, trans, rots, bda, bda_adj=None, interval=GRID_INTERVAL, lower=GRID_LOWER):
    """shift_feature of one adjacent frame: (output [n, C, H, W], grid [n, H, W, 2])."""
    n, C, H, W = x.shape
    out = np.zeros((n, C, H, W), F32)
    grids = np.zeros((n, H, W, 2), F32)
    for b in range(n):
        tf = transform(rots[0][b, 0], trans[0][b, 0], rots[1][b, 0], trans[1][b, 0], bda[b],
                       bda[b] if bda_adj is None else bda_adj[b], interval, lower)
        grids[b] = grid(tf, H, W)
        out[b] = sample(x[b], grids[b])
    return out, grids
