"""NumPy restatement of csrc/lanedet.hip (BEV-LaneDet's lane head tail and lane post-processing): the arithmetic order
stated in that file's header, operation for operation, so that the device can be held to it bit for bit.

    final_conv(feat, weight, bias)          a final 3x3 convolution densely [B, rows, H, W] (the fmaf chain)
    head_maps(feats, state)                 seg (logit), emb, sigmoid(offset), z from the four branch maps
    post_process(seg, emb, off, z, cfg)     the outputs of pd3_lanedet_post_process as a dict of arrays
    head_forward(feats, state, cfg)         the outputs of pd3_lanedet_head_forward (the same tail from head_maps)
    lanes_of(out, b)                        per frame the list of [40, 3] lanes, finishing fit_ok == 0 with np.polyfit
    synthetic_lanes(rng, B, H, W, nd, ...)  seeded maps with a few lanes two pixels wide

cfg: dict(conf, emb_margin, min_cluster_size, max_x, meter_per_pixel (x, y)).  A frame whose flag is set has all-zero
outputs but `flags` and `num_selected`.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from pv_rcnn_numpy import fmaf  # noqa: E402

F32, F64 = np.float32, np.float64
MAX_CENTRES, MAX_LANES, FIT_SAMPLES = 128, 32, 40
CFG = dict(conf=0.9, emb_margin=6.0, min_cluster_size=15, max_x=103.0, meter_per_pixel=(0.5, 0.5))
BRANCHES = ("ms_new", "me_new", "m_offset_new", "m_z")  # seg, emb, offset, z


def expf(x):
    from oracle import pyoracle as O

    x = np.ascontiguousarray(x, F32)
    return O.libm_eval(2, x.reshape(-1)).reshape(x.shape)


def sigmoid(x):
    with np.errstate(all="ignore"):
        return (F32(1) / (F32(1) + expf(-np.asarray(x, F32)))).astype(F32)


def final_conv(feat, weight, bias):
    """acc = +0; c ascending, ky, kx: acc = fmaf(v, w, acc) with v = +0 outside the map; acc + bias."""
    feat, weight, bias = np.asarray(feat, F32), np.asarray(weight, F32), np.asarray(bias, F32)
    B, C, H, W = feat.shape
    rows = weight.shape[0]
    pad = np.zeros((B, C, H + 2, W + 2), F32)
    pad[:, :, 1:-1, 1:-1] = feat
    acc = np.zeros((B, rows, H, W), F32)
    for c in range(C):
        for ky in range(3):
            for kx in range(3):
                acc = fmaf(pad[:, c, None, ky:ky + H, kx:kx + W], weight[None, :, c, ky, kx, None, None], acc)
    with np.errstate(all="ignore"):
        return (acc + bias[None, :, None, None]).astype(F32)


def head_maps(feats, state):
    """feats: the four branch maps (seg, emb, offset, z) [B, C, H, W]; state: {"<branch>.weight" / ".bias"} of the
    final convolutions -> seg, emb, sigmoid(offset), z."""
    maps = [final_conv(f, state[k + ".weight"], state[k + ".bias"]) for f, k in zip(feats, BRANCHES)]
    return maps[0], maps[1], sigmoid(maps[2]), maps[3]


def cluster(embs, gap):
    """The online clustering of one frame: embs [n, nd] float32 in selection order -> (centre id per pixel, counts) or
    None when a 129th centre would be founded."""
    n, nd = embs.shape
    gap = F32(gap)
    with np.errstate(all="ignore"):
        opened = F32(gap + F32(1))
    cen = np.zeros((MAX_CENTRES, nd), F32)
    num = np.zeros(MAX_CENTRES, np.int64)
    nc = 0
    ids = np.zeros(n, np.int32)
    for i in range(n):
        e = embs[i]
        bi, bd = -1, opened
        if nc:
            with np.errstate(all="ignore"):
                d = e[None] - cen[:nc]
                if nd == 1:
                    dist = np.abs(d[:, 0])
                else:
                    s = d[:, 0] * d[:, 0]
                    for k in range(1, nd):
                        s = s + d[:, k] * d[:, k]
                    dist = np.sqrt(s)
                m = dist < opened
            if m.any():
                dm = np.where(m, dist, F32(np.inf))
                bi = int(np.argmin(dm))  # the first of equal minima: the lowest id
                bd = dm[bi]
        if bi >= 0 and bd < gap:
            with np.errstate(all="ignore"):
                cen[bi] = (cen[bi] * F32(num[bi]) + e) / F32(num[bi] + 1)
            num[bi] += 1
            ids[i] = bi
        else:
            if nc == MAX_CENTRES:
                return None
            cen[nc], num[nc], ids[i] = e, 1, nc
            nc += 1
    return ids, num[:nc]


def _fit(Y, X, Z):
    """The cubic fits of X and Z over Y (Python floats are doubles; every operation rounds on its own) -> [40, 3]
    float32 or None."""
    Ymin, Ymax = Y[0], Y[-1]
    mid, half = (Ymin + Ymax) / 2.0, (Ymax - Ymin) / 2.0
    if not half > 0.0:
        return None
    S, bx, bz = [0.0] * 7, [0.0] * 4, [0.0] * 4
    for y, x, z in zip(Y, X, Z):
        t = (y - mid) / half
        p = [1.0, t]
        for i in range(2, 7):
            p.append(p[i - 1] * t)
        for i in range(7):
            S[i] += p[i]
        bx[0] += x
        bz[0] += z
        for i in range(1, 4):
            bx[i] += p[i] * x
            bz[i] += p[i] * z
    L = [[0.0] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(i + 1):
            s = S[i + j]
            for q in range(j):
                s -= L[i][q] * L[j][q]
            if i == j:
                if not s > 0.0:
                    return None
                L[i][i] = math.sqrt(s)
            else:
                L[i][j] = s / L[j][j]
    coef = []
    for r in (bx, bz):
        u, c = [0.0] * 4, [0.0] * 4
        for i in range(4):
            s = r[i]
            for q in range(i):
                s -= L[i][q] * u[q]
            u[i] = s / L[i][i]
        for i in range(3, -1, -1):
            s = u[i]
            for q in range(3, i, -1):
                s -= L[q][i] * c[q]
            c[i] = s / L[i][i]
        coef.append(c)
    cx, cz = coef
    step = (Ymax - Ymin) / 39.0
    out = np.zeros((FIT_SAMPLES, 3), F32)
    for k in range(FIT_SAMPLES):
        y = Ymax if k == FIT_SAMPLES - 1 else Ymin + float(k) * step
        t = (y - mid) / half
        with np.errstate(all="ignore"):
            out[k] = (F32(((cx[3] * t + cx[2]) * t + cx[1]) * t + cx[0]), F32(y),
                      F32(((cz[3] * t + cz[2]) * t + cz[1]) * t + cz[0]))
    return out


def post_process(seg, emb, off, z, cfg=CFG):
    """seg [B, 1, H, W] logits, emb [B, nd, H, W], off [B, 1, H, W] (sigmoid applied), z [B, 1, H, W]."""
    seg, emb, off, z = (np.asarray(a, F32) for a in (seg, emb, off, z))
    B, nd, H, W = emb.shape
    mx, my = (float(v) for v in cfg["meter_per_pixel"])
    max_x, conf = float(cfg["max_x"]), F32(cfg["conf"])
    out = dict(labels=np.zeros((B, H, W), np.uint8), num_lanes=np.zeros(B, np.int32),
               lane_id=np.zeros((B, MAX_LANES), np.int32), lane_rows=np.zeros((B, MAX_LANES), np.int32),
               fit_ok=np.zeros((B, MAX_LANES), np.int32), points=np.zeros((B, MAX_LANES, H, 3), F32),
               fit=np.zeros((B, MAX_LANES, FIT_SAMPLES, 3), F32), flags=np.zeros(B, np.int32),
               num_selected=np.zeros(B, np.int32))
    for b in range(B):
        with np.errstate(invalid="ignore"):
            ys, xs = np.nonzero(seg[b, 0] >= conf)  # row-major
        out["num_selected"][b] = len(ys)
        res = cluster(np.ascontiguousarray(emb[b][:, ys, xs].T), cfg["emb_margin"])
        if res is None:
            out["flags"][b] = 1
            continue
        ids, num = res
        kept = [c for c in range(len(num)) if num[c] >= int(cfg["min_cluster_size"])]
        if len(kept) > MAX_LANES:
            out["flags"][b] = 2
            continue
        lab = out["labels"][b]
        keep = np.isin(ids, kept)
        lab[ys[keep], xs[keep]] = ids[keep] + 1
        lane = 0
        for c in kept:
            rows = []
            for y in range(H - 1, -1, -1):  # the reference's reversal
                cols = np.nonzero(lab[y] == c + 1)[0]
                if not cols.size:
                    continue
                sc = sz = 0.0
                for x in cols:
                    sc += float(x) + float(off[b, 0, y, x])
                    sz += float(z[b, 0, y, x])
                with np.errstate(all="ignore"):
                    col, zr = sc / float(cols.size), F32(sz / float(cols.size))
                    xm = (max_x / mx - (float(y) + 0.5)) * mx
                    ym = (col * my - (W / 2.0) * my) * -1.0
                rows.append((xm, ym, zr))
            if len(rows) < 2:
                continue
            out["lane_id"][b, lane], out["lane_rows"][b, lane] = c + 1, len(rows)
            with np.errstate(all="ignore"):
                out["points"][b, lane, :len(rows)] = np.array([(F32(xm), F32(ym), zr) for xm, ym, zr in rows], F32)
            if len(rows) >= 4:
                with np.errstate(all="ignore"):
                    f = _fit([r[0] for r in rows], [-r[1] for r in rows], [float(r[2]) for r in rows])
                if f is not None:
                    out["fit"][b, lane], out["fit_ok"][b, lane] = f, 1
            lane += 1
        out["num_lanes"][b] = lane
    return out


def head_forward(feats, state, cfg=CFG):
    return post_process(*head_maps(feats, state), cfg)


def lanes_of(out, b):
    """The frame's lanes as the reference's __getitem__ makes them: [40, 3] each; lanes the device did not fit
    (fit_ok == 0: 2 or 3 rows) are finished with np.polyfit from `points`, as BEVLaneDet.test_forward does."""
    import warnings

    lanes = []
    for l in range(int(out["num_lanes"][b])):
        if out["fit_ok"][b, l]:
            lanes.append(np.array(out["fit"][b, l], F64))
            continue
        p = np.asarray(out["points"][b, l, :int(out["lane_rows"][b, l])], F64)
        pred = np.array([-1 * p[:, 1], p[:, 0], p[:, 2]])
        y = np.linspace(min(pred[1]), max(pred[1]), FIT_SAMPLES)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fx, fz = np.polyfit(pred[1], pred[0], 3), np.polyfit(pred[1], pred[2], 3)
        lanes.append(np.array([np.poly1d(fx)(y), y, np.poly1d(fz)(y)]).T)
    return lanes


def synthetic_lanes(rng, B, H, W, nd, lanes=4, width=2, spread=10.0, noise=0.3):
    """Seeded maps [B, 1 | nd | 1 | 1, H, W]: `lanes` slanted lanes `width` pixels wide with embeddings `spread` apart
    (far above the margin of 6), seg logits well away from the threshold, offsets in (0, 1), smooth heights."""
    seg = np.full((B, 1, H, W), -4.0, F32) + (rng.standard_normal((B, 1, H, W)) * 0.5).astype(F32)
    emb = (rng.standard_normal((B, nd, H, W)) * noise).astype(F32)
    off = rng.uniform(0.05, 0.95, (B, 1, H, W)).astype(F32)
    z = (rng.standard_normal((B, 1, H, W)) * 0.05).astype(F32)
    for b in range(B):
        for l in range(lanes):
            x0 = (l + 0.5) * W / lanes + rng.uniform(-0.5, 0.5)
            slope = rng.uniform(-0.3, 0.3) * W / max(H, 1) / lanes
            code = np.array([(l + 1) * spread * (1 if k % 2 == 0 else -1) * (k + 1) for k in range(nd)], F32)
            for y in range(H):
                xc = int(round(x0 + slope * y))
                for x in range(xc, xc + width):
                    if 0 <= x < W:
                        seg[b, 0, y, x] = F32(4.0 + rng.uniform(0, 1))
                        emb[b, :, y, x] = code + (rng.standard_normal(nd) * noise).astype(F32)
                        z[b, 0, y, x] += F32(0.01 * y + 0.1 * l)
    return seg, emb, off, z


# ---- seeded and border inputs the CPU and GPU tests share ----------------------------------------------------------
SWEEP = ((1, 1, 1), (5, 7, 2), (4, 33, 3), (13, 7, 2), (200, 48, 2))  # (H, W, B)


def sweep_cfg(H, W):
    """The reference's constants at the full size; a cluster size that small maps can reach elsewhere."""
    return dict(CFG) if H * W >= 2000 else dict(CFG, min_cluster_size=max(1, min(15, H // 2)), max_x=float(H) * 0.5 + 3.0)


def blank(B, H, W, nd):
    """Nothing selected: seg -5, emb 0, offset LOGIT 0 (sigmoid exactly 0.5), z 0."""
    return (np.full((B, 1, H, W), -5.0, F32), np.zeros((B, nd, H, W), F32), np.zeros((B, 1, H, W), F32),
            np.zeros((B, 1, H, W), F32))


def _put(maps, b, y, x, code, zval=0.0):
    seg, emb, _, z = maps
    seg[b, 0, y, x] = 5.0
    emb[b, :, y, x] = code
    z[b, 0, y, x] = zval


def border_cases():
    """name -> (seg, emb, offset LOGIT, z, cfg): integer-valued embeddings, offsets of exactly 0.5 and heights in
    eighths, so that every sum is exact and the expected decision is beyond doubt (see tests/test_lanedet_gpu.py)."""
    cases = {}
    cfg = dict(CFG, min_cluster_size=2, max_x=10.0)
    # a frame with lanes beside a frame with no selected pixel
    m = blank(2, 6, 5, 2)
    for y in range(6):
        for x in (1, 2):
            _put(m, 0, y, x, (0.0, 3.0), y / 8.0)
        _put(m, 0, y, 4, (20.0, -7.0), 1.0)
    cases["empty_frame"] = (*m, cfg)
    m = blank(1, 3, 4, 2)
    _put(m, 0, 1, 2, (1.0, 1.0))
    cases["one_pixel"] = (*m, dict(cfg, min_cluster_size=1))
    m = blank(1, 6, 5, 2)
    for y in range(6):
        for x in range(5):
            _put(m, 0, y, x, (0.0, 0.0) if x < 2 else (20.0, 1.0), (x + y) / 8.0)
    cases["all_selected"] = (*m, cfg)
    for k in (MAX_CENTRES - 1, MAX_CENTRES, MAX_CENTRES + 1):  # k centres, three of them with two pixels
        m = blank(2, 14, 10, 1)
        for i in range(k):
            _put(m, 0, i // 10, i % 10, 10.0 * i)
        for j in range(3):
            _put(m, 0, 13, j, 10.0 * j)
        _put(m, 1, 0, 0, 1.0)
        _put(m, 1, 1, 0, 2.0)
        cases[f"centres_{k}"] = (*m, cfg)
    for k in (MAX_LANES, MAX_LANES + 1):  # k clusters of two pixels in two rows
        m = blank(1, 2, MAX_LANES + 1, 1)
        for i in range(k):
            _put(m, 0, 0, i, 10.0 * i)
            _put(m, 0, 1, i, 10.0 * i, 0.25)
        cases[f"lanes_{k}"] = (*m, cfg)
    m = blank(1, 15, 4, 2)  # 14 pixels (dropped) beside 15 (kept)
    for y in range(14):
        _put(m, 0, y, 0, (0.0, 0.0))
    for y in range(15):
        _put(m, 0, y, 2, (0.0, 30.0))
    cases["min_cluster_size"] = (*m, dict(cfg, min_cluster_size=15))
    for nd in (1, 2):  # centres 0 and 10, then 5: both at distance 5 < 6, the lower id wins; then rows to make lanes
        m = blank(1, 4, 3, nd)
        pad = (0.0,) * (nd - 1)
        _put(m, 0, 0, 0, (0.0, *pad))
        _put(m, 0, 0, 1, (10.0, *pad))
        _put(m, 0, 0, 2, (5.0, *pad))
        _put(m, 0, 1, 0, (1.0, *pad))
        _put(m, 0, 1, 1, (10.0, *pad))
        cases[f"tie_nd{nd}"] = (*m, cfg)
        m = blank(1, 3, 3, nd)  # a distance exactly equal to the gap founds a centre
        _put(m, 0, 0, 0, (0.0, *pad))
        _put(m, 0, 0, 1, (6.0, *pad))
        _put(m, 0, 1, 0, (0.0, *pad))
        _put(m, 0, 1, 1, (6.0, *pad))
        cases[f"gap_nd{nd}"] = (*m, cfg)
    m = blank(1, 5, 9, 2)  # lanes of 1 (dropped), 2, 3 (fit_ok 0) and 4 rows (fit_ok 1)
    for k in range(4):
        for y in range(k + 1):
            for x in (2 * k, 2 * k + 1):
                _put(m, 0, y, x, (10.0 * k, 0.0), (y * y) / 8.0)
    cases["rows_1_to_4"] = (*m, cfg)
    m = blank(1, 6, 6, 2)  # NaN and Inf: in seg (a NaN is not selected, +Inf is), in emb (founds centres)
    for y in range(6):
        for x in (0, 1):
            _put(m, 0, y, x, (0.0, 0.0))
    m[0][0, 0, 0, 3] = np.nan
    m[0][0, 0, 1, 3] = np.inf
    m[0][0, 0, 2, 3] = -np.inf
    _put(m, 0, 3, 4, (np.nan, 0.0))
    _put(m, 0, 3, 5, (np.inf, 0.0))
    _put(m, 0, 4, 4, (np.inf, 1.0))
    _put(m, 0, 4, 5, (-np.inf, np.nan))
    m[3][0, 0, 5, 0] = np.nan
    cases["nan_inf"] = (*m, cfg)
    m = blank(1, 4, 5, 2)  # a selected pixel in each map corner
    for y, x in ((0, 0), (0, 4), (3, 0), (3, 4)):
        _put(m, 0, y, x, (0.0, 0.0), 0.5)
    cases["corners"] = (*m, dict(cfg, min_cluster_size=4))
    return cases


def identity_head(seg, emb, off_logit, z, C=4):
    """Branch maps and final weights whose convolutions reproduce the four maps exactly (a centre tap of 1 on the
    channel that holds the map, +0 elsewhere; finite maps only): the border cases through the lazy form."""
    B, nd, H, W = emb.shape
    feats = [np.zeros((B, C, H, W), F32) for _ in range(4)]
    feats[0][:, 0], feats[1][:, :nd], feats[2][:, 0], feats[3][:, 0] = seg[:, 0], emb, off_logit[:, 0], z[:, 0]
    state = {}
    for k, rows in zip(BRANCHES, (1, nd, 1, 1)):
        w = np.zeros((rows, C, 3, 3), F32)
        for r in range(rows):
            w[r, r, 1, 1] = 1.0
        state[k + ".weight"], state[k + ".bias"] = w, np.zeros(rows, F32)
    return feats, state


def random_head(rng, B, C, H, W, nd, bands=3, select=0.3):
    """Seeded branch maps (post-ReLU: non-negative) and full 3x3 weights.  Channel 0 of the emb branch holds a column
    band number and its centre taps weigh 12, so that the embeddings fall into `bands` clusters; returns (feats,
    state, conf) with conf halfway between two seg logits so that about `select` of the pixels pass."""
    feats = [np.maximum(rng.standard_normal((B, C, H, W)), 0).astype(F32) for _ in range(4)]
    feats[1][:, 0] = (np.arange(W) * bands // max(W, 1)).astype(F32)[None, None, :]
    state = {}
    for k, rows in zip(BRANCHES, (1, nd, 1, 1)):
        state[k + ".weight"] = (rng.standard_normal((rows, C, 3, 3)) * (0.5 / np.sqrt(9 * C))).astype(F32)
        state[k + ".bias"] = (rng.standard_normal(rows) * 0.1).astype(F32)
    for r in range(nd):
        state["me_new.weight"][r, 0] = 0
        state["me_new.weight"][r, 0, 1, 1] = 12.0 * (1 if r % 2 == 0 else -1)
    seg = np.sort(final_conv(feats[0], state["ms_new.weight"], state["ms_new.bias"]).reshape(-1).astype(F64))
    i = min(max(int(len(seg) * (1 - select)), 1), len(seg) - 1)
    conf = float(F32((seg[i - 1] + seg[i]) / 2)) if len(seg) > 1 else float(seg[0]) - 1.0
    return feats, state, conf
