"""NumPy restatement of csrc/smoke.hip (SMOKE's head and post-processing at inference), in the arithmetic order that
file's header states: the statistics accumulated in double in the kernel's order (1024 strided partial sums folded by
halves, two passes), fp32 with every operation rounded on its own elsewhere, the 1x1 convolutions as explicit fmaf chains
in ascending channel order from +0 with the bias added afterwards, glibc's expf / atanf (oracle.pyoracle.libm_eval),
the 3x3 inverses in double by the adjugate, keys on the bits of the float32 scores.

    stats_tables(feat, groups)                      [B, 2, G] (mean, rstd)
    class_heat(feat, tables, gamma, beta, w, b)     the clipped heat map [B, nc, H, W]
    regression_raw(feat, tables, gamma, beta, w, b) the ten regression rows before the activations [B, 10, H, W]
    activate(reg)                                   sigmoid - 0.5 on 3:6, L2 normalisation on 6:8
    peak_scores(heat) / select(heat, K)             the single exact top-K: (flat indices, scores) per frame
    select_two_stage(heat, K)                       the reference's two topk stages under the same tie rule
    post_process(heat, reg, cam, cfg)               rows [B, K, 14], counts: pd3_smoke_post_process
    head_forward(cls_feat, reg_feat, state, cam, cfg, tables=None)   pd3_smoke_head_forward
    golden_inputs(tag) / golden_state(tag) / golden_camera(tag)      the seeded inputs of python_smoke.npz

cam: dict(K [B, 3, 3], trans_mat [B, 3, 3] or down_ratios [1, 2], image_size [1, 2], depth_ref, dim_ref);
cfg: dict(max_detection, det_threshold, mode) with mode "forward" or "export".
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from pv_rcnn_numpy import fmaf  # noqa: E402

F32, F64 = np.float32, np.float64
ONE = np.uint32(0x3F800000)
PI = F32(3.14159)
STAT_THREADS = 1024


def _libm(op, x):
    from oracle import pyoracle as O

    x = np.ascontiguousarray(x, F32)
    return O.libm_eval(op, x.reshape(-1)).reshape(x.shape)


def expf(x):
    return _libm(2, x)


def atanf(x):
    return _libm(3, x)


def sigmoid(x):
    with np.errstate(all="ignore"):
        return (F32(1) / (F32(1) + expf(-np.asarray(x, F32)))).astype(F32)


# ---- a. tables ------------------------------------------------------------------------------------------------------
def _strided_sum(v):
    """The kernel's sum of a double vector: partial t adds v[t], v[t + 1024], .. in order; folded by halves."""
    pad = (-len(v)) % STAT_THREADS
    a = np.concatenate([v, np.zeros(pad, F64)]).reshape(-1, STAT_THREADS)
    p = np.zeros(STAT_THREADS, F64)
    for row in a:
        p = p + row
    s = STAT_THREADS // 2
    while s > 0:
        p[:s] = p[:s] + p[s:2 * s]
        s //= 2
    return p[0]


def stats_tables(feat, groups):
    feat = np.asarray(feat, F32)
    B, C = feat.shape[:2]
    out = np.zeros((B, 2, groups), F32)
    with np.errstate(all="ignore"):
        for b in range(B):
            for g, x in enumerate(feat[b].reshape(groups, -1).astype(F64)):
                m = _strided_sum(x) / F64(len(x))
                d = x - m
                v = _strided_sum(d * d) / F64(len(x))
                out[b, 0, g] = F32(m)
                out[b, 1, g] = F32(F64(1) / np.sqrt(v + F64(1e-5)))
    return out


def norm_relu(feat, tables, gamma, beta):
    """relu(((x - mean) * rstd) * gamma + beta), a NaN stays."""
    feat = np.asarray(feat, F32)
    C, G = feat.shape[1], tables.shape[2]
    g = np.arange(C) // (C // G)
    with np.errstate(all="ignore"):
        mean, rstd = tables[:, 0][:, g][:, :, None, None], tables[:, 1][:, g][:, :, None, None]
        v = ((feat - mean) * rstd) * np.asarray(gamma, F32)[None, :, None, None] + np.asarray(beta, F32)[None, :, None, None]
        return np.where((v > 0) | np.isnan(v), v, F32(0)).astype(F32)


def conv1x1_chain(feat, weight, bias):
    feat, bias = np.asarray(feat, F32), np.asarray(bias, F32)
    w = np.asarray(weight, F32).reshape(len(bias), -1)
    B, C, H, W = feat.shape
    acc = np.zeros((B, len(bias), H, W), F32)
    with np.errstate(all="ignore"):
        for c in range(C):
            acc = fmaf(feat[:, None, c], w[None, :, c, None, None], acc)
        return (acc + bias[None, :, None, None]).astype(F32)


def clip_hm(s):
    lo, hi = F32(1e-4), F32(1 - 1e-4)
    with np.errstate(invalid="ignore"):
        return np.where(s < lo, lo, np.where(s > hi, hi, s)).astype(F32)


def class_heat(feat, tables, gamma, beta, weight, bias):
    return clip_hm(sigmoid(conv1x1_chain(norm_relu(feat, tables, gamma, beta), weight, bias)))


def regression_raw(feat, tables, gamma, beta, weight, bias):
    return conv1x1_chain(norm_relu(feat, tables, gamma, beta), weight, bias)


def activate(reg):
    reg = np.array(reg, F32)
    with np.errstate(all="ignore"):
        reg[:, 3:6] = sigmoid(reg[:, 3:6]) - F32(0.5)
        a, b = reg[:, 6].copy(), reg[:, 7].copy()
        nrm = np.sqrt(a * a + b * b).astype(F32)
        d = np.where(nrm < F32(1e-12), F32(1e-12), nrm)
        reg[:, 6], reg[:, 7] = a / d, b / d
    return reg


# ---- c. selection -----------------------------------------------------------------------------------------------------
def peak_scores(heat):
    """[nc, H, W] -> the scores the selection sees: the heat unless an in-map neighbour is larger; a heat outside (0, 1] (a NaN
    included) is 0 and a NaN neighbour suppresses nothing."""
    h = np.asarray(heat, F32)
    nc, H, W = h.shape
    pad = np.full((nc, H + 2, W + 2), -np.inf, F32)
    pad[:, 1:-1, 1:-1] = h
    with np.errstate(invalid="ignore"):
        peak = (h > 0) & (h <= 1)  # a score outside (0, 1], a NaN included, is 0
        for dy in range(3):
            for dx in range(3):
                peak &= ~(pad[:, dy:dy + H, dx:dx + W] > h)
    return np.where(peak, h, F32(0)).astype(F32)


def score_key(s):
    return (ONE - np.ascontiguousarray(s, F32).view(np.uint32)).astype(np.uint32)


def select(heat, K):
    """The K smallest (key, flat index) pairs in that order: (indices [K], scores [K])."""
    s = peak_scores(heat).reshape(-1)
    order = np.lexsort((np.arange(len(s)), score_key(s)))[:K]
    return order, s[order]


def select_two_stage(heat, K):
    """layer_libs.py:65-116 with ties to the lower index in both topk calls: (flat indices, scores)."""
    nc, H, W = heat.shape
    s = peak_scores(heat).reshape(nc, -1)
    per = [np.lexsort((np.arange(H * W), score_key(s[c])))[:K] for c in range(nc)]  # topk per class
    sc = np.concatenate([s[c][per[c]] for c in range(nc)])
    top = np.lexsort((np.arange(len(sc)), score_key(sc)))[:K]                         # topk of the nc * K
    cls = top // K
    pix = np.concatenate(per)[top]
    return cls * (H * W) + pix, sc[top]


# ---- decode -----------------------------------------------------------------------------------------------------------
def inverse3(m):
    """Adjugate inverse in double, rounded to float32."""
    a, b, c, d, e, f, g, h, i = (F64(v) for v in np.asarray(m, F32).reshape(-1))
    with np.errstate(all="ignore"):
        c00, c01, c02 = e * i - f * h, c * h - b * i, b * f - c * e
        c10, c11, c12 = f * g - d * i, a * i - c * g, c * d - a * f
        c20, c21, c22 = d * h - e * g, b * g - a * h, a * e - b * d
        det = (a * c00 + b * c10) + c * c20
        return (np.array([c00, c01, c02, c10, c11, c12, c20, c21, c22], F64) / det).astype(F32).reshape(3, 3)


def mat3(m, p0, p1, p2):
    return [((m[r, 0] * p0 + m[r, 1] * p1) + m[r, 2] * p2).astype(F32) for r in range(3)]


def clip(v, hi):
    with np.errstate(invalid="ignore"):
        return np.where(v < 0, F32(0), np.where(v > hi, hi, v)).astype(F32)


def decode_frame(idx, scores, r, Kmat, trans, image_size, depth_ref, dim_ref, H, W, mode):
    """One frame's K rows [K, 14] from the selected flat indices, their scores and regression values r [K, 10]."""
    depth_ref, dim_ref = np.asarray(depth_ref, F32), np.asarray(dim_ref, F32).reshape(-1, 3)
    cls, p = idx // (H * W), idx % (H * W)
    ys, xs = (p // W).astype(F32), (p % W).astype(F32)
    r = np.asarray(r, F32)
    one = np.ones(len(idx), F32)
    with np.errstate(all="ignore"):
        depth = r[:, 0] * depth_ref[1] + depth_ref[0]
        px, py = r[:, 1] + xs, r[:, 2] + ys
        Ki = inverse3(Kmat)
        if mode == "forward":
            Ti = inverse3(trans)
            q = mat3(Ti, px, py, one)
        else:
            dr = np.asarray(trans, F32).reshape(-1)
            q = [dr[0] * px, dr[1] * py, one]
        q = [(v * depth).astype(F32) for v in q]
        lx, ly, lz = mat3(Ki, *q)
        dl = expf(r[:, 3]) * dim_ref[cls, 0]
        dh = expf(r[:, 4]) * dim_ref[cls, 1]
        dw = expf(r[:, 5]) * dim_ref[cls, 2]
        ly = ly + dh / F32(2)
        ray = atanf(lx / (lz + F32(1e-7)))
        alpha = atanf(r[:, 6] / (r[:, 7] + F32(1e-7)))
        alpha = alpha - np.where(r[:, 7] >= 0, PI / F32(2), -PI / F32(2)).astype(F32)
        roty = alpha + ray
        roty = np.where(roty > PI, roty - F32(2) * PI, np.where(roty < -PI, roty - (F32(-2) * PI), roty)).astype(F32)
        x0, y0 = xs - r[:, 8] / F32(2), ys - r[:, 9] / F32(2)
        x1, y1 = xs + r[:, 8] / F32(2), ys + r[:, 9] / F32(2)
        if mode == "forward":
            size = np.asarray(image_size, F32).reshape(-1)
            a, b = mat3(Ti, x0, y0, one), mat3(Ti, x1, y1, one)
            x0, y0, x1, y1 = clip(a[0], size[0]), clip(a[1], size[1]), clip(b[0], size[0]), clip(b[1], size[1])
        else:
            x0, y0, x1, y1 = dr[0] * x0, dr[1] * y0, dr[0] * x1, dr[1] * y1
        return np.stack([cls.astype(F32), alpha, x0, y0, x1, y1, dh, dw, dl, lx, ly, lz, roty, scores], 1).astype(F32)


def post_process(heat, reg, cam, cfg, _reg_at=None):
    """pd3_smoke_post_process: rows [B, K, 14] (zero past the count in forward mode), counts int32 [B]."""
    heat = np.asarray(heat, F32)
    B, nc, H, W = heat.shape
    K, mode = cfg["max_detection"], cfg["mode"]
    rows, counts = np.zeros((B, K, 14), F32), np.zeros(B, np.int32)
    for b in range(B):
        idx, sc = select(heat[b], K)
        p = idx % (H * W)
        r = np.asarray(reg[b], F32).reshape(10, -1)[:, p].T
        if _reg_at is not None:
            r = _reg_at(r)
        trans = cam["trans_mat"][b] if mode == "forward" else cam["down_ratios"]
        out = decode_frame(idx, sc, r, cam["K"][b], trans, cam.get("image_size"), cam["depth_ref"], cam["dim_ref"], H, W,
                           mode)
        with np.errstate(invalid="ignore"):
            keep = sc > F32(cfg["det_threshold"]) if mode == "forward" else np.ones(K, bool)
        rows[b][keep] = out[keep]
        counts[b] = keep.sum()
    return rows, counts


def head_forward(cls_feat, reg_feat, state, cam, cfg, groups, tables=None):
    """pd3_smoke_head_forward from the two 3x3 convolution outputs; state: the head's state dict (class_head.1 / .3,
    regression_head.1 / .3); tables = (class, regression) or None (GroupNorm: computed here)."""
    ct, rt = tables if tables is not None else (stats_tables(cls_feat, groups), stats_tables(reg_feat, groups))
    heat = class_heat(cls_feat, ct, state["class_head.1.weight"], state["class_head.1.bias"],
                      state["class_head.3.weight"], state["class_head.3.bias"])
    raw = regression_raw(reg_feat, rt, state["regression_head.1.weight"], state["regression_head.1.bias"],
                         state["regression_head.3.weight"], state["regression_head.3.bias"])
    return post_process(heat, raw, cam, cfg, _reg_at=activate), heat


def bn_tables(state, prefix, batch, eps=1e-5):
    m, v = np.asarray(state[prefix + "._mean"], F64), np.asarray(state[prefix + "._variance"], F64)
    t = np.stack([m, 1.0 / np.sqrt(v + eps)]).astype(F32)
    return np.ascontiguousarray(np.broadcast_to(t[None], (batch,) + t.shape))


# ---- the golden cases ------------------------------------------------------------------------------------------------
DIM_REF = [[3.88, 1.63, 1.53], [1.78, 1.70, 0.58], [0.88, 1.73, 0.67]]
CASES = {
    "gn32": dict(seed=2101, norm="gn", mode="forward", B=3, H=12, W=40, C=32, Cin=16, nc=3, K=10, thr=0.7),
    "gn48x": dict(seed=2202, norm="gn", mode="export", B=1, H=5, W=7, C=48, Cin=8, nc=3, K=6, thr=0.25),
    "bn256": dict(seed=2303, norm="bn", mode="forward", B=3, H=5, W=7, C=256, Cin=8, nc=2, K=8, thr=0.25, quiet_frame=2),
    "gn256": dict(seed=2404, norm="gn", mode="forward", B=1, H=12, W=40, C=256, Cin=64, nc=3, K=50, thr=0.8),
    "bn32x": dict(seed=2505, norm="bn", mode="export", B=3, H=12, W=40, C=32, Cin=16, nc=3, K=10, thr=0.7),
}
TAGS = tuple(CASES)


def groups_of(tag):
    c = CASES[tag]
    return c["C"] if c["norm"] == "bn" else (32 if c["C"] % 32 == 0 else 16)


def cfg_of(tag):
    c = CASES[tag]
    return dict(max_detection=c["K"], det_threshold=c["thr"], mode=c["mode"])


def golden_state(tag):
    """SMOKEPredictor's state dict under the reference's names, seeded."""
    c = CASES[tag]
    rng = np.random.default_rng(c["seed"])
    C, Cin, st = c["C"], c["Cin"], {}
    for head, rows in (("class_head", c["nc"]), ("regression_head", 10)):
        st[f"{head}.0.weight"] = (rng.standard_normal((C, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(F32)
        st[f"{head}.0.bias"] = (rng.standard_normal(C) * 0.1).astype(F32)
        st[f"{head}.1.weight"] = rng.uniform(0.5, 1.5, C).astype(F32)
        st[f"{head}.1.bias"] = (rng.standard_normal(C) * 0.1).astype(F32)
        if c["norm"] == "bn":
            st[f"{head}.1._mean"] = (rng.standard_normal(C) * 0.1).astype(F32)
            st[f"{head}.1._variance"] = rng.uniform(0.5, 1.5, C).astype(F32)
        scale = 2.0 if head == "class_head" else 0.5
        st[f"{head}.3.weight"] = (rng.standard_normal((rows, C, 1, 1)) * scale / np.sqrt(C)).astype(F32)
        st[f"{head}.3.bias"] = (rng.standard_normal(rows) * 0.1).astype(F32)
    st["class_head.3.bias"] = (st["class_head.3.bias"] - F32(2.19)).astype(F32)
    return st


def golden_inputs(tag):
    """features [B, Cin, H, W] float32; the `quiet_frame` is scaled down so that nothing of it passes the threshold."""
    c = CASES[tag]
    rng = np.random.default_rng(c["seed"] + 1)
    x = rng.standard_normal((c["B"], c["Cin"], c["H"], c["W"])).astype(F32)
    if "quiet_frame" in c:
        x[c["quiet_frame"]] *= F32(0.02)
    return x


def golden_camera(tag):
    """KITTI-like intrinsics and the affine of get_transfrom_matrix (image centre and width onto the map), different
    per frame."""
    c = CASES[tag]
    B, H, W = c["B"], c["H"], c["W"]
    Ks, Ts = np.zeros((B, 3, 3), F32), np.zeros((B, 3, 3), F32)
    for b in range(B):
        iw, ih = 1242.0 - 18.0 * b, 375.0 - 5.0 * b
        f = 721.5377 - 14.25 * b
        Ks[b] = [[f, 0, 609.5593 - 7.5 * b], [0, f, 172.854 + 3.25 * b], [0, 0, 1]]
        s = W / iw
        Ts[b] = [[s, 0, W / 2 - s * iw / 2], [0, s, H / 2 - s * ih / 2], [0, 0, 1]]
    return dict(K=Ks, trans_mat=Ts, down_ratios=np.array([[1242.0 / W, 375.0 / H]], F32),
                image_size=np.array([[1242.0, 375.0]], F32), depth_ref=np.array([28.01, 16.32], F32),
                dim_ref=np.array(DIM_REF[:c["nc"]], F32))
