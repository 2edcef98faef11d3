"""NumPy restatement of csrc/anchor3d_head.hip (BEVFusion's Anchor3DHead at inference), in the arithmetic order that
file's header states: fp32 with every operation rounded on its own, the 1x1 convolutions as explicit fmaf chains in
ascending channel order from +0 with the bias added afterwards, glibc's expf (oracle.pyoracle.libm_eval) inside the
sigmoid and the size decode, the oracle's rotated NMS, keys on the bits of the float32 scores.

    head_maps(feat, state)                     the three maps, every element by the kernels' chain
    get_bboxes(cls, reg, dir, anchors, cfg)    stages (a') .. (f) -> boxes [B, max_num, cs], scores, labels, counts
    head_forward(feat, state, anchors, cfg)    the lazy entry point = get_bboxes(head_maps(...)): the lazy kernels
                                               evaluate the same chains, only at fewer places
    golden_inputs(tag) / golden_state(tag)     the seeded inputs of tests/golden/python_anchor3d.npz

cfg: dict(nms_pre, max_num, score_thr, nms_thr, dir_offset, dir_limit_offset, num_classes).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from pv_rcnn_numpy import fmaf  # noqa: E402

F32 = np.float32
ONE = np.uint32(0x3F800000)
PI = F32(np.pi)


def expf(x):
    from oracle import pyoracle as O

    x = np.ascontiguousarray(x, F32)
    return O.libm_eval(2, x.reshape(-1)).reshape(x.shape)


def sigmoid(x):
    with np.errstate(all="ignore"):
        return (F32(1) / (F32(1) + expf(-np.asarray(x, F32)))).astype(F32)


def conv1x1_chain(feat, weight, bias):
    """feat [B, C, H, W], weight [rows, C(, 1, 1)], bias [rows] -> [B, rows, H, W]: per element
    fmaf(f[C-1], w[C-1], ... fmaf(f[0], w[0], +0)) + bias."""
    feat, bias = np.asarray(feat, F32), np.asarray(bias, F32)
    w = np.asarray(weight, F32).reshape(len(bias), -1)
    B, C, H, W = feat.shape
    acc = np.zeros((B, len(bias), H, W), F32)
    with np.errstate(all="ignore"):
        for c in range(C):
            acc = fmaf(feat[:, None, c], w[None, :, c, None, None], acc)
        return (acc + bias[None, :, None, None]).astype(F32)


def head_maps(feat, state):
    return tuple(conv1x1_chain(feat, state[k + ".weight"], state[k + ".bias"]) for k in ("conv_cls", "conv_reg", "conv_dir_cls"))


def score_key(s):
    """bits(1.0f) - bits(score); a NaN sorts after every number."""
    s = np.ascontiguousarray(s, F32)
    return np.where(s == s, ONE - s.view(np.uint32), ONE + np.uint32(1)).astype(np.uint32)


def max_scores(scores):
    """[N, nc] -> [N]: m = s_0, then m = s_c where s_c > m."""
    m = scores[:, 0].copy()
    for c in range(1, scores.shape[1]):
        m = np.where(scores[:, c] > m, scores[:, c], m)
    return m


def select(max_score, nms_pre):
    """The K smallest (key, index) pairs, in ascending index: topk + sort, ties at the cut to the lower index."""
    n = len(max_score)
    k = min(nms_pre, n) if nms_pre > 0 else n
    order = np.lexsort((np.arange(n), score_key(max_score)))
    return np.sort(order[:k])


def decode(anchors, deltas):
    """box_coder.py:270-310 in the kernel's order."""
    a, t = np.asarray(anchors, F32), np.asarray(deltas, F32)
    with np.errstate(all="ignore"):
        xa, ya, wa, la, ha, ra = a[:, 0], a[:, 1], a[:, 3], a[:, 4], a[:, 5], a[:, 6]
        za = a[:, 2] + ha * F32(0.5)
        diag = np.sqrt(la * la + wa * wa).astype(F32)
        xg = t[:, 0] * diag + xa
        yg = t[:, 1] * diag + ya
        zg = t[:, 2] * ha + za
        lg = expf(t[:, 4]) * la
        wg = expf(t[:, 3]) * wa
        hg = expf(t[:, 5]) * ha
        rg = t[:, 6] + ra
        zg = zg - hg * F32(0.5)
        return np.concatenate([np.stack([xg, yg, zg, wg, lg, hg, rg], 1), t[:, 7:] + a[:, 7:]], 1).astype(F32)


def direction_fix(r, dir_bit, dir_offset, dir_limit_offset):
    off, lim = F32(dir_offset), F32(dir_limit_offset)
    with np.errstate(all="ignore"):
        val = (r - off).astype(F32)
        rot = (val - (np.floor((val / PI).astype(F32) + lim).astype(F32) * PI).astype(F32)).astype(F32)
        return ((rot + off).astype(F32) + (PI * dir_bit.astype(F32)).astype(F32)).astype(F32)


def frame_bboxes(cls, reg, dirs, anchors, cfg, nms_kind="port", trace=None):
    """One frame from its maps [channels, H, W]: (boxes [n, cs], scores [n], labels [n]) with n <= max_num."""
    from oracle import pyoracle as O

    nc, cs = cfg["num_classes"], anchors.shape[1]
    cls_rows = np.ascontiguousarray(np.asarray(cls, F32).transpose(1, 2, 0).reshape(-1, nc))
    reg_rows = np.asarray(reg, F32).transpose(1, 2, 0).reshape(-1, cs)
    dir_rows = np.asarray(dirs, F32).transpose(1, 2, 0).reshape(-1, 2)
    scores_all = sigmoid(cls_rows)
    sel = select(max_scores(scores_all), cfg["nms_pre"])
    scores = scores_all[sel]
    boxes = decode(anchors[sel], reg_rows[sel])
    with np.errstate(invalid="ignore"):
        dir_bit = (dir_rows[sel, 1] > dir_rows[sel, 0]).astype(np.int32)
        nms_boxes = boxes[:, :7].copy()
        nms_boxes[:, 6] = -nms_boxes[:, 6]
        src = []  # (class, candidate) class-major
        for c in range(nc):
            cand = np.nonzero(scores[:, c] > F32(cfg["score_thr"]))[0]
            if len(cand) == 0:
                continue
            cand = cand[np.argsort(score_key(scores[cand, c]), kind="stable")]
            keep = O.nms(np.ascontiguousarray(nms_boxes[cand]), float(F32(cfg["nms_thr"])), kind=nms_kind)
            src += [(c, int(k)) for k in cand[keep]]
            if trace is not None:
                trace.setdefault("sets", []).append((c, cand, keep))
    if trace is not None:
        trace.update(sel=sel, scores=scores, boxes=boxes, total=len(src))
    if len(src) > cfg["max_num"]:
        keys = score_key(np.array([scores[k, c] for c, k in src], F32))
        src = [src[i] for i in np.argsort(keys, kind="stable")[:cfg["max_num"]]]
    lab = np.array([c for c, _ in src], np.int32)
    ks = np.array([k for _, k in src], np.int64)
    out = boxes[ks].copy()
    if len(ks):
        out[:, 6] = direction_fix(out[:, 6], dir_bit[ks], cfg["dir_offset"], cfg["dir_limit_offset"])
    return out, scores[ks, lab] if len(ks) else np.zeros(0, F32), lab


def get_bboxes(cls, reg, dirs, anchors, cfg, nms_kind="port"):
    """The device entry points' fixed-size results: boxes [B, max_num, cs], scores, labels int32, counts int32."""
    B, cs, m = cls.shape[0], anchors.shape[1], cfg["max_num"]
    boxes, scores = np.zeros((B, m, cs), F32), np.zeros((B, m), F32)
    labels, counts = np.zeros((B, m), np.int32), np.zeros(B, np.int32)
    for b in range(B):
        bx, sc, lb = frame_bboxes(cls[b], reg[b], dirs[b], np.asarray(anchors, F32), cfg, nms_kind)
        n = len(sc)
        boxes[b, :n], scores[b, :n], labels[b, :n], counts[b] = bx, sc, lb, n
    return boxes, scores, labels, counts


def head_forward(feat, state, anchors, cfg, nms_kind="port"):
    return get_bboxes(*head_maps(feat, state), anchors, cfg, nms_kind)


# ---- the golden cases ------------------------------------------------------------------------------------------------
CASES = {
    # nuScenes-like (configs/bevfusion: 7 sizes x 2 rotations, velocity columns, dir_offset 0.7854, dir_limit_offset 0)
    "nus": dict(seed=1106, B=2, C=16, H=6, W=5, num_classes=10, code_size=9, custom_values=(0, 0),
                ranges=[[-50.0, -50.0, -1.8, 50.0, 50.0, -1.8]],
                sizes=[[1.95, 4.60, 1.73], [2.40, 6.00, 2.80], [2.90, 11.0, 3.40], [0.60, 1.70, 1.30], [0.70, 2.10, 1.40],
                       [0.70, 0.70, 1.70], [0.40, 0.40, 1.10]],
                rotations=[0, 1.57], dir_offset=0.7854, dir_limit_offset=0,
                test_cfg=dict(nms_pre=100, max_num=12, score_thr=0.3, nms_thr=0.2), empty_class=7),
    # KITTI-like: 3 sizes x 2 rotations, 7-wide code, the head's default direction parameters
    "kitti": dict(seed=1201, B=2, C=32, H=5, W=7, num_classes=3, code_size=7, custom_values=(),
                  ranges=[[0.0, -40.0, -0.6, 70.0, 40.0, -0.6], [0.0, -40.0, -0.6, 70.0, 40.0, -0.6],
                          [0.0, -40.0, -1.78, 70.0, 40.0, -1.78]],
                  sizes=[[0.6, 0.8, 1.73], [0.6, 1.76, 1.73], [1.6, 3.9, 1.56]],
                  rotations=[0, 1.57], dir_offset=0, dir_limit_offset=1,
                  test_cfg=dict(nms_pre=60, max_num=10, score_thr=0.35, nms_thr=0.1), empty_class=1),
}
TAGS = tuple(CASES)


def num_anchors(tag):
    c = CASES[tag]
    return len(c["sizes"]) * len(c["rotations"])


def cfg_of(tag):
    c = CASES[tag]
    return dict(c["test_cfg"], dir_offset=c["dir_offset"], dir_limit_offset=c["dir_limit_offset"],
                num_classes=c["num_classes"])


def golden_state(tag):
    """The head's state dict (the reference's keys): seeded weights; the `empty_class` rows of conv_cls get a bias
    that keeps every score of that class below score_thr."""
    c = CASES[tag]
    rng = np.random.default_rng(c["seed"])
    A, nc, cs, C = num_anchors(tag), c["num_classes"], c["code_size"], c["C"]
    st = {}
    for name, rows, scale in (("conv_cls", A * nc, 1.0), ("conv_reg", A * cs, 0.3), ("conv_dir_cls", A * 2, 1.0)):
        st[name + ".weight"] = (rng.standard_normal((rows, C, 1, 1)) * scale / np.sqrt(C)).astype(F32)
        st[name + ".bias"] = (rng.standard_normal(rows) * 0.1).astype(F32)
    st["conv_cls.bias"].reshape(A, nc)[:, c["empty_class"]] = F32(-9.0)
    return st


def golden_inputs(tag):
    """feat [B, C, H, W] float32."""
    c = CASES[tag]
    rng = np.random.default_rng(c["seed"] + 1)
    return rng.standard_normal((c["B"], c["C"], c["H"], c["W"])).astype(F32)
