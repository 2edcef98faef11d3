"""NumPy restatement of csrc/bevformer_decoder.hip, operation for operation in float32 (the order is the one in that
file's header).

mha(q, k, v, num_heads, expf)                     pd3_mha_forward: q [B, Nq, E], k, v [B, Nk, E] -> [B, Nq, E]
dec_ca(value, offsets, logits, ref, shapes, starts, expf)      pd3_bevformer_dec_ca
threshold_test(top, thr)                          the test the loop of box_coder.py:158-166 ends with: (mode, cur)
nms_free_decode(cls, bbox, post_center_range, max_num, score_threshold, bottom_center, expf, atan2f)
    pd3_nms_free_decode: (boxes, scores, labels int32, count int32, rows int32 -- the box row of every kept entry)

`expf` / `atan2f` are float32 array functions with glibc's bits (oracle.pyoracle.libm_eval(2, x) / (4, y, x)); fmaf is
pv_rcnn_numpy's correctly rounded one.  The sampled point is tests/golden/ms_deform_attn_numpy.py's forward().
"""
import numpy as np

import bevformer_numpy as bn
import ms_deform_attn_numpy as md
from pv_rcnn_numpy import fmaf

F32 = np.float32


def mha(q, k, v, num_heads, expf):
    q, k, v = (np.asarray(t, F32) for t in (q, k, v))
    B, Nq, E = q.shape
    Nk, M = k.shape[1], num_heads
    d = E // M
    with np.errstate(all="ignore"):
        qs = (q.reshape(B, Nq, M, d) * F32(float(d) ** -0.5)).astype(F32).transpose(0, 2, 1, 3)  # [B, M, Nq, d]
        kh = k.reshape(B, Nk, M, d).transpose(0, 2, 1, 3)  # [B, M, Nk, d]
        vh = v.reshape(B, Nk, M, d).transpose(0, 2, 1, 3)
        s = np.zeros((B, M, Nq, Nk), F32)
        for c in range(d):
            s = fmaf(qs[..., :, None, c], kh[..., None, :, c], s)
        nan = np.isnan(s)
        mx = np.where(nan, -np.inf, s).max(-1).astype(F32)
        mx = np.where(nan[..., 0], s[..., 0], mx)
        e = expf((s - mx[..., None]).astype(F32)).reshape(s.shape).astype(F32)
        lanes = np.zeros(s.shape[:-1] + (-(-Nk // 64) * 64,), F32)
        lanes[..., :Nk] = e
        lanes = lanes.reshape(s.shape[:-1] + (-1, 64))
        p = np.zeros(s.shape[:-1] + (64,), F32)
        for step in range(lanes.shape[-2]):
            p = (p + lanes[..., step, :]).astype(F32)
        h = 32
        while h >= 1:
            p = (p[..., :h] + p[..., h:2 * h]).astype(F32)
            h //= 2
        a = (e / p).astype(F32)
        out = np.zeros((B, M, Nq, d), F32)
        for j in range(Nk):
            out = fmaf(a[..., j:j + 1], vh[:, :, None, j, :], out)
    return np.ascontiguousarray(out.transpose(0, 2, 1, 3)).reshape(B, Nq, E)


def dec_ca(value, offsets, logits, ref, shapes, starts, expf):
    """value [B, S, M, C], offsets [B, Q, M, L, P, 2], logits [B, Q, M, L*P], ref [B, Q, 1 or L, 2]."""
    B, Q, M, L, P, _ = offsets.shape
    a = bn.softmax(logits, expf).reshape(B, Q, M, L, P)
    with np.errstate(all="ignore"):
        off = (np.asarray(offsets, F32) / bn._normalizer(shapes)).astype(F32)
        loc = (np.asarray(ref, F32)[:, :, None, :, None, :] + off).astype(F32)
    return md.forward(np.ascontiguousarray(value, F32), loc, a, shapes, starts)


def threshold_test(top, thr):
    """(mode, cur): 0 score > cur, 1 score >= cur, 2 every score; top the best score (float32), thr a Python float."""
    top = F32(top)
    if top > F32(thr):
        return 0, F32(thr)
    tmp = float(thr)
    while True:
        tmp = tmp * 0.9
        if tmp < 0.01:
            return 2, F32(0)
        if top >= F32(tmp):
            return 1, F32(tmp)


def nms_free_decode(cls, bbox, post_center_range, max_num, score_threshold, bottom_center, expf, atan2f):
    cls, bbox = np.asarray(cls, F32), np.asarray(bbox, F32)
    B, Q, K = cls.shape
    code = bbox.shape[-1]
    r = np.asarray(post_center_range, F32)
    with np.errstate(all="ignore"):
        s = (F32(1) / (F32(1) + expf((-cls).reshape(-1)).reshape(cls.shape).astype(F32))).astype(F32).reshape(B, Q * K)
    boxes = np.zeros((B, max_num, code - 1), F32)
    scores = np.zeros((B, max_num), F32)
    labels = np.full((B, max_num), -1, np.int32)
    rows = np.full((B, max_num), -1, np.int32)
    count = np.zeros(B, np.int32)
    for b in range(B):
        nan = np.isnan(s[b])
        order = np.argsort(np.where(nan, F32(-1), s[b]) * F32(-1), kind="stable")[:max_num]
        sc, ok = s[b][order], ~nan[order]
        row, lab = order // K, order % K
        p = bbox[b][row]
        with np.errstate(all="ignore"):
            ex = lambda x: expf(np.ascontiguousarray(x)).astype(F32)  # noqa: E731
            cols = [p[:, 0], p[:, 1], p[:, 4], ex(p[:, 2]), ex(p[:, 3]), ex(p[:, 5]),
                    atan2f(np.ascontiguousarray(p[:, 6]), np.ascontiguousarray(p[:, 7])).astype(F32)]
            if code > 8:
                cols += [p[:, 8], p[:, 9]]
            bx = np.stack(cols, -1).astype(F32)
            keep = ok & (bx[:, 0] >= r[0]) & (bx[:, 1] >= r[1]) & (bx[:, 2] >= r[2]) & (bx[:, 0] <= r[3]) & \
                (bx[:, 1] <= r[4]) & (bx[:, 2] <= r[5])
            if score_threshold is not None and score_threshold > 0:
                mode, cur = threshold_test(sc[0] if ok[0] else F32(np.nan), score_threshold)
                if mode == 0:
                    keep &= sc > cur
                elif mode == 1:
                    keep &= sc >= cur
            if bottom_center:
                bx[:, 2] = (bx[:, 2] - (bx[:, 5] * F32(0.5)).astype(F32)).astype(F32)
        n = int(keep.sum())
        boxes[b, :n], scores[b, :n], labels[b, :n], rows[b, :n], count[b] = bx[keep], sc[keep], lab[keep], row[keep], n
    return boxes, scores, labels, count, rows
