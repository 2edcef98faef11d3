"""NumPy restatement of BEVDet4D's CenterHead post-processing (TEST INFRASTRUCTURE ONLY) and the seeded inputs of
python_bevdet_head.npz.

Restates CenterHeadMatch.get_bboxes (reference bevdet_centerhead.py:669-783) with CenterPointBBoxCoder.decode
(:1119-1214), get_task_detections (:785-906), nms_bev (:939-968), _circle_nms (:912-921) and circle_nms
(geometries/bbox.py:450-474) under this library's arithmetic contract: fp32 operations in the reference's order,
glibc expf / atan2f bits (oracle libm_eval), the rotated IoU + sweep of oracle.rotate_nms_pcdet_numpy, equal scores
in ascending (class, cell) order, the circle distance compared in double.  The device operator must match it bit for
bit; tests/test_bevdet_head_cpu.py pins it against the reference's own outputs."""
from __future__ import annotations

import numpy as np

f32 = np.float32
HALF_PI = f32(np.pi / 2)

# the golden's configuration: 4 tasks, one circle task, a list factor, a scalar factor != 1, nms_thr 0.5
GOLDEN_TASKS = [1, 2, 1, 2]
GOLDEN_CODER = dict(pc_range=[-19.2, -19.2], post_center_range=[-20.0, -20.0, -2.0, 20.0, 20.0, 2.0], max_num=200,
                    score_threshold=0.1, out_size_factor=8, voxel_size=[0.1, 0.1], code_size=9)
GOLDEN_TEST_CFG = dict(pc_range=[-19.2, -19.2], post_center_limit_range=[-18.0, -18.0, -1.5, 18.0, 18.0, 1.5],
                       max_per_img=500, max_pool_nms=False, min_radius=[4, 12, 1.5, 1], score_threshold=0.1,
                       out_size_factor=8, voxel_size=[0.1, 0.1], pre_max_size=150, post_max_size=30,
                       nms_type=["rotate", "rotate", "circle", "rotate"], nms_thr=[0.2, 0.2, 0.2, 0.5],
                       nms_rescale_factor=[1.0, [0.4, 0.55], 1.1, 0.7])
GOLDEN_HW = (48, 48)
GOLDEN_BATCH = 2
GOLDEN_SEED = 4_2024


def head_maps(task_classes, batch, h, w, seed, peaks=24):
    """One dict per task: heatmap with planted peaks (each peak's 3 x 3 neighbourhood slightly lower, so that NMS has
    overlapping candidates to remove) over a low background, reg in [0, 1), height around 0 with some cells outside
    the coder's z range, log-dims around 1.6 m boxes, rotation sine / cosine, velocity."""
    rng = np.random.default_rng(seed)
    out = []
    for c in task_classes:
        hm = rng.normal(-3.0, 1.0, (batch, c, h, w)).astype(f32)
        for b in range(batch):
            for k in range(c):
                ys = rng.integers(1, h - 1, peaks)
                xs = rng.integers(1, w - 1, peaks)
                for y, x in zip(ys, xs):
                    top = rng.uniform(0.5, 4.0)
                    hm[b, k, y - 1:y + 2, x - 1:x + 2] = np.maximum(
                        hm[b, k, y - 1:y + 2, x - 1:x + 2], top - rng.uniform(0.3, 1.5, (3, 3))).astype(f32)
                    hm[b, k, y, x] = top
        out.append(dict(heatmap=hm,
                        reg=rng.random((batch, 2, h, w)).astype(f32),
                        height=rng.normal(0.0, 1.0, (batch, 1, h, w)).astype(f32),
                        dim=rng.normal(0.5, 0.3, (batch, 3, h, w)).astype(f32),
                        rot=rng.normal(0.0, 1.0, (batch, 2, h, w)).astype(f32),
                        vel=rng.normal(0.0, 1.0, (batch, 2, h, w)).astype(f32)))
    return out


def golden_inputs():
    return head_maps(GOLDEN_TASKS, GOLDEN_BATCH, *GOLDEN_HW, GOLDEN_SEED)


def _per_task(v, n):
    return list(v) if isinstance(v, (list, tuple)) else [v] * n


def decode_task(O, head, frame, coder, norm_bbox=True):
    """decode + _topk for one frame of one task: (boxes [n, 9], scores [n], labels [n]) in descending score order."""
    hm = head["heatmap"][frame]
    c, h, w = hm.shape
    hw = h * w
    e = O.libm_eval(2, -hm.reshape(-1))
    s = (f32(1.0) / (f32(1.0) + e)).astype(f32)
    sel = np.argsort(-s, kind="stable")[: coder["max_num"]]  # (score desc, flat index asc)
    score = s[sel]
    cls, cell = sel // hw, sel % hw
    xs, ys = (cell % w).astype(f32), (cell // w).astype(f32)
    reg = head["reg"][frame].reshape(2, hw)[:, cell]
    osf, vs, pr = f32(coder["out_size_factor"]), np.asarray(coder["voxel_size"], f32), np.asarray(coder["pc_range"], f32)
    x = ((xs + reg[0]) * osf) * vs[0] + pr[0]
    y = ((ys + reg[1]) * osf) * vs[1] + pr[1]
    z = head["height"][frame].reshape(hw)[cell]
    d = head["dim"][frame].reshape(3, hw)[:, cell]
    if norm_bbox:
        d = O.libm_eval(2, d)
    rot = head["rot"][frame].reshape(2, hw)[:, cell]
    ang = O.libm_eval(4, rot[0], rot[1])
    vel = head["vel"][frame].reshape(2, hw)[:, cell]
    box = np.stack([x, y, z, d[0], d[1], d[2], ang, vel[0], vel[1]], 1).astype(f32)
    r = np.asarray(coder["post_center_range"], f32)
    m = np.all(box[:, :3] >= r[:3], 1) & np.all(box[:, :3] <= r[3:], 1)
    if coder["score_threshold"]:
        m &= score > f32(coder["score_threshold"])
    return box[m], score[m], cls[m].astype(np.int64)


def circle_keep(xy, thresh):
    """The circle_nms loop over points already in descending score order: kept positions."""
    x, y = xy[:, 0].astype(f32), xy[:, 1].astype(f32)
    n = len(x)
    supp = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if supp[i]:
            continue
        keep.append(i)
        dx, dy = x[i] - x[i + 1:], y[i] - y[i + 1:]
        dist = (dx * dx + dy * dy).astype(f32)
        supp[i + 1:] |= dist.astype(np.float64) <= float(thresh)
    return np.asarray(keep, np.int64)


def get_bboxes(O, heads, test_cfg, coder, task_classes, norm_bbox=True, nms_kind=None):
    """[(bboxes [n, 9], scores [n], labels int32 [n]) per frame]."""
    nms_kind = nms_kind or ("ref" if O.have_ref() else "port")
    nt = len(heads)
    batch = heads[0]["heatmap"].shape[0]
    types = _per_task(test_cfg["nms_type"], nt)
    thr = _per_task(test_cfg["nms_thr"], nt)
    rad = _per_task(test_cfg["min_radius"], nt)
    factors = test_cfg.get("nms_rescale_factor", [1.0] * nt)
    lim = np.asarray(test_cfg["post_center_limit_range"], f32)
    out = []
    for b in range(batch):
        bb, ss, ll = [], [], []
        off = 0
        for t in range(nt):
            box, score, cls = decode_task(O, heads[t], b, coder, norm_bbox)
            post = test_cfg["post_max_size"]
            if len(box) == 0:
                keep = np.zeros(0, np.int64)
            elif types[t] == "circle":
                keep = circle_keep(box[:, :2], rad[t])[:post]
            else:
                fl = factors[t]
                fc = np.asarray([fl[k] if isinstance(fl, (list, tuple)) and k < len(fl) else
                                 (1.0 if isinstance(fl, (list, tuple)) else fl) for k in range(task_classes[t])], f32)
                f = fc[cls]
                sb = box.copy()
                sb[:, 3:6] = sb[:, 3:6] * f[:, None]
                # nms_bev's form (3 <-> 4, -rot - pi/2); rotate_nms_pcdet_numpy undoes the swap and converts again
                nb = sb[:, [0, 1, 2, 4, 3, 5, 6]].copy()
                nb[:, 6] = -sb[:, 6] - HALF_PI
                keep = O.rotate_nms_pcdet_numpy(nb, score, thr[t], test_cfg["pre_max_size"], post, kind=nms_kind)
                keep = np.asarray(keep, np.int64)
                box = box.copy()
                box[:, 3:6] = (sb[:, 3:6] / f[:, None]).astype(f32)
            kb, ks, kl = box[keep], score[keep], cls[keep]
            if types[t] != "circle" and len(kb):
                m = np.all(kb[:, :3] >= lim[:3], 1) & np.all(kb[:, :3] <= lim[3:], 1)
                kb, ks, kl = kb[m], ks[m], kl[m]
            bb.append(kb)
            ss.append(ks)
            ll.append((kl + off).astype(np.int32))
            off += task_classes[t]
        bx = np.concatenate(bb).astype(f32) if bb else np.zeros((0, 9), f32)
        bx[:, 2] = bx[:, 2] - bx[:, 5] * f32(0.5)
        out.append((bx, np.concatenate(ss).astype(f32), np.concatenate(ll).astype(np.int32)))
    return out
