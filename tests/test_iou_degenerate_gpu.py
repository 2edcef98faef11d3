"""box_overlap (csrc/iou3d_geom.hpp) on the boxes a detector really hands to rotated NMS -- near-duplicates, half and
quarter turns, axis-aligned contacts, degenerate field values (tests/box_families.py) -- in each of the three kernels
it is compiled into: pairwise_kernel (iou3d_nms.hip), nms_mask_kernel (nms_gpu, the tile form) and nms_pairs_kernel
(the pooled form behind class_agnostic_nms and the CenterPoint / BEVDet post-processing).  Such pairs have polygons of
9 ... 16 vertices, which box_overlap sorts in LDS instead of in registers; the vectors of synth.nms_boxes hold three
such pairs per million.  Everything is compared bit for bit with the CPU oracle (the reference's own code where it was
compiled, else the port that is held to it); nothing is filtered out: tests/test_box_families_cpu.py holds every set
drawn here to at most 16 vertices per pair, the reference's array size."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import bevdet_head_numpy as bh  # noqa: E402
import box_families as bf  # noqa: E402
import roi_head_numpy as rn  # noqa: E402
import test_nms_post_bev_gpu as cp_base  # noqa: E402  (its _post helper and configuration, unchanged)

pytestmark = pytest.mark.gpu
F32 = np.float32
# 1.0 decides something here: the reference admits corners with a 1e-2 margin, so the polygon of two near-identical
# boxes is larger than either and their IoU exceeds 1 (up to about 1.03); 1.002 cuts through the middle of those
THRESHOLDS = (0.1, 0.5, 0.9, 0.999, 1.0, 1.002)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _kind(oracle):
    return "ref" if oracle.have_ref() else "port"


def _assert_bits(got, want, what):
    """NaN where the reference has NaN (a NaN's payload is not part of the contract), the bits everywhere else."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what)
    np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan], err_msg=what)


# ---- pairwise_kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", bf.PAIRWISE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fams", bf.PAIRWISE, ids=lambda f: f"{f[0]}-{f[1]}")
def test_pairwise_on_families(oracle, fams, sizes):
    from paddle3d_amd.ops import iou3d_nms

    a, b = bf.pairwise_case(*fams, *sizes)
    verts = oracle.overlap_vertices(a, b)
    assert verts.max() <= 16
    if sizes != (1, 1):  # degenerate pairs in all four waves of a block and in the partial blocks
        assert (verts >= 9).any(), fams
    kind = _kind(oracle)
    iou = iou3d_nms.boxes_iou_bev_gpu(_cuda(a), _cuda(b)).cpu().numpy()
    ov = iou3d_nms.boxes_overlap_bev_gpu(_cuda(a), _cuda(b)).cpu().numpy()
    _assert_bits(ov, oracle.boxes_overlap_bev(a, b, kind), f"overlap {fams} {sizes}")
    _assert_bits(iou, oracle.boxes_iou_bev(a, b, kind), f"iou {fams} {sizes}")


# ---- nms_mask_kernel + sweep (nms_gpu) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", bf.NMS_SIZES)
@pytest.mark.parametrize("family", list(bf.FAMILIES))
def test_nms_gpu_on_families(oracle, family, n):
    from paddle3d_amd.ops import iou3d_nms

    kind = _kind(oracle)
    for seed in bf.SEEDS[family]:
        boxes = bf.FAMILIES[family](seed, n)
        dev = _cuda(boxes)
        for thr in THRESHOLDS:
            keep, num = iou3d_nms.nms_gpu(dev, thr)
            np.testing.assert_array_equal(keep[: int(num[0])].numpy(), oracle.nms(boxes, thr, kind=kind),
                                          err_msg=f"{family} seed {seed} n {n} thr {thr}")


# ---- nms_cand_kernel + nms_pairs_kernel, directly (class_agnostic_nms takes boxes as they are) -------------------------
def _pooled(oracle, box, cls, thr):
    from paddle3d_amd.ops import roi_head

    cfg = {"nms_pre_maxsize": 128, "nms_post_maxsize": 128, "nms_thresh": thr}  # the pool of a set: 4096 pairs
    got = roi_head.class_agnostic_nms(_cuda(box), _cuda(cls), cfg)
    got = [g.cpu().numpy() for g in got]
    want = rn.class_agnostic_nms(oracle, box, cls, False, None, None, 128, thr, 128, kind=_kind(oracle))
    for name, g, w in zip(("boxes", "scores", "labels", "count"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if g.dtype == F32:
            _assert_bits(g, w, name)
        else:
            np.testing.assert_array_equal(g, w, err_msg=name)
    return got


@pytest.mark.parametrize("n", bf.POOL_SIZES)
@pytest.mark.parametrize("fams", (("near", "quarter"), ("wide", "mixture"), ("quarter", "specials")),
                         ids=lambda f: f"{f[0]}-{f[1]}")
def test_pooled_nms_across_the_pool_border(oracle, fams, n):
    """One cluster of n boxes makes n (n - 1) / 2 candidate pairs: 2016 and 4095 fit the pool, 4186 leave one tile
    unpooled (whichever reserves last), 8128 several, with holes in the pool.  The result does not depend on which."""
    rng = np.random.default_rng(n)
    box = np.stack([bf.FAMILIES[f](bf.SEEDS[f][0], n) for f in fams])
    cls = (rng.integers(0, 8, (2, n, 2)) / 8).astype(F32)  # tied scores: stable order
    for thr in (0.5, 0.999, 1.0, 1.002):
        first = _pooled(oracle, box, cls, thr)
        assert first[3].min() >= 1 and (first[3] < n).any()
        for _ in range(2 if n * (n - 1) // 2 > 4096 else 0):  # which tile loses the race must not matter
            again = _pooled(oracle, box, cls, thr)
            for g, h in zip(first, again):
                np.testing.assert_array_equal(g.view(np.uint8), h.view(np.uint8))


# ---- through decoded head maps --------------------------------------------------------------------------------------------
def _duplicate_cells(rng, batch, h, w):
    """Head maps in which the 16 cells of every 4 x 4 block decode to one box: reg = block centre - cell index (+-0.5,
    +-1.5: exact), equal height, dim and rot per block; a random half of the cells with rot negated in both channels
    (heading + pi); every cell but two adjacent ones per block (reg +0.5 / -0.5: exact copies) jittered at the 1e-3
    level.  Returns dict(reg [B, 2, h, w], height [B, 1, ..], dim [B, 3, ..], rot [B, 2, ..]) float32."""
    ys, xs = np.mgrid[0:h, 0:w]
    by, bx = ys // 4, xs // 4
    nb = (batch, h // 4, w // 4)

    def cells(v):  # [B, h/4, w/4] -> [B, h, w]
        return v[:, by, bx]

    reg = np.stack([np.broadcast_to(bx * 4 + 1.5 - xs, (batch, h, w)),
                    np.broadcast_to(by * 4 + 1.5 - ys, (batch, h, w))], 1).astype(np.float64)
    height = cells(rng.uniform(-2.0, 0.0, nb))[:, None]
    dim = np.log(np.stack([cells(rng.uniform(1.5, 4.5, nb)), cells(rng.uniform(0.8, 2.2, nb)),
                           cells(rng.uniform(1.4, 2.0, nb))], 1))
    ang = cells(rng.uniform(-np.pi, np.pi, nb))
    rot = np.stack([np.sin(ang), np.cos(ang)], 1)
    rot = np.where(rng.random((batch, 1, h, w)) < 0.5, -rot, rot)
    loose = ~((ys % 4 == 1) & ((xs % 4 == 1) | (xs % 4 == 2)))
    for m in (reg, dim, rot):
        m += rng.uniform(-1e-3, 1e-3, m.shape) * loose
    return dict(reg=reg.astype(F32), height=height.astype(F32), dim=dim.astype(F32), rot=rot.astype(F32))


def _block_scores(rng, batch, ncls, h, w):
    """Heat map: one level per 4 x 4 block plus cell noise, so that a top-K cut keeps whole blocks."""
    ys, xs = np.mgrid[0:h, 0:w]
    level = rng.normal(0.5, 2.0, (batch, ncls, h // 4, w // 4))[:, :, ys // 4, xs // 4]
    return (level + rng.normal(0.0, 0.3, (batch, ncls, h, w))).astype(F32)


def _assert_lds_pairs(oracle, nms_boxes, floor):
    v = oracle.overlap_vertices(nms_boxes, nms_boxes)[np.triu_indices(len(nms_boxes), 1)]
    assert v.max() <= 16
    assert (v >= 9).sum() >= floor, np.bincount(v, minlength=17)


@pytest.mark.parametrize("seed", (0, 1))
def test_centerpoint_postprocess_duplicate_cells(oracle, seed):
    rng = np.random.default_rng([seed, 31])
    tasks = []
    for ncls in (1, 2):
        t = _duplicate_cells(rng, 1, 32, 32)
        t["hm"] = _block_scores(rng, 1, ncls, 32, 32)
        t["vel"] = rng.normal(0.0, 2.0, (1, 2, 32, 32)).astype(F32)
        tasks.append(t)
    # what NMS is handed, from the reference's own decode: every cell in score order (no suppression, no cap), in the
    # NMS kernel's box form (dx <-> dy, heading -> -heading - pi/2: iou3d_nms_kernel.cu:294-308)
    cfg = cp_base.CP_CFG
    for t in tasks:
        rb, _, _ = oracle.centerpoint_postprocess([t], cfg["voxel_size"] + [8.0], cfg["point_cloud_range"] + [0.0] * 4,
                                                  cfg["post_center_range"], [0], cfg["down_ratio"],
                                                  cfg["score_threshold"], 3e38, 1000, 1024, True)
        assert len(rb) > 300
        nb = rb[:, [0, 1, 2, 4, 3, 5, 8]].copy()
        nb[:, 6] = (-rb[:, 8].astype(np.float64) - np.pi / 2).astype(F32)
        _assert_lds_pairs(oracle, nb[:400], 300)
    for thr in (0.2, 1.0, 1.001):  # IoU of the near-identical cells lies around 1
        (b, s, l), (rb, rs, rl), margins = cp_base._post(oracle, tasks, nms_iou_threshold=thr, nms_pre_max_size=1000,
                                                         nms_post_max_size=1000)
        assert b.shape == rb.shape and 20 < b.shape[0] < 1500, (b.shape, rb.shape, margins)
        np.testing.assert_array_equal(l, rl)
        np.testing.assert_array_equal(s.view(np.uint32), rs.view(np.uint32))
        np.testing.assert_array_equal(b.view(np.uint32), rb.view(np.uint32))


@pytest.mark.parametrize("seed", (0, 1))
def test_bevdet_postprocess_duplicate_cells(oracle, seed):
    """Two rotate-NMS tasks with different nms_thr: the per-set threshold argument of nms_pairs_kernel."""
    from paddle3d_amd import bevdet_head

    rng = np.random.default_rng([seed, 32])
    classes = [1, 2]
    heads = []
    for ncls in classes:
        hd = _duplicate_cells(rng, 2, 32, 32)
        hd["heatmap"] = _block_scores(rng, 2, ncls, 32, 32)
        hd["vel"] = rng.normal(0.0, 1.0, (2, 2, 32, 32)).astype(F32)
        heads.append(hd)
    coder = dict(pc_range=[-12.8, -12.8], post_center_range=[-20.0, -20.0, -10.0, 20.0, 20.0, 10.0], max_num=500,
                 score_threshold=0.1, out_size_factor=8, voxel_size=[0.1, 0.1], code_size=9)
    cfg = dict(bevdet_head.BEVDET4D_TEST_CFG, pc_range=[-12.8, -12.8],
               post_center_limit_range=[-20.0, -20.0, -10.0, 20.0, 20.0, 10.0], pre_max_size=500, post_max_size=500,
               nms_type=["rotate", "rotate"], nms_thr=[0.2, 1.001], min_radius=[4, 12],
               nms_rescale_factor=[1.0, [0.7, 0.7]])
    # what NMS is handed, from the restatement's decode (nms_bev's form, then rotate_nms_pcdet's)
    for t, hd in enumerate(heads):
        for frame in range(2):
            box, _, _ = bh.decode_task(oracle, hd, frame, coder)
            assert len(box) > 100
            nb = box[:, :7].copy()
            nb[:, 3:6] = nb[:, 3:6] * F32(1.0 if t == 0 else 0.7)
            # nms_bev turns the heading to -h - pi/2 and swaps dx, dy; rotate_nms_pcdet does the same again
            nb[:, 6] = -(-nb[:, 6] - bh.HALF_PI) - bh.HALF_PI
            _assert_lds_pairs(oracle, nb, 300)
    c = bevdet_head.CenterPointBBoxCoder(**coder)
    preds = [{k: _cuda(v) for k, v in hd.items()} for hd in heads]
    got = [(b.cpu().numpy(), s.cpu().numpy(), l.cpu().numpy()) for b, s, l in
           bevdet_head.get_bboxes(preds, cfg, c, classes)]
    want = bh.get_bboxes(oracle, heads, cfg, coder, classes)
    assert len(got) == len(want) == 2
    for (b, s, l), (rb, rs, rl) in zip(got, want):
        assert b.shape == rb.shape and 20 < b.shape[0] < 1000, (b.shape, rb.shape)
        np.testing.assert_array_equal(l, rl)
        np.testing.assert_array_equal(s.view(np.uint32), rs.view(np.uint32))
        np.testing.assert_array_equal(b.view(np.uint32), rb.view(np.uint32))
    # the two thresholds decide differently: the looser task keeps more of its candidates
    assert all((l >= 1).sum() > (l == 0).sum() for _, _, l in got)
