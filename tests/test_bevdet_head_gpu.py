"""BEVDet4D CenterHead post-processing on the device (ops/bevdet_postprocess.py, paddle3d_amd/bevdet_head.py)
against the reference's own outputs (tests/golden/python_bevdet_head.npz) and, bit for bit, against the NumPy
restatement in tests/golden/bevdet_head_numpy.py at the full BEVDet4D configuration."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import bevdet_head_numpy as bh  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BEVDET4D_CLASSES = [1, 2, 2, 1, 2, 2]


def _preds(heads):
    return [{k: torch.from_numpy(v).to(DEV) for k, v in hd.items()} for hd in heads]


def _run(heads, test_cfg, coder, classes, norm_bbox=True):
    from paddle3d_amd import bevdet_head

    c = bevdet_head.CenterPointBBoxCoder(**coder)
    res = bevdet_head.get_bboxes(_preds(heads), test_cfg, c, classes, norm_bbox=norm_bbox)
    return [(b.cpu().numpy(), s.cpu().numpy(), l.cpu().numpy()) for b, s, l in res]


def _bits_equal(got, want):
    assert len(got) == len(want)
    for (b, s, l), (rb, rs, rl) in zip(got, want):
        assert b.shape == rb.shape, (b.shape, rb.shape)
        np.testing.assert_array_equal(l, rl)
        np.testing.assert_array_equal(s.view(np.uint32), rs.view(np.uint32))
        np.testing.assert_array_equal(b.view(np.uint32), rb.view(np.uint32))


def _full_cfg():
    from paddle3d_amd import bevdet_head

    return dict(bevdet_head.BEVDET4D_TEST_CFG), dict(bevdet_head.BEVDET4D_BBOX_CODER)


def test_bevdet_head_vs_reference_python():
    gold = np.load(os.path.join(HERE, "golden", "python_bevdet_head.npz"))
    got = _run(bh.golden_inputs(), bh.GOLDEN_TEST_CFG, bh.GOLDEN_CODER, bh.GOLDEN_TASKS)
    assert len(got) == bh.GOLDEN_BATCH
    for i, (b, s, l) in enumerate(got):
        assert b.shape == gold[f"bboxes_{i}"].shape and l.dtype == np.int32
        np.testing.assert_array_equal(l, gold[f"labels_{i}"])
        np.testing.assert_allclose(s, gold[f"scores_{i}"], rtol=0, atol=2e-7)
        np.testing.assert_allclose(b, gold[f"bboxes_{i}"], rtol=2e-6, atol=2e-6)


def test_bevdet4d_config_bit_exact_vs_numpy(oracle):
    cfg, coder = _full_cfg()
    heads = bh.head_maps(BEVDET4D_CLASSES, 4, 128, 128, seed=77, peaks=60)
    got = _run(heads, cfg, coder, BEVDET4D_CLASSES)
    want = bh.get_bboxes(oracle, heads, cfg, coder, BEVDET4D_CLASSES)
    _bits_equal(got, want)
    assert all(len(b) > 100 for b, _, _ in got)


def test_batch_equals_per_frame_calls():
    cfg, coder = _full_cfg()
    heads = bh.head_maps(BEVDET4D_CLASSES, 3, 128, 128, seed=78, peaks=40)
    whole = _run(heads, cfg, coder, BEVDET4D_CLASSES)
    for f in range(3):
        one = _run([{k: np.ascontiguousarray(v[f:f + 1]) for k, v in hd.items()} for hd in heads], cfg, coder,
                   BEVDET4D_CLASSES)
        _bits_equal(one, whole[f:f + 1])


def test_saturated_heatmaps_follow_tie_rule(oracle):
    """sigmoid(30) == 1.0f: hundreds of equal scores, ordered by ascending (class, cell)."""
    cfg, coder = _full_cfg()
    heads = bh.head_maps(BEVDET4D_CLASSES, 2, 64, 64, seed=79, peaks=30)
    rng = np.random.default_rng(1)
    for hd in heads:
        hm = hd["heatmap"]
        hm[rng.random(hm.shape) < 0.08] = 30.0
    got = _run(heads, cfg, coder, BEVDET4D_CLASSES)
    want = bh.get_bboxes(oracle, heads, cfg, coder, BEVDET4D_CLASSES)
    _bits_equal(got, want)
    assert sum(int((s == 1.0).sum()) for _, s, _ in got) > 50


def test_empty_task_zero_threshold_and_scale_back_bits(oracle):
    cfg, coder = _full_cfg()
    cfg["nms_rescale_factor"] = [0.7, [0.7, 0.7], [0.4, 0.55], 1.1, [1.0, 1.0], [4.5, 9.0]]
    heads = bh.head_maps(BEVDET4D_CLASSES, 2, 64, 64, seed=80, peaks=30)
    heads[2]["heatmap"][:] = -20.0  # task 2 (bus, trailer): nothing above the threshold
    got = _run(heads, cfg, coder, BEVDET4D_CLASSES)
    want = bh.get_bboxes(oracle, heads, cfg, coder, BEVDET4D_CLASSES)
    _bits_equal(got, want)
    for _, _, l in got:
        assert not np.isin(l, [3, 4]).any() and (l == 0).any()
    # the bit-exact comparison sees the scale back: (d * 0.7) / 0.7 differs from d for some decoded car dims
    e = bh.decode_task(oracle, heads[0], 0, coder)[0][:, 3:6]
    assert ((e * np.float32(0.7)) / np.float32(0.7) != e).any()
    # score_threshold = 0: no score mask at all (the coder tests `if self.score_threshold:`)
    coder0 = dict(coder, score_threshold=0.0)
    cfg0 = dict(cfg, score_threshold=0.0)
    got0 = _run(heads, cfg0, coder0, BEVDET4D_CLASSES)
    _bits_equal(got0, bh.get_bboxes(oracle, heads, cfg0, coder0, BEVDET4D_CLASSES))
    assert sum(len(s) for _, s, _ in got0) > sum(len(s) for _, s, _ in got)
    assert any((s < 0.1).any() for _, s, _ in got0)


def _circle_nms_loop(dets, thresh):
    """bbox.circle_nms as plain Python (numba.jit as the identity), with equal scores in ascending index order."""
    x1, y1, scores = dets[:, 0], dets[:, 1], dets[:, 2]
    order = np.argsort(-scores, kind="stable")
    n = dets.shape[0]
    suppressed = np.zeros(n, np.int32)
    keep = []
    for _i in range(n):
        i = order[_i]
        if suppressed[i] == 1:
            continue
        keep.append(int(i))
        for _j in range(_i + 1, n):
            j = order[_j]
            if suppressed[j] == 1:
                continue
            dist = (x1[i] - x1[j]) ** 2 + (y1[i] - y1[j]) ** 2
            if float(dist) <= thresh:
                suppressed[j] = 1
    return keep


def test_circle_nms_vs_python_loop():
    from paddle3d_amd.ops.bevdet_postprocess import circle_nms

    rng = np.random.default_rng(81)
    for n, thr, ties in ((1, 1.0, False), (200, 0.85, False), (700, 4.0, True), (1500, 0.175, False)):
        dets = np.concatenate([rng.uniform(-20, 20, (n, 2)), rng.random((n, 1))], 1).astype(np.float32)
        if ties:
            dets[:, 2] = np.round(dets[:, 2] * 4) / 4
        got = circle_nms(torch.from_numpy(dets).to(DEV), thr)
        assert got == _circle_nms_loop(dets, thr)
    assert circle_nms(torch.zeros((0, 3), device=DEV), 1.0) == []


def test_refusals():
    from paddle3d_amd import bevdet_head
    from paddle3d_amd.ops.bevdet_postprocess import circle_nms

    cfg, coder = _full_cfg()
    c = bevdet_head.CenterPointBBoxCoder(**coder)
    heads = bh.head_maps([1, 2], 1, 32, 32, seed=82)
    cfg2 = dict(cfg, nms_type=["rotate", "circle"], nms_thr=[0.2, 0.2], min_radius=[4, 1],
                nms_rescale_factor=[1.0, [0.7, 0.7]])
    with pytest.raises(RuntimeError):  # CPU tensors: no host path
        cpu = [{k: torch.from_numpy(v) for k, v in hd.items()} for hd in heads]
        bevdet_head.get_bboxes(cpu, cfg2, bevdet_head.CenterPointBBoxCoder(**dict(coder, max_num=100)), [1, 2])
    preds = _preds(heads)
    for p in preds:
        del p["vel"]
    with pytest.raises(RuntimeError, match="vel"):
        bevdet_head.get_bboxes(preds, cfg2, c, [1, 2])
    # max_num > ncls * H * W (here 500 > 2 * 16 * 16): the reference's first paddle.topk(k > H * W) raises
    small = bh.head_maps([1, 2], 1, 16, 16, seed=83)
    with pytest.raises(RuntimeError, match="max_num"):
        bevdet_head.get_bboxes(_preds(small), cfg2, c, [1, 2])
    big = [dict(heatmap=torch.zeros((1, 1, 4097, 4096), device=DEV)) for _ in range(1)]
    for k, ch in (("reg", 2), ("height", 1), ("dim", 3), ("rot", 2), ("vel", 2)):
        big[0][k] = torch.zeros((1, ch, 4097, 4096), device=DEV)
    cfg1 = dict(cfg, nms_type=["rotate"], nms_thr=[0.2], min_radius=[1.0], nms_rescale_factor=[1.0])
    with pytest.raises(RuntimeError, match="2\\^24"):
        bevdet_head.get_bboxes(big, cfg1, c, [1])
    del big
    with pytest.raises(RuntimeError):
        circle_nms(torch.zeros((4, 3)), 1.0)
