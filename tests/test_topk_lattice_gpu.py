"""The shared block top-K selection (csrc/block_topk.hpp) on the border lattice of tests/topk_lattice.py, through
pd3_selfcheck_block_topk: every comparison is an exact integer comparison with a stable argsort.  What the cases cover
is proved in tests/test_topk_lattice_cpu.py.  The call sites' crosses at the end of this file run CenterPoint,
nms_free_decode and BEVDet; SSD's are in tests/test_pointpillars_gpu.py (test_ssd_postprocess_selection_lattice) and
Anchor3DHead's in tests/test_anchor3d_gpu.py (test_selection_lattice_*), next to the helpers they share."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_lattice as L  # noqa: E402

pytestmark = pytest.mark.gpu


def _check_group(g, form, cases, outs, what=""):
    idx, key, cut = outs
    for s, c in enumerate(cases):
        want = L.ref_select(c.keys, g.K, L.counted_mask(c.keys, g.key_bits, g.leave_out))
        wk = L.walk(c.keys, g.K, g.key_bits, g.leave_out)
        where = f"{c.id} form {form} set {s}{what}"
        assert not (cut[s] == L.TAKE_ALL).all(), f"{where}: the probe refused a set that keeps the contract"
        np.testing.assert_array_equal(idx[s], want, err_msg=f"{where}: idx is not the stable argsort's first K")
        np.testing.assert_array_equal(key[s], c.keys[want].astype(np.int64), err_msg=f"{where}: key")
        assert (int(cut[s][0]), int(cut[s][1])) == (wk.kc, wk.r), (
            f"{where}: idx is correct, but the cut is {tuple(int(v) for v in cut[s])} where the restated walk gives "
            f"{(wk.kc, wk.r)} at depth {wk.depth}: the case's coverage label (stop depth, r) is not what the device ran")


@pytest.mark.parametrize("gid", [g.id for g in L.GROUPS])
def test_primitive_equals_stable_argsort(gid):
    """Every raw-key case, the families of a group as the sets of one launch, in both forms: idx, key and the cut."""
    g = next(g for g in L.GROUPS if g.id == gid)
    cases = L.group_cases(gid)
    sets = [c.keys for c in cases]
    got = {}
    for form in g.forms:
        got[form] = L.run_probe(sets, g.K, g.key_bits, form, g.leave_out)
        _check_group(g, form, cases, got[form])
    if len(g.forms) == 2:
        np.testing.assert_array_equal(got[0][0], got[1][0], err_msg=f"{gid}: form 0 and form 1 differ")


def test_side_stream_and_set_position():
    """The same set on a side stream and as set 2 of 3 (between two other sets) returns the same bits."""
    g = next(g for g in L.GROUPS if g.key_bits == 30 and g.n >= 4096 and g.K >= 255)
    cases = {c.family: c for c in L.group_cases(g.id)}
    mine = cases["tie-rmax"]
    side = torch.cuda.Stream()
    for form in g.forms:
        alone = L.run_probe([mine.keys], g.K, g.key_bits, form, g.leave_out)
        on_side = L.run_probe([mine.keys], g.K, g.key_bits, form, g.leave_out, stream=side)
        side.synchronize()
        mid = L.run_probe([cases["whole-1"].keys, mine.keys, cases["equal"].keys], g.K, g.key_bits, form, g.leave_out)
        _check_group(g, form, [mine], alone)
        for a, b, c in zip(alone, on_side, mid):
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(a[0], c[1])


@pytest.mark.parametrize("K,counted,n", [(1, 1, 1), (64, 64, 65), (65, 3, 961), (257, 257, 1025), (1024, 1023, 4097),
                                          (1024, 1024, 16384), (513, 0, 2049)])
def test_skip_cut_takes_all_counted_keys(K, counted, n):
    """The callers' take-all cut when no more than K keys qualify: every counted key in (key, index) order, the rest of
    the list empty.  (Keys that are not counted are 0xFFFFFFFF here: the take-all cut-off itself.)"""
    rng = np.random.default_rng(L._seed("skip", K, counted, n))
    sets = []
    for s in range(3):
        keys = np.full(n, 0xFFFFFFFF, np.uint32)
        pos = rng.choice(n, counted, replace=False)
        keys[pos] = rng.integers(0, 1 << (30 if s < 2 else 3), counted)      # the last set: many equal keys
        sets.append(keys)
    for form in L.FORMS:
        idx, key, cut = L.run_probe(sets, K, 30, form, skip_cut=True)
        for s, keys in enumerate(sets):
            order = np.argsort(keys.astype(np.int64), kind="stable")[:counted]
            np.testing.assert_array_equal(idx[s][:counted], order)
            np.testing.assert_array_equal(key[s][:counted], keys[order].astype(np.int64))
            assert (idx[s][counted:] == 0xFFFFFFFF).all() and (key[s][counted:] == 0xFFFFFFFF).all()
            assert tuple(cut[s]) == (L.TAKE_ALL, 0)


def test_broken_preconditions_are_refused_on_the_device():
    """No more than K keys counted without skip_cut, more than K keys below the take-all cut with it, a left-out key
    below the cut: the set's outputs are all 0xFFFFFFFF and the sets beside it are selected as usual."""
    rng = np.random.default_rng(11)
    K, n = 100, 1500
    good = rng.integers(0, 1 << 20, n).astype(np.uint32)
    few = np.full(n, 0xFFFFFFFF, np.uint32)
    few[:K] = np.arange(K)                                   # exactly K counted: the cut needs more
    low = good.copy()
    low[::3] = 5                                             # a left-out value that sorts before keys taken
    for form in L.FORMS:
        idx, key, cut = L.run_probe([good, few, good], K, 20, form)
        assert (idx[1] == 0xFFFFFFFF).all() and (key[1] == 0xFFFFFFFF).all() and (cut[1] == 0xFFFFFFFF).all()
        want = L.ref_select(good, K, L.counted_mask(good, 20))
        np.testing.assert_array_equal(idx[0], want)
        np.testing.assert_array_equal(idx[2], want)
        idx, key, cut = L.run_probe([few, good], K, 20, form, skip_cut=True)
        assert (idx[1] == 0xFFFFFFFF).all() and (cut[1] == 0xFFFFFFFF).all()
        np.testing.assert_array_equal(idx[0], np.arange(K))
        idx, key, cut = L.run_probe([low], K, 20, form, leave_out=5)
        assert (idx[0] == 0xFFFFFFFF).all() and (cut[0] == 0xFFFFFFFF).all()


def test_refusals():
    from paddle3d_amd.ops._common import lib, ptr

    dev = torch.device("cuda", 0)
    keys = torch.zeros(2 * 20000, dtype=torch.int32, device=dev)
    FILL = 0x5A5A5A5A
    out = torch.full((3, 2 * 1024), FILL, dtype=torch.int32, device=dev)
    null = C.c_void_p(0)
    fn = lib().pd3_selfcheck_block_topk

    def call(keys=ptr(keys), sets=2, n=2000, K=100, key_bits=30, form=0, leave_out=-1, skip=0, idx=ptr(out[0]),
             key=ptr(out[1]), cut=ptr(out[2])):
        return fn(keys, sets, n, K, key_bits, form, leave_out, skip, idx, key, cut, null)

    assert call() == 0
    torch.cuda.synchronize()
    assert (out[:2, :200] != FILL).all() and (out[:2, 200:] == FILL).all()
    assert (out[2, :4] != FILL).all() and (out[2, 4:] == FILL).all()
    out.fill_(FILL)
    for bad in (dict(keys=null), dict(idx=null), dict(key=null), dict(cut=null), dict(K=0), dict(K=1025), dict(K=-1),
                dict(key_bits=0), dict(key_bits=31), dict(n=0), dict(n=-5), dict(form=1, n=16385), dict(form=2),
                dict(form=-1), dict(sets=-1), dict(leave_out=1 << 32)):
        assert call(**bad) == -1, bad
    assert call(form=0, n=16385) == 0 and call(form=1, n=16384) == 0 and call(K=1024, n=1025) == 0
    out.fill_(FILL)
    torch.cuda.synchronize()
    assert call(sets=0) == 0                                  # nothing launched, nothing written
    assert call(sets=0, keys=null) == -1
    torch.cuda.synchronize()
    assert (out == FILL).all()


# ---- the call sites ----------------------------------------------------------------------------------------------------
CP_CFG = dict(voxel_size=[0.2, 0.2], point_cloud_range=[-51.2, -51.2],
              post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], down_ratio=4, nms_iou_threshold=0.2)
LABEL_OFFSETS = [0, 1, 3, 5, 6, 8]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", [c[0] for c in L.CP_CASES])
def test_centerpoint_call_site(oracle, name):
    """centerpoint_postprocess on its LDS path (cp_topk_kernel: key_bits from the threshold, the chunk compaction), six
    tasks of six kinds per call -- continuous and quantised scores, a tie cluster across the cut and a chunk border,
    exactly pre + 1 cells above the threshold, masked cells, all scores equal -- against the full sort and the oracle,
    bit for bit.  At a threshold <= 0 the masked cells' kKeyOut is counted (digit 1's last bin) and the cut lies inside
    the real keys; tests/test_topk_lattice_cpu.py::test_call_site_labels holds the labels."""
    from paddle3d_amd import synth
    from paddle3d_amd.ops import centerpoint_postprocess as cp

    hm, masked, pre, thr, bits, _ = L.cp_case(name)
    fh, fw = L.CP_HW
    tasks = synth.center_head_outputs(L._seed("cp-maps", name) % 1000, feat_h=fh, feat_w=fw, n_peaks=0)
    for t, task in enumerate(tasks):
        task["hm"][0, 0] = hm[t].reshape(fh, fw)
        task["hm"][0, 1:] = hm[t].reshape(fh, fw) - np.float32(8.0)      # class 0 is every cell's best class
        task["height"][0, 0][masked[t].reshape(fh, fw)] = np.float32(100.0)   # outside post_center_range
    lists = {k: [_cuda(t[k]) for t in tasks] for k in ("hm", "reg", "height", "dim", "vel", "rot")}

    def run(full_sort):
        bb, ss, ll, nn = cp.centerpoint_postprocess_device(
            lists["hm"], lists["reg"], lists["height"], lists["dim"], lists["vel"], lists["rot"], CP_CFG["voxel_size"],
            CP_CFG["point_cloud_range"], CP_CFG["post_center_range"], LABEL_OFFSETS * len(tasks), CP_CFG["down_ratio"],
            thr, CP_CFG["nms_iou_threshold"], pre, 500, True, full_sort=full_sort)
        k = int(nn.item())
        return bb[0, :k].cpu().numpy(), ss[0, :k].cpu().numpy(), ll[0, :k].cpu().numpy()

    b, s, l = run(False)
    b2, s2, l2 = run(True)
    rb, rs, rl = oracle.centerpoint_postprocess(
        tasks, CP_CFG["voxel_size"] + [8.0], CP_CFG["point_cloud_range"] + [0.0] * 4, CP_CFG["post_center_range"],
        LABEL_OFFSETS, CP_CFG["down_ratio"], thr, CP_CFG["nms_iou_threshold"], pre, 500, True)
    assert b.shape == b2.shape == rb.shape and b.shape[0] > 6 * 5, (b.shape, b2.shape, rb.shape)
    for got, full, want in ((l, l2, rl), (s, s2, rs), (b, b2, rb)):
        np.testing.assert_array_equal(got, full)
        np.testing.assert_array_equal(got.view(np.uint32) if got.dtype == np.float32 else got,
                                      want.view(np.uint32) if want.dtype == np.float32 else want)
    if thr > 0:
        assert (s > np.float32(thr)).all()


@pytest.mark.parametrize("name", list(L.DECODE_CASES))
def test_nms_free_decode_call_site(name):
    """nms_free_decode with Q * K = max_num + 1 candidates at max_num 1, 64, 65, 300 and 1024: continuous and quantised
    scores, the cut inside a cluster of equal logits, and fewer numbers than max_num so that the cut lies among the NaN
    keys -- against the restatement, bit for bit."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import bevformer_decoder_numpy as dn
    from oracle import pyoracle as O

    from paddle3d_amd.ops import bevformer_decoder as ops

    expf, atan2f = (lambda x: O.libm_eval(2, x)), (lambda y, x: O.libm_eval(4, y, x))
    cls, max_num = L.decode_logits(name)
    B, Q, K = cls.shape
    rng = np.random.default_rng(L._seed("decode-boxes", name))
    bbox = (rng.standard_normal((B, Q, 10)) * 0.5).astype(np.float32)
    post = [-8.0, -8.0, -2.5, 8.0, 8.0, 4.0]
    bbox[..., 0], bbox[..., 1], bbox[..., 4] = rng.uniform(-7, 7, (B, Q)), rng.uniform(-7, 7, (B, Q)), rng.uniform(-2, 3, (B, Q))
    want = dn.nms_free_decode(cls, bbox, post, max_num, None, False, expf, atan2f)
    got = ops.nms_free_decode(_cuda(cls), _cuda(bbox), post, max_num, None, False)
    nans = int(np.isnan(cls[0]).sum())
    assert want[3].tolist() == [min(max_num, Q * K - int(np.isnan(cls[b]).sum())) for b in range(B)], (want[3], nans)
    for a, w in zip(got, want[:4]):
        a = a.cpu().numpy()
        assert a.shape == w.shape and a.dtype == w.dtype, (a.shape, w.shape, a.dtype, w.dtype)
        np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                      w.view(np.uint32) if w.dtype == np.float32 else w)


@pytest.mark.parametrize("name", list(L.BD_CASES))
def test_bevdet_call_site(oracle, name):
    """BEVDet's get_bboxes (bd_select_decode_kernel: 30-bit keys from global memory, kBdKeyNan, block_topk_compact) with
    n = ncls * hw at K + 1 and at a multiple of 1024 -+ 1, NaN scores at the cut and saturated 1.0 scores tied across
    classes, against the restatement bit for bit (tests/test_bevdet_head_gpu.py's comparison)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import bevdet_head_numpy as bh

    from paddle3d_amd import bevdet_head

    ncls, h, w, K, _ = L.BD_CASES[name]
    heads = bh.head_maps([ncls], 2, h, w, seed=L._seed("bevdet-maps", name) % 10000, peaks=0)
    heads[0]["heatmap"] = L.bd_heatmap(name)
    coder = dict(bevdet_head.BEVDET4D_BBOX_CODER, max_num=K)
    cfg = dict(bevdet_head.BEVDET4D_TEST_CFG, nms_type="rotate", nms_thr=0.2, min_radius=1.0, nms_rescale_factor=[1.0],
               pre_max_size=1024, post_max_size=500)
    c = bevdet_head.CenterPointBBoxCoder(**coder)
    preds = [{k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in hd.items()} for hd in heads]
    got = [(b.cpu().numpy(), s.cpu().numpy(), l.cpu().numpy()) for b, s, l in bevdet_head.get_bboxes(preds, cfg, c, [ncls])]
    want = bh.get_bboxes(oracle, heads, cfg, coder, [ncls])
    assert len(got) == len(want) == 2
    for (b, s, l), (rb, rs, rl) in zip(got, want):
        assert b.shape == rb.shape and len(s) > 3, (b.shape, rb.shape)
        np.testing.assert_array_equal(l, rl)
        np.testing.assert_array_equal(s.view(np.uint32), rs.view(np.uint32))
        np.testing.assert_array_equal(b.view(np.uint32), rb.view(np.uint32))
