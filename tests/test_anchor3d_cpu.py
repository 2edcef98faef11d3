"""BEVFusion's Anchor3DHead on the CPU: the NumPy restatement of the device entry points (tests/golden/anchor3d_numpy.py)
against what the reference's own Python computed (tests/golden/python_anchor3d.npz), the anchor table, the module's
plain-torch fall-back against the same file, the weight packers, the module's state-dict keys,
the refusal statuses and the maker's conditions on the committed inputs.

Bounds: the ones the maker stored, 4 x the largest error of the reference's own fp32 run against its fp64 run (one fp32
ulp of the largest output as a floor); values are compared with the fp64 run.  Labels, counts and the row order are
compared exactly: the maker keeps every score and IoU away from a decision."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import anchor3d_numpy as an  # noqa: E402
import make_anchor3d_golden as mk  # noqa: E402

F32 = np.float32
TAGS = an.TAGS


@pytest.fixture(scope="module")
def golden():
    return mk.load()


def check_frame(golden, tag, b, boxes, scores, labels):
    """One frame's rows against the golden: labels and row order exactly, values within the stored bounds."""
    want_l = golden[f"{tag}_labels_{b}"]
    assert len(scores) == len(want_l) and np.array_equal(np.asarray(labels, np.int64), want_l.astype(np.int64)), (tag, b)
    for name, got in (("bboxes", boxes), ("scores", scores)):
        want, bd = golden[f"{tag}_{name}64_{b}"], float(golden[f"{tag}_{name}_{b}_bound"])
        err = float(np.abs(np.asarray(got, np.float64) - want).max()) if want.size else 0.0
        print(f"{tag} frame {b} {name}: err {err:.3g} bound {bd:.3g} ref_err {float(golden[f'{tag}_{name}_{b}_ref_err']):.3g}")
        assert err <= bd, (tag, b, name, err, bd)


def check_padded(golden, tag, padded):
    boxes, scores, labels, counts = (np.asarray(t) for t in padded)
    for b in range(an.CASES[tag]["B"]):
        n = int(counts[b])
        check_frame(golden, tag, b, boxes[b, :n], scores[b, :n], labels[b, :n])
        assert not boxes[b, n:].any() and not scores[b, n:].any() and not labels[b, n:].any()


def build_head(tag):
    from paddle3d_amd import bevfusion_head as bh
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    c = an.CASES[tag]
    head = bh.Anchor3DHead(
        num_classes=c["num_classes"], in_channels=c["C"], feat_channels=c["C"],
        anchor_generator=dict(ranges=c["ranges"], sizes=c["sizes"], scales=[1], rotations=c["rotations"],
                              custom_values=c["custom_values"], reshape_out=True),
        bbox_coder=dict(code_size=c["code_size"]), dir_offset=c["dir_offset"], dir_limit_offset=c["dir_limit_offset"],
        test_cfg=dict(c["test_cfg"]))
    assert load_paddle_state_dict(head, an.golden_state(tag)) == []
    return head.eval()


_restated = {}


def restated(tag):
    """The restatement of the lazy entry point on the golden inputs, once per case (shared with the GPU tests)."""
    if tag not in _restated:
        _restated[tag] = an.head_forward(an.golden_inputs(tag), an.golden_state(tag), mk.anchors_of(tag), an.cfg_of(tag))
    return _restated[tag]


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_against_reference(golden, tag):
    check_padded(golden, tag, restated(tag))
    counts = restated(tag)[3]
    assert (counts == an.CASES[tag]["test_cfg"]["max_num"]).any()


@pytest.mark.parametrize("tag", TAGS)
def test_anchor_grid_is_the_reference_generator(golden, tag):
    got = mk.anchors_of(tag)
    want = golden[f"{tag}_anchors"]
    assert got.dtype == want.dtype == F32 and got.shape == want.shape and np.array_equal(got, want)
    c = an.CASES[tag]
    ns, nr = len(c["sizes"]), len(c["rotations"])
    row = ((2 * c["W"] + 3) * ns + 1) * nr + 1  # y = 2, x = 3, size 1, rotation 1
    assert np.allclose(got[row, 3:6], c["sizes"][1]) and got[row, 6] == F32(c["rotations"][1])
    assert not got[:, 7:].any() and got.shape[1] == 7 + len(c["custom_values"])


@pytest.mark.parametrize("tag", TAGS)
def test_torch_fallback_against_reference(golden, monkeypatch, tag):
    from oracle import pyoracle as O
    from paddle3d_amd import bevfusion_head as bh

    def nms_gpu(boxes, thresh):
        keep = O.nms(boxes.numpy(), float(thresh))
        return torch.from_numpy(keep), torch.tensor([len(keep)], dtype=torch.int32)

    monkeypatch.setattr(bh._nms, "nms_gpu", nms_gpu)
    head = build_head(tag)
    feats = [torch.from_numpy(an.golden_inputs(tag))]
    metas = [{}] * an.CASES[tag]["B"]
    with torch.no_grad():
        maps = head(feats)
        assert [tuple(m[0].shape[1:2]) for m in maps] == [(head.num_anchors * w,) for w in (head.num_classes, head.box_code_size, 2)]
        res = head.get_bboxes(*maps, metas)
        lazy = head.forward_get_bboxes(feats, metas)  # a CPU tensor: the fall-back again
        padded = head.forward_get_bboxes(feats, metas, return_padded=True)
    for b, (bx, sc, lb) in enumerate(res):
        assert lb.dtype == torch.int64
        check_frame(golden, tag, b, bx.numpy(), sc.numpy(), lb.numpy())
        assert torch.equal(bx, lazy[b][0]) and torch.equal(sc, lazy[b][1])
    check_padded(golden, tag, [t.numpy() for t in padded])


def test_packers_round_trip():
    from paddle3d_amd.ops import anchor3d_head as ops

    rng = np.random.default_rng(3)
    for nc, A, C in ((10, 14, 16), (3, 6, 32), (1, 1, 16), (16, 32, 48), (7, 28, 16), (13, 15, 64)):
        w = torch.from_numpy(rng.standard_normal((A * nc, C, 1, 1)).astype(F32))
        p = ops.pack_cls_weight(w, nc)
        chunks, tiles = ops._chunks(A, nc)
        assert tuple(p.shape) == (tiles, C // 4, 64) and p.is_contiguous()
        assert torch.equal(ops.unpack_cls_weight(p, A, nc), w.reshape(A * nc, C))
        assert all(na * nc <= ops.CHUNK_ROWS for _, na, _ in chunks) and sum(na for _, na, _ in chunks) == A
        # lane (m, k) of [tile][s] is w[row 16 tile + m][4 s + k] inside the first chunk
        assert p[0, C // 4 - 1, 3 * 16 + 0] == w[0, C - 1, 0, 0]
        if A * nc > 17 and chunks[0][1] * nc > 17:
            assert p[1, 0, 2 * 16 + 1] == w[17, 2, 0, 0]
    assert len(ops._chunks(32, 16)[0]) == 3 and len(ops._chunks(14, 10)[0]) == 1
    with pytest.raises(ValueError):
        ops.pack_cls_weight(torch.zeros(7, 16), 3)


def test_module_takes_the_reference_state_dict():
    for tag in TAGS:
        head = build_head(tag)
        assert sorted(head.state_dict()) == sorted(an.golden_state(tag)) == [
            "conv_cls.bias", "conv_cls.weight", "conv_dir_cls.bias", "conv_dir_cls.weight", "conv_reg.bias",
            "conv_reg.weight"]
        c = an.CASES[tag]
        assert head.num_anchors == an.num_anchors(tag) and head.box_code_size == c["code_size"]
        assert tuple(head.conv_cls.weight.shape) == (head.num_anchors * c["num_classes"], c["C"], 1, 1)


def test_predicate():
    from paddle3d_amd.ops import anchor3d_head as ops

    ok = dict(channels=384, num_classes=10, num_anchors=14, code_size=9, nms_pre=1000, max_num=500, total_anchors=560000)
    assert ops.anchor3d_supported(**ok) and ops.anchor3d_supported(**dict(ok, channels=None))
    for bad in (dict(channels=8), dict(channels=40), dict(channels=528), dict(num_classes=0), dict(num_classes=17),
                dict(num_anchors=0), dict(num_anchors=33), dict(code_size=6), dict(code_size=17), dict(nms_pre=1025),
                dict(nms_pre=0), dict(nms_pre=-1), dict(max_num=0), dict(max_num=1025), dict(use_sigmoid_cls=False),
                dict(use_direction_classifier=False)):
        assert not ops.anchor3d_supported(**dict(ok, **bad)), bad
    # no pre-selection is taken while every anchor fits the candidate list
    assert ops.anchor3d_supported(**dict(ok, nms_pre=-1, total_anchors=1024))
    assert not ops.anchor3d_supported(**dict(ok, nms_pre=-1, total_anchors=1025))
    assert ops.anchor3d_supported(**dict(ok, nms_pre=2000, total_anchors=1000))


def test_refusals_need_no_gpu():
    from paddle3d_amd import _lib, build

    build.build()
    L = _lib.lib()
    buf = np.zeros(64, F32)
    p = _lib.C.c_void_p(buf.ctypes.data)
    f = _lib.C.c_float

    def fwd(B=1, C=384, H=20, W=20, A=14, nc=10, cs=9, pre=1000, mx=500, ptr=None, ws=0):
        return L.pd3_anchor3d_head_forward(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, B, C, H, W, A, nc, cs, pre, mx, f(0.1),
                                           f(0.2), f(0.0), f(1.0), ptr, ptr, ptr, ptr, ptr, ws, None)

    def maps(B=1, H=20, W=20, A=14, nc=10, cs=9, pre=1000, mx=500, ptr=None, ws=0):
        return L.pd3_anchor3d_get_bboxes(ptr, ptr, ptr, ptr, B, H, W, A, nc, cs, pre, mx, f(0.1), f(0.2), f(0.0), f(1.0),
                                         ptr, ptr, ptr, ptr, ptr, ws, None)

    assert fwd() == -1 and maps() == -1  # a supported shape with null pointers
    assert fwd(ptr=p) == -2 and maps(ptr=p) == -2  # real pointers, no workspace: refused before any launch
    assert fwd(B=0) == 0 and maps(B=0) == 0
    for bad in (dict(C=8), dict(C=40), dict(C=528), dict(nc=17), dict(A=33), dict(cs=6), dict(cs=17), dict(pre=1025),
                dict(pre=-1), dict(mx=1025)):
        assert fwd(**bad) == -3, bad
        if "C" not in bad:
            assert maps(**bad) == -3, bad
    assert fwd(C=0) == -1 and fwd(H=0) == -1 and fwd(mx=0) == -1 and fwd(nc=0) == -1 and maps(A=0) == -1
    assert fwd(H=5, W=5, A=2, pre=-1) == -1  # 50 anchors, all taken
    q = L.pd3_anchor3d_head_workspace
    assert q(1, 200, 200, 14, 10, 9, 1000) > 4 * 560000 and q(4, 200, 200, 14, 10, 9, 1000) > 3 * q(1, 200, 200, 14, 10, 9, 1000)
    assert q(1, 200, 200, 14, 10, 9, 2000) == 0 and q(1, 200, 200, 14, 17, 9, 1000) == 0 and q(0, 20, 20, 14, 10, 9, 100) == 0
    assert q(1, 5, 7, 6, 3, 7, 1000) == q(1, 5, 7, 6, 3, 7, 210) == q(1, 5, 7, 6, 3, 7, -1) > 0


@pytest.mark.parametrize("tag", TAGS)
def test_maker_conditions_hold_on_the_committed_file(golden, tag):
    c = an.CASES[tag]
    assert os.path.getsize(mk.OUT) < 100_000
    seen = mk.check_case(tag)
    print(tag, seen)
    assert c["empty_class"] in seen["empty_classes"] and seen["over_max"] >= 1
    assert max(seen["candidates"]) > (64 if tag == "nus" else 32)  # more than one NMS tile in the nuScenes-like case
    assert not set(golden) & {"feat", "feats"} and all(k.startswith(tuple(t + "_" for t in TAGS)) for k in golden)
    for b in range(c["B"]):
        assert golden[f"{tag}_bboxes_{b}"].shape[1] == c["code_size"]
        assert float(golden[f"{tag}_bboxes_{b}_bound"]) >= 4 * float(golden[f"{tag}_bboxes_{b}_ref_err"])
