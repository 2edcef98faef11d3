"""BEVFormer's decoder, head and NMS-free decode on the CPU: the NumPy restatement of the three entry points
(tests/golden/bevformer_decoder_numpy.py) against what the reference's own Python computed
(tests/golden/python_bevformer_decoder.npz) -- the attention outputs, and, with the restatement standing in for the
device ops inside the modules of paddle3d_amd.bevformer_head, the layer, the decoder's states and reference points and
the head's outputs; the restated decode against get_bboxes; the threshold loop against a transcription; the modules'
state-dict keys; the refusal statuses; the maker's conditions on the
committed file.

Bounds: the ones the maker stored, 4 x the largest error of the reference's own fp32 run against its fp64 run (one fp32
ulp of the largest output as a floor).  Labels, rows and counts of the decode are compared exactly: the maker keeps
every score, threshold and centre further from a decision than those bounds."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import bevformer_decoder_numpy as dn  # noqa: E402
import make_bevformer_decoder_golden as mk  # noqa: E402

F32 = np.float32
TAGS = mk.TAGS
E, M = mk.EMBED, mk.HEADS


@pytest.fixture(scope="module")
def golden():
    return mk.load()


@pytest.fixture(scope="module")
def expf():
    from oracle import pyoracle as O

    return lambda x: O.libm_eval(2, x)


@pytest.fixture(scope="module")
def atan2f():
    from oracle import pyoracle as O

    return lambda y, x: O.libm_eval(4, y, x)


def _linear(st, key, x):
    """Paddle's Linear on the CPU in float32: x W + b with W [in, out]."""
    return (torch.from_numpy(np.ascontiguousarray(x)) @ torch.from_numpy(st[key + ".weight"]) +
            torch.from_numpy(st[key + ".bias"])).numpy()


def queries(tag):
    """(query_pos, query) [B, Q, E] of the decoder's first layer."""
    c, st = mk.CASES[tag], mk.state(tag)
    qe = st["query_embedding.weight"]
    return tuple(np.ascontiguousarray(np.broadcast_to(t[None], (c["B"], c["Q"], E))) for t in (qe[:, :E], qe[:, E:]))


def init_reference(tag):
    """sigmoid(reference_points(query_pos)) [B, Q, 3] in float32."""
    pos, _ = queries(tag)
    return torch.sigmoid(torch.from_numpy(_linear(mk.state(tag), "transformer.reference_points", pos))).numpy()


def mha_inputs(tag, layer=0):
    """The projected (q, k, v) [B, Q, E] of the layer's self-attention on the decoder's own queries."""
    st = mk.state(tag)
    pos, query = queries(tag)
    k = f"transformer.decoder.layers.{layer}.attentions.0.attn."
    return (_linear(st, k + "q_proj", query + pos), _linear(st, k + "k_proj", query + pos), _linear(st, k + "v_proj", query))


def ca_inputs(tag, layer=0):
    """(value [B, S, M, C], offsets [B, Q, M, 1, P, 2], logits [B, Q, M, P], ref [B, Q, 1, 2], shapes, starts)."""
    c, st = mk.CASES[tag], mk.state(tag)
    pos, query = queries(tag)
    k = f"transformer.decoder.layers.{layer}.attentions.1."
    B, Q, P = c["B"], c["Q"], mk.POINTS
    value = _linear(st, k + "value_proj", mk.inputs(tag)["bev_embed"]).reshape(B, -1, M, E // M)
    off = _linear(st, k + "sampling_offsets", query + pos).reshape(B, Q, M, 1, P, 2)
    logits = _linear(st, k + "attention_weights", query + pos).reshape(B, Q, M, P)
    sh, lsi, _ = dn.md.level_layout([c["bev"]])
    return value, off, logits, np.ascontiguousarray(init_reference(tag)[:, :, None, :2]), sh, lsi


def check_result(g, tag, name, got):
    want, bound = g[f"{tag}_{name}"], float(g[f"{tag}_{name}_bound"])
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == F32, (tag, name, got.shape, want.shape, got.dtype)
    e = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{tag} {name} err {e:.3e} bound {bound:.3e} (reference's own {float(g[f'{tag}_{name}_ref_err']):.3e})")
    assert e <= bound, (tag, name, e, bound)


def check_decode(g, tag, name, boxes, scores, labels, count, rows=None):
    """Labels, (rows) and counts equal, boxes and scores within the stored bounds, the tail zeros / -1."""
    boxes, scores, labels, count = (np.asarray(t) for t in (boxes, scores, labels, count))
    pre = f"{tag}_{name}_"
    assert labels.dtype == np.int32 and count.dtype == np.int32 and boxes.dtype == F32 and scores.dtype == F32
    assert np.array_equal(count, g[pre + "count"]), (tag, name, count, g[pre + "count"])
    assert np.array_equal(labels, g[pre + "labels"]), (tag, name)
    if rows is not None:
        assert np.array_equal(rows, g[pre + "rows"]), (tag, name)
    for k, got in (("boxes", boxes), ("scores", scores)):
        e, bound = float(np.abs(got.astype(np.float64) - g[pre + k]).max()), float(g[pre + k + "_bound"])
        print(f"{tag} {name} {k} err {e:.3e} bound {bound:.3e}")
        assert got.shape == g[pre + k].shape and e <= bound, (tag, name, k, e, bound)
    for b, n in enumerate(count):
        assert not boxes[b, n:].any() and not scores[b, n:].any() and (labels[b, n:] == -1).all()


def decode_case(g, tag, name):
    """(cls, bbox) float32 the decode `name` of the case runs on."""
    if name == "dec":
        return mk.decode_inputs(tag)
    return g[f"{tag}_all_cls_scores"][-1].astype(F32), g[f"{tag}_all_bbox_preds"][-1].astype(F32)


_cache = {}


def restated(tag, expf):
    """(mha, dec_ca) of the restatement on the first layer's inputs, once per case."""
    if tag not in _cache:
        _cache[tag] = (dn.mha(*mha_inputs(tag), M, expf), dn.dec_ca(*ca_inputs(tag), expf))
    return _cache[tag]


def restated_decode(g, tag, name, expf, atan2f):
    key = (tag, name)
    if key not in _cache:
        c = mk.CASES[tag]
        _cache[key] = dn.nms_free_decode(*decode_case(g, tag, name), c["post"], c["max_num"], c["thr"], True, expf, atan2f)
    return _cache[key]


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restated_attention_against_reference(golden, expf, tag):
    mha, ca = restated(tag, expf)
    check_result(golden, tag, "mha_sample", mha)
    check_result(golden, tag, "ca_sample", ca)


def patch_ops(monkeypatch, expf, atan2f):
    """The restatement in place of the three device ops inside paddle3d_amd.bevformer_head (CPU tensors in and out)."""
    from paddle3d_amd import bevformer_head as bh

    n = lambda t: t.detach().cpu().numpy()  # noqa: E731
    monkeypatch.setattr(bh._ops, "multihead_attention",
                        lambda q, k, v, heads: torch.from_numpy(dn.mha(n(q), n(k), n(v), heads, expf)))
    monkeypatch.setattr(bh._ops, "decoder_cross_attention_sample",
                        lambda v, o, l, r, sh, lsi: torch.from_numpy(dn.dec_ca(n(v), n(o), n(l), n(r), n(sh), n(lsi), expf)))


def build_head(tag, fused=True):
    from paddle3d_amd import bevformer_head as bh
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    head = bh.BEVFormerHead(**mk.head_cfg(tag, fused))
    assert load_paddle_state_dict(head, mk.state(tag)) == []
    return head.eval()


def first_layer_outputs(head, tag, dev="cpu"):
    """{mha_out, ca_out, layer_out} of the decoder's first layer on the decoder's own inputs ([Q, B, E])."""
    c = mk.CASES[tag]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    pos, query = (t(a.transpose(1, 0, 2)) for a in queries(tag))
    value = t(mk.inputs(tag)["bev_embed"].transpose(1, 0, 2))
    ref = t(init_reference(tag)[:, :, None, :2])
    sh = torch.tensor([list(c["bev"])], dtype=torch.int64).to(dev)
    lsi = torch.zeros(1, dtype=torch.int64).to(dev)
    layer = head.transformer.decoder.layers[0]
    kw = dict(reference_points=ref, spatial_shapes=sh, level_start_index=lsi)
    with torch.no_grad():
        return dict(mha_out=layer.attentions[0](query, query, query, None, query_pos=pos, key_pos=pos),
                    ca_out=layer.attentions[1](query, None, value, None, query_pos=pos, **kw),
                    layer_out=layer(query, None, value, pos, **kw))


def model_outputs(head, tag, dev="cpu"):
    """{dec_states, dec_refs, init_ref, all_cls_scores, all_bbox_preds} of the head on the case's BEV map."""
    bev = torch.from_numpy(mk.inputs(tag)["bev_embed"]).to(dev)
    with torch.no_grad():
        _, states, init_ref, refs = head.transformer.decode(bev, head.query_embedding.weight, head.bev_h, head.bev_w,
                                                            reg_branches=head.reg_branches)
        outs = head.forward_from_bev(bev)
    return dict(dec_states=states, dec_refs=refs, init_ref=init_ref, all_cls_scores=outs["all_cls_scores"],
                all_bbox_preds=outs["all_bbox_preds"]), outs


@pytest.mark.parametrize("tag", TAGS)
def test_modules_on_the_restatement_against_reference(golden, expf, atan2f, monkeypatch, tag):
    patch_ops(monkeypatch, expf, atan2f)
    head = build_head(tag)
    if tag in ("a", "b"):
        for name, got in first_layer_outputs(head, tag).items():
            check_result(golden, tag, name, got.numpy())
    out, _ = model_outputs(head, tag)
    for name in mk.MODEL:
        check_result(golden, tag, name, out[name].numpy())


@pytest.mark.parametrize("tag,name", [(t, n) for t in TAGS for n in mk.DECODES[t]])
def test_restated_decode_against_reference(golden, expf, atan2f, tag, name):
    boxes, scores, labels, count, rows = restated_decode(golden, tag, name, expf, atan2f)
    check_decode(golden, tag, name, boxes, scores, labels, count, rows)


def test_torch_decode_agrees_with_the_restatement(golden, expf, atan2f):
    """NMSFreeCoder's unfused route (torch, no host synchronisation) selects what the restatement selects."""
    from paddle3d_amd import bevformer_head as bh

    for tag in TAGS:
        c = mk.CASES[tag]
        coder = bh.NMSFreeCoder(mk.PC_RANGE, post_center_range=c["post"], max_num=c["max_num"], score_threshold=c["thr"],
                                num_classes=c["K"], fused=False)
        cls, bbox = (torch.from_numpy(a)[None] for a in decode_case(golden, tag, "dec"))
        got = coder.decode(dict(all_cls_scores=cls, all_bbox_preds=bbox), bottom_center=True)
        check_decode(golden, tag, "dec", *(t.numpy() for t in got))
        lst = coder.to_list(*got)
        assert [len(d["scores"]) for d in lst] == golden[f"{tag}_dec_count"].tolist() and lst[0]["labels"].dtype == torch.int64


def _loop_transcription(scores, score_threshold):
    """box_coder.py:158-166 on a descending float32 score vector -> the boolean mask."""
    thresh_mask = scores > F32(score_threshold)
    tmp_score = score_threshold
    while thresh_mask.sum() == 0:
        tmp_score *= 0.9
        if tmp_score < 0.01:
            thresh_mask = scores > -1
            break
        thresh_mask = scores >= F32(tmp_score)
    return thresh_mask


@pytest.mark.parametrize("top", [0.5, 0.29, 0.011, 0.0099, 0.0])
@pytest.mark.parametrize("thr", [0.3, 0.05, 0.009])
def test_threshold_loop_against_transcription(top, thr):
    from paddle3d_amd.bevformer_head import threshold_steps

    rng = np.random.default_rng(int(top * 1e4))
    scores = np.sort(np.concatenate([[top], rng.uniform(0, 1, 40) * top]).astype(F32))[::-1]
    want = _loop_transcription(scores, thr)
    mode, cur = dn.threshold_test(scores[0], thr)
    got = scores > cur if mode == 0 else scores >= cur if mode == 1 else np.ones_like(want)
    assert np.array_equal(got, want), (top, thr, mode, cur)
    assert want.any()
    steps = threshold_steps(thr)  # the unfused coder's table of the same loop
    if mode == 1:
        assert F32(steps[[F32(t) <= scores[0] for t in steps].index(True)]) == cur
    assert threshold_steps(thr) == mk.threshold_steps(thr)[1:]


def test_modules_take_the_reference_state_dict(golden):
    from paddle3d_amd import bevformer_head as bh
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    keys = [str(k) for k in golden["state_keys"]]
    for tag in TAGS:
        st = mk.state(tag)
        assert sorted(st) == keys
        head = build_head(tag)
        own = head.state_dict()
        assert sorted(own) == keys
        k = "transformer.decoder.layers.1.attentions.0.attn.q_proj.weight"
        assert torch.equal(own[k], torch.from_numpy(st[k]).t())  # Paddle's [in, out] placed as torch's [out, in]
        assert torch.equal(own["query_embedding.weight"], torch.from_numpy(st["query_embedding.weight"]))
        sub = {k[len("transformer.decoder."):]: v for k, v in st.items() if k.startswith("transformer.decoder.")}
        assert load_paddle_state_dict(bh.DetectionTransformerDecoder(**_decoder_cfg(tag)), sub) == []  # a part on its own
    with pytest.raises(NotImplementedError):
        head.transformer.get_bev_features()
    # a layer's `fused` reaches the cross-attention; the self-attention kernel is asked for in its own cfg
    cfg = _decoder_cfg("a")
    for a in cfg["transformerlayers"]["attn_cfgs"]:
        a.pop("fused", None)
    att = bh.DetectionTransformerDecoder(**cfg).layers[0].attentions
    assert (att[0].fused, att[1].fused) == (False, True)
    att = bh.DetectionTransformerDecoder(**cfg, fused=False).layers[0].attentions
    assert (att[0].fused, att[1].fused) == (False, False)
    assert all(a.fused for a in head.transformer.decoder.layers[1].attentions)


def _decoder_cfg(tag):
    cfg = dict(mk.head_cfg(tag)["transformer"]["decoder"])
    cfg.pop("type_name")
    return cfg


def test_refusals_need_no_gpu():
    from paddle3d_amd import _lib, build
    from paddle3d_amd.ops import bevformer_decoder as ops

    build.build()
    L = _lib.lib()
    mha = lambda Nq, Nk, d, B=1, p=None: L.pd3_mha_forward(p, p, p, B, Nq, Nk, 2, d, 0.25, p, None)  # noqa: E731
    for Nk, d in ((10, 8), (10, 24), (10, 144), (2049, 32), (10, 40)):
        assert mha(5, Nk, d) == -3 and not ops.mha_supported(d, Nk), (Nk, d)
    for d in (16, 32, 64, 128):
        assert ops.mha_supported(d, 2048) and mha(5, 2048, d) == -1  # a supported shape with null pointers
    assert mha(5, 0, 32) == -1 and mha(5, -1, 32) == -1 and mha(-1, 10, 32) == -1
    assert mha(0, 10, 32) == 0 and mha(5, 10, 32, B=0) == 0  # nothing to do is no error
    aligned = np.zeros(64, F32)
    odd = _lib.C.c_void_p(aligned.ctypes.data + 4)
    assert L.pd3_mha_forward(odd, odd, odd, 1, 1, 1, 1, 16, 0.25, odd, None) == -3
    ca = lambda C, Lv, P, Lr, B=1: L.pd3_bevformer_dec_ca(None, None, None, None, None, None, B, 10, 2, C, Lv, 5, P, Lr,  # noqa: E731
                                                          None, None)
    for args in ((30, 1, 4, 1), (32, 1, 33, 1), (32, 9, 4, 9), (2, 1, 4, 1)):
        assert ca(*args) == -3 and not ops.dec_ca_supported(*args[:3]), args
    assert ca(32, 4, 8, 4) == -1 and ca(32, 4, 8, 1) == -1 and ca(32, 4, 8, 2) == -1 and ca(32, 0, 4, 1) == -1
    assert ca(32, 1, 4, 1, B=0) == 0
    rng = np.asarray(mk.CASES["a"]["post"], F32)
    dec = lambda Q, K, code, n, thr=-1.0, B=1, r=rng.ctypes.data: L.pd3_nms_free_decode(  # noqa: E731
        None, None, r, B, Q, K, code, n, thr, 0, None, None, None, None, None)
    assert dec(10, 10, 10, 101) == -1 and dec(10, 10, 9, 10) == -1 and dec(10, 10, 10, 0) == -1
    assert dec(10, 10, 10, 10, r=None) == -1 and dec(10, 10, 10, 10, thr=float("inf")) == -1
    assert dec(10, 10, 10, 10, thr=float("nan")) == -1
    assert dec(200, 10, 10, 1025) == -3 and dec(200, 10, 8, 1024) == -1 and dec(200, 10, 8, 1024, B=0) == 0


@pytest.mark.parametrize("tag", TAGS)
def test_maker_conditions_hold_on_the_committed_file(golden, tag):
    c = mk.CASES[tag]
    assert os.path.getsize(mk.OUT) < 600_000
    for name in mk.DECODES[tag]:
        print(tag, name, mk.check_selection(golden, tag, name))
        assert golden[f"{tag}_{name}_boxes"].shape == (c["B"], c["max_num"], c["code"] - 1)
    for name, shape in (("dec_states", (mk.LAYERS, c["Q"], c["B"], E)), ("dec_refs", (mk.LAYERS, c["B"], c["Q"], 3)),
                        ("all_cls_scores", (mk.LAYERS, c["B"], c["Q"], c["K"])),
                        ("all_bbox_preds", (mk.LAYERS, c["B"], c["Q"], c["code"]))):
        assert golden[f"{tag}_{name}"].shape == shape
    count = golden[f"{tag}_dec_count"]
    if tag == "b":
        assert c["max_num"] == c["Q"] * c["K"] and 0 < count[0] < c["max_num"]
    if tag == "c":  # frame 0 passes the threshold as given, frame 1 only after the loop lowered it
        steps, top = mk.threshold_steps(c["thr"]), golden["c_dec_all_scores"].max(1)
        assert top[0] > steps[0] and 0.01 < top[1] < steps[1] and 0 < count[1] < c["max_num"]
        kept = golden["c_dec_scores"][1, :count[1]]
        first = next(t for t in steps[1:] if top[1] >= t)
        assert kept.min() >= first and (np.sort(golden["c_dec_all_scores"][1])[::-1][:c["max_num"]] >= first).sum() >= count[1]
