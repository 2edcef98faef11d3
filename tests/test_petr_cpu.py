"""PETR / PETRv2's head on the CPU: the NumPy restatement of the two entry points (tests/golden/petr_numpy.py) against
what the reference's own Python computed (tests/golden/python_petr.npz) -- the coordinates, coords_mask, the streamed
attention's output --, the mask semantics of the restatement, the modules of paddle3d_amd.petr_head with fused=False
and with the restatement standing in for the device ops, the modules' state-dict keys,
the refusal statuses and the maker's conditions on the committed file.

Bounds: the ones the maker stored, 4 x the largest error of the reference's own fp32 run against its fp64 run (one fp32
ulp of the largest output as a floor).  coords_mask and the decode's labels, rows and counts are compared exactly: the
maker keeps every normalised coordinate, score and centre further from a decision than those bounds."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import make_petr_golden as mk  # noqa: E402
import petr_numpy as pn  # noqa: E402
from test_bevformer_decoder_cpu import check_decode, check_result  # noqa: E402

F32 = np.float32
TAGS = mk.TAGS
E, M = mk.EMBED, mk.HEADS
H, W = mk.FEAT


@pytest.fixture(scope="module")
def golden():
    return mk.load()


@pytest.fixture(scope="module")
def expf():
    from oracle import pyoracle as O

    return lambda x: O.libm_eval(2, np.ascontiguousarray(x, F32).reshape(-1))


def _linear(st, key, x):
    """Paddle's Linear on the CPU in float32: x W + b with W [in, out]."""
    return (torch.from_numpy(np.ascontiguousarray(x)) @ torch.from_numpy(st[key + ".weight"]) +
            torch.from_numpy(st[key + ".bias"])).numpy()


def build_head(tag, fused=True):
    from paddle3d_amd import petr_head as ph
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    head = ph.PETRHead(**mk.head_cfg(tag, fused))
    assert load_paddle_state_dict(head, mk.state(tag)) == []
    return head.eval()


def token_masks(tag):
    """bool [B, N, H, W]: the tokens outside the cameras' images, as PETRHead.forward derives them."""
    from paddle3d_amd.petr_head import PETRHead

    c = mk.CASES[tag]
    return PETRHead._build_masks(c["B"], c["N"], mk.PAD, mk.img_shapes(tag), mk.FEAT, "cpu").numpy()


def coords_args(tag):
    c = mk.CASES[tag]
    return (mk.inputs(tag)["img2lidars"], H, W, mk.D, mk.PAD[0], mk.PAD[1], c["depth_start"], c["position_range"], c["LID"])


def ca_inputs(tag):
    """The projected (q, k, v) [B, ., E] of the first layer's cross-attention on the seeded inputs, and the key mask."""
    st, ai = mk.state(tag), mk.attn_inputs(tag)
    k = "transformer.decoder.layers.0.attentions.1.attn."
    return (_linear(st, k + "q_proj", ai["query"] + ai["query_pos"]), _linear(st, k + "k_proj", ai["memory"] + ai["key_pos"]),
            _linear(st, k + "v_proj", ai["memory"]), ai["mask"][:, 0])


_cache = {}


def restated(tag, expf):
    """(coords, coords_mask, normalised, ca_core) of the restatement, once per case."""
    if tag not in _cache:
        tm = token_masks(tag)
        ratio, mask, norm = pn.coords3d_ratio(*coords_args(tag), token_mask=tm)
        with np.errstate(all="ignore"):
            coords = np.log(ratio.astype(np.float64)).astype(F32)
        q, k, v, km = ca_inputs(tag)
        _cache[tag] = (coords, mask, norm, ratio, pn.mha_stream(q, k, v, M, expf, km))
    return _cache[tag]


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_against_reference(golden, expf, tag):
    c = mk.CASES[tag]
    coords, mask, norm, _, core = restated(tag, expf)
    check_result(golden, tag, "coords_norm", norm)
    check_result(golden, tag, "coords3d", coords)
    assert np.array_equal(mask.reshape(c["B"], c["N"], H, W), golden[f"{tag}_coords_mask"])
    if tag != "c":
        check_result(golden, tag, "ca_core", core)


def test_mask_semantics_of_the_restatement(expf):
    rng = np.random.default_rng(5)
    B, Nq, Nk, d = 2, 7, 45, 16
    q, k, v = (rng.standard_normal((B, n, M * d)).astype(F32) for n in (Nq, Nk, Nk))
    mask = rng.random((B, Nk)) < 0.3
    mask[1] = True  # every key of frame 1
    out = pn.mha_stream(q, k, v, M, expf, mask)
    assert np.isfinite(out).all()
    # a padded key is a key whose score has the fp32 value -1e9f added: the float64 softmax over those fp32 sums
    qh, kh, vh = (t.reshape(B, -1, M, d).transpose(0, 2, 1, 3) for t in (q, k, v))
    s = np.einsum("bmqc,bmkc->bmqk", (qh * F32(0.25)).astype(np.float64), kh.astype(np.float64)).astype(F32)
    t = np.where(mask[:, None, None, :], (s + F32(-1e9)).astype(F32), s).astype(np.float64)
    e = np.exp(t - t.max(-1, keepdims=True))
    want = np.einsum("bmqk,bmkc->bmqc", e / e.sum(-1, keepdims=True), vh.astype(np.float64))
    want = want.transpose(0, 2, 1, 3).reshape(B, Nq, M * d)
    assert np.abs(out - want).max() < 2e-5  # scores differ by a few ulp of ~4; frame 1's sums are multiples of 64
    # with a key unpadded and moderate scores a padded key's weight is exactly 0: its value cannot reach the output
    v2 = v.copy()
    v2[0][mask[0]] = rng.standard_normal((int(mask[0].sum()), M * d)).astype(F32) * F32(1e30)
    assert np.array_equal(pn.mha_stream(q[:1], k[:1], v2[:1], M, expf, mask[:1]), out[:1])
    # no mask and an all-false mask are the same
    assert np.array_equal(pn.mha_stream(q, k, v, M, expf, None), pn.mha_stream(q, k, v, M, expf, np.zeros_like(mask)))


def patch_ops(monkeypatch, expf):
    """The restatement in place of the device ops inside paddle3d_amd.petr_head (CPU tensors in and out)."""
    import bevformer_decoder_numpy as dn
    from paddle3d_amd import petr_head as ph

    n = lambda t: None if t is None else t.detach().cpu().numpy()  # noqa: E731
    calls = dict(stream=0, mha=0, coords=0)

    def stream(q, k, v, heads, key_padding_mask=None):
        calls["stream"] += 1
        km = n(key_padding_mask)
        return torch.from_numpy(pn.mha_stream(n(q), n(k), n(v), heads, expf, None if km is None else km.reshape(km.shape[0], -1)))

    def mha(q, k, v, heads):
        calls["mha"] += 1
        return torch.from_numpy(dn.mha(n(q), n(k), n(v), heads, lambda x: expf(x)))

    def coords(img2lidars, feat_hw, pad_hw, depth_num, depth_start, position_range, LID, token_mask=None, want_mask=False):
        calls["coords"] += 1
        out, mask = pn.coords3d(n(img2lidars), *feat_hw, depth_num, *pad_hw, depth_start, position_range, LID, n(token_mask))
        return (torch.from_numpy(out), torch.from_numpy(mask)) if want_mask else torch.from_numpy(out)

    monkeypatch.setattr(ph._ops, "multihead_attention_stream", stream)
    monkeypatch.setattr(ph._dec_ops, "multihead_attention", mha)
    monkeypatch.setattr(ph._ops, "petr_coords3d", coords)
    return calls


def piece_outputs(head, tag, dev="cpu"):
    """{sa_out, ca_out, layer_out, dec_pieces[, se_out, reg_out]} of the modules on the seeded inputs."""
    ai = mk.attn_inputs(tag)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    q, qp, mem, kp, mask = (t(ai[k]) for k in ("query", "query_pos", "memory", "key_pos", "mask"))
    dec = head.transformer.decoder
    layer = dec.layers[0]
    with torch.no_grad():
        out = dict(sa_out=layer.attentions[0](q, q, q, None, query_pos=qp, key_pos=qp),
                   ca_out=layer.attentions[1](q, mem, mem, None, query_pos=qp, key_pos=kp, key_padding_mask=mask),
                   layer_out=layer(q, mem, mem, query_pos=qp, key_pos=kp, key_padding_mask=mask),
                   dec_pieces=dec(q, key=mem, value=mem, key_pos=kp, query_pos=qp, key_padding_mask=mask, reg_branch=None))
        if mk.CASES[tag]["fpe"]:
            out["se_out"] = head.fpe(t(ai["se_x"]), t(ai["se_y"]))
        if mk.CASES[tag]["multi"]:
            out["reg_out"] = head.reg_branches[0](t(ai["reg_x"]))
    return out


def forward_args(tag, dev="cpu"):
    inp = mk.inputs(tag)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    return ([t(inp["feats"])], t(inp["img2lidars"]), mk.PAD, mk.img_shapes(tag), t(inp["timestamp"]))


def chain_outputs(head, tag, dev="cpu"):
    """The head's chain on the case's inputs: ({name: tensor} of the stored intermediate and final results, outs)."""
    from paddle3d_amd.petr_head import pos2posemb3d

    c = mk.CASES[tag]
    args = forward_args(tag, dev)
    seen = {}
    hook = head.transformer.register_forward_hook(lambda m, a, out: seen.__setitem__("dec_out", torch.nan_to_num(out[0], nan=0.0)))
    try:
        with torch.no_grad():
            outs = head(*args)
            masks = head._masks(c["B"], c["N"], mk.PAD, mk.img_shapes(tag), mk.FEAT, dev)
            feat_shape = tuple(args[0][0].shape)
            pos, cmask = head.position_embeding(feat_shape, mk.PAD, masks, args[1])
            res = dict(pos_embed=pos, coords_mask=cmask, dec_out=seen["dec_out"], all_cls_scores=outs["all_cls_scores"],
                       all_bbox_preds=outs["all_bbox_preds"])
            if tag == "a":
                res["sin_embed"] = head.positional_encoding(masks)
                res["query_embeds"] = pos2posemb3d(head.reference_points.weight, E // 2)
    finally:
        hook.remove()
    return res, outs


def check_chain(golden, tag, res):
    for name, got in res.items():
        if name == "coords_mask":
            assert np.array_equal(got.cpu().numpy(), golden[f"{tag}_coords_mask"]), (tag, name)
        else:
            check_result(golden, tag, name, got.cpu().numpy())


@pytest.mark.parametrize("tag", TAGS)
def test_unfused_modules_against_reference(golden, tag):
    head = build_head(tag, fused=False)
    if tag != "c":
        for name, got in piece_outputs(head, tag).items():
            check_result(golden, tag, name, got.numpy())
    c = mk.CASES[tag]
    with torch.no_grad():
        coords, _ = head.coords3d_torch((c["B"], c["N"], mk.IN_CH, H, W), mk.PAD, torch.from_numpy(token_masks(tag)),
                                        torch.from_numpy(mk.inputs(tag)["img2lidars"]))
    check_result(golden, tag, "coords3d", coords.numpy())
    res, outs = chain_outputs(head, tag)
    check_chain(golden, tag, res)
    with torch.no_grad():
        det = head.get_bboxes(outs)
    check_decode(golden, tag, "chain", *(t.numpy() for t in det))


@pytest.mark.parametrize("tag", TAGS)
def test_modules_on_the_restatement_against_reference(golden, expf, monkeypatch, tag):
    calls = patch_ops(monkeypatch, expf)
    head = build_head(tag, fused=True)
    if tag != "c":
        for name, got in piece_outputs(head, tag).items():
            check_result(golden, tag, name, got.numpy())
        assert (calls["mha"], calls["stream"], calls["coords"]) == (2 + mk.LAYERS, 2 + mk.LAYERS, 0), calls
    calls.update(stream=0, mha=0, coords=0)
    with torch.no_grad():
        outs = head(*forward_args(tag))
    assert (calls["mha"], calls["stream"], calls["coords"]) == (mk.LAYERS, mk.LAYERS, 1), calls
    for name in ("all_cls_scores", "all_bbox_preds"):
        check_result(golden, tag, name, outs[name].numpy())


def test_modules_take_the_reference_state_dict(golden):
    from paddle3d_amd import petr_head as ph
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    for tag in TAGS:
        keys = [str(k) for k in golden["state_keys_b" if tag == "b" else "state_keys"]]
        st = mk.state(tag)
        assert sorted(st) == keys
        own = build_head(tag).state_dict()
        assert sorted(own) == keys
        k = "transformer.decoder.layers.1.attentions.1.attn.k_proj.weight"
        assert torch.equal(own[k], torch.from_numpy(st[k]).t())  # Paddle's [in, out] placed as torch's [out, in]
        assert torch.equal(own["position_encoder.0.weight"], torch.from_numpy(st["position_encoder.0.weight"]))
        assert torch.equal(own["reference_points.weight"], torch.from_numpy(st["reference_points.weight"]))
    cfg = dict(mk.head_cfg("a")["transformer"]["decoder"])
    cfg.pop("type_name")
    sub = {k[len("transformer.decoder."):]: v for k, v in mk.state("a").items() if k.startswith("transformer.decoder.")}
    dec = ph.PETRTransformerDecoder(**cfg)
    assert load_paddle_state_dict(dec, sub) == []  # a part on its own
    with pytest.raises(NotImplementedError):
        ph.PETRHead(**dict(mk.head_cfg("a"), normedlinear=True))


def test_an_attention_can_opt_out_inside_a_layer(expf, monkeypatch):
    """The layer's, decoder's and head's `fused` reach both attentions; `fused=False` in an attention's own cfg keeps
    the torch formulation for it (on the device the kernels alone are slower than torch at PETR's shapes)."""
    from paddle3d_amd import petr_head as ph

    calls = patch_ops(monkeypatch, expf)
    cfg = mk.head_cfg("a", True)
    attns = cfg["transformer"]["decoder"]["transformerlayers"]["attns"]
    for a in attns:
        a.pop("fused")
    head = ph.PETRHead(**cfg).eval()
    assert head.fused and all(a.fused for layer in head.transformer.decoder.layers for a in layer.attentions)
    assert not any(a.fused for layer in ph.PETRHead(**dict(cfg, fused=False)).transformer.decoder.layers
                   for a in layer.attentions)
    attns[1]["fused"] = False  # the cross-attention opts out
    head = ph.PETRHead(**cfg).eval()
    assert [a.fused for a in head.transformer.decoder.layers[1].attentions] == [True, False]
    with torch.no_grad():
        outs = head(*forward_args("a"))
    assert (calls["mha"], calls["stream"], calls["coords"]) == (mk.LAYERS, 0, 1), calls
    assert torch.isfinite(outs["all_cls_scores"]).all()


def test_refusals_need_no_gpu():
    from paddle3d_amd import _lib, build
    from paddle3d_amd.ops import petr as ops

    build.build()
    L = _lib.lib()
    mha = lambda Nq, Nk, d, B=1, p=None: L.pd3_mha_stream_forward(p, p, p, None, B, Nq, Nk, 2, d, 0.25, p, None)  # noqa: E731
    for Nk, d in ((10, 8), (10, 24), (10, 144), (10, 40)):
        assert mha(5, Nk, d) == -3 and not ops.mha_stream_supported(d, Nk), (Nk, d)
    for d in (16, 32, 64, 128):
        assert ops.mha_stream_supported(d, 48000) and mha(5, 48000, d) == -1  # a supported shape with null pointers
    assert mha(5, 0, 32) == -1 and mha(5, -1, 32) == -1 and mha(-1, 10, 32) == -1
    assert mha(0, 10, 32) == 0 and mha(5, 10, 32, B=0) == 0  # nothing to do is no error
    aligned = np.zeros(64, F32)
    odd = _lib.C.c_void_p(aligned.ctypes.data + 4)
    assert L.pd3_mha_stream_forward(odd, odd, odd, None, 1, 1, 1, 1, 16, 0.25, odd, None) == -3
    rng = np.asarray(mk.CASES["a"]["position_range"], F32)
    co = lambda BN, h, w, D, r=rng.ctypes.data, ds=1.0: L.pd3_petr_coords3d(  # noqa: E731
        None, BN, h, w, D, 40, 56, ds, r, 1, None, None, None, None)
    assert co(0, 5, 7, 8) == 0 and co(2, 0, 7, 8) == 0 and co(2, 5, 0, 8) == 0 and co(2, 5, 7, 0) == 0
    assert co(2, 5, 7, 8) == -1 and co(-1, 5, 7, 8) == -1 and co(2, 5, 7, 8, r=None) == -1
    assert co(2, 5, 7, 8, ds=float("nan")) == -1
    assert co(2 ** 20, 2 ** 12, 7, 8) == -3 and not ops.coords3d_supported(2 ** 20, 2 ** 12, 7, 8)
    assert ops.coords3d_supported(6, 20, 50, 64)


@pytest.mark.parametrize("tag", TAGS)
def test_maker_conditions_hold_on_the_committed_file(golden, tag):
    c = mk.CASES[tag]
    assert os.path.getsize(mk.OUT) < 1_000_000
    seen = mk.check_discrete(golden, tag)
    print(tag, seen)
    BN = c["B"] * c["N"]
    for name, shape in (("coords_norm", (BN, 3 * mk.D, H, W)), ("coords3d", (BN, 3 * mk.D, H, W)),
                        ("pos_embed", (c["B"], c["N"], E, H, W)), ("dec_out", (mk.LAYERS, c["B"], mk.Q, E)),
                        ("all_cls_scores", (mk.LAYERS, c["B"], mk.Q, mk.K)),
                        ("all_bbox_preds", (mk.LAYERS, c["B"], mk.Q, mk.CODE))):
        assert golden[f"{tag}_{name}"].shape == shape
    m = golden[f"{tag}_coords_mask"]
    assert m.shape == (c["B"], c["N"], H, W) and m.dtype == bool
    tm = token_masks(tag)
    assert not (tm & ~m).any()  # the token mask is OR-ed in
    if tag == "a":  # the two smaller images give padded tokens: a key mask that is not empty
        assert tm[0, 1].any() and tm[1, 2].any() and not tm[0, 0].any() and 0 < tm.mean() < 0.5
    if tag == "c":  # coords_mask true for some tokens of the far camera, by the coordinates alone
        assert not tm.any() and 0 < m.mean() < 1
    assert not set(golden) & {"feats", "img2lidars"} and all(
        k.startswith(tuple(t + "_" for t in TAGS)) or k.startswith("state_keys") for k in golden)
