"""Golden vectors for BEVFormer's decoder, head and NMS-free decode from the reference's own Python, executed by line
range through tests/golden/paddle_shim.py (the technique of make_bevformer_golden.py):

    MultiheadAttention.forward            models/transformers/attentions/multihead_attention.py:95-191
    CustomMSDeformableAttention.forward   models/transformers/attentions/spatial_cross_attention.py:531-640
    DetrTransformerDecoderLayer.forward   models/transformers/decoder_layers.py:149-248
    DetectionTransformerDecoder.forward   models/transformers/decoders.py:66-136   (2 layers, box refinement)
    inverse_sigmoid                       models/transformers/transformer.py:32-48
    PerceptionTransformer.forward         models/transformers/transformer.py:361-390   (the decoder half)
    BEVFormerHead.forward                 models/detection/bevformer/bevformer_head.py:284-330   (the tail)
    BEVFormerHead.get_bboxes              models/detection/bevformer/bevformer_head.py:613-634
    NMSFreeCoder.decode_single / decode   utils/box_coder.py:133-214
    denormalize_bbox                      utils/box.py:107-138

    python tests/golden/make_bevformer_decoder_golden.py   # needs the reference checkout; writes
                                                           # python_bevformer_decoder.npz

`self` is a SimpleNamespace whose projections are seeded linear maps (state(tag): a state dict with the reference's
keys and Paddle's [in, out] Linear weights); LayerNorm is torch.  paddle.nn.MultiHeadAttention is not in the reference
tree and is restated here from its formula:
    product = matmul(q * head_dim ** -0.5, k, transpose_y=True); weights = softmax(product, -1); out = matmul(weights, v)
between q_proj / k_proj / v_proj and out_proj.  `ms_deform_attn.ms_deform_attn` is make_ms_deform_attn_golden's float64
grid_sample formulation.  What the shim lacks (paddle.log, unsqueeze with a list) is added here.  Every method runs
twice from the same float32 inputs: as written (float32) and with the shim's float32 mapped to float64.  The float64
results are stored with the bound the tests read: 4 x the largest difference between the two runs, one float32 ulp of
the largest magnitude as floor (make_bevformer_golden.bound).

The decode runs through get_bboxes twice per case: on seeded class logits and boxes built for the case (`dec_*`: centres
outside or near post_center_range, a frame whose scores all lie below the threshold), and, case a, on the head's own
output (`chain_*`).  The selection must equal the reference's exactly, so main() asserts (check_selection): among each
frame's max_num + 1 largest float64 scores neighbours differ by more than twice the score bound, no score is within the
bound of a threshold the loop visits, no centre within the box bound of a range face; and both runs select the same.

Inputs are regenerated from seeds (inputs(tag), state(tag), decode_inputs(tag)); the file holds results and bounds.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ms_deform_attn_numpy as md  # noqa: E402
from make_bevformer_golden import bound  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "python_bevformer_decoder.npz")
TR = "paddle3d/models/transformers"
EMBED, HEADS, FFN_CH, LAYERS, POINTS = 64, 2, 128, 2, 4
PC_RANGE = [-10.0, -10.0, -3.0, 10.0, 10.0, 5.0]
ORDER = ("self_attn", "norm", "cross_attn", "norm", "ffn", "norm")

CASES = {
    "a": dict(Q=37, bev=(7, 11), B=2, K=10, code=10, max_num=20, thr=None, post=[-12.0, -12.0, -4.0, 12.0, 12.0, 6.0],
              centre="inside", seed=101),
    # max_num = Q * K: every entry is taken; a third of the centres lie outside post_center_range
    "b": dict(Q=16, bev=(5, 6), B=1, K=3, code=8, max_num=48, thr=None, post=[-6.0, -6.0, -2.0, 6.0, 6.0, 3.0],
              centre="spread", seed=211),
    # frame 0 has scores above the threshold, frame 1 none: the loop lowers it; centres near the range faces
    "c": dict(Q=50, bev=(6, 5), B=2, K=10, code=10, max_num=30, thr=0.3, post=[-8.0, -8.0, -2.5, 8.0, 8.0, 4.0],
              centre="border", seed=307),
}
TAGS = tuple(CASES)
PIECES = ("mha_sample", "mha_out", "ca_sample", "ca_out", "layer_out")  # of the first layer; cases a and b
MODEL = ("dec_states", "dec_refs", "init_ref", "all_cls_scores", "all_bbox_preds")


def results(tag):
    return (PIECES if tag in ("a", "b") else ()) + MODEL


DECODES = {"a": ("dec", "chain"), "b": ("dec",), "c": ("dec",)}


def inputs(tag):
    """bev_embed [B, S, E] (the encoder's output) float32."""
    c = CASES[tag]
    rng = np.random.default_rng(c["seed"] + 1)
    return dict(bev_embed=rng.standard_normal((c["B"], c["bev"][0] * c["bev"][1], EMBED)).astype(np.float32))


def _linear_keys(tag):
    c = CASES[tag]
    keys = {"transformer.reference_points": (EMBED, 3), "transformer.can_bus_mlp.0": (18, EMBED // 2),
            "transformer.can_bus_mlp.2": (EMBED // 2, EMBED)}
    for i in range(LAYERS):
        s, x = f"transformer.decoder.layers.{i}.attentions.0.attn.", f"transformer.decoder.layers.{i}.attentions.1."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            keys[s + n] = (EMBED, EMBED)
        keys[x + "sampling_offsets"] = (EMBED, HEADS * POINTS * 2)
        keys[x + "attention_weights"] = (EMBED, HEADS * POINTS)
        keys[x + "value_proj"] = keys[x + "output_proj"] = (EMBED, EMBED)
        keys[f"transformer.decoder.layers.{i}.ffns.0.layers.0.0"] = (EMBED, FFN_CH)
        keys[f"transformer.decoder.layers.{i}.ffns.0.layers.1"] = (FFN_CH, EMBED)
        for j in (0, 3):
            keys[f"cls_branches.{i}.{j}"] = (EMBED, EMBED)
        keys[f"cls_branches.{i}.6"] = (EMBED, c["K"])
        for j in (0, 2):
            keys[f"reg_branches.{i}.{j}"] = (EMBED, EMBED)
        keys[f"reg_branches.{i}.4"] = (EMBED, c["code"])
    return keys


def _norm_keys():
    keys = ["transformer.can_bus_mlp.norm"]
    for i in range(LAYERS):
        keys += [f"transformer.decoder.layers.{i}.norms.{j}" for j in range(3)]
        keys += [f"cls_branches.{i}.{j}" for j in (1, 4)]
    return keys


def state(tag):
    """BEVFormerHead's state dict with the reference's keys (Linear weights [in, out])."""
    c = CASES[tag]
    rng = np.random.default_rng(c["seed"] + 2)
    st = {}
    for k, (n_in, n_out) in _linear_keys(tag).items():
        scale = 1.5 if k.endswith("sampling_offsets") else 1.0
        st[k + ".weight"] = (rng.standard_normal((n_in, n_out)) * scale / np.sqrt(n_in)).astype(np.float32)
        st[k + ".bias"] = (rng.standard_normal(n_out) * (1.5 if scale > 1 else 0.1)).astype(np.float32)
    for k in _norm_keys():
        st[k + ".weight"] = rng.uniform(0.5, 1.5, EMBED).astype(np.float32)
        st[k + ".bias"] = (rng.standard_normal(EMBED) * 0.1).astype(np.float32)
    st["query_embedding.weight"] = rng.standard_normal((c["Q"], 2 * EMBED)).astype(np.float32)
    st["bev_embedding.weight"] = rng.standard_normal((c["bev"][0] * c["bev"][1], EMBED)).astype(np.float32)
    st["transformer.level_embeds"] = rng.standard_normal((4, EMBED)).astype(np.float32)
    st["transformer.cams_embeds"] = rng.standard_normal((6, EMBED)).astype(np.float32)
    return st


def head_cfg(tag, fused=True):
    """Constructor arguments of paddle3d_amd.bevformer_head.BEVFormerHead for the case (the reference's config layout)."""
    c = CASES[tag]
    attn = [dict(type_name="MultiheadAttention", embed_dims=EMBED, num_heads=HEADS, dropout=0.1, fused=fused),  # opt-in
            dict(type_name="CustomMSDeformableAttention", embed_dims=EMBED, num_heads=HEADS, num_levels=1,
                 num_points=POINTS)]
    layer = dict(type_name="DetrTransformerDecoderLayer", attn_cfgs=attn, feedforward_channels=FFN_CH, ffn_dropout=0.1,
                 operation_order=ORDER)
    decoder = dict(type_name="DetectionTransformerDecoder", num_layers=LAYERS, return_intermediate=True,
                   transformerlayers=layer)
    coder = dict(type_name="NMSFreeCoder", point_cloud_range=PC_RANGE, post_center_range=c["post"], max_num=c["max_num"],
                 score_threshold=c["thr"], num_classes=c["K"])
    return dict(num_classes=c["K"], in_channels=EMBED, num_query=c["Q"], with_box_refine=True, as_two_stage=False,
                bev_h=c["bev"][0], bev_w=c["bev"][1], code_size=c["code"], bbox_coder=coder, fused=fused,
                transformer=dict(type_name="PerceptionTransformer", embed_dims=EMBED, decoder=decoder))


def decode_inputs(tag):
    """Seeded (cls [B, Q, K] logits, bbox [B, Q, code]) for the case's stand-alone decode."""
    c = CASES[tag]
    rng = np.random.default_rng(c["seed"] + 3)
    B, Q, K, code = c["B"], c["Q"], c["K"], c["code"]
    cls = rng.uniform(-4.0, 2.0, (B, Q, K))
    if c["thr"] is not None:
        cls[1] = rng.uniform(-6.0, -2.5, (Q, K))  # sigmoid <= 0.076 < thr: the loop lowers the threshold
    bbox = rng.standard_normal((B, Q, code)) * 0.4
    lo, hi = np.asarray(c["post"][:3]), np.asarray(c["post"][3:])
    if c["centre"] == "inside":
        ctr = rng.uniform(lo * 0.9, hi * 0.9, (B, Q, 3))
    elif c["centre"] == "spread":
        ctr = rng.uniform(lo * 1.5, hi * 1.5, (B, Q, 3))
    else:  # within 0.3 m of a face, on either side
        face = np.where(rng.random((B, Q, 3)) < 0.5, lo, hi)
        ctr = np.where(rng.random((B, Q, 3)) < 0.5, face + rng.uniform(-0.3, 0.3, (B, Q, 3)),
                       rng.uniform(lo * 0.9, hi * 0.9, (B, Q, 3)))
    bbox[..., 0], bbox[..., 1], bbox[..., 4] = ctr[..., 0], ctr[..., 1], ctr[..., 2]
    return cls.astype(np.float32), bbox.astype(np.float32)


def threshold_steps(thr):
    """The values the loop of box_coder.py:158-166 visits (Python doubles), the first one being thr itself."""
    steps, tmp = [float(thr)], float(thr)
    while True:
        tmp *= 0.9
        if tmp < 0.01:
            return steps
        steps.append(tmp)


def load():
    return dict(np.load(OUT))


def check_selection(g, tag, name):
    """The conditions under which the selection cannot depend on rounding; returns what it saw."""
    c = CASES[tag]
    s = g[f"{tag}_{name}_all_scores"]  # [B, Q*K] float64 sigmoid
    sb, bb = float(g[f"{tag}_{name}_scores_bound"]), float(g[f"{tag}_{name}_boxes_bound"])
    gaps, thr_margin = [], np.inf
    for b in range(c["B"]):
        top = np.sort(s[b])[::-1][:min(c["max_num"] + 1, s.shape[1])]
        gap = float(np.min(top[:-1] - top[1:]))
        assert gap > 2 * sb, (tag, name, b, "neighbouring scores", gap, sb)
        gaps.append(gap)
        if c["thr"] is not None:
            for t in threshold_steps(c["thr"]):
                m = float(np.abs(top - t).min())
                assert m > sb, (tag, name, b, "a score within the bound of threshold", t, m)
                thr_margin = min(thr_margin, m)
    ctr = g[f"{tag}_{name}_centres"]  # [B, max_num, 3] float64 centres of the selected entries
    faces = np.asarray(c["post"], np.float64)
    margin = float(min(np.abs(ctr - faces[:3]).min(), np.abs(ctr - faces[3:]).min()))
    assert margin > bb, (tag, name, "a centre within the bound of a range face", margin, bb)
    return dict(gap=min(gaps), thr_margin=thr_margin, face_margin=margin, counts=g[f"{tag}_{name}_count"].tolist())


# ---- the reference run (needs the reference checkout) ---------------------------------------------------------------


def _reference(tag, dt):
    import paddle_shim as ps

    p = ps.install(REF)
    import paddle.nn.functional as F

    ps._DT["float32"] = dt
    p.float32 = dt
    p.log = lambda x: ps._wrap(torch.log(x))
    plain_unsqueeze = ps.Tensor.unsqueeze

    def unsqueeze(self, axis):
        for a in (axis if isinstance(axis, (list, tuple)) else [axis]):
            self = torch.Tensor.unsqueeze(self, a)
        return self

    ps.Tensor.unsqueeze = unsqueeze
    try:
        return _run(tag, dt, ps, p, F)
    finally:
        ps._DT["float32"] = torch.float32
        ps.Tensor.unsqueeze = plain_unsqueeze


def _run(tag, dt, ps, p, F):
    c = CASES[tag]
    st, inp = state(tag), inputs(tag)
    bev_h, bev_w = c["bev"]
    B, Q, K = c["B"], c["Q"], c["K"]
    T = lambda a: ps._wrap(torch.from_numpy(np.ascontiguousarray(a)).to(dt))  # noqa: E731
    plain = lambda t: t.as_subclass(torch.Tensor)  # noqa: E731

    def op(value, sampling_locations, attention_weights, spatial_shapes, level_start_index, im2col_step):
        a = [plain(t).detach().double() for t in (value, sampling_locations, attention_weights)]
        out = md.grid_sample_attn(*a, plain(spatial_shapes).numpy(), plain(level_start_index).numpy())
        return ps._wrap(out.to(dt))

    common = dict(paddle=p, F=F, ms_deform_attn=types.SimpleNamespace(ms_deform_attn=op), masked_fill=None,
                  logger=types.SimpleNamespace(warning=lambda *a: None), copy=__import__("copy"),
                  warnings=__import__("warnings"), np=np)
    ex = lambda path, lines: ps.exec_lines(os.path.join(REF, path), [lines], dict(common))  # noqa: E731
    mha_forward = ex(f"{TR}/attentions/multihead_attention.py", (95, 191))["forward"]
    ca_forward = ex(f"{TR}/attentions/spatial_cross_attention.py", (531, 640))["forward"]
    layer_forward = ex(f"{TR}/decoder_layers.py", (149, 248))["forward"]
    inverse_sigmoid = ex(f"{TR}/transformer.py", (32, 48))["inverse_sigmoid"]
    common["inverse_sigmoid"] = inverse_sigmoid
    dec_forward = ex(f"{TR}/decoders.py", (66, 136))["forward"]
    denormalize_bbox = ex("paddle3d/utils/box.py", (107, 138))["denormalize_bbox"]
    common["denormalize_bbox"] = denormalize_bbox
    coder_fns = ex("paddle3d/utils/box_coder.py", (133, 214))
    common["dtype2float32"] = lambda v: v
    get_bboxes = ex("paddle3d/models/detection/bevformer/bevformer_head.py", (613, 634))["get_bboxes"]

    def linear(key, tap=None):
        w, b = torch.from_numpy(st[key + ".weight"]).to(dt), torch.from_numpy(st[key + ".bias"]).to(dt)

        def f(x):
            if tap is not None:
                tap.append(plain(x).detach().clone())
            return ps._wrap(torch.matmul(plain(x), w) + b)

        return f

    def norm(key):
        w, b = (torch.from_numpy(st[f"{key}.{n}"]).to(dt) for n in ("weight", "bias"))
        return lambda x: ps._wrap(torch.nn.functional.layer_norm(plain(x), (EMBED,), w, b, 1e-5))

    ident = lambda x: x  # noqa: E731
    taps = {"mha": [], "ca": []}

    def paddle_mha(prefix):
        """paddle.nn.MultiHeadAttention.forward restated (no mask, no dropout, no cache)."""
        qp, kp, vp = (linear(prefix + n) for n in ("q_proj", "k_proj", "v_proj"))
        op_ = linear(prefix + "out_proj", taps["mha"])
        d = EMBED // HEADS

        def f(query, key, value, attn_mask=None):
            assert attn_mask is None
            heads = lambda t: plain(t).reshape(t.shape[0], t.shape[1], HEADS, d).permute(0, 2, 1, 3)  # noqa: E731
            q, k, v = heads(qp(query)), heads(kp(key)), heads(vp(value))
            product = torch.matmul(q * (d ** -0.5), k.transpose(-1, -2))
            weights = torch.softmax(product, -1)
            out = torch.matmul(weights, v).permute(0, 2, 1, 3)
            return op_(ps._wrap(out.reshape(out.shape[0], out.shape[1], EMBED)))

        return f

    def layer_self(i):
        pre = f"transformer.decoder.layers.{i}."
        mha = types.SimpleNamespace(batch_first=False, attn=paddle_mha(pre + "attentions.0.attn."), proj_drop=ident,
                                    dropout_layer=ident)
        x = pre + "attentions.1."
        ca = types.SimpleNamespace(num_heads=HEADS, num_levels=1, num_points=POINTS, im2col_step=64, batch_first=False,
                                   dropout=ident, value_proj=linear(x + "value_proj"),
                                   sampling_offsets=linear(x + "sampling_offsets"),
                                   attention_weights=linear(x + "attention_weights"),
                                   output_proj=linear(x + "output_proj", taps["ca"]))
        fc1, fc2 = linear(pre + "ffns.0.layers.0.0"), linear(pre + "ffns.0.layers.1")
        ffn = lambda x, identity=None: (x if identity is None else identity) + fc2(torch.relu(fc1(x)))  # noqa: E731
        layer = types.SimpleNamespace(operation_order=ORDER, pre_norm=False, num_attn=2,
                                      norms=[norm(pre + f"norms.{j}") for j in range(3)], ffns=[ffn],
                                      attentions=[lambda *a, **k: mha_forward(mha, *a, **k),
                                                  lambda *a, **k: ca_forward(ca, *a, **k)])
        return layer, mha, ca

    def branch(prefix, kinds):
        fs = []
        for j, kind in enumerate(kinds):
            fs.append(dict(l=lambda j=j: linear(f"{prefix}.{j}"), n=lambda j=j: norm(f"{prefix}.{j}"),
                           r=lambda j=j: (lambda x: ps._wrap(torch.relu(plain(x)))))[kind]())

        def f(x):
            for fn in fs:
                x = fn(x)
            return x

        return f

    layers = [layer_self(i) for i in range(LAYERS)]
    cls_branches = [branch(f"cls_branches.{i}", "lnrlnrl") for i in range(LAYERS)]
    reg_branches = [branch(f"reg_branches.{i}", "lrlrl") for i in range(LAYERS)]
    decoder = types.SimpleNamespace(return_intermediate=True,
                                    layers=[(lambda *a, _l=l[0], **k: layer_forward(_l, *a, **k)) for l in layers])
    transformer = types.SimpleNamespace(embed_dims=EMBED, reference_points=linear("transformer.reference_points"),
                                        decoder=lambda **k: dec_forward(decoder, **k))
    coder = types.SimpleNamespace(point_cloud_range=PC_RANGE, post_center_range=list(c["post"]), max_num=c["max_num"],
                                  score_threshold=c["thr"], num_classes=K)
    coder.decode_single = lambda *a: coder_fns["decode_single"](coder, *a)
    coder.decode = lambda d: coder_fns["decode"](coder, d)
    head = types.SimpleNamespace(cls_branches=cls_branches, reg_branches=reg_branches, point_cloud_range=PC_RANGE,
                                 bbox_coder=coder)
    res = {}
    with torch.no_grad():
        bev = T(inp["bev_embed"])
        qe = T(st["query_embedding.weight"])
        # ---- the decoder half of PerceptionTransformer.forward, then the tail of BEVFormerHead.forward ------------------
        ns = dict(common, self=transformer, mlvl_feats=[bev], object_query_embed=qe, bev_embed=bev, bev_h=bev_h,
                  bev_w=bev_w, reg_branches=reg_branches, cls_branches=None, kwargs={})
        ps.exec_lines(os.path.join(REF, TR, "transformer.py"), [(361, 390)], ns)
        res["dec_states"], res["dec_refs"] = ns["inter_states"].numpy(), ns["inter_references_out"].numpy()
        res["init_ref"] = ns["init_reference_out"].numpy()
        hs_ns = dict(common, self=head, outputs=(ns["bev_embed"], ns["inter_states"], ns["init_reference_out"],
                                                 ns["inter_references_out"]))
        ps.exec_lines(os.path.join(REF, "paddle3d/models/detection/bevformer/bevformer_head.py"), [(284, 330)], hs_ns)
        outs = hs_ns["outs"]
        res["all_cls_scores"], res["all_bbox_preds"] = outs["all_cls_scores"].numpy(), outs["all_bbox_preds"].numpy()
        # ---- the first layer's pieces on the decoder's own inputs -------------------------------------------------------
        query_pos, query = (t[None].expand(B, Q, EMBED).permute(1, 0, 2) for t in torch.split(plain(qe), EMBED, 1))
        query_pos, query = ps._wrap(query_pos.contiguous()), ps._wrap(query.contiguous())
        ref_in = ps._wrap(plain(ns["init_reference_out"])[..., :2].unsqueeze(2).contiguous())
        sh = ps._wrap(torch.tensor([[bev_h, bev_w]], dtype=torch.int64))
        lsi = ps._wrap(torch.zeros(1, dtype=torch.int64))
        value = ns["bev_embed"]  # [S, B, E]
        layer, mha, ca = layers[0]
        for k in taps:
            taps[k].clear()
        out = mha_forward(mha, query, query, query, None, query_pos=query_pos, key_pos=query_pos)
        res["mha_sample"], res["mha_out"] = taps["mha"][0].numpy(), out.numpy()
        taps["ca"].clear()
        out = ca_forward(ca, query, None, value, None, query_pos=query_pos, reference_points=ref_in, spatial_shapes=sh,
                         level_start_index=lsi)
        res["ca_sample"], res["ca_out"] = taps["ca"][0].numpy(), out.numpy()
        res["layer_out"] = layer_forward(layer, query, None, value, query_pos, reference_points=ref_in, spatial_shapes=sh,
                                         level_start_index=lsi).numpy()
        # ---- get_bboxes ---------------------------------------------------------------------------------------------------
        for name in DECODES[tag]:
            if name == "dec":
                cls, bbox = (T(a)[None] for a in decode_inputs(tag))
            else:
                cls, bbox = (ps._wrap(plain(outs[k])[-1:].to(torch.float32).to(dt)) for k in
                             ("all_cls_scores", "all_bbox_preds"))
            coder.post_center_range = list(c["post"])
            ret = get_bboxes(head, dict(all_cls_scores=cls, all_bbox_preds=bbox), None)
            res.update(_pad_decode(c, name, plain(cls)[0], plain(bbox)[0], ret))
    return res


def _pad_decode(c, name, cls, bbox, ret):
    """get_bboxes' per-frame lists as fixed-size arrays, with the rows and centres of the selection."""
    B, n, W = c["B"], c["max_num"], c["code"] - 1
    out = {f"{name}_boxes": np.zeros((B, n, W), np.float64), f"{name}_scores": np.zeros((B, n), np.float64),
           f"{name}_labels": np.full((B, n), -1, np.int32), f"{name}_rows": np.full((B, n), -1, np.int32),
           f"{name}_count": np.zeros(B, np.int32), f"{name}_centres": np.zeros((B, n, 3), np.float64),
           f"{name}_all_scores": torch.sigmoid(cls.double()).reshape(B, -1).numpy()}
    for b, (boxes, scores, labels) in enumerate(ret):
        boxes, scores, labels = (t.as_subclass(torch.Tensor).double().numpy() for t in (boxes, scores, labels))
        k = len(scores)
        s_all = torch.sigmoid(cls[b]).reshape(-1)
        top, idx = s_all.topk(n)
        kept = np.isin(top.double().numpy(), scores)
        assert kept.sum() == k, (name, b, int(kept.sum()), k)
        rows = (idx.numpy() // c["K"])
        out[f"{name}_boxes"][b, :k], out[f"{name}_scores"][b, :k] = boxes, scores
        out[f"{name}_labels"][b, :k], out[f"{name}_rows"][b, :k], out[f"{name}_count"][b] = labels, rows[kept], k
        out[f"{name}_centres"][b] = bbox[b].double().numpy()[rows][:, [0, 1, 4]]
    return out


def main():
    out = {}
    for tag in TAGS:
        c = CASES[tag]
        r32, r64 = _reference(tag, torch.float32), _reference(tag, torch.float64)
        assert r32["dec_states"].dtype == np.float32 and r64["dec_states"].dtype == np.float64
        for k in results(tag):
            out[f"{tag}_{k}"] = r64[k]
            out[f"{tag}_{k}_bound"], out[f"{tag}_{k}_ref_err"] = bound(r32[k], r64[k])
            print(f"{tag} {k} {r64[k].shape}: |max| {np.abs(r64[k]).max():.3f}, the reference's own error "
                  f"{float(out[f'{tag}_{k}_ref_err']):.3e}, bound {float(out[f'{tag}_{k}_bound']):.3e}")
        for name in DECODES[tag]:
            for k in ("labels", "rows", "count"):
                assert np.array_equal(r32[f"{name}_{k}"], r64[f"{name}_{k}"]), (tag, name, k, "the two runs select differently")
                out[f"{tag}_{name}_{k}"] = r64[f"{name}_{k}"]
            out[f"{tag}_{name}_all_scores"] = r64[f"{name}_all_scores"]
            out[f"{tag}_{name}_centres"] = r64[f"{name}_centres"]
            for k in ("boxes", "scores"):
                out[f"{tag}_{name}_{k}"] = r64[f"{name}_{k}"]
                out[f"{tag}_{name}_{k}_bound"], out[f"{tag}_{name}_{k}_ref_err"] = bound(r32[f"{name}_{k}"], r64[f"{name}_{k}"])
            # the chain's scores carry the error of everything before them
            if name == "chain":
                sb, _ = bound(1 / (1 + np.exp(-r32["all_cls_scores"][-1].astype(np.float64))),
                              1 / (1 + np.exp(-r64["all_cls_scores"][-1])))
                out[f"{tag}_{name}_scores_bound"] = np.float64(max(float(sb), float(out[f"{tag}_{name}_scores_bound"])))
            print(tag, name, "boxes bound", float(out[f"{tag}_{name}_boxes_bound"]), "scores bound",
                  float(out[f"{tag}_{name}_scores_bound"]), check_selection(out, tag, name))
        if tag == "b":
            assert 0 < out["b_dec_count"][0] < c["max_num"], "case b: some centres outside the range, not all"
        if tag == "c":
            steps = threshold_steps(c["thr"])
            top = out["c_dec_all_scores"].max(1)
            assert top[0] > steps[0] and top[1] < steps[1] and top[1] > 0.01, top
            assert 0 < out["c_dec_count"][1] < c["max_num"], out["c_dec_count"]
    out["state_keys"] = np.array(sorted(state("a")))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
