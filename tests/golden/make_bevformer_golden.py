"""Golden vectors for BEVFormer's encoder attention from the reference's own Python, executed by line range through
tests/golden/paddle_shim.py (the technique of make_ms_deform_attn_golden.py):

    BEVFormerEncoder.get_reference_points   models/transformers/encoders.py:69-117
    BEVFormerEncoder.point_sampling         models/transformers/encoders.py:120-176
    BEVFormerEncoder.forward                models/transformers/encoders.py:178-302   (2 layers)
    BEVFormerLayer.forward                  models/transformers/encoder_layers.py:259-381
    SpatialCrossAttention.forward           models/transformers/attentions/spatial_cross_attention.py:81-212
    MSDeformableAttention3D.forward         models/transformers/attentions/spatial_cross_attention.py:310-428
    TemporalSelfAttention.forward           models/transformers/attentions/temporal_self_attention.py:140-279

    python tests/golden/make_bevformer_golden.py     # needs the reference checkout; writes python_bevformer.npz

`self` is a SimpleNamespace whose projections are seeded linear maps (state(tag): a state dict with the reference's
keys and Paddle's [in, out] Linear weights), LayerNorm and the FFN are torch, and `ms_deform_attn.ms_deform_attn` is
make_ms_deform_attn_golden's float64 grid_sample formulation.  What the shim lacks (paddle.maximum, paddle.full_like)
is added here.  Every method runs twice from the same float32 inputs: as written (float32) and with the shim's float32
mapped to float64.  The float64 results are stored with the bound the tests read: 4 x the largest difference between the
two runs, one float32 ulp of the largest magnitude as floor (make_roi_head_golden.bound).  For reference_points_cam the
bound is taken over the points in front of the camera (z > 1e-5); the components behind it (about 1e5 in size, u = x /
1e-5) are held to the same rule on a relative scale.

FORCED DEPARTURE: the reference runs one frame at a time.  SpatialCrossAttention.forward gathers every frame's queries
with frame 0's mask (`mask_per_img[0]`, line 152) but counts with each frame's own, so at a batch of 2 with different
calibrations it mixes them; its batch size is 1.  The stored batch is the stack of single-frame runs, which is what
paddle3d_amd.bevformer computes (each frame with its own mask).

Inputs are regenerated from seeds (inputs(tag), state(tag)); the file holds the calibrations and the results.
"""
import copy
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ms_deform_attn_numpy as md  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "python_bevformer.npz")
TR = "paddle3d/models/transformers"
EMBED, HEADS, FFN_CH, LAYERS = 64, 2, 128, 2
PC_RANGE = [-10.0, -10.0, -3.0, 10.0, 10.0, 5.0]
IMG_SHAPE = (48, 80, 3)  # (h, w, channels) of every image
FOCAL = 40.0
EPS = 1e-5
ORDER = ("self_attn", "norm", "cross_attn", "norm", "ffn", "norm")

CASES = {
    # Q = 77; three overlapping cameras that differ between the two frames
    "a": dict(bev=(7, 11), cams=3, levels=[[6, 10], [3, 5]], P=8, D=4, B=2, tsa_P=4, prev="random", shift=False,
              yaw=[[0.35, 1.05, 1.9], [2.6, 3.2, 4.1]], planted=[], seed=11),
    # six cameras, one of them planted to see nothing; prev_bev all zero, so the encoder takes bev_query
    "b": dict(bev=(5, 6), cams=6, levels=[[6, 10]], P=8, D=4, B=1, tsa_P=8, prev="zero", shift=False,
              yaw=[[0.2, 1.25, 2.3, 3.35, 4.4, 5.45]], planted=[4], seed=23),
    # TSA and the layer at P = 4 with shifted BEV points and a history BEV
    "c": dict(bev=(6, 5), cams=3, levels=[[5, 8]], P=4, D=4, B=2, tsa_P=4, prev="random", shift=True,
              yaw=[[0.5, 2.4, 4.6], [1.1, 3.0, 5.2]], planted=[], seed=37),
}
TAGS = tuple(CASES)
RESULTS = ("sca_sample", "sca_out", "tsa_sample", "tsa_out", "layer_out", "encoder_out")


def bound(ref32, ref64):
    err = float(np.abs(ref32.astype(np.float64) - ref64).max())
    ulp = float(np.spacing(np.float32(np.abs(ref64).max())))
    return np.float64(max(4.0 * err, ulp)), np.float64(err)


def calibrations(tag):
    """lidar2img [B, cams, 4, 4] float32: pinhole cameras near the origin looking along their yaw."""
    c = CASES[tag]
    rng = np.random.default_rng(c["seed"])
    h, w, _ = IMG_SHAPE
    K = np.array([[FOCAL, 0, w / 2, 0], [0, FOCAL, h / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
    out = np.zeros((c["B"], c["cams"], 4, 4), np.float64)
    for b in range(c["B"]):
        for i, yaw in enumerate(c["yaw"][b]):
            pos = np.concatenate([rng.uniform(-0.7, 0.7, 2), rng.uniform(0.8, 1.6, 1)])
            fwd, right, down = (np.array([np.cos(yaw), np.sin(yaw), 0.0]), np.array([np.sin(yaw), -np.cos(yaw), 0.0]),
                                np.array([0.0, 0.0, -1.0]))
            R = np.stack([right, down, fwd])
            E = np.eye(4)
            E[:3, :3], E[:3, 3] = R, -R @ pos
            if i in c["planted"]:
                E[2, 3] -= 100.0  # everything is 100 m behind this camera
            out[b, i] = K @ E
    return out.astype(np.float32)


def levels(tag):
    return md.level_layout(CASES[tag]["levels"])


def inputs(tag):
    """bev_query, bev_pos, prev_bev [B, Q, E], feats [cams, S, B, E], shift [B, 2], all float32."""
    c = CASES[tag]
    rng = np.random.default_rng(c["seed"] + 1)
    B, Q, S = c["B"], c["bev"][0] * c["bev"][1], levels(tag)[2]
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    d = dict(bev_query=f(B, Q, EMBED), bev_pos=(0.5 * f(B, Q, EMBED)).astype(np.float32), feats=f(c["cams"], S, B, EMBED))
    d["prev_bev"] = f(B, Q, EMBED) if c["prev"] == "random" else np.zeros((B, Q, EMBED), np.float32)
    d["shift"] = (rng.uniform(-0.08, 0.08, (B, 2)).astype(np.float32) if c["shift"] else np.zeros((B, 2), np.float32))
    return d


def _attention_keys(tag):
    c = CASES[tag]
    L = len(c["levels"])
    keys = {}
    for i in range(LAYERS):
        t, s = f"layers.{i}.attentions.0.", f"layers.{i}.attentions.1."
        keys[t + "sampling_offsets"] = (2 * EMBED, 2 * HEADS * c["tsa_P"] * 2)
        keys[t + "attention_weights"] = (2 * EMBED, 2 * HEADS * c["tsa_P"])
        keys[t + "value_proj"] = keys[t + "output_proj"] = (EMBED, EMBED)
        keys[s + "deformable_attention.sampling_offsets"] = (EMBED, HEADS * L * c["P"] * 2)
        keys[s + "deformable_attention.attention_weights"] = (EMBED, HEADS * L * c["P"])
        keys[s + "deformable_attention.value_proj"] = keys[s + "output_proj"] = (EMBED, EMBED)
        keys[f"layers.{i}.ffns.0.layers.0.0"] = (EMBED, FFN_CH)
        keys[f"layers.{i}.ffns.0.layers.1"] = (FFN_CH, EMBED)
    return keys


def state(tag):
    """The encoder's state dict with the reference's keys (Linear weights [in, out]); offsets of a cell or two."""
    rng = np.random.default_rng(CASES[tag]["seed"] + 2)
    st = {}
    for k, (n_in, n_out) in _attention_keys(tag).items():
        scale = 1.5 if k.endswith("sampling_offsets") else 1.0
        st[k + ".weight"] = (rng.standard_normal((n_in, n_out)) * scale / np.sqrt(n_in)).astype(np.float32)
        st[k + ".bias"] = (rng.standard_normal(n_out) * (1.5 if scale > 1 else 0.1)).astype(np.float32)
    for i in range(LAYERS):
        for j in range(3):
            st[f"layers.{i}.norms.{j}.weight"] = rng.uniform(0.5, 1.5, EMBED).astype(np.float32)
            st[f"layers.{i}.norms.{j}.bias"] = (rng.standard_normal(EMBED) * 0.1).astype(np.float32)
    return st


def encoder_cfg(tag):
    """Constructor arguments of paddle3d_amd.bevformer.BEVFormerEncoder for the case (the reference's config layout)."""
    c = CASES[tag]
    tsa = dict(type_name="TemporalSelfAttention", embed_dims=EMBED, num_heads=HEADS, num_levels=1,
               num_points=c["tsa_P"])
    sca = dict(type_name="SpatialCrossAttention", embed_dims=EMBED, num_cams=c["cams"], pc_range=PC_RANGE,
               deformable_attention=dict(type_name="MSDeformableAttention3D", embed_dims=EMBED, num_heads=HEADS,
                                         num_points=c["P"], num_levels=len(c["levels"])))
    layer = dict(type_name="BEVFormerLayer", attn_cfgs=[tsa, sca], feedforward_channels=FFN_CH, ffn_dropout=0.1,
                 operation_order=ORDER)
    return dict(transformerlayers=layer, num_layers=LAYERS, point_cloud_range=PC_RANGE, num_points_in_pillar=c["D"],
                return_intermediate=False)


def load():
    return dict(np.load(OUT))


def check_conditions(g, tag):
    """The conditions the maker writes the file under; returns what it saw."""
    c = CASES[tag]
    uv, z, mask = g[f"{tag}_reference_points_cam"], g[f"{tag}_depth"], g[f"{tag}_bev_mask"].astype(bool)
    assert np.array_equal(mask, g[f"{tag}_bev_mask_fp32"].astype(bool)), "the float32 and float64 masks differ"
    for edge in (0.0, 1.0):
        assert np.abs(uv - edge).min() > 1e-4, (tag, "u or v within 1e-4 of", edge)
    assert not ((z > EPS / 10) & (z < EPS * 10)).any(), (tag, "a depth within a factor of 10 of eps")
    hit = mask.any(-1)  # [cams, B, Q]
    count = hit.sum(0)
    share = (count >= 1).mean(-1)
    assert ((share >= 0.25) & (share <= 0.95)).all(), (tag, share)
    seen = dict(counts=sorted(set(count.reshape(-1).tolist())), share=share.round(3).tolist(),
                partial=int((hit & ~mask.all(-1)).sum()), behind=int((z < EPS).sum()),
                outside=float(g[f"{tag}_outside_share"]))
    assert seen["outside"] > 0, (tag, "no sampled location outside every level")
    if tag == "a":
        assert set(seen["counts"]) >= {0, 1, 2, 3}, seen
        assert seen["partial"] > 0 and seen["behind"] > 0, seen
    for cam in c["planted"]:
        assert not hit[cam].any(), (tag, cam, "the planted camera sees something")
    if c["prev"] == "zero":
        assert not inputs(tag)["prev_bev"].any()
    return seen


# ---- the reference run (needs the reference checkout) ---------------------------------------------------------------


def _reference(tag, dt):
    """One run of the reference's methods in dtype `dt` (torch.float32 as written, torch.float64 with the shim's
    float32 remapped), frame by frame -> {name: array stacked over the frames}."""
    import paddle_shim as ps

    p = ps.install(REF)
    import paddle.nn.functional as F

    ps._DT["float32"] = dt
    p.float32 = dt
    p.maximum = lambda a, b: ps._wrap(torch.maximum(a, b))
    p.full_like = lambda x, v, dtype=None: ps._wrap(torch.full_like(x, v, dtype=ps._dt(dtype)))
    try:
        return _run(tag, dt, ps, p, F)
    finally:
        ps._DT["float32"] = torch.float32


def _run(tag, dt, ps, p, F):
    c = CASES[tag]
    st, inp, calib = state(tag), inputs(tag), calibrations(tag)
    sh, lsi, S = levels(tag)
    bev_h, bev_w = c["bev"]
    T = lambda a: ps._wrap(torch.from_numpy(np.ascontiguousarray(a)).to(dt))  # noqa: E731
    I = lambda a: ps._wrap(torch.from_numpy(np.ascontiguousarray(a)))  # noqa: E731
    plain = lambda t: t.as_subclass(torch.Tensor)  # noqa: E731
    outside = []

    def op(value, sampling_locations, attention_weights, spatial_shapes, level_start_index, im2col_step):
        a = [plain(t).detach().double() for t in (value, sampling_locations, attention_weights)]
        loc = a[1].numpy()
        if loc.shape[3] * loc.shape[4] == len(c["levels"]) * c["P"] and a[0].shape[0] == c["cams"]:
            outside.append(float((~((loc >= 0) & (loc <= 1)).all(-1)).mean()))
        out = md.grid_sample_attn(*a, plain(spatial_shapes).numpy(), plain(level_start_index).numpy())
        return ps._wrap(out.to(dt))

    common = dict(paddle=p, F=F, ms_deform_attn=types.SimpleNamespace(ms_deform_attn=op), masked_fill=None, copy=copy,
                  warnings=warnings)
    ex = lambda path, lines: ps.exec_lines(os.path.join(REF, TR, path), [lines], dict(common))  # noqa: E731
    enc = ex("encoders.py", (69, 117))
    enc.update(ex("encoders.py", (120, 176)))
    enc_forward = ex("encoders.py", (178, 302))["forward"]
    layer_forward = ex("encoder_layers.py", (259, 381))["forward"]
    sca_forward = ex("attentions/spatial_cross_attention.py", (81, 212))["forward"]
    msda_forward = ex("attentions/spatial_cross_attention.py", (310, 428))["forward"]
    tsa_forward = ex("attentions/temporal_self_attention.py", (140, 279))["forward"]

    def linear(key, tap=None):
        w, b = torch.from_numpy(st[key + ".weight"]).to(dt), torch.from_numpy(st[key + ".bias"]).to(dt)

        def f(x):
            if tap is not None:
                tap.append(plain(x).detach().clone())
            return ps._wrap(torch.matmul(plain(x), w) + b)

        return f

    ident = lambda x: x  # noqa: E731
    taps = {"sca": [], "tsa": []}

    def layer_self(i):
        t, s = f"layers.{i}.attentions.0.", f"layers.{i}.attentions.1."
        tsa = types.SimpleNamespace(num_heads=HEADS, num_levels=1, num_points=c["tsa_P"], num_bev_queue=2, im2col_step=64,
                                    batch_first=True, dropout=ident, value_proj=linear(t + "value_proj"),
                                    sampling_offsets=linear(t + "sampling_offsets"),
                                    attention_weights=linear(t + "attention_weights"),
                                    output_proj=linear(t + "output_proj", taps["tsa"]))
        d = s + "deformable_attention."
        msda = types.SimpleNamespace(num_heads=HEADS, num_levels=len(c["levels"]), num_points=c["P"], im2col_step=64,
                                     batch_first=True, value_proj=linear(d + "value_proj"),
                                     sampling_offsets=linear(d + "sampling_offsets"),
                                     attention_weights=linear(d + "attention_weights"))
        sca = types.SimpleNamespace(num_cams=c["cams"], embed_dims=EMBED, dropout=ident,
                                    output_proj=linear(s + "output_proj", taps["sca"]),
                                    deformable_attention=lambda **kw: msda_forward(msda, **kw))
        norms = []
        for j in range(3):
            w, b = (torch.from_numpy(st[f"layers.{i}.norms.{j}.{n}"]).to(dt) for n in ("weight", "bias"))
            norms.append(lambda x, w=w, b=b: ps._wrap(torch.nn.functional.layer_norm(plain(x), (EMBED,), w, b, 1e-5)))
        fc1, fc2 = linear(f"layers.{i}.ffns.0.layers.0.0"), linear(f"layers.{i}.ffns.0.layers.1")
        ffn = lambda x, identity=None: (x if identity is None else identity) + fc2(torch.relu(fc1(x)))  # noqa: E731
        return types.SimpleNamespace(operation_order=ORDER, pre_norm=False, num_attn=2, norms=norms, ffns=[ffn],
                                     attentions=[lambda *a, **k: tsa_forward(tsa, *a, **k),
                                                 lambda *a, **k: sca_forward(sca, *a, **k)]), tsa, sca

    layers = [layer_self(i) for i in range(LAYERS)]
    encoder = types.SimpleNamespace(point_cloud_range=PC_RANGE, num_points_in_pillar=c["D"], return_intermediate=False,
                                    get_reference_points=enc["get_reference_points"],
                                    layers=[(lambda *a, _l=l[0], **k: layer_forward(_l, *a, **k)) for l in layers])
    encoder.point_sampling = lambda *a: enc["point_sampling"](encoder, *a)
    res = {k: [] for k in RESULTS + ("reference_points_cam", "bev_mask", "depth")}
    z_range = PC_RANGE[5] - PC_RANGE[2]
    with torch.no_grad():
        for b in range(c["B"]):
            metas = [dict(lidar2img=[T(m) for m in calib[b]], img_shape=[IMG_SHAPE] * c["cams"])]
            ref_3d = enc["get_reference_points"](bev_h, bev_w, z_range, c["D"], dim="3d", bs=1, dtype=dt)
            ref_2d = enc["get_reference_points"](bev_h, bev_w, dim="2d", bs=1, dtype=dt)
            ref_cam, mask = encoder.point_sampling(ref_3d, PC_RANGE, metas)
            res["reference_points_cam"].append(ref_cam.numpy()[:, 0])
            res["bev_mask"].append(mask.numpy()[:, 0])
            pts = plain(ref_3d)[0].double().numpy() * (np.asarray(PC_RANGE[3:]) - PC_RANGE[:3]) + PC_RANGE[:3]  # [D, Q, 3]
            depth = np.einsum("ck,dqk->cqd", calib[b][:, 2, :3].astype(np.float64), pts) + calib[b][:, 2, 3, None, None]
            res["depth"].append(depth)
            q, pos, prev = (T(inp[k][b:b + 1]) for k in ("bev_query", "bev_pos", "prev_bev"))
            feats = T(inp["feats"][:, :, b:b + 1])
            shift = T(inp["shift"][b:b + 1])
            sh_t, lsi_t = I(sh), I(lsi)
            _, tsa, sca = layers[0]
            for k in taps:
                taps[k].clear()
            out = sca_forward(sca, q, feats, feats, reference_points_cam=ref_cam, bev_mask=mask, spatial_shapes=sh_t,
                              level_start_index=lsi_t)
            res["sca_sample"].append(taps["sca"][0].numpy()[0])
            res["sca_out"].append(out.numpy()[0])
            hybrid = p.stack([ref_2d + shift[:, None, None, :]] * 2, 1).reshape([2, bev_h * bev_w, 1, 2])
            value = p.stack([prev, q], 1).reshape([2, bev_h * bev_w, EMBED])
            bev_sh, bev_lsi = I(np.array([[bev_h, bev_w]], np.int64)), I(np.zeros(1, np.int64))
            out = tsa_forward(tsa, q, value, value, None, query_pos=pos, reference_points=hybrid, spatial_shapes=bev_sh,
                              level_start_index=bev_lsi)
            res["tsa_sample"].append(taps["tsa"][0].numpy()[0])
            res["tsa_out"].append(out.numpy()[0])
            out = layer_forward(layers[0][0], q, feats, feats, bev_pos=pos, ref_2d=hybrid, ref_3d=ref_3d, bev_h=bev_h,
                                bev_w=bev_w, spatial_shapes=sh_t, level_start_index=lsi_t, reference_points_cam=ref_cam,
                                bev_mask=mask, prev_bev=value)
            res["layer_out"].append(out.numpy()[0])
            out = enc_forward(encoder, q.transpose([1, 0, 2]), feats, feats, bev_h=bev_h, bev_w=bev_w,
                              bev_pos=pos.transpose([1, 0, 2]), spatial_shapes=sh_t, level_start_index=lsi_t,
                              prev_bev=prev.transpose([1, 0, 2]), shift=shift, img_metas=metas)
            res["encoder_out"].append(out.numpy()[0])
    out = {k: np.stack(v, 1 if k in ("reference_points_cam", "bev_mask", "depth") else 0) for k, v in res.items()}
    out["outside_share"] = np.float64(np.mean(outside))
    return out


def main():
    out = {}
    for tag in TAGS:
        r32, r64 = _reference(tag, torch.float32), _reference(tag, torch.float64)
        assert r32["reference_points_cam"].dtype == np.float32 and r64["encoder_out"].dtype == np.float64
        out[f"{tag}_lidar2img"] = calibrations(tag)
        out[f"{tag}_bev_mask"] = r64["bev_mask"].astype(np.uint8)
        out[f"{tag}_bev_mask_fp32"] = r32["bev_mask"].astype(np.uint8)
        out[f"{tag}_depth"] = r64["depth"]
        out[f"{tag}_outside_share"] = r64["outside_share"]
        uv32, uv64 = r32["reference_points_cam"], r64["reference_points_cam"]
        front = np.broadcast_to((r64["depth"] > EPS)[..., None], uv64.shape)
        out[f"{tag}_reference_points_cam"] = uv64
        out[f"{tag}_reference_points_cam_bound"], _ = bound(uv32[front], uv64[front])
        rel = np.abs(uv32[~front].astype(np.float64) - uv64[~front]) / np.abs(uv64[~front])
        out[f"{tag}_reference_points_cam_rel_bound"] = np.float64(max(4.0 * rel.max(), float(np.finfo(np.float32).eps)))
        for k in RESULTS:
            out[f"{tag}_{k}"] = r64[k]
            out[f"{tag}_{k}_bound"], out[f"{tag}_{k}_ref_err"] = bound(r32[k], r64[k])
            print(f"{tag} {k} {r64[k].shape}: |max| {np.abs(r64[k]).max():.3f}, the reference's own error "
                  f"{float(out[f'{tag}_{k}_ref_err']):.3e}, bound {float(out[f'{tag}_{k}_bound']):.3e}")
        print(tag, "reference_points_cam bound", float(out[f"{tag}_reference_points_cam_bound"]), "relative behind",
              float(out[f"{tag}_reference_points_cam_rel_bound"]), check_conditions(out, tag))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
