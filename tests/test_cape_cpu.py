"""CAPE / CAPE-T's attention layers without a GPU: the NumPy restatement of csrc/cape.hip (tests/golden/cape_numpy.py) and
the torch form of the modules of paddle3d_amd.cape (fused=False, which is also what fused=True runs on the CPU) against
what the reference's own Python computed (tests/golden/python_cape.npz), within the bounds the maker stored: 4 x the
reference's own fp32 error.  Also: the divisors of the sine embedding against the reference's (one float32 ulp: a
correctly working powf is no further from another), the state-dict keys against the reference's, a synthetic .pdparams
loading strictly (the transformer's with dn_query_embedding kept), the 2-layer CAPETransformer in both time settings,
position_embeding's coordinates and coords_mask and MLP_Fusion with Ego_emb within their bounds, a wholly masked row
being NaN and an Inf under a masked key reaching the output in both forms as in the reference, the predicates' borders,
and the entry points' refusals and statuses, which need no device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import cape_numpy as cn  # noqa: E402
import make_cape_golden as mk  # noqa: E402

F32 = np.float32
TAGS = mk.TAGS


@pytest.fixture(scope="module")
def golden():
    return mk.load()


def _libm(op):
    from oracle import pyoracle as O

    return lambda x: O.libm_eval(op, np.ascontiguousarray(x, F32).reshape(-1))


@pytest.fixture(scope="module")
def expf():
    return _libm(2)


@pytest.fixture(scope="module")
def sincos():
    return _libm(0), _libm(1)


def check_result(golden, tag, name, got):
    want, bound = golden[f"{tag}_{name}"], float(golden[f"{tag}_{name}_bound"])
    assert got.shape == want.shape and got.dtype == F32, (name, got.shape, want.shape, got.dtype)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{tag} {name} err {err:.3e} bound {bound:.3e} (reference's own {float(golden[f'{tag}_{name}_ref_err']):.3e})")
    assert err <= bound, (tag, name, err, bound)


# ---- the modules under the reference's parameters ---------------------------------------------------------------------

_MODULES = {"QcR": lambda c, fused: ("QcR_Modulation", (mk.HIDDEN,), {}),
            "V_R": lambda c, fused: ("V_R_Modulation", (mk.HIDDEN,), {}),
            "fpe": lambda c, fused: ("SELayer", (mk.HIDDEN,), {}),
            "cross_attend": lambda c, fused: ("CrossAttention", (mk.HIDDEN, c["heads"], c["dim_head"], True),
                                              dict(fused=fused)),
            "cva": lambda c, fused: ("CrossViewAttention", (c["Q"], mk.HIDDEN, True),
                                     dict(heads=c["heads"], dim_head=c["dim_head"], conditional=True, fused=fused)),
            "cva0": lambda c, fused: ("CrossViewAttention", (c["Q"], mk.HIDDEN, True),
                                      dict(heads=c["heads"], dim_head=c["dim_head"], conditional=None, fused=fused))}


def module_state(golden, tag, name):
    """The reference's keys of module `name` with the maker's seeded values (prefix stripped)."""
    shapes = mk.key_shapes(golden, tag, name)
    st = mk.state(tag, {f"{name}.{k}": s for k, s in shapes.items()})
    return {k[len(name) + 1:]: v for k, v in st.items()}


def build(golden, tag, name, fused=False):
    from paddle3d_amd import cape
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    cls, args, kw = _MODULES[name](mk.CASES[tag], fused)
    mod = getattr(cape, cls)(*args, **kw)
    assert load_paddle_state_dict(mod, module_state(golden, tag, name)) == []
    return mod.eval()


def tensors(tag, dev="cpu"):
    return {k: torch.from_numpy(v).to(dev) for k, v in mk.inputs(tag).items()}


def module_outputs(golden, tag, fused, dev="cpu"):
    """Every stored result of the modules for one case."""
    from paddle3d_amd import cape

    i = tensors(tag, dev)
    out = {}
    with torch.no_grad():
        out["posemb"] = cape.pos2posemb3d(i["ref_points"], mk.POS_FEATS, fused=fused)
        out["posemb_world"] = cape.world_posemb3d(i["ref_points"], mk.BOUND, i["R"], i["t"], 8, fused=fused)
        out["qcr"] = build(golden, tag, "QcR").to(dev)(i["x"], i["R"])
        out["v_r"] = build(golden, tag, "V_R").to(dev)(i["feature"], i["R"])
        out["se"] = build(golden, tag, "fpe").to(dev)(i["img_embed"], i["feature"])
        k_a, q_a = i["feature"] + i["camera_pe"][:, :, None], i["x"] + i["lidar_obj_pe"]
        ca = build(golden, tag, "cross_attend", fused).to(dev)
        out["ca"] = ca(i["img_embed"], i["bev_embed"], k_a, q_a, i["feature"], i["mask"])
        p = ca.proj_dict
        out["ca_core"] = ca.core(p["k_g"](i["img_embed"]), p["q_g"](i["bev_embed"]), p["k_a"](k_a), p["q_a"](q_a),
                                 p["v"](i["feature"]), i["mask"])
        for name in ("cva", "cva0"):
            layer = build(golden, tag, name, fused).to(dev)
            out[name] = layer(i["x"], out["qcr"], i["lidar_obj_pe"], i["feature"], i["camera_pe"], i["mask"],
                              i["img_embed"], i["bev_embed"], None)
    return {k: v.cpu().numpy() for k, v in out.items() if k in mk.results(tag)}


# ---- the transformer under the reference's parameters -----------------------------------------------------------------


def build_transformer(golden, tag, fused=False):
    from paddle3d_amd import cape
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    c = mk.CASES[tag]
    att = cape.CrossViewAttention(c["Q"], mk.HIDDEN, True, heads=c["heads"], dim_head=c["dim_head"], fused=fused)
    tr = cape.CAPETransformer(att_layer=att, fused=fused, **mk.tr_args(tag))
    st = module_state(golden, tag, "tr")
    st.update({k: tr.state_dict()[k].numpy() for k in mk.BUFFERS})  # the constructor's own (checked against the keys)
    assert load_paddle_state_dict(tr, st) == []
    return tr.eval()


def build_fusion(golden, tag):
    from paddle3d_amd import cape
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    mf = cape.MLP_Fusion(mk.HIDDEN)
    assert load_paddle_state_dict(mf, module_state(golden, tag, "mf")) == []
    return mf.eval()


def transformer_outputs(golden, tag, fused, dev="cpu"):
    """Every stored result of the transformer for one case, and coords_mask."""
    from paddle3d_amd import cape

    ti = {k: torch.from_numpy(v).to(dev) for k, v in mk.tr_inputs(tag).items()}
    tc = mk.TR_CASES[tag]
    tr = build_transformer(golden, tag, fused).to(dev)
    out = {}
    with torch.no_grad():
        ego = cape.curlidar2prevlidar(ti["ext_cur"].T, ti["ext_prev"].T)
        n = tc["cams"]
        coords, cmask = tr.coords3d(ti["I_inv"].reshape(-1, n, 3, 3), mk.FEAT, mk.TR["image"],
                                    ti["mask"].reshape(-1, n, *mk.FEAT))
        out["coords3d"], out["coords_mask"] = coords, cmask
        args = (ti["feature"], ti["mask"], ti["I_inv"], ti["R_inv"], ti["t"], mk.TR["image"])
        if "tr" in mk.TR_RESULTS[tag]:
            out["tr"], ref = tr(*args)
            assert ref.shape == (1, mk.CASES[tag]["Q"], 3)
        if "tr_time" in mk.TR_RESULTS[tag]:
            out["tr_time"], out["tr_prev"], _ = tr(*args, ego_matrix=ego, return_prev_query=True)
            assert torch.equal(tr(*args, ego_matrix=ego)[0], out["tr_time"]) or dev != "cpu"
            x = tensors(tag, dev)["x"]
            out["mf_a"], out["mf_b"] = build_fusion(golden, tag).to(dev)(x[:1], x[1:], ego)
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_transformer(golden, tag, out):
    assert set(out) == set(mk.TR_RESULTS[tag]) | {"coords_mask"}
    assert out["coords_mask"].dtype == bool and np.array_equal(out["coords_mask"], golden[f"{tag}_coords_mask"])
    for name, got in out.items():
        if name != "coords_mask":
            check_result(golden, tag, name, got)


# ---- the head under the reference's parameters ------------------------------------------------------------------------


def build_head(golden, tag, fused=False):
    from paddle3d_amd import cape
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    c, t = mk.CASES[tag], mk.TR_CASES[tag]
    att = cape.CrossViewAttention(c["Q"], mk.HIDDEN, True, heads=c["heads"], dim_head=c["dim_head"], fused=fused)
    tr = cape.CAPETransformer(att_layer=att, fused=fused, **mk.head_tr_args(tag))
    coder = dict(type_name="NMSFreeCoder", point_cloud_range=mk.PC_RANGE, post_center_range=mk.POST, max_num=mk.MAX_NUM,
                 num_classes=mk.CLASSES)
    head = cape.CAPETemporalDNHead(mk.CLASSES, mk.TR["feat_dim"], num_query=c["Q"], transformer=tr, bbox_coder=coder,
                                   with_time=t["with_time"], with_prev_aux_loss=t["with_time"], code_size=mk.CODE,
                                   fused=fused)
    st = module_state(golden, tag, "head")
    st.update({"transformer." + k: tr.state_dict()[k].numpy() for k in mk.BUFFERS})
    assert load_paddle_state_dict(head, st) == []
    return head.eval()


def head_args(tag, dev="cpu"):
    hi = mk.head_inputs(tag)
    t = lambda k: torch.from_numpy(hi[k]).to(dev)  # noqa: E731
    return ([t("feature")], t("intrinsics"), t("extrinsics"), mk.TR["image"], [hi["img_shape"]],
            t("timestamp") if mk.TR_CASES[tag]["with_time"] else None)


def head_outputs(golden, tag, fused, dev="cpu"):
    """(the head's stored results with every level's branches, get_bboxes' tuple of the default last-level forward)"""
    head = build_head(golden, tag, fused).to(dev)
    args = head_args(tag, dev)
    with torch.no_grad():
        every = head(*args, all_levels=True)
        last = head(*args)
        det = head.get_bboxes(last)
    for k in ("all_cls_scores", "all_bbox_preds"):  # the default computes the last decoder level's branches only
        assert last[k].shape[0] == 1 and every[k].shape[0] == mk.TR["layers"]
        assert torch.equal(last[k][0], every[k][-1]) or dev != "cpu"
    return (dict(head_cls=every["all_cls_scores"].cpu().numpy(), head_bbox=every["all_bbox_preds"].cpu().numpy()),
            tuple(t.cpu().numpy() for t in det))


def check_head(golden, tag, out, det):
    from test_bevformer_decoder_cpu import check_decode

    for name, got in out.items():
        check_result(golden, tag, name, got)
    check_decode(golden, tag, "head", *det)  # labels, counts and row order (the labels' and boxes' order) equal


def ca_rows(golden, tag):
    """The projected rows CrossAttention hands its core, float32 NumPy: (q_a, q_g, k_a, k_g, v, scale_a, scale_g, mask)."""
    i = tensors(tag)
    ca = build(golden, tag, "cross_attend")
    p = ca.proj_dict
    with torch.no_grad():
        k_a, q_a = i["feature"] + i["camera_pe"][:, :, None], i["x"] + i["lidar_obj_pe"]
        rows = (p["q_a"](q_a), p["q_g"](i["bev_embed"]), p["k_a"](k_a), p["k_g"](i["img_embed"]), p["v"](i["feature"]),
                ca.scale_a, ca.scale_g)
    return tuple(t.detach().numpy() for t in rows) + (mk.inputs(tag)["mask"],)


# ---- the restatement against the reference ----------------------------------------------------------------------------


@pytest.mark.parametrize("tag", TAGS)
def test_restated_attention_against_the_reference(golden, expf, tag):
    q_a, q_g, k_a, k_g, v, sa, sg, mask = ca_rows(golden, tag)
    got = cn.cva(q_a, q_g, k_a, k_g, v, sa, sg, mk.CASES[tag]["heads"], expf, mask)
    check_result(golden, tag, "ca_core", got)


@pytest.mark.parametrize("tag", TAGS)
def test_restated_posemb3d_against_the_reference(golden, sincos, tag):
    from paddle3d_amd.ops import cape as ops

    i = mk.inputs(tag)
    check_result(golden, tag, "posemb", cn.posemb3d(i["ref_points"], ops.dim_t(mk.POS_FEATS), *sincos))
    check_result(golden, tag, "posemb_world",
                 cn.posemb3d(i["ref_points"], ops.dim_t(8), *sincos, bound=mk.BOUND, rot=i["R"], trans=i["t"]))


def test_dim_t_is_the_references(golden):
    """The order is the reference's (cape_transformer.py:79-80: 2 * (i // 2) / F in float32, then temperature ** that);
    two correct float32 powers of the same arguments are within one ulp of each other."""
    from paddle3d_amd.ops import cape as ops

    for feats in mk.DIM_T_FEATS:
        want = golden[f"dim_t_{feats}"]
        got = ops.dim_t(feats)
        assert got.dtype == F32 and got.shape == (feats,) and want.dtype == F32
        assert got[0] == 1.0 and got[1] == 1.0
        assert (np.abs(got.astype(np.float64) - want) <= np.spacing(want)).all(), feats
        assert np.array_equal(got[0::2], got[1::2]) and (np.diff(got[0::2]) > 0).all()
        assert np.array_equal(got, cn.dim_t(feats))
    # one ulp is enough to tell the orders apart: the float32 exponent (the reference's) under a correctly rounded power
    # is within one ulp of the stored values, the exponent formed in double is not (F = 96, where 2 k / 96 is inexact)
    want, i = golden["dim_t_96"], np.arange(96)
    ulps = lambda a: float((np.abs(a.astype(np.float64) - want) / np.spacing(want)).max())  # noqa: E731
    e32 = (F32(2) * (i // 2).astype(F32) / F32(96)).astype(F32)
    assert ulps((10000.0 ** e32.astype(np.float64)).astype(F32)) <= 1
    assert ulps((10000.0 ** (2 * (i // 2) / 96.0)).astype(F32)) > 1


# ---- the modules' torch form against the reference --------------------------------------------------------------------


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused_on_cpu"])
@pytest.mark.parametrize("tag", TAGS)
def test_modules_against_the_reference(golden, tag, fused):
    out = module_outputs(golden, tag, fused)
    assert set(out) == set(mk.results(tag))
    for name, got in out.items():
        check_result(golden, tag, name, got)


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused_on_cpu"])
@pytest.mark.parametrize("tag", TAGS)
def test_transformer_against_the_reference(golden, tag, fused):
    """position_embeding's coordinates and coords_mask (every case; c: most of the frustum outside the range), the 2-layer
    transformer without time (a) and with time, 2 x 2 cameras (b), MLP_Fusion with Ego_emb (b)."""
    check_transformer(golden, tag, transformer_outputs(golden, tag, fused))
    assert 0.5 < golden["c_coords_mask"].mean() < 1


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused_on_cpu"])
@pytest.mark.parametrize("tag", sorted(mk.HEAD_CASES))
def test_head_and_decode_against_the_reference(golden, tag, fused):
    """CAPETemporalDNHead.forward's eval path (both levels' branches, the regression tail, with and without time) and
    get_bboxes: labels, counts and row order equal to the reference's, boxes and scores within the bounds."""
    check_head(golden, tag, *head_outputs(golden, tag, fused))
    assert int(golden[f"{tag}_head_count"][0]) == mk.MAX_NUM


def test_head_state_dict_keys_and_strict_load(golden, tmp_path):
    from paddle3d_amd.checkpoint import load_paddle_state_dict, save_pdparams

    for tag in sorted(mk.HEAD_CASES):
        head = build_head(golden, tag)
        ref = mk.key_shapes(golden, tag, "head")
        assert set(head.state_dict()) == set(ref), set(head.state_dict()) ^ set(ref)
        assert {"code_weights", "cls_branches.5.6.bias", "reg_branches.0.4.weight", "transformer.dn_query_embedding.2.bias",
                "cls_branches.2.1.weight"} <= set(ref)
    st = module_state(golden, "b", "head")
    st.update({"transformer." + k: head.transformer.state_dict()[k].numpy() for k in mk.BUFFERS})
    path = str(tmp_path / "head.pdparams")
    save_pdparams(st, path)
    fresh = build_head(golden, "b")
    assert load_paddle_state_dict(fresh, path) == []
    assert np.array_equal(fresh.reg_branches[5][4].weight.detach().numpy(), st["reg_branches.5.4.weight"].T)
    assert "transformer.mf.1.proj_v_b.weight" in st and not fresh.code_weights.requires_grad


def test_constructors_carry_the_three_yaml_files_numbers():
    """configs/cape/*.yml (copied as settings under tests/golden/cape_configs) against cape_r50_1408x512(),
    capet_r50_704x256() and capet_vovnet_800x320(): the head's and the transformer's blocks and the coder's."""
    import yaml

    from paddle3d_amd import cape

    files = {"cape_r50_1408x512": "cape_r50_1408x512_24ep_wocbgs_imagenet_pretrain.yml",
             "capet_r50_704x256": "capet_r50_704x256_24ep_wocbgs_imagenet_pretrain.yml",
             "capet_vovnet_800x320": "capet_vovnet_800x320_24ep_wocbgs_load_dd3d_pretrain.yml"}
    for name, fn in files.items():
        cfg = yaml.safe_load(open(os.path.join(HERE, "golden", "cape_configs", fn)))["model"]
        assert cfg["type"] == "CAPE"
        h, t, a = cfg["pts_bbox_head"], cfg["pts_bbox_head"]["transformer"], cfg["pts_bbox_head"]["transformer"]["att_layer"]
        model = getattr(cape, name)(fused=False)
        head, tr = model.pts_bbox_head, model.pts_bbox_head.transformer
        assert h["type"] == "CAPETemporalDNHead" and t["type"] == "CAPETransformer" and a["type"] == "CrossViewAttention"
        assert (head.num_classes, head.in_channels, head.num_query) == (h["num_classes"], h["in_channels"], h["num_query"])
        assert (head.with_time, head.with_prev_aux_loss) == (h["with_time"], h.get("with_prev_aux_loss", False))
        assert head.code_weights.tolist() == h["code_weights"] and not h["normedlinear"]
        assert (tr.num_cameras, len(tr.cva_layers), tr.feat_dim, tr.depth_start, tr.depth_num, tr.with_fpe) == \
            (t["num_cameras"], t["num_layers"], t["feat_dim"], t["depth_start"], t["depth_num"], t["with_fpe"])
        assert tr.bound_host == t["bound"] and tr.with_time == h["with_time"] == cape.TRANSFORMER_CONFIGS[name][2]
        hh, ww = t["image_height"] // t["feat_stride"], t["image_width"] // t["feat_stride"]
        assert cape.TRANSFORMER_CONFIGS[name][:2] == (t["image_height"], t["image_width"])
        assert tuple(tr.image_plane.shape) == (hh * ww, 3) and tr.image_plane[0].tolist() == [t["feat_stride"] / 2] * 2 + [1]
        layer = tr.cva_layers[-1]
        assert (layer.num_queries, layer.hidden_dim, layer.heads, layer.cross_attend.dim_head) == \
            (a["num_queries"], a["hidden_dim"], a["heads"], a["dim_head"])
        assert (layer.conditional is not None) == a["conditional"] and tr.cva_layers[0].conditional is None
        assert (layer.cross_attend.proj_dict["q_g"].bias is not None) == a["qkv_bias"]
        b = h["bbox_coder"]
        coder = head.bbox_coder
        assert b["type"] == "NMSFreeCoder" and (coder.max_num, coder.num_classes) == (b["max_num"], b["num_classes"])
        assert coder.post_center_range == b["post_center_range"] and coder.point_cloud_range == b["point_cloud_range"]
        assert head.pc_range == b["point_cloud_range"] and coder.voxel_size == b["voxel_size"]


def test_transformer_state_dict_keys_and_strict_load(golden, tmp_path):
    from paddle3d_amd.checkpoint import load_paddle_state_dict, save_pdparams
    from torch import nn

    for tag in ("a", "b"):
        tr = build_transformer(golden, tag)
        ref = mk.key_shapes(golden, tag, "tr")
        own = {k: list(v.shape) for k, v in tr.state_dict().items()}
        assert set(own) == set(ref), (tag, set(own) ^ set(ref))
        linear = {n + ".weight" for n, m in tr.named_modules() if isinstance(m, nn.Linear)}
        assert all((s[::-1] if k in linear else s) == ref[k] for k, s in own.items())
        assert ("mf.1.ego_emb.ego_emb.0.weight" in own) == (tag == "b")
        assert {"dn_query_embedding.0.weight", "image_plane", "bound", "cam_bound", "cva_layers.1.conditional.layers.0.bias",
                "reference_points.weight", "position_encoder.2.bias"} <= set(own)
        assert not [k for k in own if k.startswith("cva_layers.0.conditional")]  # None on layer 0, as the reference sets it
    path = str(tmp_path / "tr.pdparams")
    st = module_state(golden, "b", "tr")
    st.update({k: tr.state_dict()[k].numpy() for k in mk.BUFFERS})
    save_pdparams(st, path)  # a synthetic .pdparams under the reference's names, training-only branches included
    fresh = build_transformer(golden, "b")
    assert load_paddle_state_dict(fresh, path) == []
    assert np.array_equal(fresh.dn_query_embedding[2].weight.detach().numpy(), st["dn_query_embedding.2.weight"].T)
    with pytest.raises(RuntimeError, match="without a place"):
        load_paddle_state_dict(fresh, {**st, "mf.2.fc.0.bias": np.zeros(mk.HIDDEN, F32)})
    assert np.array_equal(tr.image_plane.numpy()[:2], [[16, 16, 1], [48, 16, 1]])


def test_state_dict_keys_are_the_references(golden, tmp_path):
    from paddle3d_amd.checkpoint import load_paddle_state_dict, save_pdparams
    from torch import nn

    for name in _MODULES:
        mod = build(golden, "a", name)
        ref = mk.key_shapes(golden, "a", name)
        own = {k: list(v.shape) for k, v in mod.state_dict().items()}
        assert set(own) == set(ref), (name, set(own) ^ set(ref))
        linear = {n + ".weight" for n, m in mod.named_modules() if isinstance(m, nn.Linear)}
        for k, s in own.items():
            assert (s[::-1] if k in linear else s) == ref[k], (name, k, s, ref[k])
    ref = mk.key_shapes(golden, "a", "cva")
    assert {f"cross_attend.proj_dict.{n}.{w}" for n in ("q_g", "k_g", "q_a", "k_a", "v") for w in ("weight", "bias")} | \
        {"cross_attend.scale_a", "cross_attend.scale_g", "sl_layer.q_proj.weight", "conditional.layers.1.bias"} <= set(ref)
    assert not [k for k in mk.key_shapes(golden, "a", "cva0") if k.startswith("conditional")]
    # a synthetic .pdparams under the reference's names loads strictly, and a foreign key is refused
    path = str(tmp_path / "cva.pdparams")
    st = module_state(golden, "b", "cva")
    save_pdparams(st, path)
    from paddle3d_amd import cape

    c = mk.CASES["b"]
    mod = cape.CrossViewAttention(c["Q"], mk.HIDDEN, True, heads=c["heads"], dim_head=c["dim_head"])
    assert load_paddle_state_dict(mod, path) == []
    assert np.array_equal(mod.cross_attend.scale_g.detach().numpy(), st["cross_attend.scale_g"])
    assert np.array_equal(mod.sl_layer.k_proj.weight.detach().numpy(), st["sl_layer.k_proj.weight"].T)
    save_pdparams(dict(st, **{"cross_attend.scale_b": st["cross_attend.scale_a"]}), path)
    with pytest.raises(RuntimeError, match="without a place"):
        load_paddle_state_dict(mod, path)


# ---- the reference's special rows, in both forms ----------------------------------------------------------------------


def _torch_core(q_a, q_g, k_a, k_g, v, sa, sg, heads, mask):
    from paddle3d_amd import cape

    ca = cape.CrossAttention(q_a.shape[-1], heads, q_a.shape[-1] // heads, True, fused=False).eval()
    with torch.no_grad():
        ca.scale_a.copy_(torch.from_numpy(sa))
        ca.scale_g.copy_(torch.from_numpy(sg))
        t = lambda a: torch.from_numpy(a)  # noqa: E731
        return ca.core_torch(t(k_g), t(q_g), t(k_a), t(q_a), t(v), None if mask is None else t(mask)).numpy()


def test_masked_rows_and_infinities_follow_the_reference(expf):
    rng = np.random.default_rng(3)
    B, N, Q, K, M, d = 2, 2, 5, 17, 2, 16
    f = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    q_a, q_g, k_a, k_g, v = f(B, Q, M * d), f(B, N, Q, M * d), f(B, N, K, M * d), f(B, N, K, M * d), f(B, N, K, M * d)
    sa, sg = np.array([0.25, -0.3], F32), np.array([0.0, 0.2], F32)
    mask = np.zeros((B, N, K), bool)
    mask[1] = True          # every key of frame 1: its rows are NaN, as the reference's softmax of -inf everywhere
    mask[0, 1, 4] = True
    v[0, 1, 4, 3] = np.inf  # under a masked key: 0 * inf is a NaN in channel 3 of head 0
    for form in (lambda *a: cn.cva(*a[:8], expf, a[8]), _torch_core):
        out = form(q_a, q_g, k_a, k_g, v, sa, sg, M, mask)
        assert np.isnan(out[1]).all()
        nan0 = np.isnan(out[0])
        assert nan0[:, 3].all() and int(nan0.sum()) == Q
    # an Inf under an unmasked key whose weight underflowed to 0
    v[0, 1, 4, 3] = 1.0
    q_a[0, :, :d] = np.abs(q_a[0, :, :d]) * 30  # head 0 of frame 0: the score of key (0, 2) is thousands below the row's
    k_a[0, 0, 2, :d] = -40.0                    # maximum, and its weight exactly 0
    v[0, 0, 2, 5] = np.inf
    for form in (lambda *a: cn.cva(*a[:8], expf, a[8]), _torch_core):
        out = form(q_a, q_g, k_a, k_g, v, sa, sg, M, mask)
        assert np.isnan(out[0][:, 5]).all() and not np.isnan(out[0][:, :5]).any()


def test_config_transformers_carry_the_configs_numbers():
    """configs/cape/*.yml, transformer block: 6 cameras, 6 layers, feat_dim 256, stride 32, bound +-61.2 / +-10, 64 depth
    bins from 1, 900 queries, hidden 512, 8 heads of 64, conditional, qkv_bias; image sizes and with_time per config."""
    from paddle3d_amd import cape

    assert cape.TRANSFORMER_CONFIGS == {"cape_r50_1408x512": (512, 1408, False), "capet_r50_704x256": (256, 704, True),
                                        "capet_vovnet_800x320": (320, 800, True)}
    tr = cape.cape_transformer("capet_vovnet_800x320", fused=False)
    assert (tr.num_cameras, len(tr.cva_layers), tr.feat_dim, tr.depth_num, tr.depth_start) == (6, 6, 256, 64, 1)
    assert (tr.num_queries, tr.hidden_dim, tr.with_time, tr.with_fpe, len(tr.mf)) == (900, 512, True, True, 6)
    assert tuple(tr.image_plane.shape) == (10 * 25, 3) and tr.bound.flatten().tolist() == pytest.approx(
        [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0])
    assert tr.cam_position_range == [-61.2, -10.0, 1, 61.2, 10.0, 61.2]
    layer = tr.cva_layers[1]
    assert (layer.heads, layer.cross_attend.dim_head, layer.cross_attend.proj_dict["v"].bias is not None) == (8, 64, True)
    assert tr.cva_layers[0].conditional is None and layer.conditional is not None
    assert not cape.cape_transformer("cape_r50_1408x512", fused=False).with_time


def test_fused_argument():
    from paddle3d_amd import cape

    with pytest.raises(ValueError, match="fused"):
        cape.CrossAttention(64, 2, 32, True, fused="yes")
    ca = cape.CrossAttention(64, 2, 32, True, fused="force").eval()
    assert not ca.takes_kernel(torch.zeros(1, 4, 64), 3, 35)  # no device tensor: the torch form
    assert cape.CVA_FUSED_MAX_KEYS >= 1


# ---- predicates, refusals and statuses (no device) --------------------------------------------------------------------


def test_predicates():
    from paddle3d_amd.ops import cape as ops

    assert [d for d in range(1, 200) if ops.cva_supported(d)] == [16, 32, 48, 64, 80, 96, 112, 128]
    assert ops.cva_supported(64, 6, 250, 900) and ops.cva_supported(16, 1, 1, 1)
    assert [f for f in range(0, 135) if ops.posemb3d_supported(f)] == list(range(2, 129, 2))


def test_refusals_and_statuses_need_no_device():
    from paddle3d_amd import _lib
    from paddle3d_amd.ops import cape as ops

    L = _lib.lib()
    buf = np.zeros(64, F32)
    base = (buf.ctypes.data + 15) & ~15  # a 16-byte aligned host address: no entry point below reads through it
    p = C.c_void_p(base)
    null = C.c_void_p(0)
    cva = lambda B, N, Q, K, M, d, q=p: L.pd3_cape_cva_forward(q, p, p, p, p, null, p, p, B, N, Q, K, M, d, p, null)  # noqa: E731
    for d in (1, 8, 24, 144, 256):
        assert cva(1, 1, 1, 1, 1, d) == -3
    assert cva(1, 1, 1, 1, 1, 16, C.c_void_p(base + 4)) == -3  # a misaligned tensor
    assert cva(1, 0, 1, 1, 1, 16) == -1 and cva(1, 1, 1, 0, 1, 16) == -1 and cva(-1, 1, 1, 1, 1, 16) == -1
    assert cva(1, 1, 1, 1, 0, 16) == -1 and cva(1, 1, 1, 1, 1, 0) == -1
    assert cva(0, 1, 1, 1, 1, 16) == 0 and cva(1, 1, 0, 1, 1, 16) == 0  # nothing to do: no launch
    assert cva(1, 1, 1, 1, 1, 16, null) == -1
    dt = ops.dim_t(8)
    dp = C.c_void_p(dt.ctypes.data)
    pos = lambda B, N, Q, F, rot=null, tr=null, dim=dp: L.pd3_cape_posemb3d(p, null, rot, tr, dim, B, N, Q, F, p, null)  # noqa: E731
    assert pos(1, 0, 1, 7) == -3 and pos(1, 0, 1, 130) == -3
    assert pos(1, 0, 1, 0) == -1 and pos(-1, 0, 1, 8) == -1 and pos(1, 0, 1, 8, dim=null) == -1
    assert pos(1, 2, 1, 8) == -1 and pos(1, 0, 1, 8, rot=p, tr=p) == -1 and pos(1, 2, 1, 8, rot=p) == -1
    assert pos(0, 0, 5, 8) == 0 and pos(3, 2, 0, 8, rot=p, tr=p) == 0
    x = torch.zeros(1, 4, 32)
    with pytest.raises(RuntimeError, match="Unsupported device type for cape"):
        ops.cross_view_attention(x, x[:, None], x[:, None], x[:, None], x[:, None], torch.ones(2), torch.ones(2), 2)
    with pytest.raises(RuntimeError, match="Unsupported device type for cape"):
        ops.posemb3d(torch.zeros(1, 4, 3), 8)
