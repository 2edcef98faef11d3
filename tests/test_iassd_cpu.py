"""IA-SSD without a GPU: the NumPy restatement (tests/golden/iassd_numpy.py) against the reference's recorded layers
(tests/golden/python_iassd.npz, made by make_iassd_golden.py), the modules of paddle3d_amd/iassd.py on CPU tensors,
their state-dict keys and constructors, the predicate's borders, and
the statuses that need no device."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import iassd_numpy as ia  # noqa: E402
import make_iassd_golden as mk  # noqa: E402

F32 = np.float32
SA_LAYERS = [i for i, r in enumerate(mk.BACKBONE["radius_list"]) if r]


@pytest.fixture(scope="module")
def golden():
    g = mk.load()
    return g, mk.state(g, "backbone"), mk.state(g, "head")


def torch_pointnet2():
    """Stand-ins for the device ops on CPU tensors: the maker's torch forms."""
    import make_pointnet2_golden as mkp

    return types.SimpleNamespace(
        farthest_point_sample=lambda xyz, m: mkp._fps_torch(xyz, int(m)),
        gather_operation=lambda f, idx: mkp._group_torch(f, idx),
        ball_query_batch=lambda q, p, r, s: mkp._ball_torch(q, p, r, s),
        grouping_operation_batch=lambda f, idx: mkp._group_torch(f, idx))


def pooled_scales(g, st, i, dtype=F32, materialised=False):
    """The layer's scales by the restatement, concatenated: [B, m, sum c3]."""
    xyz, new_xyz = g[f"l{i}_in_xyz"], g[f"l{i}_out_new_xyz"] if i != 5 else g["l5_in_ctr_xyz"]
    feats = np.ascontiguousarray(g[f"l{i}_in_features"].transpose(0, 2, 1))  # [B, N, C]
    outs = []
    for k, (r, s) in enumerate(zip(mk.BACKBONE["radius_list"][i], mk.BACKBONE["nsample_list"][i])):
        w_pos, w_feat, rest = ia.scale_params(st, f"SA_modules.{i}", k)
        if materialised:
            outs.append(ia.sa_msg_pool(new_xyz, xyz, None, w_pos, *rest, r, s, dtype=dtype,
                                       w1_full=np.concatenate([w_pos, w_feat], 1), features=feats))
        else:
            f_in = (feats.astype(dtype) @ w_feat.astype(dtype).T).astype(dtype)
            if dtype is F32:
                f_in = torch.matmul(torch.from_numpy(feats), torch.from_numpy(w_feat).t()).numpy()
            outs.append(ia.sa_msg_pool(new_xyz, xyz, f_in, w_pos, *rest, r, s, dtype=dtype))
    return np.concatenate(outs, -1)


def rows_through(st, prefix, rows, dtype=F32):
    """A Conv1D / BatchNorm1D / ReLU stack (and a last Conv1D with bias) over [rows, C]."""
    k = 0
    while f"{prefix}.{k}.weight" in st:
        w = st[f"{prefix}.{k}.weight"].astype(dtype)
        rows = rows @ w.reshape(w.shape[0], -1).T
        if f"{prefix}.{k}.bias" in st:
            rows = rows + st[f"{prefix}.{k}.bias"].astype(dtype)
        if f"{prefix}.{k + 1}._mean" in st:
            scale, shift = ia.fold_bn(st, f"{prefix}.{k + 1}")
            rows = np.maximum(rows * scale.astype(dtype) + shift.astype(dtype), 0)
        k += 3
    return rows.astype(dtype)


@pytest.mark.parametrize("i", SA_LAYERS)
def test_restatement_equals_the_golden_layers(golden, i):
    """The restated scales, then the aggregation layer, against the reference's recorded layer output within 4 x the
    reference's own fp32 error (the bound the maker stored)."""
    g, st, _ = golden
    pooled = pooled_scales(g, st, i)
    B, m, _ = pooled.shape
    got = rows_through(st, f"SA_modules.{i}.aggregation_layer", pooled.reshape(B * m, -1)).reshape(B, m, -1)
    want = g[f"l{i}_out_new_features"].transpose(0, 2, 1)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(i, "restatement error", err, "bound", float(g[f"l{i}_out_new_features_bound"]))
    assert err <= float(g[f"l{i}_out_new_features_bound"])


@pytest.mark.parametrize("i", SA_LAYERS)
def test_factorised_first_layer_equals_the_materialised_form(golden, i):
    g, st, _ = golden
    m64 = pooled_scales(g, st, i, dtype=np.float64, materialised=True)
    m32 = pooled_scales(g, st, i, materialised=True)
    f32 = pooled_scales(g, st, i)
    ref_err = float(np.abs(m32.astype(np.float64) - m64).max())
    bound = max(4 * ref_err, float(np.spacing(F32(np.abs(m64).max()))))
    err = float(np.abs(f32.astype(np.float64) - m64).max())
    print(i, "factorised", err, "materialised fp32", ref_err)
    assert err <= bound


def test_decode_restatement_equals_the_golden(golden):
    """Columns 0-2 and 6 use exactly rounded operations only: bit for bit.  Columns 3-5 go through exp, where the
    reference's run used another libm: within the stored bound."""
    g = golden[0]
    got = ia.iassd_decode(g["head_batch_cls_preds"], g["head_center_box_preds"], g["head_centers"][:, 1:4],
                          np.asarray(mk.MEAN_SIZE, F32), 12)
    want = g["head_batch_box_preds"]
    for c in (0, 1, 2, 6):
        assert np.array_equal(got[:, c].view(np.uint32), want[:, c].view(np.uint32)), c
    assert float(np.abs(got[:, 3:6].astype(np.float64) - want[:, 3:6]).max()) <= float(g["head_batch_box_preds_bound"])


def build(g, st_b, st_h, fused=False):
    from paddle3d_amd import iassd
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    backbone = iassd.IASSD_Backbone(**mk.backbone_cfg(), fused=fused)
    head = iassd.IASSD_Head(**mk.head_cfg())
    load_paddle_state_dict(backbone, st_b)
    load_paddle_state_dict(head, st_h)
    return iassd.IASSD(backbone, head, mk.POST_CFG).eval()


def test_state_dict_keys_are_the_references(golden):
    g, st_b, st_h = golden
    model = build(g, st_b, st_h)
    for module, st in ((model.backbone, st_b), (model.head, st_h)):
        own = {k.replace(".running_mean", "._mean").replace(".running_var", "._variance"): v
               for k, v in module.state_dict().items() if not k.endswith("num_batches_tracked")}
        assert set(own) == set(st)
        for k, v in own.items():
            shape = tuple(v.shape)
            assert shape == st[k].shape or (len(shape) == 2 and shape[::-1] == st[k].shape), k  # Linear: [in, out]


def test_modules_on_cpu_tensors(golden, monkeypatch):
    """The unfused composition (pointnet2 ops replaced by their torch forms), Vote_layer, the head with the coder's
    torch fall-back: each against the recorded layer from the recorded inputs, within the stored bound."""
    from paddle3d_amd import iassd

    g, st_b, st_h = golden
    monkeypatch.setattr(iassd, "pointnet2_ops", torch_pointnet2())
    model = build(g, st_b, st_h, fused="force")  # CPU tensors never reach the kernel
    T = torch.from_numpy
    with torch.no_grad():
        for i, layer in enumerate(model.backbone.SA_modules):
            a = {k: T(g[f"l{i}_in_{k}"]) for k in ("xyz", "features", "cls_features", "ctr_xyz") if f"l{i}_in_{k}" in g}
            if i == 4:
                vote, empty, origin, off = layer(a["xyz"], a["features"])
                assert tuple(empty.shape) == (2, 16, 0) and origin is a["xyz"]
                assert float((vote - T(g["l4_out_vote_xyz"])).abs().max()) <= float(g["l4_out_vote_xyz_bound"])
                assert float((off - T(g["l4_out_ctr_offsets"])).abs().max()) <= float(g["l4_out_ctr_offsets_bound"])
                continue
            new_xyz, feats, cls = layer(**a)
            assert np.array_equal(new_xyz.numpy(), g[f"l{i}_out_new_xyz"] if i != 5 else g["l5_in_ctr_xyz"])
            assert float((feats - T(g[f"l{i}_out_new_features"])).abs().max()) <= float(g[f"l{i}_out_new_features_bound"])
            if f"l{i}_out_cls_features" in g:
                assert float((cls - T(g[f"l{i}_out_cls_features"])).abs().max()) <= float(g[f"l{i}_out_cls_features_bound"])
            else:
                assert cls is None
        bd = model.head({k: T(g[f"head_{k}"]) for k in ("centers_features", "centers", "ctr_offsets", "centers_origin")}
                        | {"sa_ins_preds": []})
    assert bd["cls_preds_normalized"] is False and torch.equal(bd["batch_index"], T(g["head_batch_index"]))
    for k in ("batch_cls_preds", "batch_box_preds"):
        assert float((bd[k] - T(g[f"head_{k}"])).abs().max()) <= float(g[f"head_{k}_bound"]), k
    # a NaN offset stays a NaN through the clamp, an offset beyond the range is cut to it
    vl = model.backbone.SA_modules[4]
    off = torch.tensor([[[np.nan, 9.0, -9.0]]])
    lim = torch.maximum(torch.minimum(off, vl.max_offset_limit), -vl.max_offset_limit)
    ref = torch.where(off > vl.max_offset_limit, vl.max_offset_limit, off)
    ref = torch.where(ref < -vl.max_offset_limit, -vl.max_offset_limit, ref)
    assert torch.equal(torch.isnan(lim), torch.isnan(ref)) and lim[0, 0, 1:].tolist() == ref[0, 0, 1:].tolist() == [3.0, -2.0]


def test_fused_argument_and_fallbacks():
    from paddle3d_amd import iassd

    kw = dict(npoint=8, sample_range=-1, sample_type="D-FPS", radii=[0.5, 1.0], nsamples=[16, 65],
              mlps=[[1, 16, 16, 32], [1, 16, 24, 32]], aggregation_mlp=[32], confidence_mlp=None, num_classes=3)
    copy_kw = lambda **o: dict({k: ([list(m) for m in v] if k == "mlps" else v) for k, v in kw.items()}, **o)  # noqa: E731
    forced = iassd.SAModuleMSG_WithSampling(**copy_kw(fused="force"))
    assert forced.scale_is_fused(0) and not forced.scale_is_fused(1)  # nsample 65 and width 24: the composition
    default = iassd.SAModuleMSG_WithSampling(**copy_kw())
    assert default.scale_is_fused(0) == ((16, 16, 32, 16) in iassd.MEASURED_FASTER)
    assert not iassd.SAModuleMSG_WithSampling(**copy_kw(fused=False)).scale_is_fused(0)
    assert not iassd.SAModuleMSG_WithSampling(**copy_kw(fused="force", pool_method="avg_pool")).scale_is_fused(0)
    with pytest.raises(NotImplementedError):
        iassd.SAModuleMSG_WithSampling(**copy_kw(dilated_group=True))
    with pytest.raises(ValueError):
        iassd.SAModuleMSG_WithSampling(**copy_kw(fused="yes"))
    assert kw["mlps"][0][0] == 1  # the caller's lists are not edited


def test_constructors_carry_the_configs():
    from paddle3d_amd import iassd

    for make, npoints, cin, car, nms in ((iassd.iassd_kitti, [4096, 1024, 512, 256, None, 256], 4, [3.9, 1.6, 1.56], 0.01),
                                         (iassd.iassd_waymo, [16384, 4096, 2048, 1024, None, 1024], 5, [4.7, 2.1, 1.7], 0.1)):
        m = make()
        b = m.backbone
        assert b.npoint_list == npoints and b.num_point_features == 512 and b.max_translate_range == [3.0, 3.0, 2.0]
        assert b.SA_modules[0].mlps[0][0].in_channels == cin - 3 + 3
        assert [[g.radius for g in l.groupers] for l in b.SA_modules if hasattr(l, "groupers")] == \
            [[0.2, 0.8], [0.8, 1.6], [1.6, 4.8], [], [4.8, 6.4]]
        widths = [[tuple(c.out_channels for c in s if isinstance(c, torch.nn.Conv2d)) for s in l.mlps]
                  for l in b.SA_modules if hasattr(l, "groupers")]
        assert widths == [[(16, 16, 32), (32, 32, 64)], [(64, 64, 128), (64, 96, 128)],
                          [(128, 128, 256), (128, 256, 256)], [], [(256, 256, 512), (256, 512, 1024)]]
        assert m.head.box_coder.mean_size[0].tolist() == pytest.approx(car) and m.head.box_coder.code_size == 30
        assert m.head.cls_center_layers[-1].out_features == 3 and m.head.box_center_layers[-1].out_features == 30
        assert m.post_process_cfg == {"score_thresh": 0.1, "nms_config": {
            "nms_thresh": nms, "nms_pre_maxsize": 4096, "nms_post_maxsize": 500}}
        # layers 1-3 are all supported shapes; the last layer's widths are refused and take the composition
        forced = make(fused="force").backbone.SA_modules
        assert [[l.scale_is_fused(k) for k in range(2)] for l in forced[:3]] == [[True, True]] * 3
        assert [forced[5].scale_is_fused(k) for k in range(2)] == [False, False]


def test_supported_borders():
    from paddle3d_amd.ops import iassd as ops

    for c, ok in ((0, False), (16, True), (17, False), (96, True), (256, True), (272, False)):
        for pos in range(3):
            w = [32, 32, 32]
            w[pos] = c
            assert ops.sa_msg_pool_supported(*w, 16) is ok, (w, ok)
    for s, ok in ((0, False), (1, True), (64, True), (65, False)):
        assert ops.sa_msg_pool_supported(16, 16, 16, s) is ok


def test_statuses_need_no_gpu():
    from paddle3d_amd import _lib, build as b

    b.build()
    L = _lib.lib()
    buf = np.zeros(64, F32)
    p, f = _lib.C.c_void_p(buf.ctypes.data), _lib.C.c_float

    def pool(B=1, m=4, n=8, c1=16, c2=16, c3=16, S=16, ld=None, ptr=p):
        return L.pd3_sa_msg_pool(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, B, m, n, c1, c2, c3, f(0.5), S,
                                 ptr, c3 if ld is None else ld, None)

    for bad in (dict(B=-1), dict(m=-1), dict(n=-1), dict(c1=-16), dict(c2=0), dict(S=0), dict(S=-3), dict(ld=15),
                dict(n=0), dict(ptr=None)):
        assert pool(**bad) == -1, bad
    for bad in (dict(c1=8), dict(c2=17), dict(c3=272), dict(c1=512), dict(S=65), dict(c2=24)):
        assert pool(**bad) == -3, bad
    assert pool(m=0) == 0 and pool(B=0) == 0 and pool(m=0, n=0, ptr=None) == 0

    def decode(m=4, K=3, bins=12, ld=3, ptr=p):
        return L.pd3_iassd_decode(ptr, ptr, ptr, ld, ptr, m, K, bins, ptr, None)

    for bad in (dict(m=-1), dict(K=0), dict(bins=0), dict(ld=2), dict(ptr=None)):
        assert decode(**bad) == -1, bad
    assert decode(m=0) == 0 and decode(m=0, ptr=None) == 0


def test_maker_conditions_hold_on_the_committed_file(golden):
    g = golden[0]
    assert os.path.getsize(mk.OUT) < 1_000_000
    assert max(len(g[f"post_scores{b}"]) for b in range(mk.B)) > 1
    assert g["empty_labels1"].tolist() == [-1.0] and g["empty_scores1"].tolist() == [0.0] and not g["empty_boxes1"].any()
    sc = 1 / (1 + np.exp(-g["head_batch_cls_preds"].astype(np.float64).max(-1)))
    assert np.abs(sc - 0.1).min() >= 1e-3
    for k in g:
        if k.endswith("_bound"):
            assert float(g[k]) >= 4 * float(g[k[:-6] + "_ref_err"])
