"""Golden vectors for IA-SSD at inference: the reference's own Python (models/detection/iassd/) executed through
tests/golden/paddle_shim.py at a small seeded model, in fp32 and in fp64.

    python tests/golden/make_iassd_golden.py        (needs the reference tree; writes python_iassd.npz)

Executed: iassd_modules.py, iassd_backbone.py and iassd_coder.py whole; iassd_head.py's class head with make_fc_layers
(:33-78), generate_predicted_boxes (:606-621) and forward (:623-663); iassd.py's post_process (:136-178) and
class_agnostic_nms (:180-212).  The pointnet2 ops are bound as make_pointnet2_golden.py binds them (the grouping keeps
the dtype, so the fp64 run groups fp64 features), nms_gpu is the oracle's.

The model: B = 2 frames of 512 points with one feature, npoint_list [128, 64, 32, 16, None, 16], the KITTI radii and
nsample, widths scaled down but still mixing 16, 48 and 64.  The parameters come from paddle_shim.fill_state; only their
keys and shapes are stored.  Recorded: every layer's inputs and outputs (fp32), each layer's output in fp64 from the same
fp32 inputs with its error bound (4 x the reference's own fp32 error), the head's logits, encodings and boxes, the
same bound for the whole model run in fp64 from the points on (e2e_*), and
post_process' lists for two cases: "post" (the model's output) and "empty" (frame 1's logits lowered by 12, so that
frame keeps nothing).

Asserted here, so that a correct implementation is never excused: the scores at every ctr_aware cut are distinct across
the cut (and the fp64 run samples the same points); no point lies within a relative 1e-4 of a query sphere in fp64;
every score is at least 1e-3 from score_thresh and every IoU at least 1e-3 from nms_thresh; a frame keeps more than one
box; the "empty" case keeps nothing in frame 1.
"""
import copy
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_pointnet2_golden as mkp  # noqa: E402
import make_roi_head_golden as mkr  # noqa: E402
import paddle_shim as ps  # noqa: E402

REF = "/root/reference"
PKG = os.path.join(REF, "paddle3d/models/detection/iassd")
OUT = os.path.join(HERE, "python_iassd.npz")
SEED = 33  # the first seeds from 31 on that meet every condition asserted in main() are 32 and 33; 33 has NMS drop more

B, N = 2, 512
MEAN_SIZE = [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]
BACKBONE = dict(
    npoint_list=[128, 64, 32, 16, None, 16],
    sample_method_list=["D-FPS", "D-FPS", "ctr_aware", "ctr_aware", None, None],
    radius_list=[[0.2, 0.8], [0.8, 1.6], [1.6, 4.8], [], [], [4.8, 6.4]],
    nsample_list=[[16, 32], [16, 32], [16, 32], [], [], [16, 32]],
    mlps=[[[16, 16, 16], [16, 16, 48]], [[16, 16, 32], [16, 48, 32]], [[32, 32, 64], [16, 48, 64]], [], [32],
          [[64, 64, 64], [48, 48, 64]]],
    layer_types=["SA_Layer", "SA_Layer", "SA_Layer", "SA_Layer", "Vote_Layer", "SA_Layer"],
    dilated_group=[False] * 6, aggregation_mlps=[[32], [32], [64], [64], [], [64]],
    confidence_mlps=[[], [32], [32], [], [], []], layer_input=[0, 1, 2, 3, 4, 3], ctr_index=[-1, -1, -1, -1, -1, 5],
    max_translate_range=[3.0, 3.0, 2.0], input_channel=4, num_classes=3)
HEAD = dict(input_channel=64, cls_fc=[32, 32], reg_fc=[32, 32], num_classes=3,
            target_config={"box_coder_config": {"angle_bin_num": 12, "use_mean_size": True, "mean_size": MEAN_SIZE}},
            loss_config=None)
POST_CFG = {"score_thresh": 0.1, "nms_config": {"nms_thresh": 0.01, "nms_pre_maxsize": 4096, "nms_post_maxsize": 500}}
NUM_LAYERS = 6


def backbone_cfg():
    return copy.deepcopy(BACKBONE)


def head_cfg():
    return copy.deepcopy(HEAD)


def _t(x):
    return x.as_subclass(torch.Tensor) if isinstance(x, torch.Tensor) else torch.as_tensor(x)


def points(rng):
    """[B * N, 5] as (b, x, y, z, intensity): uniform in 8 x 8 x 2 m, about 4 points per cubic metre."""
    xyz = rng.uniform([0, -4, -1], [8, 4, 1], (B, N, 3))
    data = np.concatenate([np.repeat(np.arange(B), N)[:, None], xyz.reshape(-1, 3), rng.uniform(0, 1, (B * N, 1))], 1)
    return data.astype(np.float32)


def _group_keep_dtype(points_, idx):
    pts, ix = _t(points_), _t(idx).long()
    Bn, C, _ = pts.shape
    return torch.gather(pts, 2, ix.reshape(Bn, 1, -1).expand(Bn, C, -1)).reshape((Bn, C) + tuple(ix.shape[1:]))


def build_reference(O):
    """The reference's classes, executed from its files."""
    p = ps.install(REF)
    T, wrap = ps.tensor, ps._wrap

    def nms_gpu(boxes, thresh):
        keep = O.nms(_t(boxes).float().numpy(), float(thresh), kind="ref" if O.have_ref() else "port")
        full = np.zeros(boxes.shape[0], np.int64)
        full[:len(keep)] = keep
        return T(full), T(np.int64(len(keep)))

    class Conv1D(p.nn.Layer):
        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias_attr=None, **_):
            super().__init__()
            self.weight = torch.nn.Parameter(torch.zeros((out_channels, in_channels, kernel_size)))
            self.bias = None if bias_attr is False else torch.nn.Parameter(torch.zeros(out_channels))

        def forward(self, x):
            return torch.nn.functional.conv1d(_t(x), self.weight, self.bias)

    p.nn.Conv1D = Conv1D
    F = sys.modules["paddle.nn.functional"]
    F.max_pool2d = lambda x, kernel_size: wrap(torch.nn.functional.max_pool2d(_t(x), tuple(kernel_size)))
    F.avg_pool2d = lambda x, kernel_size: wrap(torch.nn.functional.avg_pool2d(_t(x), tuple(kernel_size)))
    F.one_hot = lambda x, n: wrap(torch.nn.functional.one_hot(_t(x), int(n)))

    def topk(x, k, axis=-1):
        v, i = torch.topk(_t(x), int(k), dim=int(axis))
        return wrap(v), wrap(i)

    p.topk = topk
    p.nonzero = lambda x: wrap(torch.nonzero(_t(x)))
    p.shape = lambda x: list(x.shape)
    ps.Tensor.cast = lambda self, dtype: self.astype(dtype)
    ps.Tensor.__deepcopy__ = lambda self, memo: wrap(_t(self).clone())  # max_offset_limit, mean_size: plain attributes
    sys.modules["paddle3d.ops"].pointnet2_ops = types.SimpleNamespace(
        farthest_point_sample=lambda xyz, m: wrap(mkp._fps_torch(xyz, int(m))),
        gather_operation=lambda f, idx: wrap(_group_keep_dtype(f, idx)),
        ball_query_batch=lambda *a: wrap(mkp._ball_torch(*a)),
        grouping_operation_batch=lambda f, idx: wrap(_group_keep_dtype(f, idx)))
    ps._pkg("paddle3d.models.detection.iassd", PKG)
    mods = ps.load("paddle3d.models.detection.iassd.iassd_modules")
    backbone = ps.load("paddle3d.models.detection.iassd.iassd_backbone")
    coder = ps.load("paddle3d.models.detection.iassd.iassd_coder")
    base = dict(paddle=p, nn=p.nn, F=F, np=np, manager=ps._Anything("manager"),
                PointResidual_BinOri_Coder=coder.PointResidual_BinOri_Coder,
                iou3d_nms=types.SimpleNamespace(nms_gpu=nms_gpu))
    hp = os.path.join(PKG, "iassd_head.py")
    Head = ps.exec_lines(hp, [(33, 78)], dict(base))["IASSD_Head"]
    Head.build_loss = lambda self: None
    fns = ps.exec_lines(hp, [(606, 621), (623, 663)], dict(base))
    Head.generate_predicted_boxes, Head.forward = fns["generate_predicted_boxes"], fns["forward"]
    post = ps.exec_lines(os.path.join(PKG, "iassd.py"), [(136, 178), (180, 212)], dict(base))
    return p, mods, backbone.IASSD_Backbone, Head, post["post_process"], post["class_agnostic_nms"]


def record_layers(layers, calls):
    """Wrap each layer's forward: (index, positional and keyword arguments, outputs) of every call goes to `calls`."""
    for i, layer in enumerate(layers):
        def rec(*a, _f=layer.forward, _i=i, **kw):
            r = _f(*a, **kw)
            keep = lambda v: _t(v).clone() if isinstance(v, torch.Tensor) else v  # noqa: E731
            calls.append((_i, [keep(v) for v in a], {k: keep(v) for k, v in kw.items()}, [keep(v) for v in r]))
            return r
        layer.forward = rec


def to64(v):
    return ps._wrap(v.double()) if isinstance(v, torch.Tensor) and v.dtype == torch.float32 else (
        ps._wrap(v) if isinstance(v, torch.Tensor) else v)


def layer64(layer, a, kw):
    """The layer's forward in fp64 from the fp32 inputs and weights (sampling and ball query stay the fp32 ops)."""
    l64 = copy.deepcopy(layer).double()
    return [(_t(v) if isinstance(v, torch.Tensor) else v)
            for v in type(l64).forward(l64, *[to64(v) for v in a], **{k: to64(v) for k, v in kw.items()})]


def check_spheres(xyz, new_xyz, radii):
    """No point within a relative 1e-4 of a query sphere, in fp64."""
    q, p = _t(new_xyz).double().numpy(), _t(xyz).double().numpy()
    d2 = ((q[:, :, None, :] - p[:, None, :, :]) ** 2).sum(-1)
    for r in radii:
        r2 = float(np.float32(r)) ** 2
        near = np.abs(d2 - r2) <= 1e-4 * r2
        assert not near.any(), f"{int(near.sum())} pairs within 1e-4 of radius {r}"
    return [int((d2 < float(np.float32(r)) ** 2).sum(-1).min()) for r in radii], \
        [int((d2 < float(np.float32(r)) ** 2).sum(-1).max()) for r in radii]


def check_cut(cls_features, npoint):
    s = torch.sigmoid(_t(cls_features).max(-1).values).numpy()
    for b in range(s.shape[0]):
        o = np.sort(s[b])[::-1]
        assert len(np.unique(o[:npoint + 1])) == npoint + 1, "tied scores at or above a ctr_aware cut"


def post_lists(preds, prefix, out):
    for b, d in enumerate(preds):
        out[f"{prefix}_boxes{b}"] = _t(d["pred_boxes"]).numpy().reshape(-1, 7).astype(np.float32)
        out[f"{prefix}_scores{b}"] = _t(d["pred_scores"]).numpy().reshape(-1).astype(np.float32)
        out[f"{prefix}_labels{b}"] = _t(d["pred_labels"]).numpy().reshape(-1).astype(np.float32)


def main():
    from oracle import pyoracle as O

    O.build(ref=True)
    p, mods, Backbone, Head, post_process, nms = build_reference(O)
    rng = np.random.default_rng(SEED)
    data = points(rng)
    out = {"data": data}
    backbone, head = Backbone(**backbone_cfg()).eval(), Head(**head_cfg()).eval()
    out["backbone_state_shapes"] = json.dumps(ps.fill_state(backbone, SEED + 1))
    out["head_state_shapes"] = json.dumps(ps.fill_state(head, SEED + 2))
    originals = [copy.deepcopy(m) for m in backbone.SA_modules]
    backbone64 = copy.deepcopy(backbone).double()
    calls = []
    record_layers(backbone.SA_modules, calls)
    with torch.no_grad():
        bd = head(backbone({"data": ps.tensor(data), "batch_size": B}))
    assert [c[0] for c in calls] == list(range(NUM_LAYERS))
    for i, a, kw, r in calls:
        args = dict(zip(("xyz", "features", "cls_features"), a), **kw)
        for k, v in args.items():
            if isinstance(v, torch.Tensor):
                out[f"l{i}_in_{k}"] = v.numpy()
        outs = ("new_xyz", "new_features", "cls_features") if BACKBONE["layer_types"][i] == "SA_Layer" else \
            ("vote_xyz", "new_features", "xyz", "ctr_offsets")
        with torch.no_grad():
            r64 = layer64(originals[i], a, kw)
        for k, v, v64 in zip(outs, r, r64):
            if not isinstance(v, torch.Tensor) or v.numel() == 0 or k == "xyz":
                continue
            out[f"l{i}_out_{k}"] = v.numpy()
            if k == "new_xyz":  # sampled, not computed: the fp64 run must pick the same points
                assert np.array_equal(v.numpy(), v64.numpy().astype(np.float32)), f"layer {i}: fp64 samples other points"
                continue
            out[f"l{i}_out_{k}_bound"], out[f"l{i}_out_{k}_ref_err"] = mkr.bound(v.numpy(), v64.numpy())
        if BACKBONE["layer_types"][i] == "SA_Layer":
            if "ctr" in (BACKBONE["sample_method_list"][i] or ""):
                check_cut(args["cls_features"], BACKBONE["npoint_list"][i])
            if BACKBONE["radius_list"][i]:
                lo, hi = check_spheres(args["xyz"], r[0], BACKBONE["radius_list"][i])
                print(f"layer {i}: hits per query {lo} .. {hi}")

    # the whole model in fp64 from the fp32 points and weights: the bound of an end-to-end comparison
    with torch.no_grad():
        e64 = copy.deepcopy(head).double()(backbone64({"data": ps._wrap(ps.tensor(data).double()), "batch_size": B}))
    for a, b in zip(bd["encoder_xyz"][:5], e64["encoder_xyz"][:5]):  # the sampled points of layers 0-3
        assert np.array_equal(_t(a).numpy(), _t(b).numpy().astype(np.float32)), "the fp64 model samples other points"
    assert np.array_equal(_t(bd["batch_cls_preds"]).numpy().argmax(-1), _t(e64["batch_cls_preds"]).numpy().argmax(-1))
    for k in ("batch_cls_preds", "batch_box_preds"):
        out[f"e2e_{k}_bound"], out[f"e2e_{k}_ref_err"] = mkr.bound(_t(bd[k]).numpy(), _t(e64[k]).numpy())

    # the head: logits, encodings, decoded boxes; fp64 from the same fp32 features
    for k in ("centers_features", "centers", "ctr_offsets", "centers_origin", "batch_cls_preds", "batch_box_preds",
              "batch_index"):
        out[f"head_{k}"] = _t(bd[k]).numpy()
    out["head_center_box_preds"] = _t(head.forward_ret_dict["center_box_preds"]).numpy()
    with torch.no_grad():
        h64 = copy.deepcopy(head).double()
        bd64 = h64({k: (to64(_t(v)) if isinstance(v, torch.Tensor) else v) for k, v in bd.items()})
    enc64 = _t(h64.forward_ret_dict["center_box_preds"]).numpy()
    assert np.array_equal(out["head_center_box_preds"][:, 6:18].argmax(-1), enc64[:, 6:18].argmax(-1))
    assert np.array_equal(out["head_batch_cls_preds"].argmax(-1), _t(bd64["batch_cls_preds"]).numpy().argmax(-1))
    for k, v64 in (("batch_cls_preds", bd64["batch_cls_preds"]), ("batch_box_preds", bd64["batch_box_preds"]),
                   ("center_box_preds", h64.forward_ret_dict["center_box_preds"])):
        out[f"head_{k}_bound"], out[f"head_{k}_ref_err"] = mkr.bound(out[f"head_{k}"], _t(v64).numpy())

    # post_process: the model's output, and a case whose frame 1 keeps nothing
    me = types.SimpleNamespace(post_process_cfg=POST_CFG)
    me.class_agnostic_nms = types.MethodType(nms, me)
    low = _t(bd["batch_cls_preds"]).clone()
    low[_t(bd["batch_index"]) == 1] -= 12.0
    out["empty_batch_cls_preds"] = low.numpy()
    for tag, cls in (("post", bd["batch_cls_preds"]), ("empty", ps._wrap(low))):
        with torch.no_grad():
            preds = post_process(me, dict(bd, batch_cls_preds=cls))
        post_lists(preds, tag, out)
        sc = torch.sigmoid(_t(cls)).max(-1).values.numpy().reshape(B, -1)
        assert np.abs(sc - np.float32(POST_CFG["score_thresh"])).min() >= 1e-3
        boxes = out["head_batch_box_preds"].reshape(B, -1, 7)
        for b in range(B):
            ok = sc[b] >= np.float32(POST_CFG["score_thresh"])
            assert len(np.unique(sc[b][ok])) == int(ok.sum()), "tied scores"
            if ok.sum() > 1:
                assert O.iou_margin(np.ascontiguousarray(boxes[b][ok]), POST_CFG["nms_config"]["nms_thresh"]) >= 1e-3
    assert max(len(out[f"post_scores{b}"]) for b in range(B)) > 1
    assert out["empty_labels1"].tolist() == [-1.0] and out["empty_scores1"].tolist() == [0.0]
    assert not out["empty_boxes1"].any() and out["empty_labels0"].min() >= 0
    print("kept", [len(out[f"post_scores{b}"]) for b in range(B)], [len(out[f"empty_scores{b}"]) for b in range(B)])
    print({k: float(v) for k, v in out.items() if k.endswith("_bound")})
    np.savez_compressed(OUT, **{k: np.asarray(v) for k, v in out.items()})
    print(os.path.getsize(OUT), "bytes")


def load(path=OUT):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def state(g, name):
    """The recorded module's Paddle-named state dict ("backbone" or "head"), regenerated from the stored keys and
    shapes (fill_state's rule)."""
    shapes = json.loads(str(g[f"{name}_state_shapes"]))
    rng = np.random.default_rng(SEED + 1 + ("backbone", "head").index(name))
    return {key: ps.synth_param(key, tuple(shapes[key]), rng) for key in sorted(shapes)}


if __name__ == "__main__":
    main()
