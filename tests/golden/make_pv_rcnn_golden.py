"""Golden vectors for PV-RCNN's keypoint branch and RoI head from the reference's own Python, executed through
tests/golden/paddle_shim.py at small seeded shapes:

    bilinear_interpolate_paddle                 models/point_encoders/voxel_set_abstraction.py:32-67
    VoxelSetAbstraction.__init__ / get_sampled_points / interpolate_from_bev_features / forward
                                                voxel_set_abstraction.py:112-424
    PointHeadSimple.__init__ / forward          models/heads/dense_heads/point_head.py:31-153
    PVRCNNHead.__init__ / roi_grid_pool / forward (eval)
                                                models/heads/roi_heads/pvrcnn_head.py:34-197
    (with build_local_aggregation_module / StackSAModuleMSG, pointnet2_stack/pointnet2_modules.py:31-157, and the
    RoIHeadBase methods make_roi_head_golden.py runs)

    python tests/golden/make_pv_rcnn_golden.py     # needs the reference checkout; writes python_pv_rcnn.npz

Two cases, each two frames of unequal raw point and voxel counts, a BEV map and two sparse scales:
  a  40 keypoints, raw points at 16/16 (nsample 16) and 32/32 (nsample 32), x_conv1 16/16, x_conv2 32/32; RoI grid 6
     with 16/16 (nsample 16) and 32/32 (nsample 32)
  b  40 keypoints with 25 raw points in frame 1 (fewer than num_keypoints), raw points and x_conv2 at 64/64
     (nsample 16); RoI grid 3 with 64/64 (nsample 16)
The raw points hold clusters (balls with more hits than nsample), repeats (frame 0), points outside the voxels' and the
BEV map's extent (empty balls; both clip branches of the interpolation, asserted below) and, as rows 0 and 1 of frame
0, a pair at exactly the first radius (row 0 is always a keypoint, here on the map's far border: d2 == r2 is no hit).  The proposals hold boxes
partly and wholly outside the keypoints' extent.

The pointnet2 ops are bound to the torch formulations of make_pointnet2_golden.py (farthest point sampling) and
make_pointnet2_stack_golden.py (ball query; the grouping keeps the features' dtype), the sparse tensor and the NMS are
make_roi_head_golden.py's, and what the shim lacks is supplied here.  One departure is forced: get_sampled_points
tiles a frame's samples with `non_empty.tile([1, times])[:num_keypoints]`, which for a 1-D row yields a
[1, n * times] row that cannot be assigned; the flat repeat that OpenPCDet's `.repeat(times)` is stands in for it.
The weights come from paddle_shim.fill_state; only their keys and shapes are stored.

Every StackSAModuleMSG.forward call is recorded (inputs, fp32 output), repeated in fp64 from the same fp32 inputs and
weights, and the bound the tests read is stored: 4 x the largest error of the reference's own fp32 result against that
evaluation, one fp32 ulp of the largest output magnitude as a floor.  The same for point_features_before_fusion,
point_features, point_cls_scores, rcnn_cls and rcnn_reg (the fp64 FC stacks over the fp64 pooled layers).

Asserted here: no ball has a point within 1e-5 relative of its radius other than the planted exact ones, so the index
sets do not depend on rounding; every case has empty balls and balls with more hits than nsample.
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
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import make_pointnet2_golden as mkp  # noqa: E402
import make_pointnet2_stack_golden as mkps  # noqa: E402
import make_roi_head_golden as mkr  # noqa: E402
import paddle_shim as ps  # noqa: E402

REF = "/root/reference"
MODELS = os.path.join(REF, "paddle3d/models")
OUT = os.path.join(HERE, "python_pv_rcnn.npz")

PCR = [0.0, -3.0, -1.0, 6.0, 3.0, 1.0]
VOXEL = [0.25, 0.25, 0.25]
GRIDS = {"x_conv1": (8, 24, 24), "x_conv2": (4, 12, 12)}  # (Z, Y, X) at strides 1, 2
VOXELS = {"x_conv1": (260, 150), "x_conv2": (120, 75)}  # per frame
CHANNELS = {"x_conv1": 6, "x_conv2": 10}
RAW_POINTS = {"a": (300, 200), "b": (180, 25)}
BEV = {"a": (12, 6, 6, 4), "b": (8, 12, 12, 2)}  # C, H, W, stride
NUM_KEYPOINTS = 40
NUM_RAWPOINT_FEATURES = 4
NUM_CLASS = 3  # the dense head's: post_processing takes roi_labels
POST_CFG = mkr.POST_CFG
TAGS = ("a", "b")


def encoder_cfg(tag):
    if tag == "a":
        sources = ["bev", "x_conv1", "x_conv2", "raw_points"]
        sa = {"raw_points": {"mlps": [[16, 16], [32, 32]], "pool_radius": [0.5, 1.0], "nsample": [16, 32]},
              "x_conv1": {"downsample_stride": 1, "mlps": [[16, 16]], "pool_radius": [0.6], "nsample": [16]},
              "x_conv2": {"downsample_stride": 2, "mlps": [[32, 32]], "pool_radius": [1.0], "nsample": [32]}}
    else:
        sources = ["bev", "x_conv2", "raw_points"]
        sa = {"raw_points": {"mlps": [[64, 64]], "pool_radius": [0.8], "nsample": [16]},
              "x_conv2": {"downsample_stride": 2, "mlps": [[64, 64]], "pool_radius": [1.5], "nsample": [16]}}
    for name in sa:
        if name != "raw_points":
            sa[name]["in_channels"] = CHANNELS[name]
    return {"point_source": "raw_points", "num_keypoints": NUM_KEYPOINTS, "out_channels": 24, "sample_method": "FPS",
            "features_source": sources, "sa_layer": sa}


POINT_HEAD_CFG = {"cls_fc": [24, 16], "class_agnostic": True, "use_point_features_before_fusion": True,
                  "loss_config": {}}


def roi_head_cfg(tag):
    a = tag == "a"
    pool = ({"grid_size": 6, "mlps": [[16, 16], [32, 32]], "pool_radius": [0.8, 1.6], "nsample": [16, 32]} if a else
            {"grid_size": 3, "mlps": [[64, 64]], "pool_radius": [1.6], "nsample": [16]})
    pool["pool_method"] = "max_pool"
    return {"class_agnostic": True, "shared_fc": [24, 24], "cls_fc": [16, 24], "reg_fc": [16, 16], "dp_ratio": 0.3,
            "nms_config": {"test": {"nms_type": "nms_gpu", "multi_class_nms": False, "nms_pre_maxsize": 40,
                                    "nms_post_maxsize": 3 if a else 12, "nms_thresh": 0.7}},
            "roi_grid_pool": pool, "target_config": {"box_coder": "ResidualCoder"}, "loss_config": {}}


def _t(x):
    return x.as_subclass(torch.Tensor) if isinstance(x, torch.Tensor) else torch.as_tensor(x)


def raw_points(rng, tag):
    """points [N, 5] as (b, x, y, z, intensity), the frames' rows contiguous, and the per-frame counts."""
    frames = []
    for b, n in enumerate(RAW_POINTS[tag]):
        if n < NUM_KEYPOINTS:  # all distinct: the first n samples are a permutation of the frame
            pts = np.stack([rng.uniform(0.5, 5.5, n), rng.uniform(-2.5, 2.5, n), rng.uniform(-0.8, 0.8, n)], 1)
        else:
            k = n // 2
            seeds = np.stack([rng.uniform(1.0, 5.0, 4), rng.uniform(-2.0, 2.0, 4), rng.uniform(-0.5, 0.5, 4)], 1)
            clustered = seeds[rng.integers(0, 4, k)] + rng.normal(0, 0.25, (k, 3))
            wide = np.stack([rng.uniform(-0.6, 6.6, n - k), rng.uniform(-3.6, 3.6, n - k), rng.uniform(-0.9, 0.9, n - k)],
                            1)  # some outside the range: off the BEV map and away from every voxel
            pts = np.concatenate([clustered, wide])
            if b == 0:
                pts[-n // 6:] = pts[rng.integers(0, n - n // 6, n // 6)]  # repeats
                # row 0 (always a keypoint) on the BEV map's far border; row 1 exactly 0.5 from it: d2 == r2 at the
                # first radius
                pts[0], pts[1] = (6.0, 0.25, 0.0), (5.5, 0.25, 0.0)
        frames.append(np.concatenate([np.full((n, 1), b), pts, rng.uniform(0, 1, (n, 1))], 1).astype(np.float32))
    return np.concatenate(frames), [len(f) for f in frames]


def scales(rng):
    out = {}
    for name, (Z, Y, X) in GRIDS.items():
        ind = []
        for b, n in enumerate(VOXELS[name]):
            cells = np.sort(rng.choice(Z * Y * X, n, replace=False))
            z, y, x = np.unravel_index(cells, (Z, Y, X))
            ind.append(np.stack([np.full(n, b), z, y, x], 1))
        ind = np.concatenate(ind).astype(np.int32)
        out[name] = (ind, rng.standard_normal((len(ind), CHANNELS[name])).astype(np.float32))
    return out


def build_reference(O):
    """The reference's classes, executed from its files."""
    p = ps.install(REF)
    T = ps.tensor
    wrap = ps._wrap

    def nms_gpu(boxes, thresh):
        keep = O.nms(_t(boxes).float().numpy(), float(thresh), kind="ref" if O.have_ref() else "port")
        full = np.zeros(boxes.shape[0], np.int32)
        full[:len(keep)] = keep
        return T(full), int(len(keep))

    pointnet2_ops = types.SimpleNamespace(
        ball_query_stack=lambda *a: wrap(mkps._ball_stack_torch(*a)),
        grouping_operation_stack=lambda *a: wrap(mkr._group_torch(*a)),
        farthest_point_sample=lambda xyz, m: wrap(mkp._fps_torch(xyz, int(m))))

    class Conv1D(p.nn.Layer):
        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias_attr=None, **_):
            super().__init__()
            self.weight = torch.nn.Parameter(torch.zeros((out_channels, in_channels, kernel_size)))
            self.bias = None if bias_attr is False else torch.nn.Parameter(torch.zeros(out_channels))

        def forward(self, x):
            return torch.nn.functional.conv1d(_t(x), self.weight, self.bias)

    class Dropout(p.nn.Layer):
        def __init__(self, p=0.5, **_):
            super().__init__()

        def forward(self, x):
            assert not self.training
            return x

    class Loss(p.nn.Layer):  # PointHeadSimple.build_losses: never run at inference
        def __init__(self, *a, **k):
            super().__init__()

    class Sequential(p.nn.Sequential):
        def sublayers(self, include_self=False):
            mods = list(self.modules())
            return mods if include_self else mods[1:]

    nnx = types.ModuleType("nn")
    nnx.__dict__.update({k: v for k, v in vars(p.nn).items() if not k.startswith("__")})
    nnx.Conv1D, nnx.Dropout, nnx.Sequential = Conv1D, Dropout, Sequential
    torch.nn.Parameter.set_value = lambda self, value: None  # init_weights' draws: the weights are seeded below
    Fx = types.SimpleNamespace(
        max_pool2d=lambda x, kernel_size: wrap(torch.nn.functional.max_pool2d(_t(x), tuple(kernel_size))),
        avg_pool2d=lambda x, kernel_size: wrap(torch.nn.functional.avg_pool2d(_t(x), tuple(kernel_size))),
        sigmoid=lambda x: wrap(torch.sigmoid(_t(x))))

    # the 1-D tile of get_sampled_points (see the module docstring)
    tile0 = ps.Tensor.tile

    def tile(self, reps=None, repeat_times=None):
        r = list(reps if reps is not None else repeat_times)
        if self.dim() == 1 and len(r) == 2 and r[0] == 1:
            return wrap(_t(self).repeat(int(r[1])))
        return tile0(self, r)

    ps.Tensor.tile = tile
    p.cos, p.sin = (lambda x: wrap(torch.cos(_t(x)))), (lambda x: wrap(torch.sin(_t(x))))
    p.nonzero = lambda x: wrap(torch.nonzero(_t(x)))
    p.normal = lambda mean=0.0, std=1.0, shape=None: wrap(torch.zeros(tuple(shape)))  # weights are seeded below
    noop = lambda *a, **k: None  # noqa: E731
    inits = types.SimpleNamespace(reset_parameters=noop, constant_init=noop)
    base = dict(paddle=p, nn=nnx, F=Fx, np=np, pointnet2_ops=pointnet2_ops, List=list, constant_init=noop,
                kaiming_normal_init=noop, xavier_normal_init=noop, param_init=inits,
                iou3d_nms=types.SimpleNamespace(nms_gpu=nms_gpu), manager=ps._Anything("manager"),
                SigmoidFocalClassificationLoss=Loss)
    stack = os.path.join(MODELS, "common/pointnet2_stack")
    utils = ps.exec_lines(os.path.join(stack, "pointnet2_utils.py"), [(27, 89)], dict(base))
    mods = ps.exec_lines(os.path.join(stack, "pointnet2_modules.py"), [(31, 157)],
                         dict(base, pointnet2_utils=types.SimpleNamespace(QueryAndGroup=utils["QueryAndGroup"])))
    stack_modules = types.SimpleNamespace(build_local_aggregation_module=mods["build_local_aggregation_module"])
    box_utils = ps.exec_lines(os.path.join(MODELS, "common/box_utils.py"), [(17, 37), (76, 99)], dict(paddle=p))
    nms = ps.exec_lines(os.path.join(MODELS, "common/model_nms_utils.py"), [(20, 66)], dict(base))
    coder = ps.exec_lines(os.path.join(REF, "paddle3d/utils/box_coder.py"), [(22, 100)], dict(paddle=p))
    base.update(class_agnostic_nms=nms["class_agnostic_nms"], rotate_points_along_z=box_utils["rotate_points_along_z"],
                get_voxel_centers=box_utils["get_voxel_centers"], pointnet2_stack_modules=stack_modules)
    vsa = ps.exec_lines(os.path.join(MODELS, "point_encoders/voxel_set_abstraction.py"), [(32, 67), (112, 424)],
                        dict(base))
    point_head = ps.exec_lines(os.path.join(MODELS, "heads/dense_heads/point_head.py"), [(31, 268)], dict(base))
    rb = os.path.join(MODELS, "heads/roi_heads/roi_head_base.py")
    methods = ps.exec_lines(rb, [(51, 68), (69, 131), (293, 322), (324, 346)], dict(base))

    def base_init(self, num_class, model_cfg, **kwargs):  # the inference part of RoIHeadBase.__init__ (:33-43)
        nnx.Layer.__init__(self)
        self.model_cfg, self.num_class = model_cfg, num_class
        self.box_coder = coder["ResidualCoder"]()

    RoIHeadBase = type("RoIHeadBase", (nnx.Layer,), dict(
        __init__=base_init, make_fc_layers=methods["make_fc_layers"], proposal_layer=methods["proposal_layer"],
        generate_predicted_boxes=methods["generate_predicted_boxes"],
        get_global_grid_points_of_roi=methods["get_global_grid_points_of_roi"],
        get_dense_grid_points=methods["get_dense_grid_points"]))
    head = ps.exec_lines(os.path.join(MODELS, "heads/roi_heads/pvrcnn_head.py"), [(34, 197)],
                         dict(base, RoIHeadBase=RoIHeadBase, math=__import__("math")))["PVRCNNHead"]
    post = ps.exec_lines(os.path.join(MODELS, "detection/pv_rcnn/pv_rcnn.py"), [(151, 225)], dict(base))["post_processing"]
    return p, vsa, point_head["PointHeadSimple"], head, post


def record_layers(layers, calls):
    """Wrap each StackSAModuleMSG's forward: (name, kwargs, output) of every call goes to `calls`."""
    for name, layer in layers:
        def rec(*a, _f=layer.forward, _n=name, **kw):
            assert not a
            r = _f(**kw)
            calls.append((_n, {k: (_t(v).clone() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()},
                          _t(r[1]).clone()))
            return r
        layer.forward = rec


def layer64(layer, kw):
    """The layer's forward in fp64 from the fp32 inputs and weights (the ball query stays the fp32 one)."""
    l64 = copy.deepcopy(layer).double()
    kw64 = {n: (ps._wrap(v.double()) if isinstance(v, torch.Tensor) and v.dtype == torch.float32
                else (ps._wrap(v) if isinstance(v, torch.Tensor) else v)) for n, v in kw.items()}
    r = _t(type(l64).forward(l64, **kw64)[1])
    assert r.dtype == torch.float64
    return r


def check_margins(kw, radii, nsamples, what):
    """(rows without a hit, rows with more hits than nsample, pairs at exactly the radius) over the scales of a call;
    asserts that no other pair lies within 1e-5 relative of r2."""
    q, p = kw["new_xyz"].double().numpy(), kw["xyz"].double().numpy()
    qf = np.asarray(mkps._frame_rows(len(q), kw["new_xyz_batch_cnt"]))
    pc = [int(c) for c in kw["xyz_batch_cnt"]]
    pf = np.repeat(np.arange(len(pc)), pc)
    same = qf[:, None] == pf[None, :]
    d2 = ((q[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    q32, p32 = q.astype(np.float32), p.astype(np.float32)
    d = q32[:, None, :] - p32[None, :, :]
    d2_32 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    empty = over = exact = 0
    for r, s in zip(radii, nsamples):
        r2 = float(np.float32(r) * np.float32(r))
        on = same & (d2_32 == np.float32(r2)) & (d2 == r2)
        near = same & (np.abs(d2 - r2) <= 1e-5 * r2) & ~on
        assert not near.any(), f"{what}: {int(near.sum())} pairs within 1e-5 of radius {r}"
        hits = (same & (d2 < r2)).sum(1)
        empty, over, exact = empty + int((hits == 0).sum()), over + int((hits > s).sum()), exact + int(on.sum())
    return empty, over, exact


def bound(ref32, ref64):
    return mkr.bound(np.asarray(ref32), np.asarray(ref64))


def main():
    from oracle import pyoracle as O

    O.build(ref=True)
    p, vsa, PointHead, Head, post_processing = build_reference(O)
    VSA, bilinear = vsa["VoxelSetAbstraction"], vsa["bilinear_interpolate_paddle"]
    T = ps.tensor
    out = {}
    for tag in TAGS:
        rng = np.random.default_rng({"a": 45, "b": 46}[tag])
        ecfg, hcfg = encoder_cfg(tag), roi_head_cfg(tag)
        C, H, W, bev_stride = BEV[tag]
        enc = VSA(model_cfg=copy.deepcopy(ecfg), voxel_size=VOXEL, point_cloud_range=PCR, num_bev_features=C,
                  num_rawpoint_features=NUM_RAWPOINT_FEATURES)
        ph = PointHead(num_class=NUM_CLASS, input_channels=enc.num_point_features_before_fusion,
                       model_cfg=copy.deepcopy(POINT_HEAD_CFG))
        head = Head(input_channels=enc.num_point_features, model_cfg=copy.deepcopy(hcfg), num_class=1)
        for k, (name, m) in enumerate((("point_encoder", enc), ("point_head", ph), ("roi_head", head))):
            m.eval()
            out[f"{tag}_{name}_state_shapes"] = np.asarray(json.dumps(ps.fill_state(m, 70 + 3 * ord(tag) + k)))

        points, counts = raw_points(rng, tag)
        sc = scales(rng)
        bev = rng.standard_normal((2, C, H, W)).astype(np.float32)
        box, cls = mkr.proposals(rng, NUM_CLASS)
        out[f"{tag}_points"], out[f"{tag}_points_cnt"] = points, np.asarray(counts, np.int32)
        out[f"{tag}_bev"], out[f"{tag}_box_preds"], out[f"{tag}_cls_preds"] = bev, box, cls
        for name, (ind, feats) in sc.items():
            out[f"{tag}_{name}_indices"], out[f"{tag}_{name}_features"] = ind, feats
        nmsc = hcfg["nms_config"]["test"]
        for b in range(2):
            order = np.argsort(-cls[b].max(1), kind="stable")[:nmsc["nms_pre_maxsize"]]
            mkr.check_exact(O, box[b][order], cls[b].max(1), nmsc["nms_thresh"], f"{tag} proposals frame {b}")

        calls = []
        names = [("sa_rawpoints", enc.sa_rawpoints)] + [(f"sa_{n}", l) for n, l in zip(enc.sa_layer_names, enc.sa_layers)]
        names.append(("roi_pool", head.roi_grid_pool_layer))
        record_layers(names, calls)
        bd = {"batch_size": 2, "points": T(points), "spatial_features": T(bev), "spatial_features_stride": bev_stride,
              "multi_scale_3d_features": {n: mkr.Sparse(*sc[n], GRIDS[n]) for n in sc},
              "batch_box_preds": T(box), "batch_cls_preds": T(cls)}
        with torch.no_grad():
            keypoints = _t(enc.get_sampled_points(bd)).clone()
            point_bev = _t(enc.interpolate_from_bev_features(ps._wrap(keypoints.clone()), bd["spatial_features"], 2,
                                                             bev_stride=bev_stride)).clone()
            # bilinear_interpolate_paddle alone, frame 0's map at its keypoints' positions
            k0 = keypoints[:NUM_KEYPOINTS]
            xs = ((k0[:, 1] - PCR[0]) / VOXEL[0]) / bev_stride
            ys = ((k0[:, 2] - PCR[1]) / VOXEL[1]) / bev_stride
            out[f"{tag}_bilinear_x"], out[f"{tag}_bilinear_y"] = xs.numpy(), ys.numpy()
            out[f"{tag}_bilinear_out"] = _t(bilinear(T(bev[0]).transpose((1, 2, 0)), ps._wrap(xs.clone()),
                                                     ps._wrap(ys.clone()))).numpy()
            bd = enc(bd)
            assert torch.equal(_t(bd["point_coords"]), keypoints)
            bd = ph(bd)
            bd = head(bd)
            shared = head.shared_fc_layer(ps._wrap(_t(calls[-1][2]).reshape(-1, hcfg["roi_grid_pool"]["grid_size"] ** 3,
                                                                             calls[-1][2].shape[-1])
                                                   .permute(0, 2, 1).reshape(-1, head.pre_channel, 1)))
            rcnn_cls = _t(head.cls_layers(shared)).permute(0, 2, 1).squeeze(1)
            rcnn_reg = _t(head.reg_layers(shared)).permute(0, 2, 1).squeeze(1)
        out[f"{tag}_keypoints"], out[f"{tag}_point_bev"] = keypoints.numpy(), point_bev.numpy()
        for k in ("point_features_before_fusion", "point_features", "point_cls_scores", "rois", "roi_scores",
                  "batch_cls_preds", "batch_box_preds"):
            out[f"{tag}_{k}"] = _t(bd[k]).numpy()
        out[f"{tag}_roi_labels"] = _t(bd["roi_labels"]).numpy().astype(np.int64)
        out[f"{tag}_rcnn_cls"], out[f"{tag}_rcnn_reg"] = rcnn_cls.numpy(), rcnn_reg.numpy()
        assert bd["cls_preds_normalized"] is False
        assert np.array_equal(out[f"{tag}_batch_cls_preds"].reshape(-1, 1), out[f"{tag}_rcnn_cls"])
        # both clip branches of the interpolation: a floor below 0, a floor + 1 above W - 1 / H - 1
        kx = (keypoints[:, 1].numpy() - PCR[0]) / VOXEL[0] / bev_stride
        ky = (keypoints[:, 2].numpy() - PCR[1]) / VOXEL[1] / bev_stride
        assert (np.floor(kx) < 0).any() and (np.floor(kx) + 1 > W - 1).any(), "x clip branches"
        assert (np.floor(ky) < 0).any() and (np.floor(ky) + 1 > H - 1).any(), "y clip branches"
        if tag == "a":
            assert np.array_equal(keypoints[0].numpy(), points[0, :4])
        else:
            assert counts[1] < NUM_KEYPOINTS  # the tiled frame
            assert np.array_equal(keypoints[NUM_KEYPOINTS:NUM_KEYPOINTS + 15, 1:].numpy(),
                                  keypoints[NUM_KEYPOINTS + 25:, 1:].numpy())

        # every recorded layer call: inputs, fp32 output, the fp64 evaluation's bound, the margins of its balls
        assert [c[0] for c in calls] == [n for n, _ in names], [c[0] for c in calls]
        stats = np.zeros(3, np.int64)
        pooled64 = {}
        with torch.no_grad():
            for (name, kw, r), (_, layer) in zip(calls, names):
                for k in ("xyz", "xyz_batch_cnt", "new_xyz", "new_xyz_batch_cnt", "features"):
                    if kw[k] is not None:
                        out[f"{tag}_{name}_{k}"] = kw[k].numpy()
                out[f"{tag}_{name}_out"] = r.numpy()
                r64 = layer64(layer, kw)
                pooled64[name] = r64
                out[f"{tag}_{name}_bound"], out[f"{tag}_{name}_ref_err"] = bound(r.numpy(), r64.numpy())
                radii, ns = [g.radius for g in layer.groupers], [g.nsample for g in layer.groupers]
                out[f"{tag}_{name}_radii"], out[f"{tag}_{name}_nsamples"] = np.asarray(radii, np.float64), np.asarray(ns)
                stats += np.asarray(check_margins(kw, radii, ns, f"{tag} {name}"))
            assert stats[0] > 0 and stats[1] > 0, stats
            assert tag != "a" or stats[2] > 0, stats
            # downstream of the pooled layers in fp64
            feats64 = [point_bev.double()] if "bev" in ecfg["features_source"] else []
            feats64.append(pooled64["sa_rawpoints"])
            feats64 += [pooled64[f"sa_{n}"] for n in enc.sa_layer_names]
            before64 = torch.cat(feats64, -1)
            d64 = lambda m: copy.deepcopy(m).double()  # noqa: E731
            fused64 = _t(d64(enc.vsa_point_feature_fusion)(ps._wrap(before64)))
            scores64 = torch.sigmoid(_t(d64(ph.cls_layers)(ps._wrap(before64)))).max(-1).values
            G3 = hcfg["roi_grid_pool"]["grid_size"] ** 3
            flat64 = pooled64["roi_pool"].reshape(-1, G3, pooled64["roi_pool"].shape[-1]).permute(0, 2, 1)
            shared64 = d64(head.shared_fc_layer)(ps._wrap(flat64.reshape(-1, head.pre_channel, 1)))
            cls64 = _t(d64(head.cls_layers)(shared64)).permute(0, 2, 1).squeeze(1)
            reg64 = _t(d64(head.reg_layers)(shared64)).permute(0, 2, 1).squeeze(1)
        for k, v64 in (("point_features_before_fusion", before64), ("point_features", fused64),
                       ("point_cls_scores", scores64), ("rcnn_cls", cls64), ("rcnn_reg", reg64)):
            out[f"{tag}_{k}_bound"], out[f"{tag}_{k}_ref_err"] = bound(out[f"{tag}_{k}"], v64.numpy())

        me = types.SimpleNamespace(num_class=NUM_CLASS, post_process_cfg=POST_CFG,
                                   dense_head=types.SimpleNamespace(num_class=NUM_CLASS))
        with torch.no_grad():
            dicts = post_processing(me, bd)
        mkr.post_dicts(dicts, f"{tag}_post", out)
        hs = torch.sigmoid(torch.from_numpy(out[f"{tag}_batch_cls_preds"])).numpy().max(-1)
        assert np.abs(hs - np.float32(POST_CFG["score_thresh"])).min() > 1e-4
        for b in range(2):
            ok = np.nonzero(hs[b] >= np.float32(POST_CFG["score_thresh"]))[0]
            if len(ok):
                o2 = ok[np.argsort(-hs[b][ok], kind="stable")]
                mkr.check_exact(O, out[f"{tag}_batch_box_preds"][b][o2], hs[b][ok], POST_CFG["nms_config"]["nms_thresh"],
                                f"{tag} head post frame {b}", rows=out[f"{tag}_rois"][b][ok])
        print(tag, "empty / over / exact", stats.tolist(), "post", [len(out[f"{tag}_post_scores{b}"]) for b in range(2)],
              "bounds", {k[len(tag) + 1:-6]: float(v) for k, v in out.items() if k.startswith(tag) and k.endswith("_bound")})

    np.savez_compressed(OUT, **{k: np.asarray(v) for k, v in out.items()})
    print(os.path.getsize(OUT), "bytes")


def load(path=OUT):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def state(g, tag, name):
    """The recorded module's Paddle-named state dict ("point_encoder", "point_head" or "roi_head"), regenerated from
    the stored keys and shapes (fill_state's rule)."""
    shapes = json.loads(str(g[f"{tag}_{name}_state_shapes"]))
    k = ("point_encoder", "point_head", "roi_head").index(name)
    rng = np.random.default_rng(70 + 3 * ord(tag) + k)
    return {key: ps.synth_param(key, tuple(shapes[key]), rng) for key in sorted(shapes)}


def layer_names(tag):
    """The recorded StackSAModuleMSG calls of a case, in call order."""
    cfg = encoder_cfg(tag)
    return ["sa_rawpoints"] + [f"sa_{n}" for n in cfg["features_source"] if n not in ("bev", "raw_points")] + ["roi_pool"]


if __name__ == "__main__":
    main()
