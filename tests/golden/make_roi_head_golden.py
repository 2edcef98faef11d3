"""Golden vectors for Voxel R-CNN's RoI head from the reference's own Python, executed through
tests/golden/paddle_shim.py at small seeded shapes:

    class_agnostic_nms                          models/common/model_nms_utils.py:20-66
    RoIHeadBase.proposal_layer                  models/heads/roi_heads/roi_head_base.py:69-131
    RoIHeadBase.generate_predicted_boxes        roi_head_base.py:293-322 (ResidualCoder.decode_paddle, utils/box_coder.py:22-100)
    RoIHeadBase.get_global_grid_points_of_roi   roi_head_base.py:324-346
    VoxelRCNNHead.__init__ / roi_grid_pool / forward (eval)
                                                models/heads/roi_heads/voxelrcnn_head.py:31-288
    VoxelRCNN.post_processing                   models/detection/voxel_rcnn/voxel_rcnn.py:145-220

    python tests/golden/make_roi_head_golden.py     # needs the reference checkout; writes python_roi_head.npz

Two cases, each two frames of unequal voxel counts over two sparse scales (strides 1 and 2):
  a  grid 6, one class (K = 1), C1 = 16, max pool, nsample 16 / 8
  b  grid 3, three classes (K = 3: the proposals' scores and post_processing's roi_labels; the head itself is class
     agnostic), C1 = 32 (max pool) and 16 (avg pool)
The proposals hold boxes partly outside the voxel grid and boxes with no voxel in range; frame 1 has fewer NMS
survivors than nms_post_maxsize (zero-padded RoIs).  post_processing runs on the head's own outputs and on a synthetic
batch in which frame 1 passes nothing under score_thresh (the box_empty row).

The pointnet2 ops are bound to the torch formulations of make_pointnet2_stack_golden.py, iou3d_nms.nms_gpu to the
reference's compiled IoU + sweep (oracle/_ref), and what the shim lacks (Conv1D, the pools, scatter_nd, nonzero,
normal, cos / sin, a sparse tensor with indices() / values()) is supplied here.  The weights come from
paddle_shim.fill_state; only their keys and shapes are stored (paddle_shim.synth_param reproduces them).

The file also records an fp64 evaluation of every NeighborVoxelSAModuleMSG output and of rcnn_cls / rcnn_reg from the
same fp32 inputs and weights, and the error bounds the tests read: 4 x the largest error of the reference's own fp32
result against that evaluation, with one fp32 ulp of the largest output magnitude as a floor.

Asserted here, so that exact index comparisons are a property of the data: no two scores of a frame tie (but for the
head's outputs on the bit-equal zero-padded RoIs of a frame, which every implementation keeps in index order), and no
IoU of an NMS input lies within 1e-4 of its threshold.
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
import make_pointnet2_stack_golden as mkps  # noqa: E402
import paddle_shim as ps  # noqa: E402

REF = "/root/reference"
MODELS = os.path.join(REF, "paddle3d/models")
OUT = os.path.join(HERE, "python_roi_head.npz")

PCR = [0.0, -3.0, -1.0, 6.0, 3.0, 1.0]
VOXEL = [0.25, 0.25, 0.25]  # strides 1, 2 -> grids (Z, Y, X) = (8, 24, 24), (4, 12, 12)
GRIDS = {"x_conv1": (8, 24, 24), "x_conv2": (4, 12, 12)}
STRIDES = {"x_conv1": 1, "x_conv2": 2}
VOXELS = {"x_conv1": (260, 150), "x_conv2": (120, 75)}  # per frame


def model_cfg(tag):
    a = tag == "a"
    return {
        "class_agnostic": True, "shared_fc": [24, 24], "cls_fc": [16, 24], "reg_fc": [16, 16], "dp_ratio": 0.3,
        "nms_config": {"test": {"nms_type": "nms_gpu", "multi_class_nms": False, "score_thresh": 0.0,
                                "nms_pre_maxsize": 40, "nms_post_maxsize": 10 if a else 12, "nms_thresh": 0.7}},
        "roi_grid_pool": {
            "features_source": ["x_conv1", "x_conv2"], "pre_mlp": True, "grid_size": 6 if a else 3,
            "pool_layers": {
                "x_conv1": {"mlps": [[16, 8]] if a else [[32, 8]], "query_ranges": [[2, 2, 2]], "pool_radius": [0.5],
                            "nsample": [16], "pool_method": "max_pool"},
                "x_conv2": {"mlps": [[16, 8]], "query_ranges": [[1, 2, 2]], "pool_radius": [1.0], "nsample": [8],
                            "pool_method": "max_pool" if a else "avg_pool"}}},
        "target_config": {"box_coder": "ResidualCoder"},
        "loss_config": {},
    }


INPUT_CHANNELS = {"x_conv1": 6, "x_conv2": 10}
NUM_CLASS = {"a": 1, "b": 3}
POST_CFG = {"score_thresh": 0.3, "output_raw_score": False,
            "nms_config": {"multi_classes_nms": False, "nms_type": "nms_gpu", "nms_thresh": 0.1,
                           "nms_pre_maxsize": 30, "nms_post_maxsize": 6}}


def _t(x):
    return x.as_subclass(torch.Tensor) if isinstance(x, torch.Tensor) else torch.as_tensor(x)


def proposals(rng, K, A=48):
    """box_preds [2, A, 7], cls_preds [2, A, K]: car-sized boxes around the grid, some reaching outside, two far
    away; frame 1 in tight clusters, so fewer survive the NMS than nms_post_maxsize."""
    box = np.zeros((2, A, 7), np.float32)
    for b in range(2):
        if b == 0:
            c = np.stack([rng.uniform(-0.5, 6.5, A), rng.uniform(-3.5, 3.5, A), rng.uniform(-0.8, 0.8, A)], 1)
        else:
            seeds = np.stack([rng.uniform(1.0, 5.0, 5), rng.uniform(-2.0, 2.0, 5), rng.uniform(-0.5, 0.5, 5)], 1)
            c = seeds[rng.integers(0, 5, A)] + rng.normal(0, 0.03, (A, 3))
        box[b, :, :3] = c
        box[b, :, 3:6] = np.array([1.6, 0.8, 0.7]) * rng.uniform(0.8, 1.2, (A, 3))
        box[b, :, 6] = rng.uniform(-np.pi, np.pi, A) if b == 0 else rng.normal(0.3, 0.02, A)
    box[0, 0, :3] = (30.0, 30.0, 5.0)  # no voxel in range at any scale
    box[0, 1, :3] = (-0.7, 0.0, 0.0)  # half outside the grid
    cls = rng.normal(0.0, 2.0, (2, A, K)).astype(np.float32)
    cls[0, :2] += 6.0  # the far boxes are kept
    return box, cls


def scales(rng):
    """Per source: indices [N, 4] (b, z, y, x) sorted by frame, features [N, C]."""
    out = {}
    for name, (Z, Y, X) in GRIDS.items():
        ind = []
        for b, n in enumerate(VOXELS[name]):
            cells = np.sort(rng.choice(Z * Y * X, n, replace=False))
            z, y, x = np.unravel_index(cells, (Z, Y, X))
            ind.append(np.stack([np.full(n, b), z, y, x], 1))
        ind = np.concatenate(ind).astype(np.int32)
        out[name] = (ind, rng.standard_normal((len(ind), INPUT_CHANNELS[name])).astype(np.float32))
    return out


class Sparse:
    """What roi_grid_pool asks of a sparse tensor: indices() [4, N], values() [N, C], shape [B, Z, Y, X, C]."""

    def __init__(self, ind, feats, grid, dtype=torch.float32):
        self._i, self._v = ps.tensor(ind.T.copy()), ps._wrap(torch.from_numpy(feats).to(dtype))
        self.shape = [2, *grid, feats.shape[1]]

    def indices(self):
        return self._i

    def values(self):
        return self._v


def _group_torch(features, features_cnt, idx, idx_cnt):
    """make_pointnet2_stack_golden._group_stack_torch keeping the features' dtype (the fp64 evaluation)."""
    ft, ix = _t(features), _t(idx).long()
    fc = [int(c) for c in _t(features_cnt)]
    starts = torch.tensor(np.concatenate([[0], np.cumsum(fc)])[:-1])
    g = starts[torch.tensor(mkps._frame_rows(ix.shape[0], _t(idx_cnt)))][:, None] + ix
    ok = (g >= 0) & (g < ft.shape[0])
    vals = ft[g.clamp(0, max(ft.shape[0] - 1, 0))]
    return torch.where(ok[..., None], vals, torch.zeros((), dtype=ft.dtype)).permute(0, 2, 1).contiguous()


def build_reference(O):
    """The reference's classes and functions, executed from its files."""
    p = ps.install(REF)
    T = ps.tensor

    def nms_gpu(boxes, thresh):
        keep = O.nms(_t(boxes).float().numpy(), float(thresh), kind="ref" if O.have_ref() else "port")
        full = np.zeros(boxes.shape[0], np.int32)
        full[:len(keep)] = keep
        return T(full), int(len(keep))

    iou3d_nms = types.SimpleNamespace(nms_gpu=nms_gpu)
    wrap = lambda r: ps._wrap(r)  # noqa: E731
    pointnet2_ops = types.SimpleNamespace(voxel_query_wrapper=lambda *a: wrap(mkps._voxel_torch(*a)),
                                          grouping_operation_stack=lambda *a: wrap(_group_torch(*a)))

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

    nnx = types.ModuleType("nn")
    nnx.__dict__.update({k: v for k, v in vars(p.nn).items() if not k.startswith("__")})

    class Sequential(p.nn.Sequential):
        def sublayers(self, include_self=False):
            mods = list(self.modules())
            return mods if include_self else mods[1:]

    nnx.Conv1D, nnx.Dropout, nnx.Sequential = Conv1D, Dropout, Sequential
    torch.nn.Parameter.set_value = lambda self, value: None  # init_weights' draws: the weights are seeded below
    Fx = types.SimpleNamespace(
        max_pool2d=lambda x, kernel_size: wrap(torch.nn.functional.max_pool2d(_t(x), tuple(kernel_size))),
        avg_pool2d=lambda x, kernel_size: wrap(torch.nn.functional.avg_pool2d(_t(x), tuple(kernel_size))),
        sigmoid=lambda x: wrap(torch.sigmoid(_t(x))))

    def scatter_nd(index, updates, shape):
        out = torch.zeros(tuple(int(s) for s in shape), dtype=_t(updates).dtype)
        out.index_put_(tuple(_t(index).long().unbind(-1)), _t(updates), accumulate=True)
        return wrap(out)

    p.scatter_nd = scatter_nd
    p.cos, p.sin = (lambda x: wrap(torch.cos(_t(x)))), (lambda x: wrap(torch.sin(_t(x))))
    p.nonzero = lambda x: wrap(torch.nonzero(_t(x)))
    p.gather = lambda x, index, axis=0: wrap(torch.index_select(_t(x), axis, _t(index).long().reshape(-1)))
    p.normal = lambda mean=0.0, std=1.0, shape=None: wrap(torch.zeros(tuple(shape)))  # weights are seeded below
    noop = lambda *a, **k: None  # noqa: E731
    base = dict(paddle=p, nn=nnx, F=Fx, pointnet2_ops=pointnet2_ops, List=list, constant_init=noop,
                kaiming_normal_init=noop, xavier_normal_init=noop, iou3d_nms=iou3d_nms)
    stack = os.path.join(MODELS, "common/pointnet2_stack")
    vq = ps.exec_lines(os.path.join(stack, "voxel_query_utils.py"), [(28, 106)], dict(base))
    vmods = ps.exec_lines(os.path.join(stack, "voxel_pool_modules.py"), [(29, 163)], dict(
        base, voxel_query_utils=types.SimpleNamespace(VoxelQueryAndGrouping=vq["VoxelQueryAndGrouping"])))
    box_utils = ps.exec_lines(os.path.join(MODELS, "common/box_utils.py"), [(17, 37), (76, 110)], dict(paddle=p))
    nms = ps.exec_lines(os.path.join(MODELS, "common/model_nms_utils.py"), [(20, 66)], dict(base))
    coder = ps.exec_lines(os.path.join(REF, "paddle3d/utils/box_coder.py"), [(22, 100)], dict(paddle=p))
    base.update(class_agnostic_nms=nms["class_agnostic_nms"], rotate_points_along_z=box_utils["rotate_points_along_z"],
                get_voxel_centers=box_utils["get_voxel_centers"],
                generate_voxel2pinds=box_utils["generate_voxel2pinds"],
                voxelpool_stack_modules=types.SimpleNamespace(
                    NeighborVoxelSAModuleMSG=vmods["NeighborVoxelSAModuleMSG"]))
    rb = os.path.join(MODELS, "heads/roi_heads/roi_head_base.py")
    methods = ps.exec_lines(rb, [(69, 131), (293, 322), (324, 346)], dict(base))

    def base_init(self, num_class, model_cfg, **kwargs):  # the inference part of RoIHeadBase.__init__ (:33-43)
        nnx.Layer.__init__(self)
        self.model_cfg, self.num_class = model_cfg, num_class
        self.box_coder = coder["ResidualCoder"]()

    RoIHeadBase = type("RoIHeadBase", (nnx.Layer,), dict(
        __init__=base_init, proposal_layer=methods["proposal_layer"],
        generate_predicted_boxes=methods["generate_predicted_boxes"],
        get_global_grid_points_of_roi=methods["get_global_grid_points_of_roi"],
        get_dense_grid_points=methods["get_dense_grid_points"]))
    head = ps.exec_lines(os.path.join(MODELS, "heads/roi_heads/voxelrcnn_head.py"), [(31, 288)],
                         dict(base, RoIHeadBase=RoIHeadBase))["VoxelRCNNHead"]
    post = ps.exec_lines(os.path.join(MODELS, "detection/voxel_rcnn/voxel_rcnn.py"), [(145, 220)],
                         dict(base))["post_processing"]
    return p, head, post, nms["class_agnostic_nms"]


def check_exact(O, boxes, scores, thresh, what, rows=None):
    """No tie among the scores, no IoU within 1e-4 of the threshold.  rows: what each score was computed from; rows
    that are equal (the zero-padded RoIs of a frame) give equal scores and equal boxes on every implementation, so
    only ties between different rows count."""
    s = np.asarray(scores, np.float32).reshape(-1)
    distinct = len(s) if rows is None else len(np.unique(np.asarray(rows).reshape(len(s), -1), axis=0))
    assert len(np.unique(s)) == distinct, f"{what}: tied scores"
    if len(boxes) > 1:
        margin = O.iou_margin(np.ascontiguousarray(boxes, np.float32), float(thresh))
        assert margin > 1e-4, f"{what}: an IoU {margin} from the threshold"


def bound(ref32, ref64):
    err = float(np.abs(ref32.astype(np.float64) - ref64).max())
    ulp = float(np.spacing(np.float32(np.abs(ref64).max())))
    return np.float64(max(4.0 * err, ulp)), np.float64(err)


def post_dicts(dicts, prefix, out):
    for b, d in enumerate(dicts):
        out[f"{prefix}_boxes{b}"] = _t(d["box3d_lidar"]).numpy().reshape(-1, 7)
        out[f"{prefix}_scores{b}"] = _t(d["scores"]).numpy().reshape(-1)
        out[f"{prefix}_labels{b}"] = _t(d["label_preds"]).numpy().reshape(-1).astype(np.int64)


def main():
    from oracle import pyoracle as O

    O.build(ref=True)
    p, Head, post_processing, can = build_reference(O)
    T = ps.tensor
    out = {}
    for tag in ("a", "b"):
        rng = np.random.default_rng({"a": 31, "b": 32}[tag])
        K = NUM_CLASS[tag]
        cfg = model_cfg(tag)
        head = Head(input_channels=dict(INPUT_CHANNELS), model_cfg=copy.deepcopy(cfg), point_cloud_range=PCR,
                    voxel_size=VOXEL, num_class=1)  # class agnostic: one score, one box per RoI
        head.eval()
        shapes = ps.fill_state(head, 50 + ord(tag))
        out[f"{tag}_state_shapes"] = np.asarray(json.dumps(shapes))
        box, cls = proposals(rng, K)
        sc = scales(rng)
        out[f"{tag}_box_preds"], out[f"{tag}_cls_preds"] = box, cls
        for name, (ind, feats) in sc.items():
            out[f"{tag}_{name}_indices"], out[f"{tag}_{name}_features"] = ind, feats
        nmsc = cfg["nms_config"]["test"]
        for b in range(2):
            order = np.argsort(-cls[b].max(1), kind="stable")[:nmsc["nms_pre_maxsize"]]
            check_exact(O, box[b][order], cls[b].max(1), nmsc["nms_thresh"], f"{tag} proposals frame {b}")

        # every pool layer call of the fp32 run is recorded, to repeat it in fp64
        pool_calls = []
        for k, layer in enumerate(head.roi_grid_pool_layers):
            def rec(*a, _f=layer.forward, _k=k, **kw):
                r = _f(*a, **kw)
                pool_calls.append((_k, {n: (_t(v).clone() if isinstance(v, torch.Tensor) else v) for n, v in kw.items()},
                                   _t(r).clone()))
                return r
            layer.forward = rec
        bd = {"batch_size": 2, "batch_box_preds": T(box), "batch_cls_preds": T(cls),
              "multi_scale_3d_features": {n: Sparse(*sc[n], GRIDS[n]) for n in sc},
              "multi_scale_3d_strides": dict(STRIDES)}
        with torch.no_grad():
            bd = head(bd)
            rois = _t(bd["rois"]).clone()
            grid_xyz, _ = head.get_global_grid_points_of_roi(bd["rois"], grid_size=cfg["roi_grid_pool"]["grid_size"])
            pooled = head.roi_grid_pool(bd)
            del pool_calls[2:]  # the second roi_grid_pool repeats the forward's calls
            flat = pooled.reshape([pooled.shape[0], -1])
            shared = head.shared_fc_layer(flat)
            rcnn_cls = head.cls_pred_layer(head.cls_fc_layers(shared))
            rcnn_reg = head.reg_pred_layer(head.reg_fc_layers(shared))
        out[f"{tag}_rois"] = rois.numpy()
        out[f"{tag}_roi_scores"] = _t(bd["roi_scores"]).numpy()
        out[f"{tag}_roi_labels"] = _t(bd["roi_labels"]).numpy().astype(np.int64)
        out[f"{tag}_grid_xyz"] = _t(grid_xyz).numpy()
        out[f"{tag}_pooled"] = _t(pooled).numpy()
        out[f"{tag}_rcnn_cls"], out[f"{tag}_rcnn_reg"] = _t(rcnn_cls).numpy(), _t(rcnn_reg).numpy()
        out[f"{tag}_batch_cls_preds"] = _t(bd["batch_cls_preds"]).numpy()
        out[f"{tag}_batch_box_preds"] = _t(bd["batch_box_preds"]).numpy()
        assert bd["cls_preds_normalized"] is False
        nsurv = (np.abs(out[f"{tag}_rois"]).sum(-1) > 0).sum(1)
        assert nsurv[0] == nmsc["nms_post_maxsize"] and 0 < nsurv[1] < nmsc["nms_post_maxsize"], nsurv

        # the pool layers' inputs, their fp32 outputs and the fp64 evaluation of layers and FC stacks
        head64 = copy.deepcopy(head).double()
        pooled64 = []
        with torch.no_grad():
            for k, kw, r in pool_calls:
                out[f"{tag}_pool{k}_new_xyz"] = kw["new_xyz"].numpy()
                out[f"{tag}_pool{k}_new_coords"] = kw["new_coords"].numpy()  # (b, x, y, z)
                out[f"{tag}_pool{k}_xyz"] = kw["xyz"].numpy()
                out[f"{tag}_pool{k}_xyz_cnt"] = kw["xyz_batch_cnt"].numpy()
                out[f"{tag}_pool{k}_v2p"] = kw["voxel2point_indices"].numpy().astype(np.int32)
                out[f"{tag}_pool{k}_out"] = r.numpy()
                kw64 = {n: (ps._wrap(v.double()) if isinstance(v, torch.Tensor) and v.dtype == torch.float32
                            else (ps._wrap(v) if isinstance(v, torch.Tensor) else v)) for n, v in kw.items()}
                layer64 = head64.roi_grid_pool_layers[k]
                r64 = _t(type(layer64).forward(layer64, **kw64))
                assert r64.dtype == torch.float64
                out[f"{tag}_pool{k}_out64"] = r64.numpy()
                out[f"{tag}_pool{k}_bound"], out[f"{tag}_pool{k}_ref_err"] = bound(r.numpy(), r64.numpy())
                pooled64.append(r64.reshape(-1, pooled.shape[1], r64.shape[-1]))
            flat64 = torch.cat(pooled64, -1).reshape(pooled.shape[0], -1)
            shared64 = head64.shared_fc_layer(ps._wrap(flat64))
            cls64 = _t(head64.cls_pred_layer(head64.cls_fc_layers(shared64))).numpy()
            reg64 = _t(head64.reg_pred_layer(head64.reg_fc_layers(shared64))).numpy()
        out[f"{tag}_rcnn_cls64"], out[f"{tag}_rcnn_reg64"] = cls64, reg64
        out[f"{tag}_rcnn_cls_bound"], out[f"{tag}_rcnn_cls_ref_err"] = bound(out[f"{tag}_rcnn_cls"], cls64)
        out[f"{tag}_rcnn_reg_bound"], out[f"{tag}_rcnn_reg_ref_err"] = bound(out[f"{tag}_rcnn_reg"], reg64)

        # post_processing on the head's outputs: the reference sigmoids, thresholds and suppresses
        me = types.SimpleNamespace(num_class=K, post_process_cfg=POST_CFG, dense_head=types.SimpleNamespace(num_class=K))
        with torch.no_grad():
            dicts = post_processing(me, bd)
        post_dicts(dicts, f"{tag}_post", out)

        # a synthetic batch for class_agnostic_nms / post_processing alone: wide scores, frame 1 passes nothing
        box2, cls2 = proposals(rng, K, A=40)
        cls2[1] = -np.abs(cls2[1]) - 2.0  # sigmoid < 0.12 < score_thresh
        labels2 = rng.integers(1, K + 1, (2, 40)).astype(np.int64)
        out[f"{tag}_syn_box"], out[f"{tag}_syn_cls"], out[f"{tag}_syn_labels"] = box2, cls2, labels2
        bd2 = {"batch_size": 2, "batch_box_preds": T(box2), "batch_cls_preds": T(cls2), "cls_preds_normalized": False,
               "roi_labels": T(labels2)}
        with torch.no_grad():
            dicts = post_processing(me, bd2)
        post_dicts(dicts, f"{tag}_syn_post", out)
        assert out[f"{tag}_syn_post_scores1"].tolist() == [-1.0] and out[f"{tag}_syn_post_labels1"].tolist() == [-1]
        sig = torch.sigmoid(torch.from_numpy(cls2[0])).numpy().max(1)
        passed = np.nonzero(sig >= np.float32(POST_CFG["score_thresh"]))[0]
        order = passed[np.argsort(-sig[passed], kind="stable")][:POST_CFG["nms_config"]["nms_pre_maxsize"]]
        check_exact(O, box2[0][order], sig[passed], POST_CFG["nms_config"]["nms_thresh"], f"{tag} synthetic post")
        assert np.abs(sig - np.float32(POST_CFG["score_thresh"])).min() > 1e-4
        hs = torch.sigmoid(torch.from_numpy(out[f"{tag}_batch_cls_preds"])).numpy().max(-1)
        assert np.abs(hs - np.float32(POST_CFG["score_thresh"])).min() > 1e-4
        for b in range(2):
            ok = np.nonzero(hs[b] >= np.float32(POST_CFG["score_thresh"]))[0]
            if len(ok):
                o2 = ok[np.argsort(-hs[b][ok], kind="stable")]
                check_exact(O, out[f"{tag}_batch_box_preds"][b][o2], hs[b][ok], POST_CFG["nms_config"]["nms_thresh"],
                            f"{tag} head post frame {b}", rows=out[f"{tag}_rois"][b][ok])
        # class_agnostic_nms alone, without a threshold and on raw scores (the proposal layer's form), frame 0
        with torch.no_grad():
            s, l, bx = can(box_scores=T(cls2[0].max(1)), box_preds=T(box2[0]),
                           label_preds=T(cls2[0].argmax(1).astype(np.int64)), nms_config=nmsc)
        out[f"{tag}_can_scores"], out[f"{tag}_can_labels"] = _t(s).numpy(), _t(l).numpy().astype(np.int64)
        out[f"{tag}_can_boxes"] = _t(bx).numpy()
        o3 = np.argsort(-cls2[0].max(1), kind="stable")[:nmsc["nms_pre_maxsize"]]
        check_exact(O, box2[0][o3], cls2[0].max(1), nmsc["nms_thresh"], f"{tag} synthetic nms")
        print(tag, "survivors", nsurv.tolist(), "post", [len(out[f"{tag}_post_scores{b}"]) for b in range(2)],
              "bounds", {k: float(out[f"{tag}_{k}_bound"]) for k in ("pool0", "pool1", "rcnn_cls", "rcnn_reg")},
              "ref errors", {k: float(out[f"{tag}_{k}_ref_err"]) for k in ("pool0", "pool1", "rcnn_cls", "rcnn_reg")})

    np.savez_compressed(OUT, **{k: np.asarray(v) for k, v in out.items()})
    print(os.path.getsize(OUT), "bytes")


def load(path=OUT):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def state(g, tag):
    """The recorded head's Paddle-named state dict, regenerated from the stored keys and shapes (fill_state's rule)."""
    shapes = json.loads(str(g[f"{tag}_state_shapes"]))
    rng = np.random.default_rng(50 + ord(tag))
    return {k: ps.synth_param(k, tuple(shapes[k]), rng) for k in sorted(shapes)}


if __name__ == "__main__":
    main()
