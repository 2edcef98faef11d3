"""PV-RCNN's entry points (the rows of paddle3d_amd._lib.ENTRY_POINTS that name this module) under guarded
allocations: tests/guarded.py's Protocol.  Each scenario builds seeded inputs and returns `(inputs, call)`; it runs plain,
guarded with fill 0x00 and guarded with fill 0xFF (tests/guarded.py), and the test asserts: no guard band damaged (no
store outside an output), every input bit-equal to its clone, every specified output bit-equal across the three runs
(nothing depends on what a buffer held before) and not trivial.  The model scenario constructs the modules inside the
run, so their tensors are allocated under the guard too.

The last test asserts that the scenarios reach every one of them."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from guarded import Protocol  # noqa: E402

import make_pv_rcnn_golden as mk  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32

P = Protocol("test_memory_safety_pvrcnn_gpu", "memory-safety-pvrcnn", DEV)
scenario = P.scenario


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@scenario
def stack_sa_pool():
    """Every (c1, c2) of {16, 32, 64}^2 at nsample 16 and at one that is no multiple of the 16-slot tile, with and
    without features; pooled is written whole ([m, c2], every row: rows without a hit too)."""
    from paddle3d_amd.ops import pvrcnn

    g = mk.load()
    rng = np.random.default_rng(17)
    base = {k: _t(g[f"a_roi_pool_{k}"]) for k in ("new_xyz", "new_xyz_batch_cnt", "xyz", "xyz_batch_cnt")}
    n = int(base["xyz"].shape[0])
    inputs = dict(base)
    for c in (16, 32, 64):
        inputs[f"features_in{c}"] = _t(rng.standard_normal((n, c)).astype(F32))
        inputs[f"w_pos{c}"] = _t(rng.standard_normal((c, 3)).astype(F32))
        inputs[f"scale{c}"] = _t(rng.uniform(0.5, 1.5, c).astype(F32))
        inputs[f"shift{c}"] = _t(rng.normal(0, 0.3, c).astype(F32))
        for c2 in (16, 32, 64):
            inputs[f"w2_{c}_{c2}"] = _t((rng.standard_normal((c2, c)) / np.sqrt(c)).astype(F32))

    def call():
        outs = {}
        for c1 in (16, 32, 64):
            for c2 in (16, 32, 64):
                for S, feats in ((16, True), (21, False)):
                    outs[f"pooled_{c1}_{c2}_{S}"] = pvrcnn.stack_sa_pool(
                        base["new_xyz"], base["new_xyz_batch_cnt"], base["xyz"], base["xyz_batch_cnt"],
                        inputs[f"features_in{c1}"] if feats else None, inputs[f"w_pos{c1}"], inputs[f"scale{c1}"],
                        inputs[f"shift{c1}"], inputs[f"w2_{c1}_{c2}"], inputs[f"scale{c2}"], inputs[f"shift{c2}"], 0.8, S)
        return outs

    return inputs, call


@scenario
def bev_interpolate():
    """Keypoints on, inside and outside the map, a row of no frame; out is written whole (zero rows too)."""
    from paddle3d_amd.ops import pvrcnn

    g = mk.load()
    kp = np.concatenate([g["b_keypoints"], g["b_keypoints"][:3]])
    kp[-3:, 0] = (-1, 2, 0.5)
    inputs = dict(kp=_t(kp), bev=_t(g["b_bev"]), bev_odd=_t(np.random.default_rng(2).standard_normal((2, 37, 5, 7)).astype(F32)))

    def call():
        return dict(out=pvrcnn.bev_interpolate(inputs["kp"], inputs["bev"], mk.PCR, mk.VOXEL, mk.BEV["b"][3]),
                    out_odd=pvrcnn.bev_interpolate(inputs["kp"], inputs["bev_odd"], mk.PCR, mk.VOXEL, 4))

    return inputs, call


@scenario
def second_stage():
    """VoxelSetAbstraction, PointHeadSimple and PVRCNNHead with the fused layers + post_processing (padded), built
    inside the run."""
    from paddle3d_amd import pv_rcnn as pr
    from paddle3d_amd import roi_heads as rh
    from paddle3d_amd.checkpoint import load_paddle_state_dict
    from paddle3d_amd.sparse import SparseConvTensor

    g, tag = mk.load(), "b"
    inputs = {k: _t(g[f"{tag}_{k}"]) for k in ("points", "bev", "box_preds", "cls_preds")}
    inputs.update({f"{n}_{k}": _t(g[f"{tag}_{n}_{k}"]) for n in mk.GRIDS for k in ("indices", "features")})

    def call():
        enc = pr.VoxelSetAbstraction(mk.encoder_cfg(tag), mk.VOXEL, mk.PCR, num_bev_features=mk.BEV[tag][0],
                                     num_rawpoint_features=mk.NUM_RAWPOINT_FEATURES, fused=True)
        ph = pr.PointHeadSimple(mk.NUM_CLASS, enc.num_point_features_before_fusion, mk.POINT_HEAD_CFG)
        head = rh.PVRCNNHead(enc.num_point_features, mk.roi_head_cfg(tag), num_class=1, fused=True)
        for name, m in (("point_encoder", enc), ("point_head", ph), ("roi_head", head)):
            load_paddle_state_dict(m, mk.state(g, tag, name))
        model = pr.PVRCNNSecondStage(enc, ph, head).eval().to(DEV)
        feats = {n: SparseConvTensor(inputs[f"{n}_features"], inputs[f"{n}_indices"], mk.GRIDS[n], 2) for n in mk.GRIDS}
        bd = rh.pv_rcnn_second_stage({
            "batch_size": 2, "points": inputs["points"], "points_batch_cnt": g[f"{tag}_points_cnt"].tolist(),
            "spatial_features": inputs["bev"], "spatial_features_stride": mk.BEV[tag][3],
            "multi_scale_3d_features": feats, "batch_box_preds": inputs["box_preds"],
            "batch_cls_preds": inputs["cls_preds"]}, model)
        with torch.no_grad():
            post = rh.post_processing(bd, mk.POST_CFG, mk.NUM_CLASS, padded=True)
        outs = {k: bd[k] for k in ("point_coords", "point_features_before_fusion", "point_features", "point_cls_scores",
                                   "rois", "roi_scores", "roi_labels", "batch_cls_preds", "batch_box_preds")}
        outs.update({f"post_{k}": v for k, v in zip(("boxes", "scores", "labels", "count"), post)})
        return outs

    return inputs, call


@pytest.mark.parametrize("name", list(P.scenarios))
def test_scenario(name):
    P.check_scenario(name)


def test_every_launching_entry_point_is_exercised():
    """Runs last; scenarios that did not run in this process are run here in their plain form."""
    from paddle3d_amd import _lib

    P.check_complete(_lib.symbols("test_memory_safety_pvrcnn_gpu"), 2)
