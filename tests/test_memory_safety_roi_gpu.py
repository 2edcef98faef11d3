"""The RoI head's entry points (the rows of paddle3d_amd._lib.ENTRY_POINTS that name this module) under guarded
allocations: tests/guarded.py's Protocol.  Each scenario builds seeded inputs and returns `(inputs, call)`; it runs plain,
guarded with fill 0x00 and guarded with fill 0xFF (tests/guarded.py), and the test asserts: no guard band damaged (no
store outside an output or a workspace), every input bit-equal to its clone, every specified output bit-equal across
the three runs (nothing depends on what a buffer held before) and not trivial.  The head scenario constructs the
module inside the run, so its tensors are allocated under the guard too.

The last test asserts that the scenarios reach every kernel-launching one of them."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from guarded import Protocol  # noqa: E402

import make_roi_head_golden as mk  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32

P = Protocol("test_memory_safety_roi_gpu", "memory-safety-roi", DEV)
scenario = P.scenario


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pool_inputs(C1, seed):
    g = mk.load()
    rng = np.random.default_rng(seed)
    xyz = g["a_pool0_xyz"]
    return dict(new_xyz=_t(g["a_pool0_new_xyz"]), new_coords=_t(g["a_pool0_new_coords"][:, [0, 3, 2, 1]]),
                xyz=_t(xyz), point_indices=_t(g["a_pool0_v2p"]),
                features_in=_t(rng.standard_normal((xyz.shape[0], C1)).astype(F32)),
                w_pos=_t(rng.standard_normal((C1, 3)).astype(F32)),
                pos_scale=_t(rng.uniform(0.5, 1.5, C1).astype(F32)), pos_shift=_t(rng.normal(0, 0.3, C1).astype(F32)))


@scenario
def voxel_pool():
    """C1 = 16 / 32 / 64, max and avg, nsample 16 and one that is not a multiple of the sample groups; pooled is
    written whole ([m, c1], every row: rows without a hit too)."""
    from paddle3d_amd.ops import roi_head

    inputs = {f"{k}{C1}": v for C1 in (16, 32, 64) for k, v in _pool_inputs(C1, C1).items()}

    def call():
        outs = {}
        for C1 in (16, 32, 64):
            a = {k[:-2]: v for k, v in inputs.items() if k.endswith(str(C1))}
            for S, pool in ((16, "max_pool"), (7, "avg_pool")):
                outs[f"pooled_{C1}_{S}_{pool}"] = roi_head.voxel_pool(**a, max_range=[2, 2, 2], radius=0.5, nsample=S,
                                                                      pool_method=pool)
        return outs

    return inputs, call


@scenario
def grid_points_and_decode():
    """roi_grid_xyz, every stride's coords and the decoded boxes are written whole."""
    from paddle3d_amd.ops import roi_head

    g = mk.load()
    rng = np.random.default_rng(9)
    inputs = dict(rois=_t(g["b_rois"]), enc=_t(rng.normal(0, 0.3, g["b_rois"].shape).astype(F32)))

    def call():
        xyz, coords = roi_head.roi_grid_points(inputs["rois"], 5, mk.PCR, mk.VOXEL, [1, 2, 4])
        outs = dict(xyz=xyz, decoded=roi_head.rcnn_decode_boxes(inputs["rois"], inputs["enc"]))
        outs.update({f"coords{k}": c for k, c in enumerate(coords)})
        return outs

    return inputs, call


@scenario
def class_agnostic_nms():
    """With and without a threshold, with passed-in labels, a frame that passes nothing; all four outputs are written
    whole ("rows behind count are zeros")."""
    from paddle3d_amd.ops import roi_head

    g = mk.load()
    inputs = dict(box=_t(g["b_syn_box"]), cls=_t(g["b_syn_cls"]), labels=_t(g["b_syn_labels"]))

    def call():
        outs = {}
        for name, kw in (("proposal", dict(nms_config=dict(nms_pre_maxsize=33, nms_post_maxsize=12, nms_thresh=0.7))),
                         ("post", dict(nms_config=dict(nms_pre_maxsize=30, nms_post_maxsize=6, nms_thresh=0.1),
                                       score_thresh=0.3, apply_sigmoid=True, labels=inputs["labels"]))):
            r = roi_head.class_agnostic_nms(inputs["box"], inputs["cls"], **kw)
            outs.update({f"{name}_{k}": v for k, v in zip(("boxes", "scores", "labels", "count"), r)})
        return outs

    return inputs, call


@scenario
def head_forward():
    """VoxelRCNNHead.forward + post_processing (padded) with the fused pool, built inside the run."""
    from paddle3d_amd import roi_heads as rh
    from paddle3d_amd.checkpoint import load_paddle_state_dict
    from paddle3d_amd.sparse import SparseConvTensor

    g = mk.load()
    inputs = dict(box=_t(g["a_box_preds"]), cls=_t(g["a_cls_preds"]))
    inputs.update({f"{n}_{k}": _t(g[f"a_{n}_{k}"]) for n in mk.GRIDS for k in ("indices", "features")})

    def call():
        head = rh.VoxelRCNNHead(input_channels=dict(mk.INPUT_CHANNELS), model_cfg=mk.model_cfg("a"),
                                point_cloud_range=mk.PCR, voxel_size=mk.VOXEL, num_class=1, fused_pool=True).eval()
        load_paddle_state_dict(head, mk.state(g, "a"))
        head = head.to(DEV)
        feats = {n: SparseConvTensor(inputs[f"{n}_features"], inputs[f"{n}_indices"], mk.GRIDS[n], 2) for n in mk.GRIDS}
        with torch.no_grad():
            bd = head({"batch_size": 2, "batch_box_preds": inputs["box"], "batch_cls_preds": inputs["cls"],
                       "multi_scale_3d_features": feats, "multi_scale_3d_strides": dict(mk.STRIDES)})
            post = rh.post_processing(bd, mk.POST_CFG, 1, padded=True)
        outs = {k: bd[k] for k in ("rois", "roi_scores", "roi_labels", "batch_cls_preds", "batch_box_preds")}
        outs.update({f"post_{k}": v for k, v in zip(("boxes", "scores", "labels", "count"), post)})
        return outs

    return inputs, call


@pytest.mark.parametrize("name", list(P.scenarios))
def test_scenario(name):
    P.check_scenario(name)


def test_every_launching_entry_point_is_exercised():
    """Runs last; scenarios that did not run in this process are run here in their plain form."""
    from paddle3d_amd import _lib

    launching = [s for s in _lib.symbols("test_memory_safety_roi_gpu") if not s.endswith("_workspace")]
    P.check_complete(launching, 4)
