"""Voxel R-CNN's RoI head on the CPU: the NumPy restatement of the four entry points (tests/golden/roi_head_numpy.py)
against what the reference's own Python computed (tests/golden/python_roi_head.npz), and paddle3d_amd/roi_heads.py run
over the restatement (ops monkeypatched) against the recorded layer outputs, with the weights mapped from the recorded
Paddle-named state dict.

Index outputs (kept rows, labels, counts, integer coordinates) are compared exactly; the golden maker asserts that the
recorded scores do not tie and that no IoU lies within 1e-4 of a threshold.  Grid points and decoded boxes: the
tolerances tests/test_bevdet_head_cpu.py uses for decodes that go through libm (rtol = atol = 2e-6).  The pool and the
head's outputs: the bound the maker stored, 4 x the largest error of the reference's own fp32 result against the fp64
evaluation of the same sums (one fp32 ulp of the largest output as a floor)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_roi_head_golden as mk  # noqa: E402
import roi_head_numpy as rn  # noqa: E402

F32 = np.float32
TAGS = ("a", "b")
DECODE_TOL = dict(rtol=2e-6, atol=2e-6)


@pytest.fixture(scope="module")
def golden():
    return mk.load()


def _post_frames(g, prefix):
    return [(g[f"{prefix}_boxes{b}"], g[f"{prefix}_scores{b}"], g[f"{prefix}_labels{b}"]) for b in range(2)]


def _cut(boxes, scores, labels, count, thresh_given=True):
    """The padded results as the reference's per-frame lists (a frame that passed nothing: the box_empty row)."""
    out = []
    for b in range(len(count)):
        n = int(count[b]) if count[b] > 0 or not thresh_given else 1
        out.append((boxes[b, :n], scores[b, :n], labels[b, :n]))
    return out


def _restated_post(oracle, g, box, cls, K, labels_in):
    c = mk.POST_CFG["nms_config"]
    bx, sc, lb, cnt = rn.class_agnostic_nms(oracle, box, cls, True, mk.POST_CFG["score_thresh"],
                                            labels_in if K > 1 else None, c["nms_pre_maxsize"], c["nms_thresh"],
                                            c["nms_post_maxsize"])
    if K == 1:  # the caller's `+ 1` on real rows
        lb = np.where(np.arange(lb.shape[1])[None] < cnt[:, None], lb + 1, lb)
    return _cut(bx, sc, lb, cnt)


@pytest.mark.parametrize("tag", TAGS)
def test_nms_restatement_equals_reference(golden, oracle, tag):
    g, K = golden, mk.NUM_CLASS[tag]
    nmsc = mk.model_cfg(tag)["nms_config"]["test"]
    # the proposal layer: raw scores, no threshold, zero padding, labels + 1 on the padded tensor
    bx, sc, lb, cnt = rn.class_agnostic_nms(oracle, g[f"{tag}_box_preds"], g[f"{tag}_cls_preds"], False, None, None,
                                            nmsc["nms_pre_maxsize"], nmsc["nms_thresh"], nmsc["nms_post_maxsize"])
    assert np.array_equal(bx.view(np.uint32), g[f"{tag}_rois"].view(np.uint32))
    assert np.array_equal(sc.view(np.uint32), g[f"{tag}_roi_scores"].view(np.uint32))
    assert np.array_equal(lb + 1, g[f"{tag}_roi_labels"])
    assert cnt[0] == nmsc["nms_post_maxsize"] and 0 < cnt[1] < nmsc["nms_post_maxsize"]  # a frame with padding
    # class_agnostic_nms alone on the synthetic frame 0
    bx, sc, lb, cnt = rn.class_agnostic_nms(oracle, g[f"{tag}_syn_box"][:1], g[f"{tag}_syn_cls"][:1], False, None, None,
                                            nmsc["nms_pre_maxsize"], nmsc["nms_thresh"], nmsc["nms_post_maxsize"])
    n = int(cnt[0])
    assert n == len(g[f"{tag}_can_scores"])
    assert np.array_equal(bx[0, :n].view(np.uint32), g[f"{tag}_can_boxes"].view(np.uint32))
    assert np.array_equal(sc[0, :n].view(np.uint32), g[f"{tag}_can_scores"].view(np.uint32))
    assert np.array_equal(lb[0, :n], g[f"{tag}_can_labels"])
    # post_processing: sigmoid, threshold, passed-in labels (K = 3) or argmax + 1 (K = 1), the box_empty frame
    for prefix, box, cls, lab in ((f"{tag}_syn_post", g[f"{tag}_syn_box"], g[f"{tag}_syn_cls"], g[f"{tag}_syn_labels"]),
                                  (f"{tag}_post", g[f"{tag}_batch_box_preds"], g[f"{tag}_batch_cls_preds"],
                                   g[f"{tag}_roi_labels"])):
        got = _restated_post(oracle, g, box, cls, K, lab)
        for (gb, gs, gl), (wb, ws, wl) in zip(got, _post_frames(g, prefix)):
            assert np.array_equal(gl, wl), prefix  # same rows kept, in the same order
            assert np.array_equal(gb.view(np.uint32), wb.view(np.uint32)), prefix
            np.testing.assert_allclose(gs, ws, rtol=0, atol=2e-7)  # sigmoid through glibc's expf
    assert g[f"{tag}_syn_post_scores1"].tolist() == [-1.0]


@pytest.mark.parametrize("tag", TAGS)
def test_grid_points_and_decode_restatement(golden, oracle, tag):
    g = golden
    G = mk.model_cfg(tag)["roi_grid_pool"]["grid_size"]
    xyz, coords = rn.roi_grid_points(oracle, g[f"{tag}_rois"], G, mk.PCR[:3], mk.VOXEL, [1, 2])
    np.testing.assert_allclose(xyz, g[f"{tag}_grid_xyz"].reshape(-1, 3), **DECODE_TOL)
    for k in range(2):
        np.testing.assert_allclose(xyz, g[f"{tag}_pool{k}_new_xyz"], **DECODE_TOL)
        assert np.array_equal(coords[k], g[f"{tag}_pool{k}_new_coords"]), k  # every integer coordinate
    nc = g[f"{tag}_pool0_new_coords"]
    assert ((nc[:, 1:] < 0) | (nc[:, 1:] >= np.array([24, 24, 8]))).any()  # grid points outside the voxel grid
    dec = rn.rcnn_decode_boxes(oracle, g[f"{tag}_rois"], g[f"{tag}_rcnn_reg"].reshape(g[f"{tag}_rois"].shape))
    np.testing.assert_allclose(dec, g[f"{tag}_batch_box_preds"], **DECODE_TOL)


def _pool_layer(g, tag, k, fused):
    from paddle3d_amd.checkpoint import load_paddle_state_dict
    from paddle3d_amd.pointnet2_stack import NeighborVoxelSAModuleMSG

    cfg = mk.model_cfg(tag)["roi_grid_pool"]["pool_layers"][f"x_conv{k + 1}"]
    mlps = [[mk.INPUT_CHANNELS[f"x_conv{k + 1}"]] + m for m in cfg["mlps"]]
    layer = NeighborVoxelSAModuleMSG(query_ranges=cfg["query_ranges"], nsamples=cfg["nsample"],
                                     radii=cfg["pool_radius"], mlps=mlps, pool_method=cfg["pool_method"], fused=fused)
    head = f"roi_grid_pool_layers.{k}."
    load_paddle_state_dict(layer, {n[len(head):]: v for n, v in mk.state(g, tag).items() if n.startswith(head)})
    return layer.eval()


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("k", (0, 1))
def test_pool_layers_on_cpu(golden, oracle, monkeypatch, tag, k):
    """The unfused layer and the fused one (the restated pd3_voxel_pool) against the reference's layer output."""
    g = golden
    rn.patch_cpu(monkeypatch.setattr, oracle)
    T = lambda name: torch.from_numpy(g[f"{tag}_pool{k}_{name}"])  # noqa: E731
    feats = torch.from_numpy(g[f"{tag}_x_conv{k + 1}_features"])
    M = g[f"{tag}_pool{k}_new_xyz"].shape[0]
    cnt = torch.full((2,), M // 2, dtype=torch.int32)
    want, bound = g[f"{tag}_pool{k}_out"], float(g[f"{tag}_pool{k}_bound"])
    empty = rn.pn.voxel_query(g[f"{tag}_pool{k}_new_xyz"], g[f"{tag}_pool{k}_xyz"],
                              g[f"{tag}_pool{k}_new_coords"][:, [0, 3, 2, 1]], g[f"{tag}_pool{k}_v2p"], 1.0, 1, 0, 0, 0)
    assert empty.shape[0] == M
    for fused in (False, True):
        layer = _pool_layer(g, tag, k, fused)
        with torch.no_grad():
            assert layer._takes_fused(0) == fused
            got = layer(T("xyz"), T("xyz_cnt"), T("new_xyz"), cnt, T("new_coords"), feats, T("v2p")).numpy()
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"{tag} pool{k} fused={fused}: err {err:.3e} bound {bound:.3e} reference's own {float(g[f'{tag}_pool{k}_ref_err']):.3e}")
        assert got.shape == want.shape and err <= bound, (tag, k, fused, err, bound)
    # with gradients on, or in training mode, the fused flag leaves the old path in place
    layer = _pool_layer(g, tag, k, True)
    assert not layer._takes_fused(0)
    with torch.no_grad():
        assert not layer.train()._takes_fused(0)


def test_pool_restatement_edges(golden):
    """Rows without a hit are relu(shift) (max) and the sum of nsample copies / nsample (avg); slots behind the hits
    repeat the first hit in the avg."""
    g = golden
    tag, k = "b", 1
    xyz, q = g[f"{tag}_pool{k}_xyz"], g[f"{tag}_pool{k}_new_xyz"]
    co = g[f"{tag}_pool{k}_new_coords"][:, [0, 3, 2, 1]]
    rng = np.random.default_rng(3)
    f = rng.standard_normal((xyz.shape[0], 16)).astype(F32)
    w, sc, sh = (rng.standard_normal(s).astype(F32) for s in ((16, 3), (16,), (16,)))
    args = (q, co, xyz, g[f"{tag}_pool{k}_v2p"], f, w, sc, sh, [1, 2, 2], 1.0)
    v, idx = rn.voxel_pool_terms(*args, 8)
    empty = idx[:, 0] < 0
    assert empty.any() and (~empty).any()
    mx, av = rn.voxel_pool(*args, 8, 0), rn.voxel_pool(*args, 8, 1)
    relu_sh = np.maximum(sh, 0)
    assert np.array_equal(mx[empty], np.broadcast_to(relu_sh, mx[empty].shape))
    assert np.array_equal(av[empty], np.broadcast_to(relu_sh, av[empty].shape))  # 8 equal terms: an exact sum
    partial = (~empty) & (idx[:, -1] == idx[:, 0]) & (idx[:, 1] != idx[:, 0])  # filled behind the hits
    assert partial.any()
    np.testing.assert_allclose(av, rn.voxel_pool_f64(*args, 8, 1), rtol=0, atol=2e-6)
    np.testing.assert_allclose(mx, rn.voxel_pool_f64(*args, 8, 0), rtol=0, atol=2e-6)
    for S in (5, 16):  # nsample not a multiple of the 4 sample groups; more slots than hits
        np.testing.assert_allclose(rn.voxel_pool(*args, S, 1), rn.voxel_pool_f64(*args, S, 1), rtol=0, atol=2e-6)


def run_head_cpu(g, tag, oracle, setattr_, fused):
    """paddle3d_amd.roi_heads.VoxelRCNNHead on the CPU over the restatement -> (batch_dict, rcnn outputs, padded post)."""
    from paddle3d_amd.checkpoint import load_paddle_state_dict
    from paddle3d_amd.sparse import SparseConvTensor

    rh = rn.patch_cpu(setattr_, oracle)
    head = rh.VoxelRCNNHead(input_channels=dict(mk.INPUT_CHANNELS), model_cfg=mk.model_cfg(tag),
                            point_cloud_range=mk.PCR, voxel_size=mk.VOXEL, num_class=1, fused_pool=fused).eval()
    assert load_paddle_state_dict(head, mk.state(g, tag)) == []
    feats = {n: SparseConvTensor(torch.from_numpy(g[f"{tag}_{n}_features"]), torch.from_numpy(g[f"{tag}_{n}_indices"]),
                                 mk.GRIDS[n], 2) for n in mk.GRIDS}
    bd = {"batch_size": 2, "batch_box_preds": torch.from_numpy(g[f"{tag}_box_preds"]),
          "batch_cls_preds": torch.from_numpy(g[f"{tag}_cls_preds"]), "multi_scale_3d_features": feats,
          "multi_scale_3d_strides": dict(mk.STRIDES)}
    seen = {}
    hook = head.reg_pred_layer.register_forward_hook(lambda m, i, o: seen.__setitem__("reg", o.detach().numpy()))
    with torch.no_grad():
        bd = head(bd)
        post = rh.post_processing(bd, mk.POST_CFG, mk.NUM_CLASS[tag], padded=True)
        frames = rh.post_processing(bd, mk.POST_CFG, mk.NUM_CLASS[tag])
    hook.remove()
    return bd, seen["reg"], post, frames


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("fused", (False, True))
def test_head_on_cpu_reproduces_reference(golden, oracle, monkeypatch, tag, fused):
    g = golden
    bd, reg, post, frames = run_head_cpu(g, tag, oracle, monkeypatch.setattr, fused)
    assert np.array_equal(bd["rois"].numpy().view(np.uint32), g[f"{tag}_rois"].view(np.uint32))
    assert np.array_equal(bd["roi_scores"].numpy().view(np.uint32), g[f"{tag}_roi_scores"].view(np.uint32))
    assert np.array_equal(bd["roi_labels"].numpy(), g[f"{tag}_roi_labels"])
    assert bd["cls_preds_normalized"] is False
    cls = bd["batch_cls_preds"].numpy()
    for name, got, want in (("rcnn_cls", cls.reshape(-1, 1), g[f"{tag}_rcnn_cls"]), ("rcnn_reg", reg, g[f"{tag}_rcnn_reg"])):
        err, bound = float(np.abs(got.astype(np.float64) - want).max()), float(g[f"{tag}_{name}_bound"])
        print(f"{tag} {name} fused={fused}: err {err:.3e} bound {bound:.3e}")
        assert got.shape == want.shape and err <= bound, (name, err, bound)
    np.testing.assert_allclose(bd["batch_box_preds"].numpy(), g[f"{tag}_batch_box_preds"], rtol=2e-6, atol=4e-6)
    want = _post_frames(g, f"{tag}_post")
    boxes, scores, labels, count = (t.numpy() for t in post)
    assert [int(c) for c in count] == [len(w[1]) if w[1][0] >= 0 else 0 for w in want]
    for b, (d, (wb, ws, wl)) in enumerate(zip(frames, want)):
        assert np.array_equal(d["label_preds"].numpy(), wl), b
        np.testing.assert_allclose(d["scores"].numpy(), ws, rtol=0, atol=1e-6)
        np.testing.assert_allclose(d["box3d_lidar"].numpy(), wb, rtol=2e-6, atol=4e-6)
        n = len(ws)
        assert np.array_equal(boxes[b, :n], d["box3d_lidar"].numpy()) and not boxes[b, max(n, 1):].any()


def test_kitti_constructor_and_refusals():
    from paddle3d_amd import roi_heads as rh

    head = rh.voxel_rcnn_head_kitti_car()
    assert [tuple(l.mlps_pos[0][0].weight.shape[:2]) for l in head.roi_grid_pool_layers] == [(32, 3)] * 3
    assert head.shared_fc_layer[0].in_features == 6 ** 3 * 96 and head.reg_pred_layer.out_features == 7
    assert all(l.fused == rh.FUSED_POOL_DEFAULT for l in head.roi_grid_pool_layers)
    names = set(head.state_dict())
    assert {"roi_grid_pool_layers.0.mlps_in.0.0.weight", "shared_fc_layer.4.weight", "cls_pred_layer.bias"} <= names
    with pytest.raises(NotImplementedError):
        head.train()(dict())
    with pytest.raises(NotImplementedError):
        rh.class_agnostic_nms(None, None, {"multi_class_nms": True})
    with pytest.raises(NotImplementedError):
        rh.ResidualCoder(encode_angle_by_sincos=True)


def test_abi_table_and_workspace_need_no_gpu():
    from paddle3d_amd import _lib

    L = _lib.lib()
    ws = L.pd3_class_agnostic_nms_workspace(2, 70400, 2048)
    assert 2 * 70400 * 4 * 6 <= ws < 64 * 2 ** 20
    assert L.pd3_class_agnostic_nms_workspace(2, 70400, 0) == 0 and L.pd3_class_agnostic_nms_workspace(2, 1 << 30, 8) == 0
    # refusals that need no launch
    assert L.pd3_voxel_pool(*([None] * 8), 4, 4, 1, 1, 1, 1, 24, 1.0, 16, 1, 1, 1, 0, None, None) == -3
    assert L.pd3_voxel_pool(*([None] * 8), 4, 4, 1, 1, 1, 1, 32, 1.0, 65, 1, 1, 1, 0, None, None) == -3
    assert L.pd3_voxel_pool(*([None] * 8), 4, 4, 1, 1, 1, 1, 32, 1.0, 16, 1, 1, 1, 2, None, None) == -1
