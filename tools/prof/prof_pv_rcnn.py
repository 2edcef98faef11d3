"""Time PV-RCNN's second stage (paddle3d_amd/pv_rcnn.py, roi_heads.PVRCNNHead, csrc/pvrcnn.hip) at the KITTI
configuration's shapes (configs/pv_rcnn/pv_rcnn_005voxel_kitti.yml): B = 2 and 4 frames, 16 384 raw points and 2048
keypoints per frame, a 256 x 200 x 176 BEV map, four sparse scales (41 x 1600 x 1408 / 21 x 800 x 704 / 11 x 400 x 352 /
5 x 200 x 176 cells, about 35k / 30k / 12k / 5k voxels per frame, 16 / 32 / 64 / 64 channels), 128 RoIs x 6^3 grid
points per frame (nms_post_maxsize raised from the test configuration's 100 to the 128 the issue of this tool names),
70 400 anchors.

  scale    every scale of every StackSAModuleMSG (raw points, x_conv1..4, the RoI grid pool): the scale's forward with
           fused=True (pd3_stack_sa_pool behind one matmul over the source rows) against fused=False (the forward as
           it was: ball query, two groupings, masks, concat, Conv2d / BN / ReLU twice on [1, C, M, nsample], max
           pool), same module and weights
  bev      interpolate_from_bev_features: pd3_bev_interpolate against the reference's per-frame composition in torch
  head     PVRCNNHead.forward, fused against unfused
  stage    VoxelSetAbstraction -> PointHeadSimple -> PVRCNNHead, fused against unfused

Both sides of a pair run in one process, alternating, after 3 warm-up calls; a window is `--iters` calls between two
device synchronisations, `--repeats` windows per side; the table shows the median and the spread (max - min) of the
windows in us per call.  `grouped` is the size of the [M, 3 + C, nsample] tensor the unfused scale writes.

    python tools/prof/prof_pv_rcnn.py [--iters 20] [--repeats 7] [--batches 2 4] [--json PATH]
Run under `rocprofv3 --kernel-trace --stats -- python tools/prof/prof_pv_rcnn.py --iters 2 --repeats 1` for kernel
times."""
import argparse
import json
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from paddle3d_amd import pv_rcnn as pr  # noqa: E402
from paddle3d_amd import roi_heads as rh  # noqa: E402
from paddle3d_amd.ops import pvrcnn  # noqa: E402
from paddle3d_amd.pointnet2_stack import StackSAModuleMSG  # noqa: E402
from paddle3d_amd.sparse import SparseConvTensor  # noqa: E402
from prof_roi_head import pair, proposals  # noqa: E402

DEV = "cuda"
RANGE, VOXEL = rh.PV_RCNN_KITTI_RANGE, rh.PV_RCNN_KITTI_VOXEL
SCALES = {"x_conv1": (1, (41, 1600, 1408), 35000, 16), "x_conv2": (2, (21, 800, 704), 30000, 32),
          "x_conv3": (4, (11, 400, 352), 12000, 64), "x_conv4": (8, (5, 200, 176), 5000, 64)}


def scene(batch, seed=7):
    """Clustered voxels of the four scales, raw points on the finest scale's voxels, a BEV map."""
    rng = np.random.default_rng(seed)
    Z, Y, X = SCALES["x_conv1"][1]
    feats, pts, counts = {}, [], []
    cells_f = []
    for b in range(batch):
        c = np.stack([rng.integers(4, Z - 4, 160), rng.integers(40, Y - 40, 160), rng.integers(40, X - 40, 160)], 1)
        cells = (c[rng.integers(0, 160, 60000)] + np.round(rng.normal(0, [3, 16, 16], (60000, 3)))).astype(np.int64)
        cells = np.clip(cells, 0, [Z - 1, Y - 1, X - 1])
        cells_f.append(cells)
        pick = cells[rng.integers(0, len(cells), 16384)]
        xyz = (pick[:, ::-1] + rng.random((16384, 3))) * np.array(VOXEL) + np.array(RANGE[:3])
        pts.append(np.concatenate([np.full((16384, 1), b), xyz, rng.random((16384, 1))], 1))
        counts.append(16384)
    for name, (stride, (z, y, x), n, ch) in SCALES.items():
        ind = []
        for b in range(batch):
            cc = np.minimum(cells_f[b] // stride, [z - 1, y - 1, x - 1])
            flat = np.unique((cc[:, 0] * y + cc[:, 1]) * x + cc[:, 2])
            flat = np.sort(rng.permutation(flat)[:n - (n // 20) * (b % 2)])
            zz, yy, xx = np.unravel_index(flat, (z, y, x))
            ind.append(np.stack([np.full(len(flat), b), zz, yy, xx], 1))
        ind = torch.from_numpy(np.concatenate(ind).astype(np.int32)).to(DEV)
        f = torch.from_numpy(rng.standard_normal((ind.shape[0], ch)).astype(np.float32)).to(DEV)
        feats[name] = SparseConvTensor(f, ind, (z, y, x), batch)
    points = torch.from_numpy(np.concatenate(pts).astype(np.float32)).to(DEV)
    bev = torch.from_numpy(rng.standard_normal((batch, 256, 200, 176)).astype(np.float32)).to(DEV)
    return points, counts, feats, bev


def one_scale(layer, k):
    """Scale k of a StackSAModuleMSG as a layer of its own (the same grouper and mlp objects)."""
    m = StackSAModuleMSG.__new__(StackSAModuleMSG)
    nn.Module.__init__(m)
    m.fused, m.use_xyz, m.pool_method = layer.fused, layer.use_xyz, layer.pool_method
    m.groupers, m.mlps = nn.ModuleList([layer.groupers[k]]), nn.ModuleList([layer.mlps[k]])
    return m.eval()


def bev_per_frame(keypoints, bev, stride):
    """interpolate_from_bev_features as the reference composes it (voxel_set_abstraction.py:32-67, 180-213), with the
    frames' keypoint ranges known on the host."""
    x = (keypoints[:, 1] - RANGE[0]) / VOXEL[0] / stride
    y = (keypoints[:, 2] - RANGE[1]) / VOXEL[1] / stride
    out, per = [], keypoints.shape[0] // bev.shape[0]
    for k in range(bev.shape[0]):
        im = bev[k].permute(1, 2, 0)
        cx, cy = x[k * per:(k + 1) * per], y[k * per:(k + 1) * per]
        x0, y0 = torch.floor(cx).long(), torch.floor(cy).long()
        x1, y1 = x0 + 1, y0 + 1
        x0, x1 = x0.clamp(0, im.shape[1] - 1), x1.clamp(0, im.shape[1] - 1)
        y0, y1 = y0.clamp(0, im.shape[0] - 1), y1.clamp(0, im.shape[0] - 1)
        wa, wb = (x1 - cx) * (y1 - cy), (x1 - cx) * (cy - y0)
        wc, wd = (cx - x0) * (y1 - cy), (cx - x0) * (cy - y0)
        out.append(im[y0, x0] * wa[:, None] + im[y1, x0] * wb[:, None] + im[y0, x1] * wc[:, None] + im[y1, x1] * wd[:, None])
    return torch.cat(out, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "prof_pv_rcnn.py measures on the GPU only"
    torch.manual_seed(0)
    rows = []
    for batch in a.batches:
        points, counts, feats, bev = scene(batch)
        model = rh.pv_rcnn_kitti(fused=True).to(DEV).eval()
        for m in model.modules():  # non-trivial BatchNorm statistics
            if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
        model.roi_head.model_cfg["nms_config"]["test"]["nms_post_maxsize"] = 128
        enc, head = model.point_encoder, model.roi_head
        layers = [enc.sa_rawpoints, *enc.sa_layers, head.roi_grid_pool_layer]

        def set_fused(f):
            for l in layers:
                l.fused = f

        box, cls = proposals(batch)
        cls = cls.expand(-1, -1, 3).contiguous()

        def bd():
            return {"batch_size": batch, "points": points, "points_batch_cnt": counts, "spatial_features": bev,
                    "spatial_features_stride": 8, "multi_scale_3d_features": feats, "batch_box_preds": box,
                    "batch_cls_preds": cls}

        with torch.no_grad():
            # every StackSAModuleMSG call of one forward, recorded with its arguments
            calls = []
            hooks = [l.register_forward_pre_hook(lambda m, args, kw, _n=n: calls.append((_n, m, kw)), with_kwargs=True)
                     for n, l in zip(["raw_points", *enc.sa_layer_names, "roi_pool"], layers)]
            full = model(bd())
            for h in hooks:
                h.remove()
            for name, layer, kw in calls:
                M, C = int(kw["new_xyz"].shape[0]), 0 if kw["features"] is None else int(kw["features"].shape[1])
                for k in range(len(layer.mlps)):
                    sc = one_scale(layer, k)

                    def run(fused, sc=sc, kw=kw):
                        sc.fused = fused
                        return sc(**kw)[1]

                    diff = float((run(True) - run(False)).abs().max())
                    (tf, sf), (tu, su) = pair(lambda: run(True), lambda: run(False), a.iters, a.repeats)
                    g = layer.groupers[k]
                    rows.append(dict(what=f"{name} r={g.radius} S={g.nsample} {layer.mlps[k][0].out_channels}/"
                                          f"{layer.mlps[k][3].out_channels}", B=batch, fused_us=tf, fused_spread=sf,
                                     unfused_us=tu, unfused_spread=su, max_abs_diff=diff, M=M,
                                     grouped_MB=M * (3 + C) * g.nsample * 4 / 1e6))
            kp = full["point_coords"]
            # torch divides by a host scalar on the device as a product with its reciprocal: the sample positions
            # differ from the true division's in the last bit (1.5e-5 at x = 176), the weights with them
            assert torch.allclose(pvrcnn.bev_interpolate(kp, bev, RANGE, VOXEL, 8), bev_per_frame(kp, bev, 8), atol=1e-3)
            (tf, sf), (tu, su) = pair(lambda: pvrcnn.bev_interpolate(kp, bev, RANGE, VOXEL, 8),
                                      lambda: bev_per_frame(kp, bev, 8), a.iters, a.repeats)
            rows.append(dict(what="bev interpolate", B=batch, fused_us=tf, fused_spread=sf, unfused_us=tu, unfused_spread=su))

            def head_bd():
                d = bd()
                d.update({k: full[k] for k in ("point_coords", "point_features", "point_cls_scores")})
                return d

            def run_head(f):
                set_fused(f)
                return head(head_bd())

            def run_stage(f):
                set_fused(f)
                return model(bd())

            (tf, sf), (tu, su) = pair(lambda: run_head(True), lambda: run_head(False), a.iters, a.repeats)
            rows.append(dict(what="head forward", B=batch, fused_us=tf, fused_spread=sf, unfused_us=tu, unfused_spread=su))
            (tf, sf), (tu, su) = pair(lambda: run_stage(True), lambda: run_stage(False), max(a.iters // 4, 1), a.repeats)
            rows.append(dict(what="second stage", B=batch, fused_us=tf, fused_spread=sf, unfused_us=tu, unfused_spread=su))
            assert full["batch_box_preds"].shape == (batch, 128, 7)
    print(f"{'what':<32}{'B':>3}{'new us':>10}{'spread':>8}{'old us':>10}{'spread':>8}{'old/new':>8}  notes")
    for r in rows:
        note = ""
        if "grouped_MB" in r:
            note = f"M {r['M']}; grouped {r['grouped_MB']:.0f} MB; max |fused - unfused| {r['max_abs_diff']:.2e}"
        wins = r["unfused_us"] - r["fused_us"] > max(r["fused_spread"], r["unfused_spread"])
        print(f"{r['what']:<32}{r['B']:>3}{r['fused_us']:>10.1f}{r['fused_spread']:>8.1f}{r['unfused_us']:>10.1f}"
              f"{r['unfused_spread']:>8.1f}{r['unfused_us'] / r['fused_us']:>8.2f}  {'wins' if wins else 'NO WIN'}  {note}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
