"""Time Voxel R-CNN's RoI head (paddle3d_amd/roi_heads.py, csrc/roi_head.hip) at the KITTI configuration's shapes
(configs/voxel_rcnn/voxel_rcnn_005voxel_kitti_car.yml): B = 2 and 4 frames, 100 RoIs x 6^3 grid points per frame, three
sparse scales (21 x 800 x 704 / 11 x 400 x 352 / 5 x 200 x 176 cells, about 30k / 12k / 5k voxels per frame, 32 / 64 /
64 channels in, 32 after mlps_in, nsample 16, query range 4), 70 400 anchors.

  pool     per scale, NeighborVoxelSAModuleMSG.forward with fused=True (pd3_voxel_pool) against fused=False (the
           forward as it was: voxel query, two groupings, masks, Conv2d + BatchNorm2d on [1, 3, M, 16], add, ReLU,
           pool), same module and weights
  head     VoxelRCNNHead.forward with fused_pool=True against fused_pool=False
  proposal class_agnostic_nms for the batch in one call against the per-frame composition (max / argmax, stable_argsort,
           gather, nms_gpu_device, gather in a Python loop with the host read of the count it needs)

Both sides of a pair run in one process, alternating, after a warm-up; a window is `--iters` calls between two device
synchronisations, `--repeats` windows per side; the table shows the median and the spread (max - min) of the windows
in us per call.  `needed` is the bytes the pool has to move computed from the shapes (query and coordinate rows,
window cells, the voxel centres and feature rows of the hits, the output) and `share` is needed bytes / median time
over the 8 TB/s HBM peak: the share of HBM peak, not a kernel's efficiency (the time holds every launch of the layer).

    python tools/prof/prof_roi_head.py [--iters 20] [--repeats 7] [--json PATH]
Run under `rocprofv3 --kernel-trace --stats -- python tools/prof/prof_roi_head.py --iters 2 --repeats 1` for kernel
times."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddle3d_amd import roi_heads as rh  # noqa: E402
from paddle3d_amd.ops import iou3d_nms, pointnet2_ops, roi_head, sort  # noqa: E402
from paddle3d_amd.pointnet2_stack import generate_voxel2pinds  # noqa: E402
from paddle3d_amd.sparse import SparseConvTensor  # noqa: E402

HBM_PEAK = 8.0e12
DEV = "cuda"
RANGE, VOXEL = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0], [0.05, 0.05, 0.1]
SCALES = {"x_conv2": (2, (21, 800, 704), 30000, 32), "x_conv3": (4, (11, 400, 352), 12000, 64),
          "x_conv4": (8, (5, 200, 176), 5000, 64)}


def scene(batch, seed=7, rois_per_frame=100):
    """Clustered voxels of the three scales and RoIs on the clusters (the scene of tests/test_roi_head_gpu.py)."""
    rng = np.random.default_rng(seed)
    Z, Y, X = SCALES["x_conv2"][1]
    cells_f, rois = [], []
    for b in range(batch):
        c = np.stack([rng.integers(2, Z - 2, 160), rng.integers(20, Y - 20, 160), rng.integers(20, X - 20, 160)], 1)
        cells = (c[rng.integers(0, 160, 40000)] + np.round(rng.normal(0, [2, 8, 8], (40000, 3)))).astype(np.int64)
        cells_f.append(np.clip(cells, 0, [Z - 1, Y - 1, X - 1]))
        centre = (c[:rois_per_frame, [2, 1, 0]] + 0.5) * np.array([0.1, 0.1, 0.2]) + np.array(RANGE[:3])
        size = np.array([3.9, 1.6, 1.56]) * rng.uniform(0.8, 1.2, (rois_per_frame, 3))
        rois.append(np.concatenate([centre, size, rng.uniform(-np.pi, np.pi, (rois_per_frame, 1))], 1))
    feats = {}
    for name, (stride, (z, y, x), n, ch) in SCALES.items():
        ind = []
        for b in range(batch):
            cc = np.minimum(cells_f[b] // (stride // 2), [z - 1, y - 1, x - 1])
            flat = np.unique((cc[:, 0] * y + cc[:, 1]) * x + cc[:, 2])
            flat = np.sort(rng.permutation(flat)[:n - (n // 20) * (b % 2)])
            zz, yy, xx = np.unravel_index(flat, (z, y, x))
            ind.append(np.stack([np.full(len(flat), b), zz, yy, xx], 1))
        ind = torch.from_numpy(np.concatenate(ind).astype(np.int32)).to(DEV)
        f = torch.from_numpy(rng.standard_normal((ind.shape[0], ch)).astype(np.float32)).to(DEV)
        feats[name] = SparseConvTensor(f, ind, (z, y, x), batch)
    return feats, torch.from_numpy(np.stack(rois).astype(np.float32)).to(DEV)


def proposals(batch, seed=11, A=70400):
    rng = np.random.default_rng(seed)
    box = np.zeros((batch, A, 7), np.float32)
    box[..., 0], box[..., 1] = rng.uniform(0, 70.4, (batch, A)), rng.uniform(-40, 40, (batch, A))
    box[..., 2] = rng.uniform(-2.0, 0.0, (batch, A))
    box[..., 3:6] = np.array([3.9, 1.6, 1.56]) * rng.uniform(0.8, 1.2, (batch, A, 3))
    box[..., 6] = rng.uniform(-np.pi, np.pi, (batch, A))
    cls = rng.normal(-4.0, 1.5, (batch, A, 1)).astype(np.float32)
    for b in range(batch):
        for o in rng.integers(0, A, 150):
            near = rng.integers(0, A, 24)
            box[b, near] = box[b, o] + rng.normal(0, [0.3, 0.3, 0.1, 0.1, 0.05, 0.05, 0.05], (24, 7))
            cls[b, near, 0] = rng.normal(2.0, 1.5, 24)
    return torch.from_numpy(box).to(DEV), torch.from_numpy(cls).to(DEV)


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def pair(fa, fb, iters, repeats, warm=3):
    """Alternating windows of two callables -> ((median, spread) of a, (median, spread) of b) in us per call."""
    for _ in range(warm):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(repeats):
        ta.append(window(fa, iters))
        tb.append(window(fb, iters))
    return tuple((statistics.median(t), max(t) - min(t)) for t in (ta, tb))


def pool_bytes(M, hits, window_cells, C1=32):
    """Bytes one scale's pool has to move: per query its xyz and coords, the window's cells of the voxel-to-row map,
    per hit the voxel's centre and its feature row, and the output row."""
    return M * (12 + 16) + M * window_cells * 4 + hits * (12 + C1 * 4) + M * C1 * 4


def per_frame_proposals(box, cls, cfg):
    """The composition a caller had before: per frame, on the device ops that were there."""
    B = int(box.shape[0])
    post = cfg["nms_post_maxsize"]
    rois, scores = box.new_zeros((B, post, 7)), box.new_zeros((B, post))
    labels = torch.zeros((B, post), dtype=torch.int64, device=box.device)
    for b in range(B):
        s, l = cls[b].max(dim=1)
        order = sort.stable_argsort(s, descending=True)[:cfg["nms_pre_maxsize"]]
        bx = box[b][order].contiguous()
        keep, num = iou3d_nms.nms_gpu_device(bx, cfg["nms_thresh"])
        sel = order[keep[:int(num)].long()[:post]]  # the host read of the count
        n = int(sel.shape[0])
        rois[b, :n], scores[b, :n], labels[b, :n] = box[b][sel], s[sel], l[sel]
    return rois, scores, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "prof_roi_head.py measures on the GPU only"
    torch.manual_seed(0)
    rows = []
    for batch in (2, 4):
        feats, rois = scene(batch)
        head_f = rh.voxel_rcnn_head_kitti_car(fused_pool=True).to(DEV).eval()
        head_u = rh.voxel_rcnn_head_kitti_car(fused_pool=False).to(DEV).eval()
        head_u.load_state_dict(head_f.state_dict())
        strides = [SCALES[n][0] for n in SCALES]
        with torch.no_grad():
            grid_xyz, coords = roi_head.roi_grid_points(rois, 6, RANGE, VOXEL, strides)
            M = int(grid_xyz.shape[0])
            qcnt = torch.full((batch,), M // batch, dtype=torch.int32, device=DEV)
            for k, name in enumerate(SCALES):
                sp = feats[name]
                stride, grid, _, _ = SCALES[name]
                size = torch.tensor([v * stride for v in VOXEL], device=DEV)
                xyz = (sp.indices[:, 1:4].flip(1).float() + 0.5) * size + torch.tensor(RANGE[:3], device=DEV)
                cnt = torch.bincount(sp.indices[:, 0].long(), minlength=batch).int()
                v2p = generate_voxel2pinds([batch, *grid, 32], sp.indices)
                layer = head_f.roi_grid_pool_layers[k]
                args = (xyz, cnt, grid_xyz, qcnt, coords[k], sp.features, v2p)

                def run(fused, layer=layer, args=args):
                    layer.fused = fused
                    return layer(*args)

                diff = float((run(True) - run(False)).abs().max())
                (tf, sf), (tu, su) = pair(lambda: run(True), lambda: run(False), a.iters, a.repeats)
                layer.fused = True
                g = layer.groupers[0]
                co = torch.cat([coords[k][:, :1], coords[k][:, 1:].flip(1)], 1).contiguous()
                q = pointnet2_ops.voxel_query_wrapper(grid_xyz, xyz, co, v2p, g.radius, g.nsample, *g.max_range)
                hit = q[:, 0] >= 0
                hits = int(((q != q[:, :1]).sum(1)[hit] + 1).sum())  # distinct slots of the rows with a hit
                need = pool_bytes(M, hits, 9 ** 3)
                rows.append(dict(what=f"pool {name}", B=batch, fused_us=tf, fused_spread=sf, unfused_us=tu,
                                 unfused_spread=su, max_abs_diff=diff, rows_with_hit=float(hit.float().mean()),
                                 needed_MB=need / 1e6, share_of_hbm_peak=need / (tf * 1e-6) / HBM_PEAK,
                                 unfused_tensors_MB=M * 16 * (32 + 3 + 1) * 4 / 1e6))
            box, cls = proposals(batch)

            def bd():
                return {"batch_size": batch, "batch_box_preds": box, "batch_cls_preds": cls,
                        "multi_scale_3d_features": feats, "multi_scale_3d_strides": {n: SCALES[n][0] for n in SCALES}}

            (tf, sf), (tu, su) = pair(lambda: head_f(bd()), lambda: head_u(bd()), a.iters, a.repeats)
            rows.append(dict(what="head forward", B=batch, fused_us=tf, fused_spread=sf, unfused_us=tu, unfused_spread=su))
            cfg = rh.KITTI_CAR_MODEL_CFG["nms_config"]["test"]
            one = roi_head.class_agnostic_nms(box, cls, cfg)
            ref = per_frame_proposals(box, cls, cfg)
            assert torch.equal(one[0], ref[0]) and torch.equal(one[2], ref[2])
            (tf, sf), (tu, su) = pair(lambda: roi_head.class_agnostic_nms(box, cls, cfg),
                                      lambda: per_frame_proposals(box, cls, cfg), a.iters, a.repeats)
            rows.append(dict(what="proposal nms", B=batch, fused_us=tf, fused_spread=sf, unfused_us=tu, unfused_spread=su))
    print(f"{'what':<16}{'B':>3}{'new us':>10}{'spread':>8}{'old us':>10}{'spread':>8}{'old/new':>8}  notes")
    for r in rows:
        note = ""
        if "needed_MB" in r:
            note = (f"needed {r['needed_MB']:.1f} MB = {100 * r['share_of_hbm_peak']:.2f} % of HBM peak; unfused tensors "
                    f"{r['unfused_tensors_MB']:.0f} MB; rows with a hit {100 * r['rows_with_hit']:.0f} %; "
                    f"max |fused - unfused| {r['max_abs_diff']:.2e}")
        print(f"{r['what']:<16}{r['B']:>3}{r['fused_us']:>10.1f}{r['fused_spread']:>8.1f}{r['unfused_us']:>10.1f}"
              f"{r['unfused_spread']:>8.1f}{r['unfused_us'] / r['fused_us']:>8.2f}  {note}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
