"""Time the pointnet2 batch ops and points_in_boxes (paddle3d_amd/ops/pointnet2_ops.py, roiaware_pool3d.py,
csrc/pointnet2.hip) at IA-SSD's shapes against the torch composition a user would otherwise write on the GPU:

  fps        KITTI B = 8, 16384 -> 4096 and 4096 -> 1024; Waymo B = 1, 65536 -> 16384.  Torch: the loop of
             torch.minimum / argmax / index (no host synchronisation).  Reported as ns per iteration next to the
             design's floor: per-lane VALU work (N points x ~15 VALU ops over 64 lanes per clock per CU), the wave
             reduction (6 __shfl_xor steps on a 64-bit key) and one barrier.
  group      ball query + grouping at the SA-layer shapes (KITTI layer 1: 16384 points, 4096 centres, r 0.2 / 0.8,
             nsample 16 / 32, C = 1 + 3).  Torch: cdist-free distance matrix, topk of the hit mask, gather.  Grouping
             reported as a fraction of 8 TB/s (idx read, out written, points read once).
  boxes      points_in_boxes at 16384 points x 64 boxes.  Torch: a vectorised test and argmax.

Device time per call from CUDA events over `--iters` calls after a warm-up.

    python tools/prof/prof_pointnet2.py [--iters 5] [--only fps group boxes]
Run under `rocprofv3 --kernel-trace --stats -- python ...` (with `--iters 1`) for kernel times."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddle3d_amd.ops import pointnet2_ops as P  # noqa: E402
from paddle3d_amd.ops import roiaware_pool3d as R  # noqa: E402

HBM = 8.0e12
CLOCK = 2.4e9
FPS_OPS_PER_POINT = 15  # 3 sub, 3 mul, 2 add, min, compare, 5 selects


def _time(fn, iters, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def _cloud(b, n, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    lo = torch.tensor([0.0, -40.0, -3.0], device="cuda")
    hi = torch.tensor([70.4, 40.0, 1.0], device="cuda")
    return lo + torch.rand((b, n, 3), device="cuda", generator=g) * (hi - lo)


def torch_fps(xyz, m):
    B, N, _ = xyz.shape
    temp = torch.full((B, N), 1e10, device=xyz.device)
    idx = torch.zeros((B, m), dtype=torch.int64, device=xyz.device)
    cur = torch.zeros((B,), dtype=torch.int64, device=xyz.device)
    ar = torch.arange(B, device=xyz.device)
    for j in range(1, m):
        c = xyz[ar, cur]
        d = ((xyz - c[:, None]) ** 2).sum(-1)
        temp = torch.minimum(temp, d)
        cur = temp.argmax(-1)
        idx[:, j] = cur
    return idx


def torch_ball_group(new_xyz, xyz, feats, r, s):
    d2 = ((new_xyz[:, :, None] - xyz[:, None]) ** 2).sum(-1)
    N = xyz.shape[1]
    key = torch.where(d2 < r * r, torch.arange(N, device=xyz.device), N)
    idx = key.topk(s, dim=-1, largest=False, sorted=True).values
    idx = torch.where(idx == N, idx[..., :1], idx)
    B, C = feats.shape[:2]
    g = torch.gather(feats, 2, idx.reshape(B, 1, -1).expand(B, C, -1))
    return g.reshape(B, C, idx.shape[1], s)


def torch_boxes(pts, boxes):
    c, s = torch.cos(-boxes[..., 6]), torch.sin(-boxes[..., 6])
    sx = pts[:, :, None, 0] - boxes[:, None, :, 0]
    sy = pts[:, :, None, 1] - boxes[:, None, :, 1]
    lx = sx * c[:, None] - sy * s[:, None]
    ly = sx * s[:, None] + sy * c[:, None]
    inside = ((pts[:, :, None, 2] - boxes[:, None, :, 2]).abs() <= boxes[:, None, :, 5] / 2) & \
        (lx.abs() < boxes[:, None, :, 3] / 2 + 1e-5) & (ly.abs() < boxes[:, None, :, 4] / 2 + 1e-5)
    return torch.where(inside.any(-1), inside.int().argmax(-1), -1)


def fps(iters):
    for name, B, N, M in (("kitti 16384->4096", 8, 16384, 4096), ("kitti 4096->1024", 8, 4096, 1024),
                          ("waymo 65536->16384", 1, 65536, 16384)):
        xyz = _cloud(B, N)
        per = -(-N // 1024)
        valu = N * FPS_OPS_PER_POINT / 64  # cycles of one CU's VALU per iteration
        t_tiers = {}
        for tier in ((1, 2) if N <= 16384 else (2,)):
            t_tiers[tier] = _time(lambda: P.farthest_point_sample(xyz, M, tier=tier), iters)
        t_torch = _time(lambda: torch_fps(xyz, M), 1, warm=0 if N > 16384 else 1)
        same = torch.equal(P.farthest_point_sample(xyz, M).long(), torch_fps(xyz, M)) if N <= 4096 else None
        line = "  ".join(f"tier {k} {v / 1e3:9.2f} ms = {v * 1e3 / (M - 1):7.1f} ns/iter" for k, v in t_tiers.items())
        print(f"fps {name} (B {B}, {per} points per lane): {line}   torch {t_torch / 1e3:9.2f} ms = "
              f"{t_torch * 1e3 / (M - 1):8.1f} ns/iter   VALU floor {valu:.0f} cycles = {valu / CLOCK * 1e9:.0f} ns/iter"
              + ("" if same is None else f"   same as torch: {same}"))


def group(iters):
    B, N, M, C = 8, 16384, 4096, 4
    xyz = _cloud(B, N, 1) / 20
    feats = torch.randn(B, C, N, device="cuda")
    new_xyz = xyz[:, :M].contiguous()
    for r, s in ((0.2, 16), (0.8, 32)):
        idx = P.ball_query_batch(new_xyz, xyz, r, s)
        t_bq = _time(lambda: P.ball_query_batch(new_xyz, xyz, r, s), iters)
        t_g = _time(lambda: P.grouping_operation_batch(feats, idx), iters)
        t_torch = _time(lambda: torch_ball_group(new_xyz, xyz, feats, r, s), iters)
        ok = torch.equal(P.grouping_operation_batch(feats, idx), torch_ball_group(new_xyz, xyz, feats, r, s))
        nbytes = B * M * s * 4 + B * C * M * s * 4 + B * C * N * 4
        print(f"ball query + group r {r} nsample {s} (B {B}, N {N}, {M} centres, C {C}): ball query {t_bq:8.1f} us, "
              f"group {t_g:7.1f} us ({nbytes / 1e6:.1f} MB = {nbytes / (t_g * 1e-6) / HBM:.3f} of 8 TB/s), "
              f"sum {t_bq + t_g:8.1f} us   torch {t_torch:9.1f} us   same: {ok}")


def boxes(iters):
    pts = _cloud(1, 16384, 2)
    bx = torch.cat([_cloud(1, 64, 3), torch.rand(1, 64, 3, device="cuda") * 4 + 1,
                    torch.rand(1, 64, 1, device="cuda") * 6 - 3], -1)
    t = _time(lambda: R.points_in_boxes_gpu(pts, bx), iters)
    t_torch = _time(lambda: torch_boxes(pts, bx), iters)
    print(f"points_in_boxes 16384 points x 64 boxes: {t:7.1f} us   torch {t_torch:7.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", nargs="+", default=["fps", "group", "boxes"])
    a = ap.parse_args()
    for name in a.only:
        {"fps": fps, "group": group, "boxes": boxes}[name](a.iters)


if __name__ == "__main__":
    main()
