"""Time CaDDN's frustum-to-voxel and map-to-BEV stage (paddle3d_amd/ops/caddn.py, csrc/caddn.hip) at the KITTI shape of
configs/caddn/*.yml (375 x 1242 image, 94 x 311 feature map, C = 64, LID with 80 bins, a 280 x 376 x 25 grid, 1600 -> 64
map_to_bev), B = 1 and B = 2:

  fused      frustum_to_bev: pack, weight repack and the MFMA kernel; no voxel volume
  voxel+conv frustum_to_voxel and a torch 1x1 convolution with the folded BatchNorm and ReLU
  torch      the composition a user would otherwise write on the same GPU: softmax (x) features as [B, 64, 80, h, w],
             F.grid_sample on the grid of frustum_grid, the transpose, the 1x1 convolution

Device time per call from CUDA events over `--iters` back-to-back calls, no synchronisation inside.  Next to the times:
each path's compulsory HBM bytes (every tensor the path has to read or write once, intermediates included) and the
corner bytes the fused kernel gathers (4 feature rows of C floats and 8 probabilities per voxel, plus the repacked
weight once per 64-column tile) against the 7 TB/s L2 -> CU figure of DESIGN.md.

    python tools/prof/prof_caddn_f2v.py [--iters 20] [--batches 1 2]
Run under `rocprofv3 --kernel-trace --stats -- python ...` (with `--iters` small) for kernel times and launches."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddle3d_amd.ops import caddn  # noqa: E402

PC_RANGE, VOXEL = [2, -30.08, -3.0, 46.8, 30.08, 1.0], [0.16, 0.16, 0.16]
DISC = {"mode": "LID", "num_bins": 80, "depth_min": 2.0, "depth_max": 46.8}
GRID = (280, 376, 25)
IMAGE, FEAT, C, C_OUT = (375, 1242), (94, 311), 64, 64
HBM, GATHER = 8.0e12, 7.0e12


def _time(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def kitti_calib(B):
    """KITTI's Tr_velo_to_cam (rectified) and P2, the same for every frame."""
    l2c = np.array([[0.0002, -0.9999, -0.0106, 0.0594], [0.0104, 0.0106, -0.9999, -0.0751],
                    [0.9999, 0.0001, 0.0105, -0.2721], [0, 0, 0, 1]], np.float32)
    c2i = np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]],
                   np.float32)
    return np.repeat(l2c[None], B, 0), np.repeat(c2i[None], B, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 2])
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    X, Y, Z = GRID
    h, w = FEAT
    D = DISC["num_bins"]
    for B in a.batches:
        g = torch.Generator(device="cpu").manual_seed(B)
        feats = torch.randn((B, C, h, w), generator=g).to(dev)
        logits = (1.5 * torch.randn((B, D + 1, h, w), generator=g)).to(dev)
        l2c, c2i = (torch.from_numpy(x).to(dev) for x in kitti_calib(B))
        shape = torch.tensor([IMAGE] * B, dtype=torch.int32, device=dev)
        weight = (torch.randn((C_OUT, C * Z), generator=g) / 40).to(dev)
        scale, shift = torch.rand(C_OUT, generator=g).to(dev) + 0.5, (0.1 * torch.randn(C_OUT, generator=g)).to(dev)
        geo = (l2c, c2i, shape, GRID, PC_RANGE[:3], VOXEL, DISC)

        def conv(voxel):
            return torch.relu(F.conv2d(voxel.flatten(1, 2), weight[:, :, None, None]) * scale[None, :, None, None]
                              + shift[None, :, None, None])

        def fused():
            return caddn.frustum_to_bev(feats, logits, *geo, weight, scale, shift)

        def voxel_conv():
            return conv(caddn.frustum_to_voxel(feats, logits, *geo))

        def torch_path():
            frustum = torch.softmax(logits.unsqueeze(1), 2)[:, :, :-1] * feats.unsqueeze(2)
            grid = caddn.frustum_grid(*geo[:3], *geo[3:])
            return conv(F.grid_sample(frustum, grid, mode="bilinear", padding_mode="zeros",
                                      align_corners=False).permute(0, 1, 4, 3, 2))

        ref = torch_path()
        d_fused, d_vc = float((fused() - ref).abs().max()), float((voxel_conv() - ref).abs().max())
        share = float((caddn.frustum_to_voxel(feats, logits, *geo).abs().amax(1) > 0).float().mean())
        del ref
        torch.cuda.empty_cache()
        maps = B * h * w * (C + D + 1) * 4
        packed = B * h * w * (C + D) * 4
        bev = B * C_OUT * Y * X * 4
        voxel = B * C * Z * Y * X * 4
        frustum = B * C * D * h * w * 4
        grid = B * X * Y * Z * 3 * 4
        wbytes = C_OUT * C * Z * 4
        hbm = {"fused": maps + 2 * packed + 3 * wbytes + bev,
               "voxel+conv": maps + 2 * packed + 2 * voxel + wbytes + bev,
               "torch": maps + B * h * w * (D + 1) * 4 * 2 + 2 * frustum + 2 * grid + 2 * 2 * voxel + wbytes + bev}
        corner = B * X * Y * Z * (4 * C + 8) * 4 + B * ((X * Y + 63) // 64) * wbytes
        t = {k: _time(f, a.iters) for k, f in (("fused", fused), ("voxel+conv", voxel_conv), ("torch", torch_path))}
        print(f"B = {B}: features [{B}, {C}, {h}, {w}], {D} bins, grid {GRID}, {C * Z} -> {C_OUT}; share of voxels with a "
              f"sample {share:.2f}; max |fused - torch| = {d_fused:.3g}, |voxel+conv - torch| = {d_vc:.3g}")
        for k in ("fused", "voxel+conv", "torch"):
            s = t[k] * 1e-6
            print(f"  {k:<11}{t[k]:10.1f} us   HBM {hbm[k] / 1e6:8.1f} MB = {hbm[k] / s / 1e12:5.2f} TB/s "
                  f"({hbm[k] / s / HBM:.3f} of 8)")
        s = t["fused"] * 1e-6
        print(f"  fused gathers {corner / 1e6:.1f} MB of corner rows and weight fragments = {corner / s / 1e12:.2f} TB/s "
              f"({corner / s / GATHER:.3f} of 7); MFMA {2.0 * B * X * Y * C * Z * C_OUT / s / 1e12:.1f} TFLOP/s fp32")
        print(f"  torch / fused = {t['torch'] / t['fused']:.1f}, voxel+conv / fused = {t['voxel+conv'] / t['fused']:.1f}")
        del feats, logits
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
