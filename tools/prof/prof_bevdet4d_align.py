"""Time BEVDet4D's temporal alignment (paddle3d_amd/bevdet4d.align_concat: 8 adjacent frames warped into the current
ego frame and concatenated behind it, 9 x 80 x 128 x 128 per batch element) against the composed torch path the
reference's data flow needs (4x4 poses, torch.linalg.inv, 8 grid_sample launches, cat).

Device time per call from CUDA events over `--iters` back-to-back calls, no synchronisation inside, two ways:
  warm  the same inputs and output every call (at B = 1 the ~94 MB working set stays in the 256 MiB Infinity Cache)
  cold  calls rotate over enough input sets that more than 256 MiB of inputs lies between two uses of one set
Bytes moved per batch element: 8 adjacent maps read + the current map read + 9 maps written (80 x 128 x 128 fp32
each), reported against the 8 TB/s HBM peak.

    python tools/prof/prof_bevdet4d_align.py [--batch 1 8] [--iters 50]
Run under `rocprofv3 --kernel-trace --stats -- python ...` (with `--iters` small) for the launch count."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import bevdet4d_align_numpy as ba  # noqa: E402

from paddle3d_amd import bevdet4d  # noqa: E402

C, H, W, NADJ = 80, 128, 128, 8
PEAK = 8.0e12


def torch_align(feats, rots, trans, bda, interval=(0.8, 0.8), lower=(-51.2, -51.2)):
    """The reference's shift_feature + concat in torch (bevdet4d.py:90-159, :291-298)."""
    n = feats[0].shape[0]
    dev = feats[0].device
    xs = torch.linspace(0, W - 1, W, device=dev).reshape(1, W).expand(H, W)
    ys = torch.linspace(0, H - 1, H, device=dev).reshape(H, 1).expand(H, W)
    grid = torch.stack((xs, ys, torch.ones_like(xs)), -1).reshape(1, H, W, 3, 1)
    bda4 = torch.zeros(n, 4, 4, device=dev)
    bda4[:, :3, :3] = bda
    bda4[:, 3, 3] = 1
    f2b = torch.zeros(3, 3, device=dev)
    f2b[0, 0], f2b[1, 1], f2b[0, 2], f2b[1, 2], f2b[2, 2] = interval[0], interval[1], lower[0], lower[1], 1
    inv_f2b = torch.linalg.inv(f2b)
    norm = torch.tensor([W - 1.0, H - 1.0], device=dev)
    c0 = torch.zeros(n, 4, 4, device=dev)
    c0[:, :3, :3], c0[:, :3, 3], c0[:, 3, 3] = rots[0][:, 0], trans[0][:, 0], 1
    c0 = bda4 @ c0
    out = [feats[0]]
    idx = torch.tensor([0, 1, 3], device=dev)
    for k in range(1, len(feats)):
        c1 = torch.zeros(n, 4, 4, device=dev)
        c1[:, :3, :3], c1[:, :3, 3], c1[:, 3, 3] = rots[k][:, 0], trans[k][:, 0], 1
        l = (c0 @ torch.linalg.inv(bda4 @ c1)).index_select(1, idx).index_select(2, idx)
        tf = (inv_f2b @ l @ f2b).reshape(n, 1, 1, 3, 3)
        g = (tf @ grid)[..., :2, 0] / norm * 2.0 - 1.0
        out.append(torch.nn.functional.grid_sample(feats[k], g, align_corners=True))
    return torch.cat(out, 1)


def _sets(B, count, seed):
    rng = np.random.default_rng(seed)
    rots, trans = ba.poses(rng, B, NADJ)
    rd = [torch.from_numpy(r).cuda() for r in rots]
    td = [torch.from_numpy(t).cuda() for t in trans]
    bd = torch.from_numpy(np.broadcast_to(ba.bda_matrix(rot_deg=5.0), (B, 3, 3)).copy()).cuda()
    sets = []
    for _ in range(count):
        feats = [torch.rand(B, C, H, W, device="cuda") * 2 - 1 for _ in range(NADJ + 1)]
        sets.append(feats)
    return sets, rd, td, bd


def _time(fn, n_sets, iters):
    for i in range(max(3, n_sets)):
        fn(i % n_sets)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i % n_sets)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    for B in a.batch:
        per_set = (NADJ + 1) * B * C * H * W * 4 * 2  # inputs + output
        n_cold = max(2, -(-(512 << 20) // per_set) + 1)
        sets, rd, td, bd = _sets(B, n_cold, 17 + B)
        hip = lambda i: bevdet4d.align_concat(sets[i], rd, td, bd)  # noqa: E731
        ref = lambda i: torch_align(sets[i], rd, td, bd)  # noqa: E731
        diff = float((hip(0) - ref(0)).abs().max())
        moved = (NADJ * B * C * H * W + B * C * H * W + (NADJ + 1) * B * C * H * W) * 4
        for name, fn in (("hip", hip), ("torch", ref)):
            for mode, n_sets in (("warm", 1), ("cold", n_cold)):
                ms = _time(fn, n_sets, a.iters)
                print(f"B={B} {name:5s} {mode}: {ms * 1e3:8.1f} us per call, {moved / 1e6:.0f} MB moved, "
                      f"{moved / (ms * 1e-3) / 1e12:.2f} TB/s = {moved / (ms * 1e-3) / PEAK:.2f} of 8 TB/s"
                      + (f" ({n_sets} rotating sets, {n_sets * per_set / 2**20:.0f} MiB)" if n_sets > 1 else ""))
        print(f"B={B} max |hip - torch| = {diff:.3g}")
        del sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
