"""Time BEVFusion's Anchor3DHead at inference (csrc/anchor3d_head.hip, paddle3d_amd/bevfusion_head.py) at the shape of
configs/bevfusion/bevf_pp_2x8_1x_nusc.yaml: a 384 x 200 x 200 map, 14 anchors per cell, 10 classes, a 9-wide box code,
nms_pre = 1000, max_num = 500, B = 1 and 4, on three paths over the same inputs on the same commit:

  lazy       forward_get_bboxes(fused="force"): conv_cls densely (only the per-anchor maximum is written), conv_reg /
             conv_dir_cls / the class scores at the 1000 selected anchors, per-class NMS of the batch at once
  maps       forward (the three dense 1x1 convolutions through ops/conv.py) + get_bboxes (the from-maps kernels)
  torch      forward + the module's plain-torch transcription of the reference (fused=False): transposes, sigmoid,
             topk, sort, gathers, and per class nonzero / argsort / ops.iou3d_nms.nms_gpu with its host reads

Reported in us as the median of `--repeats` windows of `--iters` calls with the smallest and largest window; the paths
alternate inside each repeat, after a warm-up of each.  A window is a host clock around calls that end in a device
synchronise.  Also printed: the C-ABI calls of each path (tests/guarded.py's launch ledger), the agreement of the paths'
results, and what is derived from the shape rather than measured: the bytes each path moves through HBM for the head's
maps (the lazy path reads the feature map once and writes 4 * H * W * A bytes per frame; the other two also write and
read back the [B, 140 + 126 + 28, H, W] maps, and the torch path the [B, 140, H, W] score map and the transposes).

The conv_cls bias is init_bias_by_prob(0.01) as the reference initialises it and score_thr = 0.05, so that the candidate
sets have the size a trained head gives them (tens per class), not the thousand a symmetric random head would.

    python tools/prof/anchor3d_head.py [--iters 20] [--repeats 5]
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from paddle3d_amd import _lib  # noqa: E402
from paddle3d_amd import bevfusion_head as bh  # noqa: E402

SHAPE = dict(C=384, H=200, W=200, nc=10, cs=9)
SIZES = [[1.95017717, 4.60718145, 1.72270761], [2.4560939, 6.73778078, 2.73004906], [2.94046906, 11.1885991, 3.47030982],
         [0.60058911, 1.68452161, 1.27192197], [0.76279481, 2.09973778, 1.44403034], [0.66344886, 0.7256437, 1.75748069],
         [0.39694519, 0.40359262, 1.06232151]]
TEST_CFG = dict(nms_pre=1000, max_num=500, score_thr=0.05, nms_thr=0.2)


def make_head(device, seed=0):
    torch.manual_seed(seed)
    head = bh.Anchor3DHead(
        SHAPE["nc"], SHAPE["C"], SHAPE["C"],
        anchor_generator=dict(ranges=[[-50.0, -50.0, -1.8, 50.0, 50.0, -1.8]], sizes=SIZES, scales=[1], rotations=[0, 1.57],
                              custom_values=[0, 0]),
        bbox_coder=dict(code_size=SHAPE["cs"]), dir_offset=0.7854, dir_limit_offset=0, test_cfg=dict(TEST_CFG))
    with torch.no_grad():
        head.conv_cls.weight.normal_(0, 0.05)
        head.conv_cls.bias.fill_(-math.log((1 - 0.01) / 0.01))
        head.conv_reg.weight.normal_(0, 0.01)
        head.conv_reg.bias.zero_()
    return head.eval().to(device)


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def measure(fns, iters, repeats):
    for fn in fns.values():
        for _ in range(3):
            fn()
    rows = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            rows[k].append(window(fn, iters))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in rows.items()}


def ledger(fn):
    from guarded import launch_ledger

    symbols = _lib.symbols("test_memory_safety_gpu") + _lib.symbols("test_memory_safety_anchor3d_gpu")
    with launch_ledger(_lib.lib(), symbols) as calls:
        fn()
    return {k: v for k, v in calls.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("anchor3d_head: needs the GPU (a CPU run says nothing about these times)")
    dev = torch.device("cuda", 0)
    head = make_head(dev)
    C, H, W, nc, cs = (SHAPE[k] for k in ("C", "H", "W", "nc", "cs"))
    A = head.num_anchors
    gen = torch.Generator(dev).manual_seed(1)
    with torch.no_grad():
        for B in (1, 4):
            x = [torch.randn(B, C, H, W, device=dev, generator=gen)]
            metas = [{}] * B
            fns = {"lazy": lambda: head.forward_get_bboxes(x, metas, fused="force", return_padded=True),
                   "maps": lambda: head.get_bboxes(*head(x), metas, return_padded=True),
                   "torch": lambda: head.get_bboxes(*head(x), metas, fused=False, return_padded=True)}
            res = {k: fn() for k, fn in fns.items()}
            print(f"B = {B}: counts lazy {res['lazy'][3].tolist()} maps {res['maps'][3].tolist()} torch {res['torch'][3].tolist()}")
            for k in ("maps", "torch"):
                same = torch.equal(res[k][3], res["lazy"][3]) and torch.equal(res[k][2], res["lazy"][2])
                diff = float((res[k][0] - res["lazy"][0]).abs().max()) if same else float("nan")
                print(f"  {k} vs lazy: labels and counts equal {same}, max |box difference| {diff:.3g}")
            for k, fn in fns.items():
                print(f"  C-ABI calls, {k}: {ledger(fn)}")
            t = measure(fns, a.iters if B == 1 else max(1, a.iters // 2), a.repeats)
            for k, (med, lo, hi) in t.items():
                print(f"  B = {B} {k:6s} {med:10.1f} us  [{lo:.1f} .. {hi:.1f}]  maps / this = {t['maps'][0] / med:5.2f}")
            feat = B * C * H * W * 4
            maps = B * A * (nc + cs + 2) * H * W * 4
            print(f"  derived: feature map {feat / 1e6:.1f} MB; lazy reads it once and writes {B * H * W * A * 4 / 1e6:.2f} MB "
                  f"of maximum scores; the three maps are {maps / 1e6:.1f} MB, written and read once by `maps` "
                  f"({(3 * feat + 2 * maps) / 1e6:.1f} MB with three feature reads), and `torch` adds the score map and the "
                  f"transposed copies ({(3 * feat + 4 * maps + 3 * B * A * nc * H * W * 4) / 1e6:.1f} MB); "
                  f"conv_cls is {2 * A * nc * C * H * W * B / 1e9:.2f} Gflop, the three convolutions "
                  f"{2 * A * (nc + cs + 2) * C * H * W * B / 1e9:.2f} Gflop")


if __name__ == "__main__":
    main()
