"""Time SqueezeSegV3's pieces (csrc/squeezeseg.hip, paddle3d_amd/squeezesegv3.py) at the reference's shapes: N = 1, a
64 x 1024 range image, SAC stages (C, H, W) = (32, 64, 1024), (64, 64, 512), (128, 64, 256), (256, 64, 128).

  1. the SAC block up to its 1x1 layer on three paths over the same inputs:
       kernel     ops.squeezeseg.sac_isk_forward (one launch, no [N, 9C, H, W] tensor)
       torch      squeezesegv3.sac_isk_composition: unfold, conv7x7, sigmoid, product, conv1x1 with the folded BatchNorms --
                  the three 9C tensors formed (what fused=False runs)
     with the flop floor 2 * 9C * (147 + C) * HW, the fraction of the fp32 matrix peak the kernel reaches and the bytes it
     has to move (xyz, feature, the weights once, Y) against the three 75.5 MB tensors it does not form;
  2. the 3x3 stride-1 layer (C -> C, BatchNorm folded, relu) at the same shapes on every kernel of ops/conv.py whose
     predicate takes it, against torch;
  3. the whole SACRangeNet21 and SACRangeNet53 + head forward, fused and unfused, and pd3_range_project on a
     120 000-point scan.

Reported in us as the median of `--repeats` windows of `--iters` calls with the smallest and largest window; the paths
alternate inside each repeat, after a warm-up of each.  A window is a host clock around calls that end in a device
synchronise.

    python tools/prof/squeezeseg.py [--iters 20] [--repeats 5] [--only block|conv|net]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddle3d_amd import squeezesegv3 as sq  # noqa: E402
from paddle3d_amd.ops import squeezeseg as ops  # noqa: E402

STAGES = ((32, 64, 1024), (64, 64, 512), (128, 64, 256), (256, 64, 128))
PEAK_TFLOPS = 157.0  # fp32 matrix pipe


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def measure(fns, iters, repeats):
    """{name: (median, min, max)} us per call; the paths alternate inside each repeat, after a warm-up of each."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    rows = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            rows[k].append(window(fn, iters))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in rows.items()}


def show(title, res, base):
    for k, (med, lo, hi) in res.items():
        print(f"  {title:30s} {k:10s} {med:10.1f} us  [{lo:.1f} .. {hi:.1f}]  {base} / this = {res[base][0] / med:5.2f}",
              flush=True)


def randomise(module, seed):
    """Seeded non-trivial BatchNorm statistics (the constructors leave mean 0, variance 1)."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=gen) * 1.5 + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=gen) * 0.1)
    return module


def blocks(a, dev, gen):
    for C, H, W in STAGES:
        torch.manual_seed(C)
        blk = randomise(sq.SACISKBlock(C, fused="force"), C).to(dev).eval()
        f = blk._params()
        xyz = torch.randn(1, 3, H, W, device=dev, generator=gen)
        feat = torch.randn(1, C, H, W, device=dev, generator=gen)
        fns = {"kernel": lambda: ops.sac_isk_forward(xyz, feat, f["w1p"], f["s_a"], f["t_a"], f["w2p"], f["s_m"], f["t_m"]),
               "torch": lambda: sq.sac_isk_composition(xyz, feat, f["w"], f["s_a"], f["t_a"], f["v"], f["s_m"], f["t_m"])}
        got, want = fns["kernel"](), fns["torch"]()
        print(f"C = {C}, {H} x {W}: max |kernel - torch| = {float((got - want).abs().max()):.3g} (|max| "
              f"{float(want.abs().max()):.3g})")
        res = measure(fns, a.iters, a.repeats)
        show(f"SAC block to the 1x1, C = {C}", res, "torch")
        flop = 2 * 9 * C * (147 + C) * H * W
        moved = (3 + 2 * C) * H * W * 4 + (9 * C * 148 + 9 * C * C + 20 * C) * 4
        print(f"  derived: floor {flop / 1e9:.1f} Gflop = {flop / PEAK_TFLOPS / 1e6:.0f} us at {PEAK_TFLOPS:.0f} Tflop/s; the "
              f"kernel reaches {flop / res['kernel'][0] / 1e6:.1f} Tflop/s ({100 * flop / res['kernel'][0] / 1e6 / PEAK_TFLOPS:.0f} %); "
              f"it must move {moved / 1e6:.1f} MB; each of U, A, P it does not form is {9 * C * H * W * 4 / 1e6:.1f} MB",
              flush=True)


def convs(a, dev, gen):
    for C, H, W in STAGES:
        torch.manual_seed(C)
        layer = randomise(sq.ConvBNLayer(C, C, 3, padding=1), C).to(dev).eval()
        x = torch.randn(1, C, H, W, device=dev, generator=gen)
        fns = {}
        for name in ("torch", "direct", "winograd", "winograd43"):
            if name == "torch" or sq.conv3x3_kernel_for(name, C, C, H, W, dev) == name:
                fns[name] = lambda name=name: sq.conv3x3_bn_act(layer, x, "relu", name)
        want = fns["torch"]()
        for name, fn in fns.items():
            print(f"C = {C}: max |{name} - torch| = {float((fn() - want).abs().max()):.3g} (|max| {float(want.abs().max()):.3g})")
        show(f"conv3x3 + BN + relu, C = {C}", measure(fns, a.iters, a.repeats), "torch")


def nets(a, dev, gen):
    image = torch.randn(1, 5, 64, 1024, device=dev, generator=gen)
    for layers in (21, 53):
        models = {}
        for name, fused in (("fused", "force"), ("default", True), ("unfused", False)):
            torch.manual_seed(layers)
            models[name] = randomise(sq.SqueezeSegV3(sq.SACRangeNet(5, layers, fused=fused)), layers).to(dev).eval()
        lg = {k: m.logits(image) for k, m in models.items()}
        same = float((lg["fused"].argmax(1) == lg["unfused"].argmax(1)).float().mean())
        print(f"SACRangeNet{layers}: max |fused - unfused| logits = {float((lg['fused'] - lg['unfused']).abs().max()):.3g} "
              f"(|max| {float(lg['unfused'].abs().max()):.3g}), same argmax on {100 * same:.3f} % of the pixels")
        fns = {k: (lambda m=m: m.export_forward(image)) for k, m in models.items()}
        show(f"SACRangeNet{layers} + head, 64 x 1024", measure(fns, max(1, a.iters // 4), a.repeats), "unfused")
    n = 120000
    r = torch.rand(n, device=dev, generator=gen) * 58 + 2
    yaw = (torch.rand(n, device=dev, generator=gen) * 2 - 1) * np.pi
    pitch = torch.deg2rad(torch.rand(n, device=dev, generator=gen) * 28 - 25)
    pts = torch.stack([r * pitch.cos() * yaw.cos(), r * pitch.cos() * yaw.sin(), r * pitch.sin(),
                       torch.rand(n, device=dev, generator=gen)], 1).contiguous()
    off = torch.tensor([0, n], dtype=torch.int32, device=dev)
    res = measure({"kernel": lambda: ops.range_project(pts, off)}, a.iters, a.repeats)
    show("range_project, 120k points", res, "kernel")
    print(f"  pixels taken: {int((ops.range_project(pts, off)[1] >= 0).sum())} of {64 * 1024}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=("block", "conv", "net"), default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("squeezeseg: needs the GPU (a CPU run says nothing about these times)")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(dev).manual_seed(1)
    with torch.no_grad():
        for name, fn in (("block", blocks), ("conv", convs), ("net", nets)):
            if a.only in (None, name):
                fn(a, dev, gen)


if __name__ == "__main__":
    main()
