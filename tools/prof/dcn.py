"""Time the modulated deformable convolution (csrc/deform_conv.hip, paddle3d_amd/mm_resnet.py) at the shapes of the two
CAPE ResNet-50 configs' DCN stages --

    cape_r50_1408x512   stage 3: 6 cameras,  256 channels, 32 x 88     stage 4: 6 cameras,  512 channels, 16 x 44
    capet_r50_704x256   stage 3: 12 cameras, 256 channels, 16 x 44     stage 4: 12 cameras, 512 channels, 8 x 22

-- one DeformableConvV2 as the bottleneck runs it (conv_offset, the DCN, norm2 folded, relu) in its three forms on the same
commit: fused=False (the torch composition: the yardstick), fused=True (the default) and fused="force" (the kernel); and
the op alone (pd3_deform_conv2d_forward against deform_conv2d_composition on the same offsets and mask).  With --stages
also the whole DCN stages (ResLayer of 6 and of 3 bottlenecks) in the three forms, with --sweep the layer at smaller
feature maps, where the border of ops.deform_conv.DCN_FUSED_MIN_PIXELS is looked for.

Reported in us as the median of `--repeats` windows of `--iters` calls with the smallest and largest window; the forms
alternate inside each repeat, after a warm-up of each.  A window is a host clock around calls that end in a device
synchronise.  Also printed: the largest difference between the forms' results, the kernel's FLOP count (2 * pixels * 9
Cin * Cout) and the fraction of the fp32 matrix peak (155 TFLOP/s measured, MI355X_MICROARCH.md) the op-alone time is.

    python tools/prof/dcn.py [--iters 20] [--repeats 5] [--stages] [--sweep] [--json FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddle3d_amd import mm_resnet as MR  # noqa: E402
from paddle3d_amd.ops import deform_conv as ops  # noqa: E402

PEAK = 155e12
SHAPES = {"cape_stage3": (6, 256, 32, 88), "cape_stage4": (6, 512, 16, 44), "capet_stage3": (12, 256, 16, 44),
          "capet_stage4": (12, 512, 8, 22)}
SWEEP = {"sweep_256_8x11": (1, 256, 8, 11), "sweep_256_16x22": (1, 256, 16, 22), "sweep_256_16x44": (2, 256, 16, 44),
         "sweep_512_4x11": (1, 512, 4, 11), "sweep_512_8x22": (2, 512, 8, 22), "sweep_64_32x88": (6, 64, 32, 88)}
STAGES = {"cape_stage3": (6, 512, 256, 6, 64, 176), "cape_stage4": (6, 1024, 512, 3, 32, 88),
          "capet_stage3": (12, 512, 256, 6, 32, 88), "capet_stage4": (12, 1024, 512, 3, 16, 44)}  # N, inplanes, planes, blocks, H, W


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


def randomise(module, gen):
    for name, p in module.named_parameters():
        if name.endswith("conv_offset.weight"):
            p.copy_(torch.randn(p.shape, device=p.device, generator=gen) * 0.02)
        elif p.dim() > 1:
            p.copy_(torch.randn(p.shape, device=p.device, generator=gen) / float(np.sqrt(p[0].numel())))
        else:
            p.copy_(torch.rand(p.shape, device=p.device, generator=gen) + 0.5)
    for name, b in module.named_buffers():
        if name.endswith("running_var"):
            b.copy_(torch.rand(b.shape, device=b.device, generator=gen) + 0.5)
        elif name.endswith("running_mean"):
            b.copy_(torch.randn(b.shape, device=b.device, generator=gen) * 0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--stages", action="store_true", help="also time the whole DCN stages 3 and 4")
    ap.add_argument("--sweep", action="store_true", help="also time smaller feature maps")
    ap.add_argument("--json", default=None, help="write the medians to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dcn: needs the GPU (a CPU run says nothing about these times)")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(dev).manual_seed(1)
    report = {}
    shapes = dict(SHAPES)
    if a.sweep:
        shapes.update(SWEEP)
    with torch.no_grad():
        for name, (N, ch, H, W) in shapes.items():
            x = torch.randn(N, ch, H, W, device=dev, generator=gen)
            norm = torch.nn.BatchNorm2d(ch).to(dev).eval()
            forms = {}
            for fused in (False, True, "force"):
                m = MR.DeformableConvV2(ch, ch, 3, padding=1, bias_attr=False, fused=fused).to(dev).eval()
                if forms:
                    m.load_state_dict(forms["False"].state_dict())
                else:
                    randomise(m, gen)
                    randomise(norm, gen)
                forms[str(fused)] = m
            om = forms["False"].conv_offset(x)
            offset, mask = om[:, :18], om[:, 18:]
            sig = torch.sigmoid(mask)
            w = forms["False"].conv_dcn.weight
            packed = ops.pack_deform_conv_weight(w)
            fns = {"op torch": lambda: MR.deform_conv2d_composition(x, offset, sig, w, None, 1, 1, 1),
                   "op kernel": lambda: ops.deform_conv2d_packed(x, offset, mask, packed, None, None, False, True, 1, 1, 1)}
            fns.update({f"layer {k}": (lambda m=m: m(x, norm, True)) for k, m in forms.items()})
            diff_op = float((fns["op torch"]() - fns["op kernel"]()).abs().max())
            diff_layer = float((fns["layer False"]() - fns["layer force"]()).abs().max())
            t = measure(fns, a.iters, a.repeats)
            pixels, flop = N * H * W, 2.0 * N * H * W * 9 * ch * ch
            frac = flop / (t["op kernel"][0] * 1e-6) / PEAK
            print(f"{name}: {N} x {ch} x {H} x {W}, {pixels} pixels, {flop / 1e9:.2f} GFLOP, form "
                  f"{ops.tiles_per_wave(pixels, ch)}, default takes the kernel: {forms['True'].takes_kernel(x)}; "
                  f"max |torch - kernel| op {diff_op:.3g} layer {diff_layer:.3g}")
            for k, (med, lo, hi) in t.items():
                base = t["op torch" if k.startswith("op") else "layer False"][0]
                print(f"  {k:12s} {med:10.1f} us  [{lo:.1f} .. {hi:.1f}]  torch / this = {base / med:5.2f}")
            print(f"  op kernel: {flop / (t['op kernel'][0] * 1e-6) / 1e12:.1f} TFLOP/s, {100 * frac:.1f} % of the fp32 matrix "
                  f"peak; its arithmetic floor is {flop / PEAK * 1e6:.1f} us")
            report[name] = dict(pixels=pixels, channels=ch, gflop=flop / 1e9, peak_fraction=frac,
                                **{k.replace(" ", "_") + "_us": v[0] for k, v in t.items()})
            del forms, fns, x, om
        if a.stages:
            for name, (N, inplanes, planes, blocks, H, W) in STAGES.items():
                x = torch.randn(N, inplanes, H, W, device=dev, generator=gen)
                forms = {}
                for fused in (False, True, "force"):
                    m = MR.ResLayer(MR.Bottleneck, inplanes, planes, blocks, stride=2, style="caffe",
                                    dcn=dict(type_name="DeformConv2D", deformable_groups=1), fused=fused).to(dev).eval()
                    if forms:
                        m.load_state_dict(forms["False"].state_dict())
                    else:
                        randomise(m, gen)
                    forms[str(fused)] = m
                fns = {k: (lambda m=m: m(x)) for k, m in forms.items()}
                ref = fns["False"]()
                t = measure(fns, max(1, a.iters // 4), a.repeats)
                print(f"{name}: whole stage, {blocks} bottlenecks on {N} x {inplanes} x {H} x {W}")
                for k, (med, lo, hi) in t.items():
                    d = float((fns[k]() - ref).abs().max())
                    print(f"  fused={k:5s} {med / 1e3:8.2f} ms  [{lo / 1e3:.2f} .. {hi / 1e3:.2f}]  unfused / this = "
                          f"{t['False'][0] / med:5.2f}  max |this - unfused| {d:.3g}")
                report[name]["stage_us"] = {k: v[0] for k, v in t.items()}
                del forms, fns, x, ref
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
