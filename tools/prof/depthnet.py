"""Time BEVDepth's depth network (csrc/depthnet.hip, paddle3d_amd/bevdepth.py) at the shapes of
configs/bevdet/bevdet4d_r50_depth_nuscenes.yml -- 512 channels on 16 x 44 maps, 118 depth bins, 80 context channels; 54
maps (6 cameras x 9 frames) a sample and 6 maps for a single frame -- in its three forms on the same commit: fused=False
(the module's own torch composition: the yardstick), fused=True (the default) and fused="force" (the kernels):

    ASPP              the module alone (pd3_aspp_forward against five branches, a concatenation and conv1)
    tail              pd3_depth_softmax_split against softmax + permute(0, 2, 3, 1).contiguous()
    DepthNet          the whole network
    view transformer  LSSViewTransformerBEVDepth.forward with accelerate=True (the index sets prepared once)

Reported in us as the median of `--repeats` windows of `--iters` calls with the smallest and largest window; the forms
alternate inside each repeat, after a warm-up of each.  A window is a host clock around calls that end in a device
synchronise.  Also printed: the largest difference between the forms' results, and for the ASPP the multiply-adds the
kernels do (the in-range taps only, ops.depthnet.in_range_taps), what a dense dilated convolution does, and the fraction
of the fp32 matrix peak (157 TFLOP/s, MI355X_MICROARCH.md) the forced ASPP's time is of its own work.

    python tools/prof/depthnet.py [--iters 10] [--repeats 5] [--json FILE]
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

from paddle3d_amd import bevdepth as BD  # noqa: E402
from paddle3d_amd import synth  # noqa: E402
from paddle3d_amd.ops import depthnet as ops  # noqa: E402

PEAK = 157e12
CH, H, W, D, CTX = 512, 16, 44, 118, 80
MAPS = {"sample_54": (1, 54), "frame_6": (1, 6)}  # (B, N)
FORMS = (False, True, "force")


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
    for p in module.parameters():
        if p.dim() > 1:
            p.copy_(torch.randn(p.shape, device=p.device, generator=gen) / float(np.sqrt(p[0].numel())))
        else:
            p.copy_(torch.rand(p.shape, device=p.device, generator=gen) - 0.5)
    for name, b in module.named_buffers():
        if name.endswith("running_var"):
            b.copy_(torch.rand(b.shape, device=b.device, generator=gen) + 0.5)
        elif name.endswith("running_mean"):
            b.copy_(torch.randn(b.shape, device=b.device, generator=gen) * 0.1)
    for m in module.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            m.weight.copy_(torch.rand(m.weight.shape, device=m.weight.device, generator=gen) + 0.5)


def three_forms(make, dev, gen):
    forms = {}
    for fused in FORMS:
        m = make(fused).to(dev).eval()
        if forms:
            m.load_state_dict(forms["False"].state_dict())
        else:
            randomise(m, gen)
        forms[str(fused)] = m
    return forms


def show(title, t, diff, extra=""):
    print(f"{title}: max |unfused - force| {diff:.3g}{extra}")
    for k, (med, lo, hi) in t.items():
        print(f"  fused={k:5s} {med:10.1f} us  [{lo:.1f} .. {hi:.1f}]  unfused / this = {t['False'][0] / med:5.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None, help="write the medians to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("depthnet: needs the GPU (a CPU run says nothing about these times)")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(dev).manual_seed(1)
    report = {}
    taps = ops.in_range_taps(H, W)
    with torch.no_grad():
        for name, (B, N) in MAPS.items():
            n = B * N
            rep = report.setdefault(name, dict(maps=n))
            x = torch.randn(n, CH, H, W, device=dev, generator=gen)
            # ---- ASPP ----
            forms = three_forms(lambda f: BD.ASPP(CH, CH, fused=f), dev, gen)
            fns = {k: (lambda m=m: m(x)) for k, m in forms.items()}
            diff = float((fns["False"]() - fns["force"]()).abs().max())
            t = measure(fns, a.iters, a.repeats)
            useful = 2.0 * n * CH * CH * (sum(taps) + 4 * H * W)  # the branches' in-range taps and the 4 Cmid projection
            dense = 2.0 * n * CH * CH * H * W * (28 + 5)
            frac = useful / (t["force"][0] * 1e-6) / PEAK
            show(f"{name} ASPP {n} x {CH} x {H} x {W}", t, diff,
                 f"; kernels {useful / 1e9:.1f} GFLOP, dense composition {dense / 1e9:.1f} GFLOP, default takes the kernel: "
                 f"{forms['True'].takes_kernel(x)}")
            print(f"  forced: {useful / (t['force'][0] * 1e-6) / 1e12:.1f} TFLOP/s of its own work, {100 * frac:.1f} % of the "
                  f"fp32 matrix peak; its arithmetic floor is {useful / PEAK * 1e6:.1f} us")
            rep["aspp_us"] = {k: v[0] for k, v in t.items()}
            rep["aspp_peak_fraction"], rep["aspp_gflop"] = frac, useful / 1e9
            del forms, fns
            # ---- tail ----
            z = torch.randn(n, D + CTX, H, W, device=dev, generator=gen) * 3
            fns = {"False": lambda: (torch.softmax(z[:, :D], 1), z[:, D:].permute(0, 2, 3, 1).contiguous()),
                   "force": lambda: ops.depth_softmax_split(z, D)}
            diff = float((fns["False"]()[0] - fns["force"]()[0]).abs().max())
            t = measure(fns, a.iters * 4, a.repeats)
            nbytes = 4.0 * n * H * W * (2 * D + 2 * CTX)
            show(f"{name} tail {n} x ({D} + {CTX}) x {H} x {W}", t, diff,
                 f"; {nbytes / 1e6:.1f} MB read + written, {nbytes / (t['force'][0] * 1e-6) / 1e9:.0f} GB/s forced")
            rep["tail_us"] = {k: v[0] for k, v in t.items()}
            del fns, z
            # ---- DepthNet ----
            mlp = torch.randn(B, N, 27, device=dev, generator=gen)
            forms = three_forms(lambda f: BD.DepthNet(CH, CH, CTX, D, fused=f), dev, gen)
            fns = {k: (lambda m=m: m(x, mlp)) for k, m in forms.items()}
            diff = float((fns["False"]() - fns["force"]()).abs().max())
            t = measure(fns, max(1, a.iters // 2), a.repeats)
            show(f"{name} DepthNet", t, diff)
            rep["depthnet_us"] = {k: v[0] for k, v in t.items()}
            del forms, fns
            # ---- the whole view transformer, index sets prepared once ----
            cams = {k: torch.from_numpy(v).to(dev) for k, v in synth.camera_rig(0, n_cam=N, batch=B).items()}
            geo = [cams[k] for k in ("rots", "trans", "cam2imgs", "post_rots", "post_trans", "bda")]

            def make(f):
                return BD.LSSViewTransformerBEVDepth(in_channels=CH, out_channels=CTX, accelerate=True,
                                                     depthnet_cfg=dict(use_dcn=False), fused=f)

            forms = three_forms(make, dev, gen)
            inp = [x.reshape(B, N, CH, H, W), *geo, forms["False"].get_mlp_input(*geo) * 0 + mlp]
            fns = {k: (lambda m=m: m(inp)) for k, m in forms.items()}
            diff = float((fns["False"]()[0] - fns["force"]()[0]).abs().max())
            t = measure(fns, max(1, a.iters // 2), a.repeats)
            show(f"{name} view transformer", t, diff)
            rep["view_transformer_us"] = {k: v[0] for k, v in t.items()}
            del forms, fns, x
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
