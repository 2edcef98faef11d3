"""Time CAPE / CAPE-T's cross-view attention (csrc/cape.hip, paddle3d_amd/cape.py) at the shapes of the three configs
under configs/cape: 900 queries, 8 heads of 64 (hidden 512), 6 cameras, stride-32 feature maps, at B = 1 frame-set --

    capet_r50_704x256      K =  8 x 22 = 176 keys per camera, 1056 in all, two frames (with_time stacks them: b = 2)
    capet_vovnet_800x320   K = 10 x 25 = 250 keys per camera, 1500 in all, two frames
    cape_r50_1408x512      K = 16 x 44 = 704 keys per camera, 4224 in all, one frame

on two paths over the same projected rows on the same commit:

  torch      CrossAttention.core_torch, the module's own composition (fused=False): two einsums, scales, add, fill,
             softmax, einsum -- it forms the three [b, heads, n, Q, K] tensors and the permuted copies
  kernel     pd3_cape_cva_forward, one launch

and, with --layers, one CrossViewAttention layer (projections, attention core, proj, MLP, sl_layer) in the three forms
fused=False / True / "force"; six such layers are a transformer's attention work.  Reported in us as the median of
`--repeats` windows of `--iters` calls with the smallest and largest window; the paths alternate inside each repeat,
after a warm-up of each.  A window is a host clock around calls that end in a device synchronise.  Also printed: the
largest difference of the two paths' results, and what is derived from the shape rather than measured: the bytes of the
tensors the torch path forms and the kernel does not, and the bytes the kernel has to read once (its floor at the HBM
rate of MI355X_MICROARCH.md is bytes / 8 TB/s).  Kernel times come from a run of their own:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/prof/cape.py --iters 5 --repeats 1

    python tools/prof/cape.py [--iters 20] [--repeats 5] [--layers] [--transformer] [--sweep] [--json FILE]

--transformer times the six-layer CAPETransformer of each config (cape_transformer(config, fused): position embedding,
feature projection, embeddings, six CrossViewAttention layers, the temporal fusion under with_time) in the three forms.
--sweep adds the same two paths at smaller feature maps (6 cameras of K = 16 .. 128 keys, b = 2), where the border of
paddle3d_amd.cape.CVA_FUSED_MAX_KEYS is looked for, and sl_layer's core alone (pd3_mha_forward against torch at 900 x
900, 8 heads of 64, b = 2).
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

from paddle3d_amd import cape as CP  # noqa: E402
from paddle3d_amd.ops import cape as ops  # noqa: E402

Q, HEADS, DIM_HEAD, CAMS = 900, 8, 64, 6
CONFIGS = {"capet_r50_704x256": dict(b=2, K=8 * 22), "capet_vovnet_800x320": dict(b=2, K=10 * 25),
           "cape_r50_1408x512": dict(b=1, K=16 * 44)}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--layers", action="store_true", help="also time one CrossViewAttention layer in its three forms")
    ap.add_argument("--transformer", action="store_true", help="also time each config's six-layer transformer")
    ap.add_argument("--sweep", action="store_true", help="also time smaller key counts and sl_layer's core")
    ap.add_argument("--json", default=None, help="write the medians to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cape: needs the GPU (a CPU run says nothing about these times)")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(dev).manual_seed(1)
    E = HEADS * DIM_HEAD
    x = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    report = {}
    configs = dict(CONFIGS)
    if a.sweep:
        configs.update({f"sweep_K{K}": dict(b=2, K=K) for K in (16, 32, 64, 88, 128)})
    with torch.no_grad():
        for name, c in configs.items():
            b, K = c["b"], c["K"]
            ca = CP.CrossAttention(E, HEADS, DIM_HEAD, True, fused="force").eval().to(dev)
            q_a, q_g, k_a, k_g, v = x(b, Q, E), x(b, CAMS, Q, E), x(b, CAMS, K, E), x(b, CAMS, K, E), x(b, CAMS, K, E)
            mask = torch.rand(b, CAMS, K, device=dev, generator=gen) < 0.1
            fns = {"torch": lambda: ca.core_torch(k_g, q_g, k_a, q_a, v, mask),
                   "kernel": lambda: ops.cross_view_attention(q_a, q_g, k_a, k_g, v, ca.scale_a, ca.scale_g, HEADS, mask)}
            diff = float((fns["torch"]() - fns["kernel"]()).abs().max())
            t = measure(fns, a.iters, a.repeats)
            scores = b * HEADS * CAMS * Q * K * 4
            rows = (b * Q * E + b * CAMS * Q * E + 3 * b * CAMS * K * E) * 4
            print(f"{name}: b = {b}, N * K = {CAMS * K}; max |torch - kernel| {diff:.3g}")
            for k, (med, lo, hi) in t.items():
                print(f"  {k:6s} {med:10.1f} us  [{lo:.1f} .. {hi:.1f}]  torch / this = {t['torch'][0] / med:5.2f}")
            print(f"  derived: each of dot_g, dot_a, dot and the softmax output is {scores / 1e6:.1f} MB, formed by the torch "
                  f"path only; the kernel reads {rows / 1e6:.1f} MB of rows once ({rows / 8e12 * 1e6:.1f} us at 8 TB/s) and "
                  f"k_a, k_g a second time; {2 * 3 * b * HEADS * Q * CAMS * K * DIM_HEAD / 1e9:.2f} Gflop counted once")
            report[name] = dict(keys=CAMS * K, b=b, torch_us=t["torch"][0], kernel_us=t["kernel"][0], max_diff=diff)
            if a.layers and name in CONFIGS:
                args = (x(b, Q, E), x(b, CAMS, Q, E), x(b, Q, E), x(b, CAMS, K, E), x(b, CAMS, E), mask, x(b, CAMS, K, E),
                        x(b, CAMS, Q, E), None)
                layers = {}
                for fused in (False, True, "force"):
                    torch.manual_seed(2)
                    layers[str(fused)] = CP.CrossViewAttention(Q, E, True, heads=HEADS, dim_head=DIM_HEAD,
                                                               fused=fused).eval().to(dev)
                lf = {k: (lambda m=m: m(*args)) for k, m in layers.items()}
                ref = lf["False"]()
                tl = measure(lf, max(1, a.iters // 2), a.repeats)
                for k, (med, lo, hi) in tl.items():
                    d = float((lf[k]() - ref).abs().max())
                    print(f"  layer fused={k:5s} {med:10.1f} us  [{lo:.1f} .. {hi:.1f}]  unfused / this = "
                          f"{tl['False'][0] / med:5.2f}  six layers {6 * med / 1e3:.2f} ms  max |this - unfused| {d:.3g}")
                report[name]["layer_us"] = {k: v[0] for k, v in tl.items()}
        if a.transformer:
            for name, (ih, iw, with_time) in CP.TRANSFORMER_CONFIGS.items():
                nc, h, w = (12 if with_time else 6), ih // 32, iw // 32
                K = torch.tensor([[0.8 * iw, 0, iw / 2], [0, 0.8 * iw, ih / 2], [0, 0, 1]], device=dev)
                R = torch.linalg.qr(x(1, nc, 3, 3)).Q
                args = (x(1, nc, 256, h, w), torch.rand(1, nc, h, w, device=dev, generator=gen) < 0.05,
                        torch.linalg.inv(K).expand(1, nc, 3, 3).contiguous(), R, x(1, nc, 3, 1), (ih, iw))
                kw = dict(ego_matrix=torch.eye(4, device=dev)) if with_time else {}
                forms = {}
                for fused in (False, True, "force"):
                    torch.manual_seed(3)
                    forms[str(fused)] = CP.cape_transformer(name, fused).eval().to(dev)
                tf = {k: (lambda m=m: m(*args, **kw)[0]) for k, m in forms.items()}
                ref = tf["False"]()
                tt = measure(tf, max(1, a.iters // 4), a.repeats)
                print(f"{name}: six-layer transformer, {nc} cameras of {h} x {w}")
                for k, (med, lo, hi) in tt.items():
                    d = float((tf[k]() - ref).abs().max())
                    print(f"  fused={k:5s} {med / 1e3:8.2f} ms  [{lo / 1e3:.2f} .. {hi / 1e3:.2f}]  unfused / this = "
                          f"{tt['False'][0] / med:5.2f}  max |this - unfused| {d:.3g}")
                report.setdefault(name, {})["transformer_us"] = {k: v[0] for k, v in tt.items()}
                del forms, tf
        if a.sweep:
            from paddle3d_amd.ops import bevformer_decoder as dec

            q, k, v = x(2, Q, E), x(2, Q, E), x(2, Q, E)

            def torch_core():
                qh, kh, vh = (t.reshape(2, Q, HEADS, DIM_HEAD).permute(0, 2, 1, 3) for t in (q, k, v))
                p = torch.softmax(torch.matmul(qh * (DIM_HEAD ** -0.5), kh.transpose(-1, -2)), -1)
                return torch.matmul(p, vh).permute(0, 2, 1, 3).reshape(2, Q, E)

            fns = {"torch": torch_core, "kernel": lambda: dec.multihead_attention(q, k, v, HEADS)}
            t = measure(fns, a.iters, a.repeats)
            print(f"sl_layer's core, b = 2, {Q} x {Q}, {HEADS} heads of {DIM_HEAD}: max |torch - kernel| "
                  f"{float((fns['torch']() - fns['kernel']()).abs().max()):.3g}")
            for k_, (med, lo, hi) in t.items():
                print(f"  {k_:6s} {med:10.1f} us  [{lo:.1f} .. {hi:.1f}]  torch / this = {t['torch'][0] / med:5.2f}")
            report["sl_core"] = dict(torch_us=t["torch"][0], kernel_us=t["kernel"][0])
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
