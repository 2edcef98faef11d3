"""Time IA-SSD's set abstraction and box decode at inference (csrc/iassd.hip, paddle3d_amd/iassd.py) at the shapes of
configs/iassd/iassd_kitti.yaml (16384 points, B = 1 and 4) and at the npoints of iassd_waymo.yaml (65536 points, B = 1),
on two paths over the same inputs on the same commit:

  fused      pd3_sa_msg_pool: features @ W1[:, 3:]^T over the source points, then one launch per scale
  unfused    the composition over the existing ops (ball_query_batch, grouping_operation_batch twice, subtract, concat,
             three times conv / BN / ReLU, max): what SAModuleMSG_WithSampling(fused=False) runs -- the baseline

per scale (the query points are the layer's own FPS / top-K sample of a seeded uniform cloud of the config's density,
so the hit counts are the ones the layer sees) and for the whole forward of the model (fused="force" against
fused=False; the last layer's widths are refused by the kernel and run the composition on both paths).  The decode
kernel is timed against the coder's torch fall-back on 256 and 1024 rows per frame.

Reported in us as the median of `--repeats` windows of `--iters` calls with the smallest and largest window; the paths
alternate inside each repeat, after a warm-up of each.  A window is a host clock around calls that end in a device
synchronise.  "spread" is (largest - smallest) / median of a path's windows; a scale counts as faster on the kernel when
the medians differ by more than the larger of the two spreads (the rule MEASURED_FASTER in paddle3d_amd/iassd.py follows).

    python tools/prof/iassd.py [--iters 20] [--repeats 5] [--skip-waymo]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddle3d_amd import iassd  # noqa: E402

# the clouds' extents: KITTI's camera-visible range, Waymo's full range
EXTENT = {"kitti": ([0.0, -40.0, -3.0], [70.4, 40.0, 1.0]), "waymo": ([-75.2, -75.2, -2.0], [75.2, 75.2, 4.0])}


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


def report(label, t, base="unfused", new="fused"):
    spread = {k: (hi - lo) / med for k, (med, lo, hi) in t.items()}
    for k, (med, lo, hi) in t.items():
        print(f"  {label} {k:8s} {med:10.1f} us  [{lo:.1f} .. {hi:.1f}]  spread {100 * spread[k]:.1f} %")
    gain = t[base][0] / t[new][0]
    faster = t[base][0] - t[new][0] > max(spread.values()) * t[base][0]
    print(f"  {label} {base} / {new} = {gain:.2f}  faster beyond the spread: {faster}")
    return gain, faster


def cloud(tag, B, n, channels, gen, dev):
    lo, hi = (torch.tensor(v, device=dev) for v in EXTENT[tag])
    xyz = lo + (hi - lo) * torch.rand(B, n, 3, device=dev, generator=gen)
    # a ground plane and some clusters, so that small radii find neighbours as in a scan
    xyz[:, : n // 2, 2] = lo[2] + 0.3 * torch.rand(B, n // 2, device=dev, generator=gen)
    feats = torch.rand(B, n, channels, device=dev, generator=gen)
    batch = torch.arange(B, device=dev, dtype=torch.float32).repeat_interleave(n)[:, None]
    return torch.cat([batch, xyz.reshape(-1, 3), feats.reshape(B * n, -1)], dim=1)


def scales(model, data, B, iters, repeats, label):
    """Per scale of layers 0-2 and 5: the inputs are the ones the forced model's forward gives the layer."""
    taken = {}
    hooks = [layer.register_forward_pre_hook(lambda mod, a, kw, _i=i: taken.__setitem__(_i, (a, kw)), with_kwargs=True)
             for i, layer in enumerate(model.backbone.SA_modules)]
    model({"data": data, "batch_size": B})
    for h in hooks:
        h.remove()
    results = {}
    for i, layer in enumerate(model.backbone.SA_modules):
        if not isinstance(layer, iassd.SAModuleMSG_WithSampling) or len(layer.groupers) == 0:
            continue
        a, kw = taken[i]
        xyz, features = a[0], a[1]
        new_xyz = kw.get("ctr_xyz")
        if new_xyz is None:
            new_xyz = iassd.sample_points(xyz, layer.npoint, layer.sample_type, a[2] if len(a) > 2 else None)[1]
        new_xyz, fd = new_xyz.contiguous(), layer._fold()
        for k, g in enumerate(layer.groupers):
            m = layer.mlps[k]
            key = (m[0].out_channels, m[3].out_channels, m[6].out_channels, int(g.nsample))
            name = f"{label} layer {i} scale {k} {key} r {g.radius} n {xyz.shape[1]} m {new_xyz.shape[1]}"
            if not layer.scale_is_fused(k):
                print(f"  {name}: refused by the kernel, the composition on both paths")
                continue
            w_pos, w_feat, *rest = fd["scales"][k]
            pts = features.transpose(1, 2)

            def fused():
                from paddle3d_amd.ops import iassd as ops

                return ops.sa_msg_pool(new_xyz, xyz, torch.matmul(pts, w_feat.t()), w_pos, *rest, g.radius, g.nsample)

            t = measure({"fused": fused, "unfused": lambda: layer._unfused_scale(k, xyz, new_xyz, features)}, iters, repeats)
            diff = float((fused().transpose(1, 2) - layer._unfused_scale(k, xyz, new_xyz, features)).abs().max())
            print(f"  {name}: max |fused - unfused| {diff:.3g}")
            results[(i, k) + key] = report(f"{label} L{i}S{k}", t)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-waymo", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("iassd: needs the GPU (a CPU run says nothing about these times)")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(dev).manual_seed(1)
    torch.manual_seed(0)
    faster = {}
    with torch.no_grad():
        for tag, make, n, channels, batches in (("kitti", iassd.iassd_kitti, 16384, 1, (1, 4)),
                                                ("waymo", iassd.iassd_waymo, 65536, 2, (1,))):
            if tag == "waymo" and a.skip_waymo:
                continue
            forced, plain = make(fused="force").to(dev).eval(), make(fused=False).to(dev).eval()
            plain.load_state_dict(forced.state_dict())
            for B in batches:
                data = cloud(tag, B, n, channels, gen, dev)
                label = f"{tag} B = {B}"
                res = scales(forced, data, B, a.iters, a.repeats, label)
                if B == 1:
                    faster.update({k[2:]: v for k, v in res.items()})
                t = measure({"fused": lambda: forced({"data": data, "batch_size": B}),
                             "unfused": lambda: plain({"data": data, "batch_size": B})}, max(1, a.iters // 4), a.repeats)
                report(f"{label} forward", t)
        coder = iassd.PointResidual_BinOri_Coder(use_mean_size=True, mean_size=[[3.9, 1.6, 1.56], [0.8, 0.6, 1.73],
                                                                                 [1.76, 0.6, 1.73]]).to(dev)
        for rows in (256, 1024):
            cls = torch.randn(rows, 3, device=dev, generator=gen)
            box = torch.randn(rows, 30, device=dev, generator=gen)
            ctr = torch.randn(rows, 4, device=dev, generator=gen)
            t = measure({"fused": lambda: coder.decode(box, ctr[:, 1:4], cls),
                         "unfused": lambda: coder.decode_paddle(box, ctr[:, 1:4], cls.argmax(-1) + 1)}, a.iters * 5, a.repeats)
            report(f"decode {rows} rows", t)
    print("scales measured faster on the kernel at B = 1, beyond the spread (c1, c2, c3, nsample):",
          sorted(k for k, (_, f) in faster.items() if f))
    print("scales not faster:", sorted(k for k, (_, f) in faster.items() if not f))


if __name__ == "__main__":
    main()
