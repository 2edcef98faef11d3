"""Time SMOKE's head and post-processing at inference (csrc/smoke.hip, paddle3d_amd/smoke.py) at the shape of
configs/smoke/smoke_dla34_no_dcn_kitti.yml: a 64 x 96 x 320 feature map, a head width of 256 with 32-group GroupNorm,
3 classes, max_detection = 50, B = 1 and 8, on three paths over the same inputs on the same commit:

  torch      (a) the module's plain-torch transcription of the reference on the device (fused=False): two 3x3
             convolutions, GroupNorm, ReLU, 1x1, the activations, max_pool2d, two topk, gathers, two batched inverses,
             the decode
  dense      (b) the stacked 3x3 convolution, torch's GroupNorm / ReLU / 1x1 layers and activations, and
             pd3_smoke_post_process (fused="dense")
  lazy       (c) the stacked 3x3 convolution and pd3_smoke_head_forward (fused="lazy"): tables, class branch,
             select-and-decode with the regression branch at the 50 selected pixels

Reported in us as the median of `--repeats` windows of `--iters` calls with the smallest and largest window; the paths
alternate inside each repeat, after a warm-up of each.  A window is a host clock around calls that end in a device
synchronise.  Also printed: the C-ABI calls of each path (tests/guarded.py's launch ledger), the agreement of the paths'
results, and what is derived from the shape rather than measured: the bytes each of this file's kernels has to read once
(its floor at the HBM rate of MI355X_MICROARCH.md is bytes / 8 TB/s).  Kernel times come from a run of their own:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/prof/smoke.py --iters 5 --repeats 1 --paths lazy,dense

    python tools/prof/smoke.py [--iters 20] [--repeats 5] [--conv winograd43|torch]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from paddle3d_amd import _lib  # noqa: E402
from paddle3d_amd import smoke as S  # noqa: E402

SHAPE = dict(Cin=64, C=256, H=96, W=320, nc=3, K=50)


def make_model(device, seed=0):
    torch.manual_seed(seed)
    model = S.smoke_dla34_no_dcn_kitti(torch.nn.Identity())
    with torch.no_grad():
        for m in model.heads.modules():
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.1)
    return model.eval().to(device)


def targets(B, device):
    K = torch.tensor([[721.5377, 0, 609.5593], [0, 721.5377, 172.854], [0, 0, 1]], device=device).repeat(B, 1, 1)
    s = SHAPE["W"] / 1280.0
    T = torch.tensor([[s, 0, 0], [0, s, 0], [0, 0, 1]], device=device).repeat(B, 1, 1)
    return dict(K=K, trans_mat=T, image_size=torch.tensor([[1280.0, 384.0]], device=device))


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

    symbols = _lib.symbols("test_memory_safety_gpu") + _lib.symbols("test_memory_safety_smoke_gpu")
    with launch_ledger(_lib.lib(), symbols) as calls:
        fn()
    return {k: v for k, v in calls.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--paths", default="torch,dense,lazy")
    ap.add_argument("--conv", default=None, help="the stacked 3x3 convolution's kernel (SMOKEPredictor.conv_kernel)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("smoke: needs the GPU (a CPU run says nothing about these times)")
    dev = torch.device("cuda", 0)
    model = make_model(dev)
    if a.conv is not None:
        model.heads.conv_kernel = a.conv
    Cin, C, H, W, nc, K = (SHAPE[k] for k in ("Cin", "C", "H", "W", "nc", "K"))
    gen = torch.Generator(dev).manual_seed(1)
    forms = {"torch": False, "dense": "dense", "lazy": "lazy"}
    with torch.no_grad():
        for B in (1, 8):
            x, tg = torch.randn(B, Cin, H, W, device=dev, generator=gen), targets(B, dev)
            fns = {k: (lambda f=forms[k]: model.head_padded(x, targets=tg, fused=f)) for k in a.paths.split(",")}
            res = {k: fn() for k, fn in fns.items()}
            print(f"B = {B}: counts " + " ".join(f"{k} {r[1].tolist()}" for k, r in res.items()))
            first = next(iter(res))
            for k in list(res)[1:]:
                same = torch.equal(res[k][1], res[first][1]) and torch.equal(res[k][0][..., 0], res[first][0][..., 0])
                diff = float((res[k][0] - res[first][0]).abs().max()) if same else float("nan")
                print(f"  {k} vs {first}: classes and counts equal {same}, max |row difference| {diff:.3g}")
            for k, fn in fns.items():
                print(f"  C-ABI calls, {k}: {ledger(fn)}")
            t = measure(fns, a.iters if B == 1 else max(1, a.iters // 2), a.repeats)
            for k, (med, lo, hi) in t.items():
                print(f"  B = {B} {k:6s} {med:10.1f} us  [{lo:.1f} .. {hi:.1f}]  {first} / this = {t[first][0] / med:5.2f}")
            one = B * C * H * W * 4
            heat = B * nc * H * W * 4
            print(f"  derived, read once: smoke_stats_kernel both branches' maps {2 * one / 1e6:.1f} MB (twice: two passes); "
                  f"smoke_class_kernel one map {one / 1e6:.1f} MB, writes the heat map {heat / 1e6:.2f} MB; "
                  f"smoke_select_kernel the heat map {heat / 1e6:.2f} MB and {B * K * C * 4 / 1e3:.1f} KB of regression "
                  f"columns; the dense path also normalises and convolves the regression map: {2 * one / 1e6:.1f} MB more "
                  f"read and {(one + B * 10 * H * W * 4) / 1e6:.1f} MB written; the stacked convolution reads "
                  f"{B * Cin * H * W * 4 / 1e6:.1f} MB and writes {2 * one / 1e6:.1f} MB ({2 * 9 * Cin * 2 * C * H * W * B / 1e9:.1f} Gflop)")


if __name__ == "__main__":
    main()
