"""Time DD3D's heads and post-processing at inference (csrc/dd3d.hip, paddle3d_amd/dd3d.py) at KITTI's evaluation shape
of configs/dd3d/dd3d_dla_34_kitti.yml: 384 x 1280 after padding, levels 48 x 160, 24 x 80, 12 x 40, 6 x 20 and 3 x 10 at
strides 8 .. 128, 256 channels, 5 classes, FrozenBN towers of four convolutions, pre_nms_topk 1000, post_nms_topk 100,
nms_thresh 0.75, B = 1 (and 4), on three paths over the same inputs on the same commit:

  torch      (a) the module's plain-torch transcription of the reference on the device (fused=False): the 59 predictor
             channels densely, then FCOS2DInference / FCOS3DInference / nms_and_top_k with their host synchronisations
  dense      (b) the 59 predictor channels by torch's convolutions and pd3_dd3d_post_process (fused="dense")
  lazy       (c) cls_logits and centerness by torch's convolutions and pd3_dd3d_head_forward (fused="lazy"): the other 54
             predictor channels are never formed, 4 + 11 rows are evaluated per selected entry

Two windows per path: `tail` starts from the three towers' outputs (what differs between the paths), `head` from the
FPN's features (towers included: twelve 256 -> 256 convolutions per level that every path runs alike).  Reported in us
as the median of `--repeats` windows of `--iters` calls with the smallest and largest window; the paths alternate
inside each repeat, after a warm-up of each.  A window is a host clock around calls that end in a device synchronise.
The class logits carry a bias so that the frame has several hundred candidates per level, as a scene with objects has;
`--bias` moves it.  Also printed: the candidates per level, the C-ABI calls of each path (tests/guarded.py's launch
ledger) and the agreement of the paths' results.  Kernel times come from a run of their own:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/prof/dd3d.py --iters 5 --repeats 1 --paths lazy,dense

    python tools/prof/dd3d.py [--iters 20] [--repeats 5] [--batches 1,4] [--bias -6.0]
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
from paddle3d_amd import dd3d as D  # noqa: E402

SHAPES = ((48, 160), (24, 80), (12, 40), (6, 20), (3, 10))
STRIDES = (8, 16, 32, 64, 128)
C, NC = 256, 5


def make_model(device, bias, seed=0):
    torch.manual_seed(seed)
    head2 = D.FCOS2DHead(list(STRIDES), [C] * 5, num_classes=NC, version="v2", norm="FrozenBN")
    head3 = D.FCOS3DHead(list(STRIDES), [C] * 5, num_classes=NC, norm="FrozenBN")
    model = D.DD3D(None, "none", None, head2, D.FCOS2DInference(num_classes=NC), head3, D.FCOS3DInference(num_classes=NC),
                   do_nms=True, num_classes=NC, input_strides=STRIDES)
    with torch.no_grad():
        head2.cls_logits.bias.fill_(bias)
        head2.box2d_reg.bias.fill_(0.5)
        for m in model.modules():
            if isinstance(m, D.FrozenBatchNorm2d):
                m.weight.uniform_(0.8, 1.2)
                m.bias.normal_(0, 0.1)
    return model.eval().to(device)


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

    with launch_ledger(_lib.lib(), _lib.symbols("test_memory_safety_dd3d_gpu")) as calls:
        fn()
    return {k: v for k, v in calls.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--paths", default="torch,dense,lazy")
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--bias", type=float, default=-6.0, help="bias of cls_logits: sets the number of candidates")
    ap.add_argument("--windows", default="tail,head")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dd3d: needs the GPU (a CPU run says nothing about these times)")
    dev = torch.device("cuda", 0)
    model = make_model(dev, a.bias)
    gen = torch.Generator(dev).manual_seed(1)
    forms = {"torch": False, "dense": "dense", "lazy": "lazy"}
    with torch.no_grad():
        for B in (int(b) for b in a.batches.split(",")):
            feats = [torch.randn(B, C, h, w, device=dev, generator=gen) for h, w in SHAPES]
            K = torch.tensor([[721.5377, 0, 609.5593], [0, 721.5377, 172.854], [0, 0, 1]], device=dev).repeat(B, 1, 1)
            towers = model.towers(feats)
            logits = model.fcos2d_head.predict(towers[0], towers[1])
            s = [torch.sigmoid(lg) * torch.sigmoid(ct) for lg, ct in zip(logits[0], logits[2])]
            print(f"B = {B}: candidates per level (frame 0) {[int((x[0] > 0.05).sum()) for x in s]}")
            tail = {k: (lambda f=forms[k]: model.tail_padded(*towers, K, fused=f)) for k in a.paths.split(",")}
            head = {k: (lambda f=forms[k]: model.head_padded(feats, K, fused=f)) for k in a.paths.split(",")}
            res = {k: fn() for k, fn in tail.items()}
            print("  counts " + " ".join(f"{k} {r[1].tolist()}" for k, r in res.items()))
            first = next(iter(res))
            for k in list(res)[1:]:
                same = torch.equal(res[k][1], res[first][1]) and torch.equal(res[k][0][..., 6], res[first][0][..., 6])
                diff = float((res[k][0] - res[first][0]).abs().max()) if same else float("nan")
                print(f"  {k} vs {first}: classes and counts equal {same}, max |row difference| {diff:.3g}")
            for k, fn in tail.items():
                print(f"  C-ABI calls, {k}: {ledger(fn)}")
            for name, fns in (("tail", tail), ("head", head)):
                if name not in a.windows.split(","):
                    continue
                t = measure(fns, a.iters if B == 1 else max(1, a.iters // 2), a.repeats)
                for k, (med, lo, hi) in t.items():
                    print(f"  B = {B} {name} {k:6s} {med:10.1f} us  [{lo:.1f} .. {hi:.1f}]  {first} / this = "
                          f"{t[first][0] / med:5.2f}")


if __name__ == "__main__":
    main()
