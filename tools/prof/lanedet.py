"""Time BEV-LaneDet's lane head tail and lane post-processing at inference (csrc/lanedet.hip, paddle3d_amd/
bev_lanedet.py) at the shape of configs/bev_lanedet/bev_lanedet_apollo_576x1024.yml: a 200 x 48 BEV map, the four
branches' 64-channel maps, nd = 2, B = 1 and 4, on synthetic lanes (five lanes two pixels wide over 140 rows: 1400
selected pixels; pass --lanes / --rows for others), on three paths over the same inputs on the same commit:

  torch      (a) the transcription: the four final convolutions by torch on the device, the maps copied to the host,
             the reference's clustering, canvas, row means and np.polyfit in NumPy (bev_lanedet.lanes_numpy)
  dense      (b) the four final convolutions on grouped_conv3x3_small and pd3_lanedet_post_process (fused="dense")
  lazy       (c) pd3_lanedet_head_forward from the branch maps (fused="lazy"): the seg convolution densely, emb / offset
             / z at the selected pixels

The branch maps are built so that the final convolutions reproduce the synthetic maps (the lanes, and with them the
selected-pixel count, the centres and the rows, are the same on every path).  Reported in us as the median of
`--repeats` windows of `--iters` calls with the smallest and largest window; the paths alternate inside each repeat,
after a warm-up of each.  A window is a host clock around calls that end in a device synchronise.  Also printed: the
C-ABI calls of each path and the agreement of the paths' results.  Kernel times come from a run of their own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \
        python tools/prof/lanedet.py --iters 5 --repeats 1 --paths lazy,dense

    python tools/prof/lanedet.py [--iters 20] [--repeats 5] [--lanes 5] [--rows 140]
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
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import lanedet_numpy as ln  # noqa: E402

from paddle3d_amd import _lib  # noqa: E402
from paddle3d_amd import bev_lanedet as M  # noqa: E402
from paddle3d_amd.ops import lanedet as A  # noqa: E402

H, W, ND, C = 200, 48, 2, 64


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

    symbols = _lib.symbols("test_memory_safety_gpu") + _lib.symbols("test_memory_safety_lanedet_gpu")
    with launch_ledger(_lib.lib(), symbols) as calls:
        fn()
    return {k: v for k, v in calls.items() if v}


def make_inputs(B, lanes, rows, dev, seed=0):
    """Branch maps [B, 64, H, W] and a head whose final convolutions reproduce synthetic lanes of `rows` rows."""
    rng = np.random.default_rng(seed)
    seg, emb, off, z = ln.synthetic_lanes(rng, B, H, W, ND, lanes=lanes)
    seg[:, :, rows:] = -5.0
    logit = np.log(off / (1 - off)).astype(np.float32)
    feats, state = ln.identity_head(seg, emb, logit, z, C=C)
    head = M.InstanceEmbeddingOffsetYZ(64, ND).eval().to(dev)
    with torch.no_grad():
        for k in ln.BRANCHES:
            getattr(head, k)[6].weight.copy_(torch.from_numpy(state[k + ".weight"]))
            getattr(head, k)[6].bias.copy_(torch.from_numpy(state[k + ".bias"]))
    return [torch.from_numpy(f).to(dev) for f in feats], head


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--paths", default="torch,dense,lazy")
    ap.add_argument("--lanes", type=int, default=5)
    ap.add_argument("--rows", type=int, default=140, help="rows of the map that hold lanes (140: 1400 selected pixels)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lanedet: needs the GPU (a CPU run says nothing about these times)")
    dev = torch.device("cuda", 0)
    post = dict(ln.CFG)
    with torch.no_grad():
        for B in (1, 4):
            maps, head = make_inputs(B, a.lanes, a.rows, dev)
            wb = [t for b in head.branches() for t in (b[6].weight, b[6].bias)]

            def lazy():
                return A.lanedet_head_forward(*maps, *wb, **post)

            def dense():
                seg, emb, off, z = head.final_maps(maps)
                return A.lanedet_post_process(seg, emb, off, z, offset_is_logit=True, **post)

            def transcription():
                seg, emb, off, z = (b[6](m) for b, m in zip(head.branches(), maps))
                host = torch.cat([seg, emb, torch.sigmoid(off), z], 1).cpu().numpy()
                return [M.lanes_numpy(host[i], **post) for i in range(B)]

            fns = {k: f for k, f in (("torch", transcription), ("dense", dense), ("lazy", lazy)) if k in a.paths.split(",")}
            res = {k: fn() for k, fn in fns.items()}
            packs = {k: r for k, r in res.items() if k != "torch"}
            for k, r in packs.items():
                print(f"B = {B} {k}: selected {r.num_selected.tolist()} lanes {r.num_lanes.tolist()} flags "
                      f"{r.flags.tolist()} rows {r.lane_rows[0, :int(r.num_lanes[0])].tolist()}")
            if len(packs) == 2:
                same = all(torch.equal(getattr(packs["lazy"], f), getattr(packs["dense"], f)) for f in A.LanePack._fields)
                print(f"  lazy and dense bit-equal: {same}")
            if "torch" in res and packs:
                r = next(iter(packs.values()))
                canvas_same = all(np.array_equal(res["torch"][i][0], r.labels[i].cpu().numpy()) for i in range(B))
                fits = np.stack([f for _, _, f in res["torch"][0][1]])
                diff = float(np.abs(fits - r.fit[0, :len(fits)].cpu().numpy()).max())
                print(f"  transcription vs device: canvas equal {canvas_same}, max |fit difference| frame 0 {diff:.3g}")
            for k, fn in fns.items():
                print(f"  C-ABI calls, {k}: {ledger(fn)}")
            t = measure(fns, a.iters if B == 1 else max(1, a.iters // 2), a.repeats)
            first = next(iter(t))
            for k, (med, lo, hi) in t.items():
                print(f"  B = {B} {k:6s} {med:10.1f} us  [{lo:.1f} .. {hi:.1f}]  {first} / this = {t[first][0] / med:5.2f}")


if __name__ == "__main__":
    main()
