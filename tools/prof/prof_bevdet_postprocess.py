"""Time the BEVDet4D CenterHead post-process (decode + Scale-NMS / circle NMS + merge, ops/bevdet_postprocess.py) at
the BEVDet4D config: 6 tasks, 128 x 128 maps, max_num 500, pre 1000, post 83.  Device time of the launch sequence
per batch (CUDA events over `--iters` back-to-back calls, no synchronisation inside).

    python tools/prof/prof_bevdet_postprocess.py [--batch 8] [--iters 200]
Run under `rocprofv3 --kernel-trace --stats -- python ...` for the per-kernel split and the launch count."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import bevdet_head_numpy as bh  # noqa: E402

from paddle3d_amd import bevdet_head  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    classes = [t["num_class"] for t in bevdet_head.BEVDET4D_TASKS]
    heads = bh.head_maps(classes, a.batch, 128, 128, seed=7, peaks=60)
    preds = [{k: torch.from_numpy(v).to(dev) for k, v in hd.items()} for hd in heads]
    coder = bevdet_head.CenterPointBBoxCoder(**bevdet_head.BEVDET4D_BBOX_CODER)
    cfg = bevdet_head.BEVDET4D_TEST_CFG
    run = lambda: bevdet_head.get_bboxes_device(preds, cfg, coder, classes)  # noqa: E731
    for _ in range(10):
        out = run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        out = run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    print(f"bevdet postprocess B={a.batch}: {ms * 1000:.1f} us per batch ({ms * 1000 / a.batch:.1f} us per frame), "
          f"rows per frame {out[3].tolist()}")


if __name__ == "__main__":
    main()
