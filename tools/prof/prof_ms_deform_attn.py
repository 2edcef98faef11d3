"""Time ms_deform_attn (paddle3d_amd/ops/ms_deform_attn.py, csrc/ms_deform_attn.hip) forward and forward + backward
at BEVFormer-tiny's three call sites and a four-level shape, against the torch composition a user would otherwise
write on the GPU (F.grid_sample per level over the heads, weighted sum: ms_deform_attn_numpy.grid_sample_attn).

Device time per call from CUDA events over `--iters` back-to-back calls, no synchronisation inside.  Reported per
shape:
  HBM      compulsory bytes (value, locations and weights read once, out written once) against 8 TB/s
  gather   corner-row bytes (4 corners x C x 4 B per (b, q, m, l, p)) against the 7 TB/s L2 -> CU gather ceiling
  atomics  backward only: grad_value's added bytes (= the corner-row bytes) against ~1.3 TB/s of float atomics

    python tools/prof/prof_ms_deform_attn.py [--iters 50] [--shapes tsa sca decoder four_level]
Run under `rocprofv3 --kernel-trace --stats -- python ...` (with `--iters` small) for kernel times and launches."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import ms_deform_attn_numpy as md  # noqa: E402

from paddle3d_amd.ops import ms_deform_attn as msda  # noqa: E402

SHAPES = {
    "tsa": dict(B=2, Q=2500, M=8, C=32, shapes=[[50, 50]], P=4),
    "sca": dict(B=6, Q=2500, M=8, C=32, shapes=[[15, 25]], P=8),
    "decoder": dict(B=1, Q=900, M=8, C=32, shapes=[[50, 50]], P=4),
    "four_level": dict(B=2, Q=10000, M=8, C=32, shapes=[[100, 176], [50, 88], [25, 44], [13, 22]], P=4),
}
HBM, GATHER, ATOMIC = 8.0e12, 7.0e12, 1.3e12


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    a = ap.parse_args()
    for name in a.shapes:
        c = SHAPES[name]
        B, Q, M, C, P = c["B"], c["Q"], c["M"], c["C"], c["P"]
        value, loc, attn, sh, st = md.random_case(np.random.default_rng(1), B, Q, M, C, c["shapes"], P)
        L, S = sh.shape[0], value.shape[1]
        v, l, w = (torch.from_numpy(x).cuda() for x in (value, loc, attn))
        shd, std = torch.from_numpy(sh).cuda(), torch.from_numpy(st).cuda()
        go = torch.randn(B, Q, M * C, device="cuda")
        vg, lg, wg = (x.clone().requires_grad_() for x in (v, l, w))

        def hip_fwd():
            return msda.ms_deform_attn(v, l, w, shd, std, 64)

        def torch_fwd():
            return md.grid_sample_attn(v, l, w, sh, st)

        def hip_fb():
            msda.ms_deform_attn(vg, lg, wg, shd, std, 64).backward(go)

        def torch_fb():
            md.grid_sample_attn(vg, lg, wg, sh, st).backward(go)

        diff = float((hip_fwd() - torch_fwd()).abs().max())
        hbm = (B * S * M * C + B * Q * M * L * P * 3 + B * Q * M * C) * 4
        rows = B * Q * M * L * P * 4 * C * 4
        t = {k: _time(f, a.iters) for k, f in (("hip_fwd", hip_fwd), ("torch_fwd", torch_fwd), ("hip_fb", hip_fb),
                                               ("torch_fb", torch_fb))}
        print(f"{name}: value [{B}, {S}, {M}, {C}], Q {Q}, L {L}, P {P}; HBM {hbm / 1e6:.1f} MB, corner rows "
              f"{rows / 1e6:.1f} MB; max |hip - torch| = {diff:.3g}")
        f = t["hip_fwd"] * 1e-6
        print(f"  forward      hip {t['hip_fwd']:8.1f} us   torch {t['torch_fwd']:8.1f} us   "
              f"HBM {hbm / f / 1e12:.2f} TB/s = {hbm / f / HBM:.3f} of 8;  gather {rows / f / 1e12:.2f} TB/s = "
              f"{rows / f / GATHER:.3f} of 7")
        fb = t["hip_fb"] * 1e-6
        print(f"  fwd + bwd    hip {t['hip_fb']:8.1f} us   torch {t['torch_fb']:8.1f} us   "
              f"atomic floor {rows / ATOMIC * 1e6:.1f} us; bwd-only estimate {t['hip_fb'] - t['hip_fwd']:.1f} us "
              f"(atomics {rows / ((t['hip_fb'] - t['hip_fwd']) * 1e-6) / 1e12:.2f} TB/s)")
        del v, l, w, vg, lg, wg
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
