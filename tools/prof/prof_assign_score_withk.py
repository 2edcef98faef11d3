"""Time assign_score_withk (paddle3d_amd/ops/assign_score_withk.py, csrc/assign_score_withk.hip) at the four PAConv
layer shapes (B = 32, N = 1024, K = 20, M = 8, O = 64 / 64 / 128 / 256) against the torch composition a user would
otherwise write: gather the neighbour rows into [B, N, K, M, O], subtract the centers and contract with einsum, with
autograd for the backward.  Also one whole PAConv mirror training step (batch 32, 1024 points, dropout 0.5) on the
device op and on the composition.

Per layer: forward, backward (all three gradients) and forward + backward per call, in us, from CUDA events over
`--iters` calls after a warm-up.  Bytes: `gathered` = B*N*K*M*O*4 (the K-fold neighbour rows the forward and
grad_scores read), `compulsory` = every input read once and every output written once; the rates are those bytes
over the measured time.  The gather floor is gathered bytes at the 16.8 TB/s L2-gather rate.

    python tools/prof/prof_assign_score_withk.py [--iters 20]
Run under `rocprofv3 --kernel-trace --stats -- python ...` (with `--iters 2`) for kernel times."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddle3d_amd.ops import assign_score_withk as A  # noqa: E402
from paddle3d_amd.paconv import PAConv  # noqa: E402

L2_GATHER = 16.8e12
B, N, K, M = 32, 1024, 20, 8
WIDTHS = (64, 64, 128, 256)


def _time(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def composition(scores, points, centers, knn_idx):
    b = torch.arange(points.shape[0], device=points.device)[:, None, None]
    rows = points[b, knn_idx]  # B, N, K, M, O
    return torch.einsum("bnkmo,bnkm->bon", rows - centers[:, :, None], scores)


def inputs(O, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    s = torch.rand((B, N, K, M), device="cuda", generator=g) + 0.5
    p = torch.randn((B, N, M, O), device="cuda", generator=g)
    c = torch.randn((B, N, M, O), device="cuda", generator=g)
    x = torch.randn((B, N, 3), device="cuda", generator=g)
    idx = torch.cdist(x, x).topk(K, dim=-1, largest=False)[1]
    go = torch.randn((B, O, N), device="cuda", generator=g)
    return s, p, c, idx, go


def layer(O, iters):
    s, p, c, idx, go = inputs(O)
    sg, pg, cg = (t.clone().requires_grad_() for t in (s, p, c))
    t_fwd = _time(lambda: A.assign_score_withk(s, p, c, idx), iters)
    t_bwd = _time(lambda: A.assign_score_withk_backward(go, s, p, c, idx), iters)
    t_fb = _time(lambda: A.assign_score_withk(sg, pg, cg, idx).backward(go), iters)
    c_fwd = _time(lambda: composition(s, p, c, idx), iters)
    out = composition(sg, pg, cg, idx)
    c_bwd = _time(lambda: torch.autograd.grad(out, (sg, pg, cg), go, retain_graph=True), iters)
    c_fb = _time(lambda: composition(sg, pg, cg, idx).backward(go), iters)
    gathered = B * N * K * M * O * 4
    fwd_bytes = (2 * B * N * M * O + B * N * K * M + B * O * N) * 4 + B * N * K * 8
    bwd_bytes = fwd_bytes + 2 * B * N * M * O * 4 + B * N * K * M * 4  # + grad outputs
    return dict(O=O, fwd=t_fwd, bwd=t_bwd, fb=t_fb, torch_fwd=c_fwd, torch_bwd=c_bwd, torch_fb=c_fb,
                gathered_GB=gathered / 1e9, fwd_GB=fwd_bytes / 1e9, bwd_GB=bwd_bytes / 1e9,
                floor_us=gathered / L2_GATHER * 1e6)


def train_step(iters, use_torch):
    torch.manual_seed(0)
    model = PAConv().cuda().train()
    if use_torch:
        model.assign_score_withk = composition
    opt = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9)
    x = torch.randn((B, N, 3), device="cuda")
    y = torch.randint(0, 40, (B,), device="cuda")

    def step():
        opt.zero_grad()
        model({"data": x, "labels": y})["loss"].backward()
        opt.step()
    return _time(step, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    print(f"B={B} N={N} K={K} M={M}; times in us per call (device op | torch composition)")
    print(" O  | fwd        | bwd        | fwd+bwd      | gathered GB | fwd GB/s-compulsory | gather floor us | "
          "fwd/floor | bwd/floor")
    for O in WIDTHS:
        r = layer(O, a.iters)
        print(f"{O:3d} | {r['fwd']:7.1f} | {r['torch_fwd']:7.1f} | {r['bwd']:7.1f} | {r['torch_bwd']:7.1f} | "
              f"{r['fb']:7.1f} | {r['torch_fb']:7.1f} | {r['gathered_GB']:.2f} | "
              f"fwd {r['fwd_GB'] / r['fwd'] * 1e3:.2f} TB/s, bwd {r['bwd_GB'] / r['bwd'] * 1e3:.2f} TB/s "
              f"compulsory; gathered {r['gathered_GB'] / r['fwd'] * 1e3:.1f} TB/s fwd | {r['floor_us']:.0f} | "
              f"{r['fwd'] / r['floor_us']:.2f} | {r['bwd'] / r['floor_us']:.2f}", flush=True)
    if not a.no_step:
        print(f"training step (batch {B}, {N} points): device op {train_step(max(3, a.iters // 4), False) / 1e3:.2f} "
              f"ms, torch composition {train_step(max(3, a.iters // 4), True) / 1e3:.2f} ms", flush=True)


if __name__ == "__main__":
    main()
