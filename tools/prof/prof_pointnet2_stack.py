"""Time the pointnet2 stack ops (paddle3d_amd/ops/pointnet2_ops.py, csrc/pointnet2_stack.hip) at PV-RCNN's and
Voxel R-CNN's shapes against the torch composition a user would otherwise write on the GPU:

  ball       ball_query_stack, PV-RCNN VSA: B = 2 frames of 16384 / 15000 raw points, 2048 keypoints each, radii
             0.4 / 0.8 / 2.4 / 4.8, nsample 16 / 32.  Torch: per frame a distance matrix, the hit mask and a stable
             sort of the hit keys.  Reported as queries per us.
  voxel      voxel_query_wrapper, Voxel R-CNN x_conv2: a 21 x 800 x 704 grid per frame, ~30k voxels per frame, 100 RoIs
             x 216 grid points per frame, range 4 (9 x 9 x 9 cells), radius 0.4 / 1.6, nsample 16.  Torch: the gather
             of the whole window, the hit mask, a stable sort.  Queries per us.
  group      grouping_operation_stack forward at Voxel R-CNN's x_conv2 layer (43 200 rows x C = 32 x nsample 16) and
             at a PV-RCNN raw-point layer (4096 rows x C = 4 x nsample 32), and the backward at the first shape.
             Torch: a row gather + permute (forward), index_add_ (backward).  Reported as a fraction of the 8 TB/s
             HBM peak and of the 6.29 TB/s a float4 copy reaches; the bytes are out written, idx read and each
             feature row read once (the backward: grad_out read, grad_features zeroed and added once).

Device time per call from CUDA events over `--iters` calls after a warm-up.

    python tools/prof/prof_pointnet2_stack.py [--iters 20] [--only ball voxel group]
Run under `rocprofv3 --kernel-trace --stats -- python ...` (with `--iters 2`) for kernel times."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddle3d_amd import pointnet2_stack as L  # noqa: E402
from paddle3d_amd.ops import pointnet2_ops as P  # noqa: E402

HBM = 8.0e12
HBM_COPY = 6.29e12


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


def _pick(hit, vals, nsample):
    n = hit.shape[1]
    ar = torch.arange(n, device=hit.device)
    order = torch.sort(torch.where(hit, ar, n + ar), dim=-1, stable=True).indices[:, :nsample]
    sel = torch.gather(vals, 1, order)
    cnt = hit.sum(-1, keepdim=True)
    idx = torch.where(torch.arange(nsample, device=hit.device) < cnt, sel, sel[:, :1])
    idx = torch.where(cnt > 0, idx, torch.zeros_like(idx))
    idx[:, 0] = torch.where(cnt[:, 0] > 0, idx[:, 0], torch.full_like(idx[:, 0], -1))
    return idx.int()


def torch_ball(q, qs, p, ps, radius, nsample):
    """qs / ps: per-frame row ranges known on the host (the composition needs them there)."""
    r2 = torch.tensor(radius, device=q.device) ** 2
    out = []
    for (q0, q1), (p0, p1) in zip(qs, ps):
        d = q[q0:q1, None, :] - p[None, p0:p1, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        hit = d2 < r2
        out.append(_pick(hit, torch.arange(p1 - p0, device=q.device).expand(hit.shape), nsample))
    return torch.cat(out)


def torch_voxel(q, p, co, pi, radius, nsample, rz, ry, rx):
    B, Z, Y, X = pi.shape
    dz, dy, dx = torch.meshgrid(*[torch.arange(-r, r + 1, device=q.device) for r in (rz, ry, rx)], indexing="ij")
    z, y, x = co[:, 1:2] + dz.reshape(1, -1), co[:, 2:3] + dy.reshape(1, -1), co[:, 3:4] + dx.reshape(1, -1)
    b = co[:, :1].expand_as(z)
    ok = (b >= 0) & (b < B) & (z >= 0) & (z < Z) & (y >= 0) & (y < Y) & (x >= 0) & (x < X)
    ni = torch.where(ok, pi[b.clamp(0, B - 1), z.clamp(0, Z - 1), y.clamp(0, Y - 1), x.clamp(0, X - 1)], -1)
    ok &= ni >= 0
    d = p[ni.clamp(min=0).long()] - q[:, None, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    r2 = torch.tensor(radius, device=q.device) ** 2
    return _pick(ok & ~(d2 > r2), ni, nsample)


def pv_scene():
    g = torch.Generator(device="cuda").manual_seed(0)
    lo = torch.tensor([0.0, -40.0, -3.0], device="cuda")
    hi = torch.tensor([70.4, 40.0, 1.0], device="cuda")
    p = lo + torch.rand((31384, 3), device="cuda", generator=g) * (hi - lo)
    pick = torch.cat([torch.randperm(16384, device="cuda", generator=g)[:2048],
                      16384 + torch.randperm(15000, device="cuda", generator=g)[:2048]])
    q = p[pick] + 0.3 * torch.randn((4096, 3), device="cuda", generator=g)
    qc = torch.tensor([2048, 2048], dtype=torch.int32, device="cuda")
    pc = torch.tensor([16384, 15000], dtype=torch.int32, device="cuda")
    return q.contiguous(), qc, p.contiguous(), pc


def voxel_scene():
    g = torch.Generator(device="cuda").manual_seed(1)
    Z, Y, X = 21, 800, 704
    ind, rois = [], []
    for b in range(2):
        c = torch.stack([torch.randint(2, Z - 2, (160,), device="cuda", generator=g),
                         torch.randint(20, Y - 20, (160,), device="cuda", generator=g),
                         torch.randint(20, X - 20, (160,), device="cuda", generator=g)], 1)
        sd = torch.tensor([2.0, 8.0, 8.0], device="cuda")
        cells = c[torch.randint(0, 160, (36000,), device="cuda", generator=g)] + \
            torch.round(torch.randn((36000, 3), device="cuda", generator=g) * sd).long()
        cells = torch.minimum(cells.clamp(min=0), torch.tensor([Z - 1, Y - 1, X - 1], device="cuda"))
        flat = torch.unique((cells[:, 0] * Y + cells[:, 1]) * X + cells[:, 2])
        flat = torch.sort(flat[torch.randperm(flat.numel(), device="cuda", generator=g)][:30000 - 1500 * b]).values
        ind.append(torch.stack([torch.full_like(flat, b), flat // (Y * X), flat // X % Y, flat % X], 1))
        rois.append(c[:100])
    ind = torch.cat(ind).int().contiguous()
    vs, lo = torch.tensor([0.1, 0.1, 0.2], device="cuda"), torch.tensor([0.0, -40.0, -3.0], device="cuda")
    xyz = ((ind[:, [3, 2, 1]].float() + 0.5) * vs + lo).contiguous()
    lin = torch.linspace(-1.2, 1.2, 6, device="cuda")
    grid = torch.stack(torch.meshgrid(lin, lin, lin, indexing="ij"), -1).reshape(-1, 3)
    new_xyz = torch.cat([(((r[:, [2, 1, 0]].float() + 0.5) * vs + lo)[:, None] + grid[None]).reshape(-1, 3)
                         for r in rois]).contiguous()
    b = torch.arange(2, device="cuda").repeat_interleave(100 * 216)[:, None]
    cxyz = torch.floor((new_xyz - lo) / vs).long()
    new_coords = torch.cat([b, cxyz[:, [2, 1, 0]]], 1).int().contiguous()
    pinds = L.generate_voxel2pinds([2, Z, Y, X, 32], ind)
    cnt = torch.bincount(ind[:, 0].long(), minlength=2).int()
    return xyz, cnt, new_xyz, new_coords, pinds


def run_ball(iters):
    q, qc, p, pc = pv_scene()
    qs, ps = [(0, 2048), (2048, 4096)], [(0, 16384), (16384, 31384)]
    print("ball_query_stack  PV-RCNN VSA, B = 2 (16384 / 15000 points, 2 x 2048 keypoints)")
    print(f"  {'radius':>6} {'ns':>3} {'device us':>10} {'q/us':>7} {'torch us':>10} {'speed-up':>8}  equal")
    for radius, ns in ((0.4, 16), (0.8, 32), (2.4, 16), (4.8, 32)):
        f = lambda: P.ball_query_stack(q, qc, p, pc, radius, ns)  # noqa: E731
        ft = lambda: torch_ball(q, qs, p, ps, radius, ns)  # noqa: E731
        t, tt = _time(f, iters), _time(ft, max(1, iters // 4))
        print(f"  {radius:6.1f} {ns:3d} {t:10.1f} {4096 / t:7.1f} {tt:10.1f} {tt / t:8.1f}  {torch.equal(f(), ft())}")


def run_voxel(iters):
    xyz, cnt, new_xyz, new_coords, pinds = voxel_scene()
    M = int(new_xyz.shape[0])
    print(f"voxel_query  Voxel R-CNN x_conv2, B = 2, grid 21 x 800 x 704, {int(cnt.sum())} voxels, {M} queries, "
          "range 4")
    print(f"  {'radius':>6} {'ns':>3} {'device us':>10} {'q/us':>7} {'torch us':>10} {'speed-up':>8}  equal")
    for radius in (0.4, 1.6):
        f = lambda: P.voxel_query_wrapper(new_xyz, xyz, new_coords, pinds, radius, 16, 4, 4, 4)  # noqa: E731
        ft = lambda: torch_voxel(new_xyz, xyz, new_coords, pinds, radius, 16, 4, 4, 4)  # noqa: E731
        t, tt = _time(f, iters), _time(ft, max(1, iters // 4))
        print(f"  {radius:6.1f} {16:3d} {t:10.1f} {M / t:7.1f} {tt:10.1f} {tt / t:8.1f}  {torch.equal(f(), ft())}")


def run_group(iters):
    print("grouping_operation_stack")
    print(f"  {'shape':<30} {'device us':>10} {'MB':>7} {'of 8 TB/s':>9} {'of copy':>8} {'torch us':>9} equal")
    g = torch.Generator(device="cuda").manual_seed(2)
    for name, N, C, M, S in (("x_conv2 fwd 43200 x 32 x 16", 58500, 32, 43200, 16),
                             ("raw fwd 4096 x 4 x 32", 31384, 4, 4096, 32)):
        feat = torch.randn((N, C), device="cuda", generator=g)
        fc = torch.tensor([N // 2, N - N // 2], dtype=torch.int32, device="cuda")
        ic = torch.tensor([M // 2, M - M // 2], dtype=torch.int32, device="cuda")
        idx = torch.randint(0, N // 2, (M, S), device="cuda", generator=g, dtype=torch.int32)
        start = torch.cat([torch.zeros(M // 2, device="cuda", dtype=torch.long),
                           torch.full((M - M // 2,), N // 2, device="cuda", dtype=torch.long)])
        rows = (start[:, None] + idx).reshape(-1)
        f = lambda: P.grouping_operation_stack(feat, fc, idx, ic)  # noqa: E731
        ft = lambda: feat[rows].view(M, S, C).permute(0, 2, 1).contiguous()  # noqa: E731
        t, tt = _time(f, iters), _time(ft, iters)
        nbytes = M * C * S * 4 + M * S * 4 + N * C * 4
        print(f"  {name:<30} {t:10.1f} {nbytes / 1e6:7.1f} {nbytes / t * 1e6 / HBM:9.0%} "
              f"{nbytes / t * 1e6 / HBM_COPY:8.0%} {tt:9.1f} {torch.equal(f(), ft())}")
        if C == 32:
            go = torch.randn((M, C, S), device="cuda", generator=g)
            fb = lambda: P.grouping_operation_stack_grad(go, fc, idx, ic, N)  # noqa: E731
            fbt = lambda: torch.zeros((N, C), device="cuda").index_add_(  # noqa: E731
                0, rows, go.permute(0, 2, 1).reshape(-1, C))
            t, tt = _time(fb, iters), _time(fbt, iters)
            nbytes = M * C * S * 4 + M * S * 4 + N * C * 4 * 2
            print(f"  {'x_conv2 bwd 43200 x 32 x 16':<30} {t:10.1f} {nbytes / 1e6:7.1f} "
                  f"{nbytes / t * 1e6 / HBM:9.0%} {nbytes / t * 1e6 / HBM_COPY:8.0%} {tt:9.1f} "
                  f"{torch.allclose(fb(), fbt(), atol=1e-4)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", nargs="*", default=["ball", "voxel", "group"])
    a = ap.parse_args()
    for name in a.only:
        {"ball": run_ball, "voxel": run_voxel, "group": run_group}[name](a.iters)


if __name__ == "__main__":
    main()
