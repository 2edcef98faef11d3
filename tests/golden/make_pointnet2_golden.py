"""Golden vectors for the pointnet2 batch ops and points_in_boxes from the reference's own Python, executed through
tests/golden/paddle_shim.py at small seeded shapes:

    QueryAndGroup (models/detection/iassd/iassd_modules.py:29-60)
    SAModuleMSG_WithSampling.forward (iassd_modules.py:159-241): D-FPS 2048 -> 512 with radii 0.2 / 0.8 and
        nsample 16 / 32, then ctr_aware 512 -> 128 with radius 0.8, nsample 16; the MLPs are the identity and the
        pool is max_pool (F.max_pool2d supplied here)
    roiaware_pool3d.points_in_boxes_gpu in the call form of point_head.py:198-206: points_single.unsqueeze(0) and
        gt_boxes[k:k+1, :, 0:7] of an [B, M, 8] tensor

    python tests/golden/make_pointnet2_golden.py     # needs /root/reference; writes python_pointnet2.npz

`pointnet2_ops` and `roiaware_pool3d` are bound to independent torch formulations: FPS as a plain loop whose ties are
broken by np.lexsort on (k, bitreverse(k mod bs)), ball query as a full distance matrix plus a stable selection,
grouping / gather as advanced indexing, boxes as a direct vectorised test.  Every call records what the caller hands
the op and the result.  That pins the layouts: (B, N, 3) against the flipped (B, 3, N), the centre subtraction,
the concat order under use_xyz, and 7 box columns with z at the centre.  The input cloud repeats points, as KITTI's
SamplePoint does when a frame has fewer points than it samples.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import paddle_shim as ps  # noqa: E402
import pointnet2_numpy as pn  # noqa: E402

REF = "/root/reference"
MOD = os.path.join(REF, "paddle3d/models/detection/iassd/iassd_modules.py")
QAG = (29, 60)
SA_FORWARD = (159, 241)


def _t(x):
    return x.as_subclass(torch.Tensor) if isinstance(x, torch.Tensor) else torch.as_tensor(x)


def _fps_torch(xyz, m):
    xyz = _t(xyz).float()
    B, N, _ = xyz.shape
    L = min(N.bit_length() - 1, 10)
    k = np.arange(N)
    t = k & ((1 << L) - 1)
    rev = np.array([int(format(v, f"0{L}b")[::-1], 2) if L else 0 for v in t])
    out = torch.zeros((B, m), dtype=torch.int32)
    for b in range(B):
        temp = torch.full((N,), 1e10)
        old = 0
        for j in range(1, m):
            d = xyz[b] - xyz[b, old]
            d = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            temp = torch.fmin(d, temp)
            cand = torch.nonzero(temp == temp.max()).flatten().numpy()
            old = int(cand[np.lexsort((cand, rev[cand]))[0]])
            out[b, j] = old
    return out


def _ball_torch(new_xyz, xyz, radius, nsample):
    q, p = _t(new_xyz).float(), _t(xyz).float()
    d = q[:, :, None, :] - p[:, None, :, :]  # new - x
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    hit = d2 < torch.tensor(radius, dtype=torch.float32) ** 2
    N = p.shape[1]
    # stable selection: hits first in index order
    key = torch.where(hit, torch.arange(N), N + torch.arange(N))
    order = torch.sort(key, dim=-1, stable=True).indices[..., :nsample]
    cnt = hit.sum(-1, keepdim=True)
    first = order[..., :1]
    slot = torch.arange(nsample)
    idx = torch.where(slot < cnt, order, first)
    idx = torch.where(cnt > 0, idx, torch.zeros_like(idx))
    return idx.int()


def _group_torch(points, idx):
    pts, ix = _t(points).float(), _t(idx).long()
    B, C, _ = pts.shape
    flat = ix.reshape(B, 1, -1).expand(B, C, -1)
    return torch.gather(pts, 2, flat).reshape((B, C) + tuple(ix.shape[1:]))


def _boxes_torch(pts, boxes):
    p, bx = _t(pts).float(), _t(boxes).float()
    c, s = torch.cos(-bx[..., 6]), torch.sin(-bx[..., 6])
    sx = p[:, :, None, 0] - bx[:, None, :, 0]
    sy = p[:, :, None, 1] - bx[:, None, :, 1]
    lx = sx * c[:, None] + sy * (-s[:, None])
    ly = sx * s[:, None] + sy * c[:, None]
    m = np.float64(np.float32(1e-5))
    zin = ~((p[:, :, None, 2] - bx[:, None, :, 2]).abs().double() > bx[:, None, :, 5].double() / 2.0)
    inside = zin & (lx.abs().double() < bx[:, None, :, 3].double() / 2.0 + m) & \
        (ly.abs().double() < bx[:, None, :, 4].double() / 2.0 + m)
    first = torch.where(inside.any(-1), inside.int().argmax(-1), torch.full(inside.shape[:2], -1))
    return first.int()


def main():
    p = ps.install(REF)
    import paddle.nn.functional as F

    calls = []

    def rec(name, fn):
        def op(*a):
            r = fn(*a)
            calls.append((name, [(_t(x).numpy().copy() if isinstance(x, torch.Tensor) else np.asarray(x)) for x in a],
                          r.numpy().copy()))
            return ps._wrap(r)
        return op

    pointnet2_ops = types.SimpleNamespace(
        farthest_point_sample=rec("fps", _fps_torch), gather_operation=rec("gather", _group_torch),
        ball_query_batch=rec("ball_query", _ball_torch), grouping_operation_batch=rec("group", _group_torch))
    roiaware_pool3d = types.SimpleNamespace(points_in_boxes_gpu=rec("points_in_boxes", _boxes_torch))

    def max_pool2d(x, kernel_size):
        return ps._wrap(torch.nn.functional.max_pool2d(_t(x), kernel_size=tuple(kernel_size)))

    def topk(x, k, axis=-1):
        v, i = torch.topk(_t(x), int(k), dim=int(axis))
        return ps._wrap(v), ps._wrap(i)

    Fx = types.SimpleNamespace(max_pool2d=max_pool2d, sigmoid=F.sigmoid)
    if not hasattr(p, "topk"):
        p.topk = topk
    ns = ps.exec_lines(MOD, [QAG], dict(paddle=p, nn=p.nn, F=Fx, pointnet2_ops=pointnet2_ops, List=list))
    QueryAndGroup = ns["QueryAndGroup"]
    sa = ps.exec_lines(MOD, [SA_FORWARD], dict(paddle=p, F=Fx, pointnet2_ops=pointnet2_ops))["forward"]

    rng = np.random.default_rng(7)
    B, N, C = 1, 2048, 2
    base = rng.uniform(0.0, 2.0, (B, 1536, 3)).astype(np.float32)
    dup = base[:, rng.integers(0, 1536, N - 1536)]  # SamplePoint repeats points of a short frame
    xyz_np = np.concatenate([base, dup], 1)
    feat_np = rng.standard_normal((B, C, N)).astype(np.float32)
    out = {"xyz": xyz_np, "features": feat_np}

    def layer(npoint, sample_type, radii, nsamples):
        s = types.SimpleNamespace(npoint=npoint, sample_type=sample_type,
                                  groupers=[QueryAndGroup(r, n, use_xyz=True) for r, n in zip(radii, nsamples)],
                                  mlps=[lambda x: x for _ in radii], pool_method="max_pool",
                                  aggregation_layer=None, confidence_layer=None)
        return s

    with torch.no_grad():
        xyz, feat = ps.tensor(xyz_np), ps.tensor(feat_np)
        new_xyz, new_feat, _ = sa(layer(512, "D-FPS", [0.2, 0.8], [16, 32]), xyz, feat)
        out["sa1_new_xyz"] = _t(new_xyz).numpy()
        out["sa1_new_features"] = _t(new_feat).numpy()
        cls = ps.tensor(rng.standard_normal((B, 512, 3)).astype(np.float32))
        out["sa2_cls_features"] = _t(cls).numpy()
        new_xyz2, new_feat2, _ = sa(layer(128, "ctr_aware", [0.8], [16]), new_xyz, new_feat, cls_features=cls)
        out["sa2_new_xyz"] = _t(new_xyz2).numpy()
        # one QueryAndGroup layer on its own, output recorded whole
        qag = QueryAndGroup(0.8, 16, use_xyz=True)
        out["qag_out"] = _t(qag(new_xyz, new_xyz2, new_feat)).numpy()

        # points_in_boxes as point_head.py:198-206 calls it: 8-column gt_boxes, the k-th frame's [1, M, 7] slice
        gt = np.zeros((2, 6, 8), np.float32)
        gt[..., 0:3] = rng.uniform(0.3, 1.7, (2, 6, 3))
        gt[..., 3:6] = rng.uniform(0.2, 0.9, (2, 6, 3))
        gt[..., 6] = rng.uniform(-np.pi, np.pi, (2, 6))
        gt[..., 7] = rng.integers(1, 4, (2, 6))
        gt[1, 5] = 0.0  # an all-zero padding row
        out["gt_boxes"] = gt
        gtt = ps.tensor(gt)
        for k in range(2):
            roiaware_pool3d.points_in_boxes_gpu(ps.tensor(xyz_np[0]).unsqueeze(axis=0), gtt[k:k + 1, :, 0:7])

    counts = {}
    for name, args, res in calls:
        i = counts.get(name, 0)
        counts[name] = i + 1
        for j, a in enumerate(args):
            if name in ("gather", "group") and j == 0:
                continue  # the grouped tensors are xyz / features, recorded once above
            out[f"{name}{i}_arg{j}"] = a
        if name not in ("gather", "group"):
            out[f"{name}{i}_out"] = res
        else:
            out[f"{name}{i}_src_shape"] = np.asarray(args[0].shape)
            out[f"{name}{i}_src_sum"] = np.float64(args[0].astype(np.float64).sum())
    print({k: v for k, v in counts.items()})
    # the restatement reproduces every recorded call
    for name, args, res in calls:
        if name == "fps":
            assert np.array_equal(pn.farthest_point_sample(args[0], int(args[1])), res)
        elif name == "ball_query":
            assert np.array_equal(pn.ball_query(args[0], args[1], float(args[2]), int(args[3])), res)
        elif name in ("gather", "group"):
            assert np.array_equal(pn.group(args[0], args[1]).view(np.uint32), res.view(np.uint32))
    # an array equal to one stored before it is stored as the string "@<that key>" (load() resolves it)
    packed = {}
    for key, a in out.items():
        a = np.ascontiguousarray(a)
        same = next((k for k, b in packed.items() if b.dtype == a.dtype and b.shape == a.shape and a.ndim
                     and b.tobytes() == a.tobytes()), None)
        packed[key] = np.asarray("@" + same) if same else a
    np.savez_compressed(os.path.join(HERE, "python_pointnet2.npz"), **packed)
    print(os.path.getsize(os.path.join(HERE, "python_pointnet2.npz")), "bytes")


def load(path=os.path.join(HERE, "python_pointnet2.npz")):
    """The golden file as a dict, aliases resolved."""
    z = np.load(path)
    raw = {k: z[k] for k in z.files}
    return {k: (raw[str(v)[1:]] if v.dtype.kind == "U" else v) for k, v in raw.items()}


if __name__ == "__main__":
    main()
