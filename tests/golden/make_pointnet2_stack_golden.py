"""Golden vectors for the pointnet2 stack ops from the reference's own Python, executed through
tests/golden/paddle_shim.py at small seeded shapes:

    QueryAndGroup (models/common/pointnet2_stack/pointnet2_utils.py:27-89)
    build_local_aggregation_module + StackSAModuleMSG (pointnet2_modules.py:31-157), forward with radii 0.5 / 1.0,
        nsample 16 / 32, max_pool: PV-RCNN's RoI-grid and VSA layer form
    voxel_query + VoxelQueryAndGrouping (voxel_query_utils.py:28-106)
    NeighborVoxelSAModuleMSG (voxel_pool_modules.py:29-163), query ranges (2, 2, 2) and (1, 2, 3): Voxel R-CNN's form
    generate_voxel2pinds (models/common/box_utils.py:102-110)

    python tests/golden/make_pointnet2_stack_golden.py     # needs /root/reference; writes python_pointnet2_stack.npz

`pointnet2_ops` is bound to independent torch formulations: the ball query as a per-frame full distance matrix with
a stable selection, the voxel query as a gather of the whole window in (dz, dy, dx) order with a stable selection,
grouping as advanced indexing from per-frame starts.  What the shim lacks (Conv1D, max_pool2d / avg_pool2d with
kernel_size=, scatter_nd, the weight initialisers) is supplied here.  Every op call records what the caller hands
the op and the result; the layers' outputs and the seeded weights are recorded too.  The inputs hold two frames of
unequal size, repeated points, grid points outside the voxel grid, empty balls and points at exactly d2 == r2.
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
import pointnet2_stack_numpy as pn  # noqa: E402

REF = "/root/reference"
STACK = os.path.join(REF, "paddle3d/models/common/pointnet2_stack")
UTILS, MODULES = os.path.join(STACK, "pointnet2_utils.py"), os.path.join(STACK, "pointnet2_modules.py")
VQ_UTILS, VQ_MODULES = os.path.join(STACK, "voxel_query_utils.py"), os.path.join(STACK, "voxel_pool_modules.py")
BOX_UTILS = os.path.join(REF, "paddle3d/models/common/box_utils.py")

VOXEL = 0.25  # voxel edge: centres (i + 0.5) * 0.25 are exact in fp32
GRID = (2, 4, 12, 12)  # B, Z, Y, X


def _t(x):
    return x.as_subclass(torch.Tensor) if isinstance(x, torch.Tensor) else torch.as_tensor(x)


def _frame_rows(m, cnt):
    """Rows of each frame by the reference's scan, written as the loop it is."""
    cnt = [int(c) for c in cnt]
    out = []
    for r in range(m):
        b, run = 0, cnt[0]
        for k in range(1, len(cnt)):
            if r < run:
                break
            run += cnt[k]
            b = k
        out.append(b)
    return out


def _pick(hit, vals, nsample):
    """Stable selection of the first nsample hits per row, fill with the first, [-1, 0, ...] without a hit."""
    L = hit.shape[1]
    key = torch.where(hit, torch.arange(L), L + torch.arange(L))
    order = torch.sort(key, dim=-1, stable=True).indices
    sel = torch.gather(vals, 1, order[:, :nsample]) if L else torch.zeros((hit.shape[0], 0), dtype=vals.dtype)
    if sel.shape[1] < nsample:
        sel = torch.cat([sel, torch.zeros((hit.shape[0], nsample - sel.shape[1]), dtype=vals.dtype)], 1)
    cnt = hit.sum(-1, keepdim=True)
    idx = torch.where(torch.arange(nsample) < cnt, sel, sel[:, :1])
    idx = torch.where(cnt > 0, idx, torch.zeros_like(idx))
    idx[:, 0] = torch.where(cnt[:, 0] > 0, idx[:, 0], torch.full_like(idx[:, 0], -1))
    return idx.int()


def _ball_stack_torch(new_xyz, new_cnt, xyz, xyz_cnt, radius, nsample):
    q, p = _t(new_xyz).float(), _t(xyz).float()
    nc, pc = [int(c) for c in _t(new_cnt)], [int(c) for c in _t(xyz_cnt)]
    r2 = torch.tensor(radius, dtype=torch.float32) ** 2
    frame = _frame_rows(q.shape[0], nc)
    starts = np.concatenate([[0], np.cumsum(pc)])
    out = torch.zeros((q.shape[0], int(nsample)), dtype=torch.int32)
    for b in sorted(set(frame)):
        rows = torch.tensor([r for r, f in enumerate(frame) if f == b])
        pts = p[starts[b]:starts[b + 1]]
        d = q[rows][:, None, :] - pts[None, :, :]  # new - x
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        hit = d2 < r2
        out[rows] = _pick(hit, torch.arange(pts.shape[0]).expand(hit.shape), int(nsample))
    return out


def _voxel_torch(new_xyz, xyz, new_coords, point_indices, radius, nsample, z_range, y_range, x_range):
    q, p = _t(new_xyz).float(), _t(xyz).float()
    co, pi = _t(new_coords).long(), _t(point_indices).long()
    B, Z, Y, X = pi.shape
    r2 = torch.tensor(radius, dtype=torch.float32) ** 2
    dz, dy, dx = torch.meshgrid(torch.arange(-z_range, z_range + 1), torch.arange(-y_range, y_range + 1),
                                torch.arange(-x_range, x_range + 1), indexing="ij")
    z = co[:, 1:2] + dz.reshape(1, -1)
    y = co[:, 2:3] + dy.reshape(1, -1)
    x = co[:, 3:4] + dx.reshape(1, -1)
    b = co[:, 0:1].expand_as(z)
    ok = (b >= 0) & (b < B) & (z >= 0) & (z < Z) & (y >= 0) & (y < Y) & (x >= 0) & (x < X)
    ni = torch.where(ok, pi[b.clamp(0, B - 1), z.clamp(0, Z - 1), y.clamp(0, Y - 1), x.clamp(0, X - 1)], -1)
    ok &= (ni >= 0) & (ni < p.shape[0])
    d = p[ni.clamp(min=0)] - q[:, None, :]  # x_per - new_x
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    hit = ok & ~(d2 > r2)
    return _pick(hit, ni, int(nsample))


def _group_stack_torch(features, features_cnt, idx, idx_cnt):
    ft, ix = _t(features).float(), _t(idx).long()
    fc = [int(c) for c in _t(features_cnt)]
    starts = torch.tensor(np.concatenate([[0], np.cumsum(fc)])[:-1])
    g = starts[torch.tensor(_frame_rows(ix.shape[0], _t(idx_cnt)))][:, None] + ix
    ok = (g >= 0) & (g < ft.shape[0])
    vals = ft[g.clamp(0, max(ft.shape[0] - 1, 0))]
    return torch.where(ok[..., None], vals, torch.zeros(())).permute(0, 2, 1).contiguous()


def pv_inputs(rng):
    """Two frames of 300 / 200 points (60 / 40 of them repeats), 40 / 24 keypoints, C = 4 features."""
    frames, cents = [], []
    for n, m in ((300, 40), (200, 24)):
        base = rng.uniform(0.0, 2.0, (n - n // 5, 3)).astype(np.float32)
        pts = np.concatenate([base, base[rng.integers(0, len(base), n // 5)]])
        frames.append(pts)
        cents.append(rng.uniform(0.0, 2.0, (m, 3)).astype(np.float32))
    # frame 1: a keypoint with one point at exactly radius 0.5 (d2 == r2 == 0.25): empty at 0.5, a hit at 1.0
    frames[1][-1] = (5.5, 5.0, 5.0)
    cents[1][3] = (5.0, 5.0, 5.0)
    cents[0][5] = (10.0, 10.0, 10.0)  # an empty ball at every radius
    return dict(pv_xyz=np.concatenate(frames), pv_xyz_cnt=np.array([300, 200], np.int32),
                pv_new_xyz=np.concatenate(cents), pv_new_cnt=np.array([40, 24], np.int32),
                pv_features=rng.standard_normal((500, 4)).astype(np.float32))


def voxel_inputs(rng):
    """Sparse voxels of two frames (100 / 70 cells of a 4 x 12 x 12 grid) at their centres, 16 grid points each."""
    B, Z, Y, X = GRID
    ind = []
    for b, n in ((0, 100), (1, 70)):
        cells = np.sort(rng.choice(Z * Y * X, n, replace=False))
        z, y, x = np.unravel_index(cells, (Z, Y, X))
        ind.append(np.stack([np.full(n, b), z, y, x], 1))
    ind = np.concatenate(ind).astype(np.int32)
    xyz = ((ind[:, [3, 2, 1]].astype(np.float32) + 0.5) * VOXEL).astype(np.float32)
    lo, hi = np.array([-0.3, -0.3, -0.2], np.float32), np.array([3.3, 3.3, 1.2], np.float32)
    new_xyz = (lo + rng.random((32, 3), dtype=np.float32) * (hi - lo)).astype(np.float32)  # some outside the grid
    new_xyz[0] = xyz[7] + np.array([0.5, 0.0, 0.0], np.float32)  # exactly radius 0.5 from voxel 7 (a hit)
    new_xyz[20] = (10.0, 10.0, 10.0)  # the window misses the grid: an empty ball
    b = np.repeat(np.arange(2), 16)[:, None]
    new_coords = np.concatenate([b, np.floor(new_xyz / VOXEL)], 1).astype(np.int32)  # (b, x, y, z)
    return dict(vx_indices=ind, vx_xyz=xyz, vx_xyz_cnt=np.array([100, 70], np.int32),
                vx_features=rng.standard_normal((170, 4)).astype(np.float32), vx_new_xyz=new_xyz,
                vx_new_cnt=np.array([16, 16], np.int32), vx_new_coords=new_coords)


def main():
    p = ps.install(REF)
    calls = []

    def rec(name, fn):
        def op(*a):
            r = fn(*a)
            calls.append((name, [(_t(x).numpy().copy() if isinstance(x, torch.Tensor) else np.asarray(x)) for x in a],
                          r.numpy().copy()))
            return ps._wrap(r)
        return op

    pointnet2_ops = types.SimpleNamespace(ball_query_stack=rec("ball_query", _ball_stack_torch),
                                          voxel_query_wrapper=rec("voxel_query", _voxel_torch),
                                          grouping_operation_stack=rec("group", _group_stack_torch))

    class Conv1D(p.nn.Layer):
        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias_attr=None, **_):
            super().__init__()
            self.weight = torch.nn.Parameter(torch.zeros((out_channels, in_channels, kernel_size)))
            self.bias = None if bias_attr is False else torch.nn.Parameter(torch.zeros(out_channels))
            self._s, self._p = stride, padding

        def forward(self, x):
            return torch.nn.functional.conv1d(_t(x), self.weight, self.bias, self._s, self._p)

    nnx = types.ModuleType("nn")
    nnx.__dict__.update({k: v for k, v in vars(p.nn).items() if not k.startswith("__")})
    nnx.Conv1D = Conv1D
    Fx = types.SimpleNamespace(
        max_pool2d=lambda x, kernel_size: ps._wrap(torch.nn.functional.max_pool2d(_t(x), tuple(kernel_size))),
        avg_pool2d=lambda x, kernel_size: ps._wrap(torch.nn.functional.avg_pool2d(_t(x), tuple(kernel_size))))
    if not hasattr(p, "scatter_nd"):
        def scatter_nd(index, updates, shape):
            out = torch.zeros(tuple(int(s) for s in shape), dtype=_t(updates).dtype)
            out.index_put_(tuple(_t(index).long().unbind(-1)), _t(updates), accumulate=True)
            return ps._wrap(out)
        p.scatter_nd = scatter_nd
    noop = lambda *a, **k: None  # noqa: E731  (weights are seeded by ps.fill_state below)
    base = dict(paddle=p, nn=nnx, F=Fx, pointnet2_ops=pointnet2_ops, List=list, constant_init=noop,
                kaiming_normal_init=noop)
    utils = ps.exec_lines(UTILS, [(27, 89)], dict(base))
    mods = ps.exec_lines(MODULES, [(31, 157)],
                         dict(base, pointnet2_utils=types.SimpleNamespace(QueryAndGroup=utils["QueryAndGroup"])))
    vq = ps.exec_lines(VQ_UTILS, [(28, 106)], dict(base))
    vmods = ps.exec_lines(VQ_MODULES, [(29, 163)], dict(
        base, voxel_query_utils=types.SimpleNamespace(VoxelQueryAndGrouping=vq["VoxelQueryAndGrouping"])))
    v2p = ps.exec_lines(BOX_UTILS, [(102, 110)], dict(paddle=p))["generate_voxel2pinds"]

    rng = np.random.default_rng(11)
    out = {}
    out.update(pv_inputs(rng))
    out.update(voxel_inputs(rng))
    T = lambda k: ps.tensor(out[k])  # noqa: E731

    with torch.no_grad():
        # PV-RCNN: one QueryAndGroup on its own, then build_local_aggregation_module + StackSAModuleMSG.forward
        new_features, idx = utils["QueryAndGroup"](0.5, 16, use_xyz=True)(
            T("pv_xyz"), T("pv_xyz_cnt"), T("pv_new_xyz"), T("pv_new_cnt"), T("pv_features"))
        out["qag_out"], out["qag_idx"] = _t(new_features).numpy(), _t(idx).numpy()
        config = {"mlps": [[8, 16], [8, 8]], "pool_radius": [0.5, 1.0], "nsample": [16, 32]}
        sa, c_out = mods["build_local_aggregation_module"](4, config)
        sa.eval()
        shapes = ps.fill_state(sa, 21)
        out["sa_c_out"] = np.int64(c_out)
        for k in shapes:
            out[f"sa_state/{k}"] = sa.state_dict()[k].numpy().copy()
        _, nf = sa(T("pv_xyz"), T("pv_xyz_cnt"), T("pv_new_xyz"), T("pv_new_cnt"), T("pv_features"))
        out["sa_new_features"] = _t(nf).numpy()

        # Voxel R-CNN: the voxel-to-row map, voxel_query, VoxelQueryAndGrouping, NeighborVoxelSAModuleMSG
        pinds = v2p(list(GRID) + [4], T("vx_indices"))
        out["voxel2pinds"] = _t(pinds).numpy()
        coords_bzyx = ps.tensor(out["vx_new_coords"][:, [0, 3, 2, 1]])
        idx, empty = vq["voxel_query"]([2, 2, 2], 0.5, 16, T("vx_xyz"), T("vx_new_xyz"), coords_bzyx, pinds)
        out["vq_idx"], out["vq_empty"] = _t(idx).numpy(), _t(empty).numpy()
        gf, gx, empty = vq["VoxelQueryAndGrouping"]([1, 2, 3], 1.0, 8)(
            coords_bzyx, T("vx_xyz"), T("vx_xyz_cnt"), T("vx_new_xyz"), T("vx_new_cnt"), T("vx_features"), pinds)
        out["vqg_features"], out["vqg_xyz"], out["vqg_empty"] = (_t(gf).numpy(), _t(gx).numpy(),
                                                                 _t(empty).numpy())
        nv = vmods["NeighborVoxelSAModuleMSG"](query_ranges=[[2, 2, 2], [1, 2, 3]], radii=[0.5, 1.0],
                                               nsamples=[16, 8], mlps=[[4, 8, 8], [4, 8, 16]], use_xyz=True,
                                               pool_method="max_pool")
        nv.eval()
        shapes = ps.fill_state(nv, 22)
        for k in shapes:
            out[f"nv_state/{k}"] = nv.state_dict()[k].numpy().copy()
        out["nv_out"] = _t(nv(T("vx_xyz"), T("vx_xyz_cnt"), T("vx_new_xyz"), T("vx_new_cnt"), T("vx_new_coords"),
                              T("vx_features"), pinds)).numpy()

    counts = {}
    for name, args, res in calls:
        i = counts.get(name, 0)
        counts[name] = i + 1
        for j, a in enumerate(args):
            out[f"{name}{i}_arg{j}"] = a
        out[f"{name}{i}_out"] = res
    print(counts)
    # the restatement reproduces every recorded call
    for name, args, res in calls:
        if name == "ball_query":
            got = pn.ball_query_stack(*args[:4], float(args[4]), int(args[5]))
        elif name == "voxel_query":
            got = pn.voxel_query(*args[:4], float(args[4]), *(int(a) for a in args[5:]))
        else:
            got = pn.group_stack(*args)
        assert np.array_equal(got.view(np.uint32), res.view(np.uint32)), name
    # an array equal to one stored before it is stored as the string "@<that key>" (load() resolves it)
    packed = {}
    for key, a in out.items():
        a = np.ascontiguousarray(a)
        same = next((k for k, b in packed.items() if b.dtype == a.dtype and b.shape == a.shape and a.ndim
                     and b.tobytes() == a.tobytes()), None)
        packed[key] = np.asarray("@" + same) if same else a
    np.savez_compressed(os.path.join(HERE, "python_pointnet2_stack.npz"), **packed)
    print(os.path.getsize(os.path.join(HERE, "python_pointnet2_stack.npz")), "bytes")


def load(path=os.path.join(HERE, "python_pointnet2_stack.npz")):
    """The golden file as a dict, aliases resolved."""
    z = np.load(path)
    raw = {k: z[k] for k in z.files}
    return {k: (raw[str(v)[1:]] if v.dtype.kind == "U" else v) for k, v in raw.items()}


def state(g, prefix):
    """The recorded Paddle state dict of a layer ("sa" or "nv")."""
    head = prefix + "_state/"
    return {k[len(head):]: v for k, v in g.items() if k.startswith(head)}


if __name__ == "__main__":
    main()
