"""The NumPy restatement of the pointnet2 stack ops (tests/golden/pointnet2_stack_numpy.py) against what the
reference's PV-RCNN / Voxel R-CNN Python hands the ops and gets back (tests/golden/python_pointnet2_stack.npz), against
a literal per-row transcription of the reference kernels on the edge cases, and the layers of
paddle3d_amd/pointnet2_stack.py run on the CPU over the restatement (their index bookkeeping, masks and MLPs)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_pointnet2_stack_golden as mk  # noqa: E402
import pointnet2_stack_numpy as pn  # noqa: E402

F32 = np.float32


@pytest.fixture(scope="module")
def golden():
    return mk.load()


def _s(a):
    return np.asarray(a).reshape(-1)[0]


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- literal transcriptions of the reference kernels, one row at a time --------------------------------------------
def ref_frame(row, cnt):
    b, run = 0, int(cnt[0])
    for k in range(1, len(cnt)):
        if row < run:
            break
        run += int(cnt[k])
        b = k
    return b


def ref_ball_row(row, new_xyz, new_cnt, xyz, xyz_cnt, radius, nsample):
    """ball_query_gpu_stack.cu:36-79 for consistent counts."""
    b = ref_frame(row, new_cnt)
    start = sum(int(c) for c in xyz_cnt[:b])
    r2 = F32(F32(radius) * F32(radius))
    nx, ny, nz = new_xyz[row]
    idx = [0] * nsample
    cnt = 0
    with np.errstate(invalid="ignore"):
        for k in range(int(xyz_cnt[b])):
            x, y, z = xyz[start + k]
            d2 = F32(F32(F32((nx - x) * (nx - x)) + F32((ny - y) * (ny - y))) + F32((nz - z) * (nz - z)))
            if d2 < r2:
                if cnt == 0:
                    idx = [k] * nsample
                idx[cnt] = k
                cnt += 1
                if cnt >= nsample:
                    break
    if cnt == 0:
        idx[0] = -1
    return idx


def ref_voxel_row(row, new_xyz, xyz, new_coords, pi, radius, nsample, zr, yr, xr):
    """voxel_query_gpu.cu:21-86 for in-range batch and point indices."""
    R1, R2, R3 = pi.shape[1:]
    r2 = F32(F32(radius) * F32(radius))
    nx, ny, nz = new_xyz[row]
    b, cz, cy, cx = (int(v) for v in new_coords[row])
    idx = [0] * nsample
    cnt = 0
    with np.errstate(invalid="ignore"):
        for dz in range(-zr, zr + 1):
            z = cz + dz
            if z < 0 or z >= R1:
                continue
            for dy in range(-yr, yr + 1):
                y = cy + dy
                if y < 0 or y >= R2:
                    continue
                for dx in range(-xr, xr + 1):
                    x = cx + dx
                    if x < 0 or x >= R3:
                        continue
                    ni = int(pi[b, z, y, x])
                    if ni < 0:
                        continue
                    px, py, pz = xyz[ni]
                    d2 = F32(F32(F32((px - nx) * (px - nx)) + F32((py - ny) * (py - ny))) + F32((pz - nz) * (pz - nz)))
                    if d2 > r2:
                        continue
                    if cnt < nsample:
                        if cnt == 0:
                            idx = [ni] * nsample
                        idx[cnt] = ni
                        cnt += 1
    if cnt == 0:
        idx[0] = -1
    return idx


# ---- the recorded calls and layer outputs ---------------------------------------------------------------------------
def test_restatement_equals_recorded_calls(golden):
    g = golden
    n = {"ball_query": 0, "voxel_query": 0, "group": 0}
    for key in g:
        for name in n:
            if key.startswith(name) and key.endswith("_out") and key[len(name):-4].isdigit():
                n[name] += 1
    assert n == {"ball_query": 3, "voxel_query": 4, "group": 12}
    for i in range(n["ball_query"]):
        a = [g[f"ball_query{i}_arg{j}"] for j in range(6)]
        assert np.array_equal(pn.ball_query_stack(*a[:4], float(_s(a[4])), int(_s(a[5]))), g[f"ball_query{i}_out"])
    for i in range(n["voxel_query"]):
        a = [g[f"voxel_query{i}_arg{j}"] for j in range(9)]
        got = pn.voxel_query(*a[:4], float(_s(a[4])), *(int(_s(v)) for v in a[5:]))
        assert np.array_equal(got, g[f"voxel_query{i}_out"]), i
    for i in range(n["group"]):
        a = [g[f"group{i}_arg{j}"] for j in range(4)]
        assert np.array_equal(_bits(pn.group_stack(*a)), _bits(g[f"group{i}_out"])), i


def test_golden_covers_the_edges(golden):
    g = golden
    bq0, bq2 = g["ball_query0_out"], g["ball_query2_out"]
    # keypoint 3 of frame 1 has one point at exactly d2 == r2 = 0.25: no hit at radius 0.5, a hit at 1.0
    assert bq0[43].tolist()[:3] == [-1, 0, 0] and bq2[43, 0] == 199 and (bq2[43] == 199).all()
    assert bq0[5, 0] == -1 and bq2[5, 0] == -1  # the far keypoint: empty at every radius
    assert (bq2[:, -1] != bq2[:, 0]).any() and ((bq0[:, -1] == bq0[:, 0]) & (bq0[:, 0] >= 0)).any()  # full, filled
    # the voxel query counts the point at exactly d2 == r2 (voxel 7, first in window order) as a hit
    assert g["voxel_query0_out"][0, 0] == 7
    assert g["vq_empty"][20] and g["vqg_empty"][20]
    nc = g["vx_new_coords"]
    assert ((nc[:, 1:] < 0) | (nc[:, 1:] >= np.array([12, 12, 4]))).any()  # grid points outside the grid
    assert len(np.unique(g["pv_xyz"][:300], axis=0)) < 300  # repeated points
    assert g["pv_xyz_cnt"].tolist() == [300, 200] and g["vx_xyz_cnt"].tolist() == [100, 70]


# ---- edge rules against the literal transcription ------------------------------------------------------------------
def test_ball_query_edge_rules():
    rng = np.random.default_rng(1)
    p = rng.uniform(-1, 1, (50, 3)).astype(F32)
    q = rng.uniform(-1, 1, (30, 3)).astype(F32)
    p[4], q[0] = (0.5, 0.0, 0.0), (0.0, 0.0, 0.0)  # d2 == r2
    p[7] = (np.nan, 0.0, 0.0)
    p[8] = p[9] = (0.1, 0.1, 0.1)  # a repeated point
    for qc, pc in (([10, 20], [25, 25]), ([10, 0, 20], [20, 0, 30]), ([0, 30], [10, 40]), ([5, 5], [25, 25])):
        for nsample in (1, 4, 60):
            got = pn.ball_query_stack(q, qc, p, pc, 0.5, nsample)
            want = [ref_ball_row(r, q, qc, p, pc, 0.5, nsample) for r in range(len(q))]
            assert np.array_equal(got, np.array(want, np.int32)), (qc, pc, nsample)
    # the boundary is no hit, the NaN point is never a hit
    assert 4 not in pn.ball_query_stack(q[:1], [1], p, [50], 0.5, 50)[0].tolist()
    assert 7 not in pn.ball_query_stack(np.zeros((1, 3), F32), [1], p, [50], 10.0, 50)[0].tolist()
    # rows past the total count go to the last frame
    f = pn.frames(30, [5, 5])
    assert f[:5].tolist() == [0] * 5 and (f[5:] == 1).all()
    assert pn.frames(6, [0, 2, 0, 3]).tolist() == [1, 1, 3, 3, 3, 3]
    assert pn.frames(3, [4]).tolist() == [0, 0, 0]


def test_ball_query_fill_and_clamp():
    p = np.array([[0, 0, 0], [9, 9, 9], [0.1, 0, 0], [9, 9, 9], [0.2, 0, 0]], F32)
    got = pn.ball_query_stack(np.zeros((2, 3), F32), [1, 1], p, [5, 0], 0.5, 5)
    assert got[0].tolist() == [0, 2, 4, 0, 0] and got[1].tolist() == [-1, 0, 0, 0, 0]
    # a frame reaching past xyz is clamped to it; a negative count reads as 0
    got = pn.ball_query_stack(np.zeros((2, 3), F32), [1, 1], p, [-3, 9], 0.5, 4)
    assert got[0].tolist() == [-1, 0, 0, 0] and got[1].tolist() == [0, 2, 4, 0]


def test_voxel_query_edge_rules():
    rng = np.random.default_rng(2)
    grid = np.full((2, 4, 5, 6), -1, np.int32)
    cells = rng.choice(2 * 4 * 5 * 6, 70, replace=False)
    grid.reshape(-1)[cells] = rng.permutation(70)
    xyz = rng.uniform(0, 1.5, (70, 3)).astype(F32)
    xyz[3] = (np.nan, 0, 0)
    new_xyz = rng.uniform(0, 1.5, (25, 3)).astype(F32)
    co = np.concatenate([rng.integers(0, 2, (25, 1)), rng.integers(-1, 5, (25, 1)), rng.integers(-1, 6, (25, 1)),
                         rng.integers(-1, 7, (25, 1))], 1).astype(np.int32)
    for rngs in ((1, 1, 1), (0, 2, 1), (2, 0, 3), (3, 3, 3)):
        for nsample in (1, 5, 40):
            got = pn.voxel_query(new_xyz, xyz, co, grid, 0.6, nsample, *rngs)
            want = [ref_voxel_row(r, new_xyz, xyz, co, grid, 0.6, nsample, *rngs) for r in range(25)]
            assert np.array_equal(got, np.array(want, np.int32)), (rngs, nsample)
    # hit order is dz, then dy, then dx; the surface and NaN are hits; out-of-range b and indices are skipped
    g = np.full((1, 3, 3, 3), -1, np.int32)
    g[0, 0, 1, 1], g[0, 1, 0, 2], g[0, 1, 1, 0], g[0, 2, 1, 1], g[0, 1, 2, 1] = 0, 1, 2, 3, 9
    pts = np.array([[0, 0, 0.5], [0, 0, 0], [0, 0, 0], [np.nan, 0, 0]], F32)
    one = np.zeros((1, 3), F32)
    assert pn.voxel_query(one, pts, [[0, 1, 1, 1]], g, 0.5, 5, 1, 1, 1)[0].tolist() == [0, 1, 2, 3, 0]
    assert pn.voxel_query(one, pts, [[1, 1, 1, 1]], g, 0.5, 3, 1, 1, 1)[0].tolist() == [-1, 0, 0]
    assert pn.voxel_query(one, pts, [[-1, 1, 1, 1]], g, 0.5, 3, 1, 1, 1)[0].tolist() == [-1, 0, 0]
    assert pn.voxel_query(one, pts, [[0, 1, 1, 1]], g, 0.5, 3, -1, 1, 1)[0].tolist() == [-1, 0, 0]
    # the ball query with the same points: the surface and NaN are not hits
    assert pn.ball_query_stack(one, [1], pts, [4], 0.5, 4)[0].tolist() == [1, 2, 1, 1]


def test_group_stack_rules():
    f = np.arange(12, dtype=F32).reshape(6, 2)
    idx = np.array([[0, 1], [-1, 2], [3, 0]], np.int32)
    out = pn.group_stack(f, [2, 4], idx, [1, 2])
    # row 0: frame 0 (start 0); rows 1, 2: frame 1 (start 2); -1 reads the previous frame's last row
    assert out[0].T.tolist() == [[0, 1], [2, 3]]
    assert out[1].T.tolist() == [[2, 3], [8, 9]] and out[2].T.tolist() == [[10, 11], [4, 5]]
    out = pn.group_stack(f, [2, 4], np.array([[-1, 9]], np.int32), [1, 0])  # outside [0, N): 0
    assert (out == 0).all()
    go = np.ones((3, 2, 2), F32)
    gr = pn.group_stack_grad(go, [2, 4], idx, [1, 2], 6)
    assert gr[:, 0].tolist() == [1, 2, 1, 0, 1, 1]  # global rows 0, 1 | 1, 4 | 5, 2


# ---- the layers on the CPU over the restatement ---------------------------------------------------------------------
@pytest.fixture()
def cpu_layers(monkeypatch):
    from paddle3d_amd import pointnet2_stack as L

    def ball(new_xyz, new_cnt, xyz, xyz_cnt, radius, nsample):
        return torch.from_numpy(pn.ball_query_stack(new_xyz.numpy(), new_cnt.numpy(), xyz.numpy(), xyz_cnt.numpy(),
                                                    radius, nsample))

    def voxel(new_xyz, xyz, new_coords, pi, radius, nsample, zr, yr, xr):
        return torch.from_numpy(pn.voxel_query(new_xyz.numpy(), xyz.numpy(), new_coords.numpy(), pi.numpy(), radius,
                                               nsample, zr, yr, xr))

    def group(features, fc, idx, ic):
        return torch.from_numpy(pn.group_stack(features.detach().numpy(), fc.numpy(), idx.numpy(), ic.numpy()))

    monkeypatch.setattr(L.pointnet2_ops, "ball_query_stack", ball)
    monkeypatch.setattr(L.pointnet2_ops, "voxel_query_wrapper", voxel)
    monkeypatch.setattr(L.pointnet2_ops, "grouping_operation_stack", group)
    return L


def test_layers_on_cpu_reproduce_golden(golden, cpu_layers):
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    g, L = golden, cpu_layers
    T = lambda k: torch.from_numpy(g[k])  # noqa: E731
    nf, idx = L.QueryAndGroup(0.5, 16)(T("pv_xyz"), T("pv_xyz_cnt"), T("pv_new_xyz"), T("pv_new_cnt"),
                                       T("pv_features"))
    assert np.array_equal(_bits(nf.numpy()), _bits(g["qag_out"])) and np.array_equal(idx.numpy(), g["qag_idx"])
    config = {"mlps": [[8, 16], [8, 8]], "pool_radius": [0.5, 1.0], "nsample": [16, 32]}
    cfg = copy.deepcopy(config)
    sa, c_out = L.build_local_aggregation_module(4, cfg)
    assert c_out == 24 and cfg["mlps"] == [[7, 8, 16], [7, 8, 8]]  # input channels prepended, + 3 in place
    load_paddle_state_dict(sa, mk.state(g, "sa"))
    with torch.no_grad():
        _, out = sa.eval()(T("pv_xyz"), T("pv_xyz_cnt"), T("pv_new_xyz"), T("pv_new_cnt"), T("pv_features"))
        assert np.array_equal(_bits(out.numpy()), _bits(g["sa_new_features"]))
        pinds = L.generate_voxel2pinds([2, 4, 12, 12, 4], T("vx_indices"))
        assert np.array_equal(pinds.numpy(), g["voxel2pinds"])
        bzyx = T("vx_new_coords")[:, [0, 3, 2, 1]].contiguous()
        idx, empty = L.voxel_query([2, 2, 2], 0.5, 16, T("vx_xyz"), T("vx_new_xyz"), bzyx, pinds)
        assert np.array_equal(idx.numpy(), g["vq_idx"]) and np.array_equal(empty.numpy(), g["vq_empty"])
        gf, gx, empty = L.VoxelQueryAndGrouping([1, 2, 3], 1.0, 8)(
            bzyx, T("vx_xyz"), T("vx_xyz_cnt"), T("vx_new_xyz"), T("vx_new_cnt"), T("vx_features"), pinds)
        assert np.array_equal(_bits(gf.numpy()), _bits(g["vqg_features"]))
        assert np.array_equal(_bits(gx.numpy()), _bits(g["vqg_xyz"]))
        assert np.array_equal(empty.numpy(), g["vqg_empty"])
        nv = L.NeighborVoxelSAModuleMSG(query_ranges=[[2, 2, 2], [1, 2, 3]], radii=[0.5, 1.0], nsamples=[16, 8],
                                        mlps=[[4, 8, 8], [4, 8, 16]])
        load_paddle_state_dict(nv, mk.state(g, "nv"))
        out = nv.eval()(T("vx_xyz"), T("vx_xyz_cnt"), T("vx_new_xyz"), T("vx_new_cnt"), T("vx_new_coords"),
                        T("vx_features"), pinds)
        assert np.array_equal(_bits(out.numpy()), _bits(g["nv_out"]))


def test_voxel_grouping_bookkeeping(golden, cpu_layers):
    g, L = golden, cpu_layers
    T = lambda k: torch.from_numpy(g[k])  # noqa: E731
    bzyx = T("vx_new_coords")[:, [0, 3, 2, 1]].contiguous()
    pinds = L.generate_voxel2pinds([2, 4, 12, 12, 4], T("vx_indices"))
    glob, empty = L.voxel_query([1, 2, 3], 1.0, 8, T("vx_xyz"), T("vx_new_xyz"), bzyx, pinds)
    grouper = L.VoxelQueryAndGrouping([1, 2, 3], 1.0, 8)
    seen = {}
    orig = L.pointnet2_ops.grouping_operation_stack

    def spy(features, fc, idx, ic):
        seen["idx"] = idx.clone()
        return orig(features, fc, idx, ic)

    L.pointnet2_ops.grouping_operation_stack = spy
    grouper(bzyx, T("vx_xyz"), T("vx_xyz_cnt"), T("vx_new_xyz"), T("vx_new_cnt"), T("vx_features"), pinds)
    # frame-local: the second half of the rows has the first frame's 100 voxels subtracted; empty rows are 0
    want = glob.numpy().astype(np.int64) - np.repeat([0, 100], 16)[:, None]
    want[empty.numpy()] = 0
    assert np.array_equal(seen["idx"].numpy(), want)
    assert (seen["idx"].numpy() >= 0).all() and empty.numpy().any()
    # rows must split into B equal groups (the reference's reshape)
    with pytest.raises(RuntimeError):
        grouper(bzyx[:31], T("vx_xyz"), T("vx_xyz_cnt"), T("vx_new_xyz")[:31], T("vx_new_cnt"), T("vx_features"),
                pinds)


def test_query_and_group_masks(cpu_layers):
    L = cpu_layers
    xyz = torch.tensor([[0, 0, 0], [0.1, 0, 0], [5, 5, 5], [5.1, 5, 5]], dtype=torch.float32)
    new_xyz = torch.tensor([[0, 0, 0], [9, 9, 9], [5, 5, 5]], dtype=torch.float32)
    feat = torch.arange(8, dtype=torch.float32).reshape(4, 2) + 1
    out, idx = L.QueryAndGroup(0.5, 3)(xyz, torch.tensor([2, 2], dtype=torch.int32), new_xyz,
                                       torch.tensor([2, 1], dtype=torch.int32), feat)
    assert idx.tolist() == [[0, 1, 0], [0, 0, 0], [0, 1, 0]]
    assert (out[1] == 0).all() and not (out[0] == 0).all()  # the empty ball: zero xyz and features
    assert out[2, 3:].T.tolist() == [[5, 6], [7, 8], [5, 6]]  # frame 1's rows 0, 1 are rows 2, 3 of xyz
    with pytest.raises(AssertionError):  # the reference's count asserts, only on request
        L.QueryAndGroup(0.5, 3, check_counts=True)(xyz, torch.tensor([2, 1], dtype=torch.int32), new_xyz,
                                                   torch.tensor([2, 1], dtype=torch.int32), feat)


def test_voxel2pinds_rows_past_n_dev():
    from paddle3d_amd import pointnet2_stack as L

    ind = torch.tensor([[0, 0, 1, 2], [1, 1, 0, 0], [0, 1, 1, 1], [1, 1, 1, 1]], dtype=torch.int32)
    full = L.generate_voxel2pinds([2, 2, 2, 3, 8], ind)
    assert full[0, 0, 1, 2] == 0 and full[1, 1, 0, 0] == 1 and (full >= 0).sum() == 4
    part = L.generate_voxel2pinds([2, 2, 2, 3, 8], ind, n_dev=torch.tensor([2], dtype=torch.int32))
    assert (part >= 0).sum() == 2 and part[0, 1, 1, 1] == -1


def test_ops_refuse_cpu_tensors():
    from paddle3d_amd.ops import pointnet2_ops as P

    z, c = torch.zeros((4, 3)), torch.tensor([4], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="ball_query_stack"):
        P.ball_query_stack(z, c, z, c, 0.5, 4)
    with pytest.raises(RuntimeError, match="voxel_query_wrapper"):
        P.voxel_query_wrapper(z, z, torch.zeros((4, 4), dtype=torch.int32), torch.zeros((1, 2, 2, 2),
                                                                                         dtype=torch.int32),
                              0.5, 4, 1, 1, 1)
    with pytest.raises(RuntimeError, match="grouping_operation_stack"):
        P.grouping_operation_stack(z, c, torch.zeros((4, 2), dtype=torch.int32), c)
