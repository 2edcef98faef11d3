"""CaDDN's frustum-to-voxel and map-to-BEV stage on the CPU: the NumPy restatement of the three entry points
(tests/golden/caddn_numpy.py) against what the reference's own Python computed (tests/golden/python_caddn.npz), the
factorised form against the materialised one, the workspace queries and refusal statuses, and the maker's conditions on the
committed file.

Bounds: the ones the maker stored, 4 x the largest error of the reference's own fp32 result against its fp64 run (one
fp32 ulp of the largest output as a floor).  The factorised sample differs from the materialised one by the order of
eight products and seven sums, each of which the reference's fp32 run rounds too: the same bound holds for it."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import caddn_numpy as cn  # noqa: E402
import make_caddn_golden as mk  # noqa: E402

F32 = np.float32
TAGS = mk.TAGS


@pytest.fixture(scope="module")
def golden():
    return mk.load()


@pytest.fixture(scope="module")
def expf():
    from oracle import pyoracle as O

    return lambda x: O.libm_eval(2, x)


def case_args(g, tag):
    """(image_features, depth_logits, lidar_to_cam, cam_to_img, image_shape, grid, pc_min, voxel_size, disc_cfg)."""
    c = mk.CASES[tag]
    feats, logits = mk.inputs(tag)
    return (feats, logits, g[f"{tag}_lidar_to_cam"], g[f"{tag}_cam_to_img"], g[f"{tag}_image_shape"], mk.grid_size(tag),
            c["pc_range"][:3], c["voxel_size"], c["disc_cfg"])


def grid_errors(got, g, tag):
    """(largest error over the coordinates finite in both, misplaced -2 outside the unsure set)."""
    want, unsure = g[f"{tag}_grid"], g[f"{tag}_grid_unsure"]
    both = (got != -2) & (want != -2)
    err = float(np.abs(np.where(both, got.astype(np.float64) - want, 0)).max())
    return err, int((((got == -2) != (want == -2)) & ~unsure).sum())


_cache = {}


def restated(g, tag, expf):
    """(grid, voxel_features, spatial_features) of the restatement, computed once per case."""
    if tag not in _cache:
        args = case_args(g, tag)
        w, sc, sh = cn.fold_bn(mk.state(g, tag))
        _cache[tag] = (cn.frustum_grid(*args[2:]), cn.frustum_to_voxel(*args, expf),
                       cn.frustum_to_bev(*args, w, sc, sh, expf))
    return _cache[tag]


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_against_reference(golden, expf, tag):
    g = golden
    grid, voxel, bev = restated(g, tag, expf)
    err, misplaced = grid_errors(grid, g, tag)
    print(f"{tag} grid err {err:.3e} bound {float(g[f'{tag}_grid_bound']):.3e} misplaced {misplaced}")
    assert grid.shape == g[f"{tag}_grid"].shape and err <= float(g[f"{tag}_grid_bound"]) and misplaced == 0
    for name, got in (("voxel_features", voxel), ("spatial_features", bev)):
        want, bound = g[f"{tag}_{name}"], float(g[f"{tag}_{name}_bound"])
        e = float(np.abs(got.astype(np.float64) - want).max())
        print(f"{tag} {name} err {e:.3e} bound {bound:.3e} (reference's own {float(g[f'{tag}_{name}_ref_err']):.3e})")
        assert got.shape == want.shape and got.dtype == F32 and e <= bound, (tag, name, e, bound)
    for b in mk.CASES[tag]["planted"]:  # a frame without a sample: zeros, and relu(shift) in every column
        _, sc, sh = cn.fold_bn(mk.state(g, tag))
        assert not voxel[b].any()
        assert np.array_equal(bev[b], np.broadcast_to(np.maximum(sh, 0)[:, None, None], bev[b].shape))


@pytest.mark.parametrize("tag", TAGS)
def test_factorised_against_materialised(golden, expf, tag):
    """The frustum volume formed, sampled with torch's 5-D grid_sample through the restatement's grid, transposed."""
    g = golden
    args = case_args(g, tag)
    grid, voxel, _ = restated(g, tag, expf)
    feats, logits = torch.from_numpy(args[0]), torch.from_numpy(args[1])
    frustum = torch.softmax(logits.unsqueeze(1), 2)[:, :, :-1] * feats.unsqueeze(2)
    mat = torch.nn.functional.grid_sample(frustum, torch.from_numpy(grid), mode="bilinear", padding_mode="zeros",
                                          align_corners=False).permute(0, 1, 4, 3, 2).numpy()
    err = float(np.abs(mat.astype(np.float64) - voxel).max())
    print(f"{tag} factorised against materialised {err:.3e}")
    assert err <= float(g[f"{tag}_voxel_features_bound"])
    assert (np.abs(voxel) > 0).mean() > 0.2


def test_workspace_queries_and_refusals_need_no_gpu():
    from paddle3d_amd import _lib, build

    build.build()
    L = _lib.lib()
    assert L.pd3_frustum_to_voxel_workspace(1, 64, 80, 94, 311) >= 94 * 311 * (64 + 80) * 4
    assert L.pd3_frustum_to_bev_workspace(1, 64, 80, 94, 311, 25, 64) >= 94 * 311 * (64 + 80) * 4 + 1600 * 64 * 4
    mn = np.zeros(3, F32)
    vs = np.ones(3, F32)
    for C, CO, Z in ((24, 64, 8), (64, 80, 8), (64, 64, 33), (80, 16, 8), (16, 8, 4)):
        st = L.pd3_frustum_to_bev(None, None, None, None, None, 1, C, 12, 4, 4, 8, 8, Z, mn.ctypes.data, vs.ctypes.data, 0,
                                  1.0, 9.0, None, None, None, CO, None, None, 0, None)
        assert st == -3, (C, CO, Z, st)
    assert L.pd3_frustum_to_bev(None, None, None, None, None, 1, 16, 12, 4, 4, 8, 8, 8, mn.ctypes.data, vs.ctypes.data, 3,
                                1.0, 9.0, None, None, None, 16, None, None, 0, None) == -1  # no such mode


@pytest.mark.parametrize("tag", TAGS)
def test_maker_conditions_hold_on_the_committed_file(golden, tag):
    seen = mk.check_conditions(golden, tag)
    print(tag, seen)
    assert os.path.getsize(mk.OUT) < 1_000_000
    c = mk.CASES[tag]
    B = len(c["image_shape"])
    X, Y, Z = mk.grid_size(tag)
    assert golden[f"{tag}_grid"].shape == (B, X, Y, Z, 3)
    assert golden[f"{tag}_voxel_features"].shape == (B, c["C"], Z, Y, X)
    assert golden[f"{tag}_spatial_features"].shape == (B, c["C_out"], Y, X)
    shp = np.asarray(c["image_shape"])
    if B > 1:  # the maximum over the batch is no single row
        assert not any((shp[b] == shp.max(0)).all() for b in range(B))
