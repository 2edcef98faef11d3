"""BEVDet4D temporal alignment without a GPU: the C ABI is declared and exported, the Python layer refuses CPU
tensors, and the NumPy restatement the GPU tests compare the device operator with bit for bit reproduces the
reference's own shift_feature (tests/golden/python_bevdet4d_align.npz, made by
tests/golden/make_bevdet4d_align_golden.py)."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import bevdet4d_align_numpy as ba  # noqa: E402

GRID_TOL = 2e-6   # normalised units
OUT_TOL = 3e-4    # inputs in [-1, 1]


@pytest.fixture(scope="module")
def built():
    from paddle3d_amd import build

    return build.build()


def test_header_declares_and_library_exports(built):
    hdr = open(os.path.join(ROOT, "include", "paddle3d_amd.h")).read()
    assert "pd3_bevdet4d_align" in set(re.findall(r"\b(pd3_\w+)\s*\(", hdr))
    out = subprocess.check_output(["nm", "-D", "--defined-only", built], text=True)
    assert "pd3_bevdet4d_align" in {line.split()[-1] for line in out.splitlines() if " T " in line}
    from paddle3d_amd import _lib

    assert _lib.lib().pd3_bevdet4d_align.argtypes is not None


def test_python_layer_refuses_cpu_tensors():
    from paddle3d_amd import bevdet4d

    assert bevdet4d.BEVDET4D_NUM_ADJ == 8
    x = torch.zeros(1, 4, 16, 16)
    rots = torch.eye(3).expand(1, 6, 3, 3)
    trans = torch.zeros(1, 6, 3)
    with pytest.raises(RuntimeError, match="bevdet4d_align"):
        bevdet4d.shift_feature(x, [trans, trans], [rots, rots], torch.eye(3)[None])
    with pytest.raises(RuntimeError, match="bevdet4d_align"):
        bevdet4d.align_concat([x, x], [rots, rots], [trans, trans], torch.eye(3)[None])


def test_restatement_reproduces_reference_golden():
    gold = np.load(os.path.join(HERE, "golden", "python_bevdet4d_align.npz"))
    worst_g = worst_o = 0.0
    for i in range(len(ba.GOLDEN_CASES)):
        c = ba.golden_case(i)
        out, grid = ba.shift_feature(c["input"], c["trans"], c["rots"], c["bda"], c["bda_adj"])
        out, grid = ba.at_pixels(out, grid, ba.golden_pixels(i))
        assert grid.shape == gold[f"grid_{i}"].shape and out.shape == gold[f"out_{i}"].shape
        dg = float(np.abs(grid - gold[f"grid_{i}"]).max())
        do = float(np.abs(out - gold[f"out_{i}"]).max())
        worst_g, worst_o = max(worst_g, dg), max(worst_o, do)
        assert dg <= GRID_TOL, (c["name"], dg)
        assert do <= OUT_TOL, (c["name"], do)
    print(f"restatement vs reference: grid max |d| {worst_g:.3g} (normalised), output max |d| {worst_o:.3g}")
    # the golden exercises what it is meant to: the last case moves part of the grid out of range
    g = gold[f"grid_{len(ba.GOLDEN_CASES) - 1}"]
    outside = float(((np.abs(g[..., 0]) > 1) | (np.abs(g[..., 1]) > 1)).mean())
    assert 0.2 < outside < 0.8
    assert ba.GOLDEN_CASES[3][6] is not None  # one bda_adj case


def test_transform_matches_float64_matrix_algebra():
    """tf composed in the written-out order equals the matrix product of the reference's formula in float64 (to fp32
    rounding), including a flipping, scaling bda and a distinct bda_adj."""
    rng = np.random.default_rng(3)
    rots, trans = ba.poses(rng, 1, 1, yaw_max_deg=10.0, trans_max=5.0)
    D = ba.bda_matrix(rot_deg=17.0, flip_x=True, scale=1.05)
    Da = ba.bda_matrix(rot_deg=-4.0, flip_y=True, scale=0.9)

    def h(R, t):
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = R, t
        return m

    def b4(d):
        m = np.eye(4)
        m[:3, :3] = d
        return m

    c0 = b4(D.astype(np.float64)) @ h(rots[0][0, 0].astype(np.float64), trans[0][0, 0].astype(np.float64))
    c1 = b4(Da.astype(np.float64)) @ h(rots[1][0, 0].astype(np.float64), trans[1][0, 0].astype(np.float64))
    l = (c0 @ np.linalg.inv(c1))[np.ix_([0, 1, 3], [0, 1, 3])]
    f2b = np.array([[0.8, 0, -51.2], [0, 0.8, -51.2], [0, 0, 1]], np.float64)
    f2b[0, 0] = f2b[1, 1] = float(np.float32(0.8))
    f2b[0, 2] = f2b[1, 2] = float(np.float32(-51.2))
    want = (np.linalg.inv(f2b) @ l @ f2b)[:2].reshape(-1)
    got = ba.transform(rots[0][0, 0], trans[0][0, 0], rots[1][0, 0], trans[1][0, 0], D, Da)
    assert got.dtype == np.float32
    np.testing.assert_allclose(got.astype(np.float64), want, rtol=2e-7, atol=1e-5)


def test_restatement_zeroes_non_finite_and_far_coordinates():
    """The float-side range check: NaN / Inf and far-away coordinates sample nothing (all zeros, no index)."""
    x = ba.features(np.random.default_rng(4), (3, 8, 8))
    for v in (math.nan, math.inf, -math.inf, 1e30, -1e30, 3.0e9):
        g = np.full((8, 8, 2), v, np.float32)
        assert not ba.sample(x, g).any()
    # ix = -0.5, iy = 3.5: only the column-0 corners of rows 3 and 4 are in range, each with weight 0.25
    g = np.zeros((8, 8, 2), np.float32)
    g[..., 0] = np.float32(-1.0 - 1.0 / 7.0)
    want = 0.25 * (x[:, 3, 0] + x[:, 4, 0])
    np.testing.assert_allclose(ba.sample(x, g), np.broadcast_to(want[:, None, None], (3, 8, 8)), atol=1e-6)


def test_concat_layout_and_current_frame_copy():
    rng = np.random.default_rng(5)
    B, C, H, W, nadj = 2, 3, 16, 20, 2
    rots, trans = ba.poses(rng, B, nadj)
    feats = [ba.features(rng, (B, C, H, W)) for _ in range(nadj + 1)]
    bda = ba.bda_matrix(rot_deg=5.0)[None].repeat(B, 0)
    out, grids = ba.align_concat(feats, [rots[0]] * nadj, [trans[0]] * nadj, rots[1:], trans[1:], [bda] * nadj)
    assert out.shape == (B, (nadj + 1) * C, H, W) and grids.shape == (nadj * B, H, W, 2)
    np.testing.assert_array_equal(out[:, :C], feats[0])
    for k in range(1, nadj + 1):
        one, g = ba.shift_feature(feats[k], [trans[0], trans[k]], [rots[0], rots[k]], bda)
        np.testing.assert_array_equal(out[:, k * C:(k + 1) * C], one)
        np.testing.assert_array_equal(grids[(k - 1) * B:k * B], g)
