"""ms_deform_attn without a GPU: the C ABI is declared, exported and bound, the Python layer refuses CPU tensors,
and the NumPy restatement the GPU tests compare the device operator with bit for bit agrees with an independent
torch formulation (F.grid_sample per level and head) in value and in gradient."""
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
import ms_deform_attn_numpy as md  # noqa: E402

SYMS = ("pd3_ms_deform_attn_forward", "pd3_ms_deform_attn_backward")


@pytest.fixture(scope="module")
def built():
    from paddle3d_amd import build

    return build.build()


def test_header_declares_and_library_exports(built):
    hdr = open(os.path.join(ROOT, "include", "paddle3d_amd.h")).read()
    declared = set(re.findall(r"\b(pd3_\w+)\s*\(", hdr))
    out = subprocess.check_output(["nm", "-D", "--defined-only", built], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    from paddle3d_amd import _lib

    for s in SYMS:
        assert s in declared and s in exported
        assert getattr(_lib.lib(), s).argtypes is not None


def test_python_layer_refuses_cpu_tensors():
    from paddle3d_amd.ops import ms_deform_attn as op

    value, loc, attn, sh, st = md.random_case(np.random.default_rng(0), 1, 4, 2, 8, [[3, 4]], 2)
    args = [torch.from_numpy(x) for x in (value, loc, attn, sh, st)]
    with pytest.raises(RuntimeError, match="Unsupported device type for ms_deform_attn operator."):
        op.ms_deform_attn(*args, 64)
    with pytest.raises(RuntimeError, match="Unsupported device type for ms_deform_attn operator."):
        op.ms_deform_attn_backward(torch.zeros(1, 4, 16), *args, 64)


def _edge_heavy_case(seed):
    """Random multi-level shapes; a third of the points outside the map, a sixth exactly on h / w = -1, 0, H - 1
    or H (and the same for w)."""
    rng = np.random.default_rng(seed)
    shapes = [[int(rng.integers(1, 9)), int(rng.integers(1, 9))] for _ in range(int(rng.integers(1, 5)))]
    value, loc, attn, sh, st = md.random_case(rng, 2, 40, int(rng.integers(1, 4)), int(rng.integers(1, 6)), shapes,
                                              int(rng.integers(1, 5)), np.float64, -0.6, 1.6)
    for l in range(sh.shape[0]):
        for k, n in ((0, sh[l, 1]), (1, sh[l, 0])):
            edge = rng.random(loc.shape[:3] + (loc.shape[4],)) < 1 / 6
            pick = rng.choice(np.array([-1.0, 0.0, n - 1.0, float(n)]), size=edge.shape)
            view = loc[:, :, :, l, :, k]
            view[edge] = ((pick + 0.5) / n)[edge]
    return value, loc, attn, sh, st


@pytest.mark.parametrize("seed", range(6))
def test_restatement_matches_grid_sample_fp64(seed):
    value, loc, attn, sh, st = _edge_heavy_case(seed)
    want = md.grid_sample_attn(*(torch.from_numpy(x) for x in (value, loc, attn)), sh, st).numpy()
    got = md.forward(value, loc, attn, sh, st)
    assert got.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("seed", range(4))
def test_restatement_backward_matches_autograd_fp64(seed):
    rng = np.random.default_rng(100 + seed)
    value, loc, attn, sh, st = md.random_case(rng, 2, 30, 3, 5, [[6, 8], [3, 5], [2, 2]], 3, np.float64, -0.2, 1.2)
    # away from integer coordinates: the op is only piecewise smooth there
    for l in range(sh.shape[0]):
        for k, n in ((0, sh[l, 1]), (1, sh[l, 0])):
            x = loc[:, :, :, l, :, k] * n - 0.5
            loc[:, :, :, l, :, k] = (np.floor(x) + np.clip(x - np.floor(x), 0.05, 0.95) + 0.5) / n
    ts = [torch.from_numpy(x.copy()).requires_grad_() for x in (value, loc, attn)]
    out = md.grid_sample_attn(*ts, sh, st)
    go = rng.standard_normal(tuple(out.shape))
    out.backward(torch.from_numpy(go))
    gv, gl, ga = md.backward(go, value, loc, attn, sh, st)
    for got, t in ((gv, ts[0]), (gl, ts[1]), (ga, ts[2])):
        np.testing.assert_allclose(got, t.grad.numpy(), rtol=0, atol=1e-11)


@pytest.mark.parametrize("case", ["tsa", "sca", "decoder"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_matches_reference_callers_golden(case, dtype):
    """What TemporalSelfAttention, MSDeformableAttention3D (Z-anchor interleave) and CustomMSDeformableAttention hand
    the op, recorded by tests/golden/make_ms_deform_attn_golden.py from the reference's own forward methods."""
    g = np.load(os.path.join(HERE, "golden", "python_ms_deform_attn.npz"))
    value, loc, attn = (g[f"{case}_{n}"].astype(dtype) for n in ("value", "sampling_locations", "attention_weights"))
    sh, st = g[f"{case}_spatial_shapes"], g[f"{case}_level_start_index"]
    assert sh.dtype == np.int64 and st.dtype == np.int64 and int(g[f"{case}_im2col_step"]) == 64
    B, S, M, C = value.shape
    assert loc.shape[:3] == (B, loc.shape[1], M) and loc.shape[-1] == 2 and S == int((sh[:, 0] * sh[:, 1]).sum())
    got = md.forward(value, loc, attn, sh, st)
    assert np.abs(got - g[f"{case}_out"].reshape(got.shape)).max() <= 1e-5


def test_golden_pins_the_callers_layout():
    """The recorded op inputs carry the callers' layout: TSA batches the bev queue (2 x bs), SCA's points are
    num_points x num_Z_anchors (8 = 2 x 4), and the levels are SCA's two maps.  Reading the locations as (y, x)
    instead of (x, y) gives a different result, so the recorded outputs pin the order."""
    g = np.load(os.path.join(HERE, "golden", "python_ms_deform_attn.npz"))
    assert g["tsa_value"].shape[0] == 2 and g["tsa_sampling_locations"].shape[4] == 4
    assert g["sca_sampling_locations"].shape[3:] == (2, 8, 2)
    assert g["sca_spatial_shapes"].tolist() == [[6, 10], [3, 5]]
    for case in ("tsa", "sca", "decoder"):
        value, loc, attn = (g[f"{case}_{n}"].astype(np.float64) for n in ("value", "sampling_locations",
                                                                           "attention_weights"))
        sh, st = g[f"{case}_spatial_shapes"], g[f"{case}_level_start_index"]
        want = g[f"{case}_out"].reshape(value.shape[0], loc.shape[1], -1)
        assert np.abs(md.forward(value, loc[..., ::-1].copy(), attn, sh, st) - want).max() > 1e-2


def test_restatement_out_of_range_rows_count_zero():
    value, loc, attn, sh, st = md.random_case(np.random.default_rng(7), 1, 20, 2, 4, [[4, 4], [2, 2]], 2, np.float64)
    S = value.shape[1]
    # level 1 moved entirely past S: it contributes nothing, so the result is level 0's alone
    moved = md.forward(value, loc, attn, sh, st + np.array([0, S], np.int64))
    alone = md.forward(value, loc[:, :, :, :1], attn[:, :, :, :1], sh[:1], st[:1])
    np.testing.assert_array_equal(moved, alone)
