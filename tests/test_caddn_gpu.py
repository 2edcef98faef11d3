"""CaDDN's frustum-to-voxel and map-to-BEV stage on the device: the three entry points of csrc/caddn.hip against what
the reference's own Python computed (tests/golden/python_caddn.npz) and against their NumPy restatement
(tests/golden/caddn_numpy.py), and the modules of paddle3d_amd/caddn.py with the golden state dict.

Against the recorded reference: the bounds the maker stored (4 x the reference's own fp32 error against its fp64 run).
Against the restatement, and frustum_to_bev against itself under another placement of a frame, a padded grid or another
stream: bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import caddn_numpy as cn  # noqa: E402
import make_caddn_golden as mk  # noqa: E402
import test_caddn_cpu as cpu  # noqa: E402
from guarded import launch_ledger  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
TAGS = mk.TAGS


@pytest.fixture(scope="module")
def golden():
    return mk.load()


@pytest.fixture(scope="module")
def expf():
    from oracle import pyoracle as O

    return lambda x: O.libm_eval(2, x)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _ops():
    from paddle3d_amd.ops import caddn
    return caddn


def _dev_args(args):
    """case_args with the five arrays on the device."""
    return tuple(_t(a) for a in args[:5]) + tuple(args[5:])


def _folded(g, tag):
    return cn.fold_bn(mk.state(g, tag))


def _bev(args, folded):
    return _ops().frustum_to_bev(*_dev_args(args), *[_t(a) for a in folded]).cpu().numpy()


@pytest.mark.parametrize("tag", TAGS)
def test_frustum_grid_against_reference(golden, expf, tag):
    g = golden
    args = cpu.case_args(g, tag)
    got = _ops().frustum_grid(*_dev_args(args)[2:]).cpu().numpy()
    err, misplaced = cpu.grid_errors(got, g, tag)
    print(f"{tag} grid err {err:.3e} bound {float(g[f'{tag}_grid_bound']):.3e} misplaced -2: {misplaced}")
    assert got.shape == g[f"{tag}_grid"].shape
    assert err <= float(g[f"{tag}_grid_bound"]) and misplaced == 0
    assert np.array_equal(_bits(got), _bits(cpu.restated(g, tag, expf)[0]))


@pytest.mark.parametrize("tag", TAGS)
def test_voxel_and_bev_against_reference_and_restatement(golden, expf, tag):
    g = golden
    args = cpu.case_args(g, tag)
    _, voxel_r, bev_r = cpu.restated(g, tag, expf)
    voxel = _ops().frustum_to_voxel(*_dev_args(args)).cpu().numpy()
    bev = _bev(args, _folded(g, tag))
    for name, got, rest in (("voxel_features", voxel, voxel_r), ("spatial_features", bev, bev_r)):
        want, bound = g[f"{tag}_{name}"], float(g[f"{tag}_{name}_bound"])
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"{tag} {name} err {err:.3e} bound {bound:.3e}; bits differing from the restatement: "
              f"{int((_bits(got) != _bits(rest)).sum())}")
        assert got.shape == want.shape and err <= bound, (tag, name, err, bound)
        assert np.array_equal(_bits(got), _bits(rest)), (tag, name)
    for b in mk.CASES[tag]["planted"]:  # no sample in the frame: zeros, and relu(shift) in every column
        assert not voxel[b].any()
        sh = _folded(g, tag)[2]
        assert np.array_equal(bev[b], np.broadcast_to(np.maximum(sh, 0)[:, None, None], bev[b].shape))


@pytest.mark.parametrize("tag", ("a", "c"))
def test_bev_does_not_depend_on_placement(golden, tag):
    """A frame alone against inside the batch at another position; X and Y padded by extra columns; another stream."""
    g = golden
    args, folded = cpu.case_args(g, tag), _folded(g, tag)
    ref = _bev(args, folded)
    B = len(ref)
    top = np.asarray(args[4]).max(0, keepdims=True)  # a frame alone keeps the batch's normalisation
    for b in range(B):
        alone = _bev(tuple(a[b:b + 1] for a in args[:4]) + (top,) + args[5:], folded)
        assert np.array_equal(_bits(alone[0]), _bits(ref[b])), (tag, b, "alone")
    order = np.roll(np.arange(B), 1)
    moved = _bev(tuple(a[order] for a in args[:5]) + args[5:], folded)
    assert np.array_equal(_bits(moved), _bits(ref[order])), (tag, "moved")
    X, Y, Z = args[5]
    padded = _bev(args[:5] + ((X + 3, Y + 2, Z),) + args[6:], folded)
    assert padded.shape == (B, ref.shape[1], Y + 2, X + 3)
    assert np.array_equal(_bits(padded[:, :, :Y, :X]), _bits(ref)), (tag, "padded")
    stream = torch.cuda.Stream(DEV)
    dev, fd = _dev_args(args), [_t(a) for a in folded]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        other = _ops().frustum_to_bev(*dev, *fd)
    stream.synchronize()
    assert np.array_equal(_bits(other.cpu().numpy()), _bits(ref)), (tag, "stream")


@pytest.mark.parametrize("tag", TAGS)
def test_bev_against_voxel_and_convolution(golden, tag):
    g = golden
    args = cpu.case_args(g, tag)
    w, sc, sh = (_t(a) for a in _folded(g, tag))
    voxel = _ops().frustum_to_voxel(*_dev_args(args))
    comp = torch.relu(torch.nn.functional.conv2d(voxel.flatten(1, 2), w[:, :, None, None]) * sc[None, :, None, None]
                      + sh[None, :, None, None]).cpu().numpy()
    bev = _bev(args, _folded(g, tag))
    err = float(np.abs(bev.astype(np.float64) - comp).max())
    print(f"{tag} fused against voxel + conv {err:.3e} bound {float(g[f'{tag}_spatial_features_bound']):.3e}")
    assert err <= float(g[f"{tag}_spatial_features_bound"])


def _module(g, tag, fused):
    from paddle3d_amd import caddn
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    c = mk.CASES[tag]
    m = caddn.FrustumToBEV(mk.f2v_cfg(tag), c["disc_cfg"], mk.map_to_bev_cfg(tag), fused=fused)
    left = load_paddle_state_dict(m, {f"map_to_bev.{k}": v for k, v in mk.state(g, tag).items()})  # CADDN's own keys
    assert left == []
    return m.eval().to(DEV)


def _batch(g, tag):
    return {"trans_lidar_to_cam": _t(g[f"{tag}_lidar_to_cam"]), "trans_cam_to_img": _t(g[f"{tag}_cam_to_img"]),
            "image_shape": _t(g[f"{tag}_image_shape"])}


@pytest.mark.parametrize("fused", (True, False))
@pytest.mark.parametrize("tag", TAGS)
def test_modules_reproduce_the_reference(golden, tag, fused):
    from paddle3d_amd import _lib, caddn

    g = golden
    feats, logits = (_t(a) for a in mk.inputs(tag))
    m = _module(g, tag, fused)
    bd = _batch(g, tag)
    with torch.no_grad(), launch_ledger(_lib.lib(), _lib.symbols("test_memory_safety_caddn_gpu")) as calls:
        out = m(feats, logits, bd)
    assert bool(calls.get("pd3_frustum_to_bev")) == fused and bool(calls.get("pd3_frustum_to_voxel")) != fused
    assert out is bd["spatial_features"]
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - g[f"{tag}_spatial_features"]).max())
    print(f"{tag} fused={fused} spatial_features err {err:.3e} bound {float(g[f'{tag}_spatial_features_bound']):.3e}")
    assert err <= float(g[f"{tag}_spatial_features_bound"])
    if fused:
        return
    # the reference's own route, frustum volume and grid in memory: FFE.create_frustum_features, FrustumGridGenerator,
    # Sampler; and FrustumToVoxel's route without them
    with torch.no_grad():
        bd["frustum_features"] = caddn.FFE.create_frustum_features(feats, logits)
        unfused = m.f2v(bd)["voxel_features"].cpu().numpy()
        del bd["frustum_features"]
        bd["image_features"], bd["depth_logits"] = feats, logits
        direct = m.f2v(bd)["voxel_features"].cpu().numpy()
    for name, got in (("unfused", unfused), ("direct", direct)):
        err = float(np.abs(got.astype(np.float64) - g[f"{tag}_voxel_features"]).max())
        print(f"{tag} {name} voxel_features err {err:.3e} bound {float(g[f'{tag}_voxel_features_bound']):.3e}")
        assert got.shape == g[f"{tag}_voxel_features"].shape and err <= float(g[f"{tag}_voxel_features_bound"])


def test_refused_shapes_return_unsupported_and_the_module_falls_back(golden):
    from paddle3d_amd import _lib, caddn
    from paddle3d_amd._lib import Paddle3DAmdError

    g, tag = golden, "a"
    args = cpu.case_args(g, tag)
    rng = np.random.default_rng(5)
    X, Y, Z = args[5]
    for C, CO, Zr in ((24, 16, Z), (16, 24, Z), (80, 16, Z), (16, 80, Z), (16, 16, 33)):
        feats = rng.standard_normal((2, C, 12, 40)).astype(F32)
        a = (feats,) + args[1:5] + ((X, Y, Zr),) + args[6:]
        folded = ((rng.standard_normal((CO, C * Zr)) / 16).astype(F32), np.ones(CO, F32), np.zeros(CO, F32))
        assert not _ops().frustum_to_bev_supported(C, CO, Zr)
        with pytest.raises(Paddle3DAmdError, match=r"status -3"):
            _bev(a, folded)
    # a module at such a shape: frustum_to_voxel and a convolution, fused or not
    c = mk.CASES[tag]
    cfg = dict(mk.map_to_bev_cfg(tag), in_channels=24 * Z, out_channels=40)
    feats = _t(rng.standard_normal((2, 24, 12, 40)).astype(F32))
    logits = _t(mk.inputs(tag)[1])
    torch.manual_seed(3)
    outs = []
    for fused in (True, False):
        m = caddn.FrustumToBEV(mk.f2v_cfg(tag), c["disc_cfg"], cfg, fused=fused).eval().to(DEV)
        if outs:
            m.load_state_dict(first.state_dict())
        first = m
        with torch.no_grad(), launch_ledger(_lib.lib(), _lib.symbols("test_memory_safety_caddn_gpu")) as calls:
            outs.append(m(feats, logits, _batch(g, tag)))
        assert calls.get("pd3_frustum_to_voxel") and not calls.get("pd3_frustum_to_bev")
    assert outs[0].shape == (2, 40, Y, X) and torch.equal(outs[0], outs[1]) and float(outs[0].abs().max()) > 0


@pytest.mark.parametrize("fused", (True, False))
def test_forward_has_no_host_sync(golden, fused):
    g, tag = golden, "c"
    feats, logits = (_t(a) for a in mk.inputs(tag))
    m = _module(g, tag, fused)
    with torch.no_grad():
        m(feats, logits, _batch(g, tag))  # warm-up: code objects, allocator
    bd = _batch(g, tag)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            out = m(feats, logits, bd)
            grid = m.f2v.grid_generator(bd["trans_lidar_to_cam"], bd["trans_cam_to_img"], bd["image_shape"])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    X, Y, Z = mk.grid_size(tag)
    assert out.shape == (3, mk.CASES[tag]["C_out"], Y, X) and grid.shape == (3, X, Y, Z, 3)
