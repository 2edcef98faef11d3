"""SqueezeSegV3 on the device.  pd3_sac_isk_forward is held bit-equal to the NumPy restatement of its header
(tests/golden/squeezeseg_numpy.py) on seeded sweeps over every path of the tiling -- heights below the 7x7 halo, widths
around the 16-pixel segment and past the 64-pixel workgroup, channel counts from the smallest to 64 and once at 256 --,
with shifts at which expf overflows and underflows, with a NaN pixel and an Inf weight; a frame gives the same bits
alone, elsewhere in the batch and on a side stream.  pd3_range_project equals its restatement exactly, on random scans
and on ties, an empty frame, a NaN point, a zero point, one point, and all points in one pixel.  Refusals, the
fall-back, host synchronisation and launch counts are at the end.  The tests against the reference's golden results
are in the second half of the file."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from guarded import launch_ledger  # noqa: E402

import make_squeezeseg_golden as mk  # noqa: E402
import squeezeseg_numpy as sn  # noqa: E402
import test_squeezeseg_cpu as cpu  # noqa: E402
from test_squeezeseg_cpu import expf, golden  # noqa: E402,F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
MEAN, STD = (12.12, 10.88, 0.23, -1.04, 0.21), (12.32, 11.47, 6.91, 0.86, 0.16)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(got, want):
    """Bit equality of two float32 arrays, a NaN matching any NaN (the sign and payload of a NaN are not part of the
    arithmetic the header fixes)."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and
                np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def device_params(p):
    from paddle3d_amd.ops import squeezeseg as ops

    return (ops.pack_sac_attention_weight(_t(p["w"])), _t(p["s_a"]), _t(p["t_a"]), ops.pack_sac_mlp_weight(_t(p["v"])),
            _t(p["s_m"]), _t(p["t_m"]))


def run_kernel(xyz, feat, p):
    from paddle3d_amd.ops import squeezeseg as ops

    out = ops.sac_isk_forward(_t(xyz), _t(feat), *device_params(p))
    assert out is not None
    return out.cpu().numpy()


def restate(xyz, feat, p, expf):
    return sn.sac_isk(xyz, feat, p["w"], p["s_a"], p["t_a"], p["v"], p["s_m"], p["t_m"], expf)


# (C, H, W): every H of {1, 2, 3, 4, 7}, every W of {1, 3, 15, 16, 17, 31, 33} and 65 (past the workgroup's 64 pixels),
# every C of {16, 32, 48, 64}, each value at least twice and in different company
SWEEP = [(16, 1, 1), (16, 2, 3), (32, 3, 15), (32, 4, 16), (48, 7, 17), (48, 1, 31), (64, 2, 33), (64, 3, 65),
         (16, 7, 65), (32, 1, 17), (48, 4, 3), (64, 7, 16), (16, 3, 31), (32, 2, 1), (48, 2, 33), (64, 4, 15)]


@pytest.mark.parametrize("C,H,W", SWEEP)
def test_sac_isk_sweep(expf, C, H, W):
    p = cpu.block_params(C, 100 + C + H, big_z=True)
    xyz, feat = cpu.block_inputs(2, C, H, W, 7 * C + 31 * H + W)
    got, want = run_kernel(xyz, feat, p), restate(xyz, feat, p, expf)
    assert np.isfinite(want).all() and (want > 0).any()
    assert same_bits(got, want), f"{int((got != want).sum())} of {want.size} differ, max {np.abs(got - want).max():.3e}"


def test_sac_isk_at_256_channels(expf):
    """C = 256, the widest stage: 64 accumulators per lane."""
    p = cpu.block_params(256, 5, big_z=True)
    xyz, feat = cpu.block_inputs(1, 256, 2, 17, 6)
    got, want = run_kernel(xyz, feat, p), restate(xyz, feat, p, expf)
    assert same_bits(got, want), f"{int((got != want).sum())} of {want.size} differ, max {np.abs(got - want).max():.3e}"


def test_sac_isk_at_128_channels(expf):
    """C = 128, the smallest count at which two waves share a segment (the grid is small here)."""
    p = cpu.block_params(128, 7, big_z=True)
    xyz, feat = cpu.block_inputs(2, 128, 1, 18, 8)
    got, want = run_kernel(xyz, feat, p), restate(xyz, feat, p, expf)
    assert same_bits(got, want), f"{int((got != want).sum())} of {want.size} differ, max {np.abs(got - want).max():.3e}"


@pytest.mark.parametrize("C", [128, 256])
def test_sac_isk_one_or_two_waves_per_segment(C):
    """768 segments (48 frames of 1 x 256) run with one wave per segment; any of the frames alone (16 segments) runs with
    two waves sharing each segment's output channels.  The bits are the same."""
    from paddle3d_amd.ops import squeezeseg as ops

    dp = device_params(cpu.block_params(C, 31))
    xyz, feat = (_t(a) for a in cpu.block_inputs(48, C, 1, 256, 32))
    whole = ops.sac_isk_forward(xyz, feat, *dp)
    for n in (0, 29, 47):
        alone = ops.sac_isk_forward(xyz[n:n + 1], feat[n:n + 1], *dp)
        assert torch.equal(alone[0], whole[n])
    assert bool(torch.isfinite(whole).all()) and bool((whole > 0).any())


def test_sac_isk_nan_pixel_and_inf_weight(expf):
    """A NaN in xyz reaches every output whose 7x7 window holds it and a NaN feature value its 3x3 neighbourhood, as in
    the torch composition with direct convolutions.  An Inf attention weight makes z infinite inside the image (a gate of exactly 0 or 1) and NaN
    where its tap falls on the zero padding: the header's fmaf(+0, w, .)."""
    C, H, W = 32, 4, 19
    p = cpu.block_params(C, 9)
    xyz, feat = cpu.block_inputs(2, C, H, W, 11)
    xyz[1, 0, 2, 7] = np.nan
    feat[0, 3, 1, 12] = np.nan
    got, want = run_kernel(xyz, feat, p), restate(xyz, feat, p, expf)
    assert np.isnan(want).any() and np.isfinite(want).any()
    assert same_bits(got, want)
    # the composition on the CPU, whose convolutions are direct (a device convolution may run a transform-domain
    # algorithm, which spreads a NaN over its whole tile)
    tc = cpu.composition(torch.from_numpy(xyz), torch.from_numpy(feat), p).numpy()
    assert np.array_equal(np.isnan(tc), np.isnan(want))
    p["w"][5, 1, 0, 6] = np.inf
    p["w"][40, 2, 3, 3] = -np.inf
    got, want = run_kernel(xyz, feat, p), restate(xyz, feat, p, expf)
    assert np.isnan(want[0, :, 0]).all() and np.isfinite(want[0, :, 3, :8]).all()
    assert same_bits(got, want)


def test_sac_isk_alone_elsewhere_and_on_a_side_stream(expf):
    from paddle3d_amd.ops import squeezeseg as ops

    C, H, W = 48, 3, 37
    p = cpu.block_params(C, 21)
    dp = device_params(p)
    xyz, feat = cpu.block_inputs(3, C, H, W, 22)
    whole = ops.sac_isk_forward(_t(xyz), _t(feat), *dp).cpu().numpy()
    alone = ops.sac_isk_forward(_t(xyz[1:2]), _t(feat[1:2]), *dp).cpu().numpy()
    moved = ops.sac_isk_forward(_t(xyz[[1, 0]]), _t(feat[[1, 0]]), *dp).cpu().numpy()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = ops.sac_isk_forward(_t(xyz), _t(feat), *dp)
    torch.cuda.current_stream(DEV).wait_stream(side)
    assert same_bits(alone[0], whole[1]) and same_bits(moved[0], whole[1]) and same_bits(moved[1], whole[0])
    assert same_bits(other.cpu().numpy(), whole)
    assert same_bits(whole, restate(xyz, feat, p, expf))


PROJ_CASES = {}


def proj_case(fn):
    PROJ_CASES[fn.__name__] = fn
    return fn


@proj_case
def two_scans():
    return np.concatenate([cpu.scan(1500, 1), cpu.scan(700, 2)]), [0, 1500, 2200], 8, 64


@proj_case
def ties():
    a = cpu.scan(300, 3)
    a[200:260] = a[20:80]          # equal depths in one pixel: the smaller index wins
    a[280] = a[0]                  # and the pixel of point 0 (masked out by proj_mask)
    return a, [0, 300], 8, 64


@proj_case
def empty_frames_and_bad_points():
    a = cpu.scan(400, 4)
    a[5, 0] = np.nan
    a[6, 1] = np.inf
    a[7, 2] = -np.inf
    a[8, :3] = 0
    a[9, :3] = (0, 0, 2.5)         # straight up: z / depth = 1
    a[10, 3] = np.nan              # a NaN remission is no coordinate
    return a, [0, 0, 250, 250, 400], 5, 33


@proj_case
def one_point():
    return np.array([[3.0, -4.0, -0.5, 0.7]], F32), [0, 1], 64, 1024


@proj_case
def one_pixel():
    return cpu.scan(500, 5), [0, 500], 1, 1


@proj_case
def no_points():
    return np.zeros((0, 4), F32), [0, 0, 0], 3, 7


@pytest.mark.parametrize("name", list(PROJ_CASES))
def test_range_project_equals_the_restatement(name):
    from paddle3d_amd.ops import squeezeseg as ops

    pts, off, H, W = PROJ_CASES[name]()
    want = sn.range_project(pts, off, H, W, 3.0, -25.0, MEAN, STD)
    image, idx, mask, py, px = ops.range_project(_t(pts), _t(np.asarray(off, np.int32)), H, W, 3.0, -25.0, MEAN, STD)
    assert mask.dtype == torch.bool and idx.dtype == torch.int32 and py.dtype == torch.int32
    assert np.array_equal(py.cpu().numpy(), want["proj_y"]) and np.array_equal(px.cpu().numpy(), want["proj_x"])
    assert np.array_equal(idx.cpu().numpy(), want["proj_idx"])
    assert np.array_equal(mask.cpu().numpy(), want["proj_mask"])
    assert same_bits(image.cpu().numpy(), want["image"])
    if name == "ties":
        assert (want["proj_idx"] >= 200).sum() < 40 and want["proj_idx"][0, want["proj_y"][0], want["proj_x"][0]] == 0
        assert not want["proj_mask"][0, want["proj_y"][0], want["proj_x"][0]]
    if name == "empty_frames_and_bad_points":
        assert want["proj_y"][5:9].tolist() == [-1] * 4 and want["proj_y"][9] == 0
        assert (want["proj_idx"][0] == -1).all() and (want["proj_idx"][2] == -1).all()


def test_refusals_and_errors():
    from paddle3d_amd import _lib
    from paddle3d_amd.ops import squeezeseg as ops
    from paddle3d_amd.ops._common import ptr, stream_ptr

    lib = _lib.lib()
    for C in (8, 24, 272):
        xyz, feat = (_t(a) for a in cpu.block_inputs(1, C, 2, 5, 1))
        dummy = torch.zeros(16, device=DEV)
        with launch_ledger(lib, _lib.symbols("test_memory_safety_squeezeseg_gpu")) as n:
            assert ops.sac_isk_forward(xyz, feat, *([dummy] * 6)) is None
        assert not any(n.values())
        out = torch.full_like(feat, 7.0)
        st = lib.pd3_sac_isk_forward(ptr(xyz), ptr(feat), *([ptr(dummy)] * 6), 1, C, 2, 5, ptr(out), stream_ptr(DEV))
        assert st == -3 and bool((out == 7.0).all())
    xyz, feat = (_t(a) for a in cpu.block_inputs(1, 16, 2, 5, 1))
    dp = device_params(cpu.block_params(16, 1))
    out = torch.empty_like(feat)
    assert lib.pd3_sac_isk_forward(ptr(xyz), ptr(feat), *(ptr(t) for t in dp), 1, 16, 0, 5, ptr(out), stream_ptr(DEV)) == -3
    assert lib.pd3_sac_isk_forward(ptr(xyz), ptr(feat), *(ptr(t) for t in dp), -1, 16, 2, 5, ptr(out), stream_ptr(DEV)) == -1
    assert lib.pd3_sac_isk_forward(ptr(xyz), ptr(feat), *(ptr(t) for t in dp), 0, 16, 2, 5, ptr(out), stream_ptr(DEV)) == 0
    assert lib.pd3_sac_isk_forward(ptr(None), ptr(feat), *(ptr(t) for t in dp), 1, 16, 2, 5, ptr(out), stream_ptr(DEV)) == -1
    with pytest.raises(RuntimeError):
        ops.sac_isk_forward(xyz, feat.double(), *dp)
    with pytest.raises(RuntimeError):
        ops.sac_isk_forward(xyz[:, :2], feat, *dp)
    with pytest.raises(RuntimeError):
        ops.sac_isk_forward(xyz, feat, dp[0][:1], *dp[1:])
    with pytest.raises(RuntimeError):
        ops.sac_isk_forward(xyz.cpu(), feat.cpu(), *dp)
    pts, off = _t(cpu.scan(10, 1)), _t(np.array([0, 10], np.int32))
    with pytest.raises(RuntimeError):
        ops.range_project(pts, off, 0, 8)
    with pytest.raises(RuntimeError):
        ops.range_project(pts, off, 8, 8, fov_up=-25.0, fov_down=3.0)
    with pytest.raises(RuntimeError):
        ops.range_project(pts, off, 8, 8, std=(1, 1, 0, 1, 1))
    with pytest.raises(RuntimeError):
        ops.range_project(pts, off.long(), 8, 8)
    ws = torch.empty(8, dtype=torch.int64, device=DEV)
    mean, std = np.zeros(5), np.ones(5)
    o = [torch.empty(64 * 5, device=DEV) for _ in range(5)]
    st = lib.pd3_range_project(ptr(pts), 10, ptr(off), 1, 8, 8, 3.0, -25.0, ptr(mean), ptr(std), *(ptr(t) for t in o),
                               ptr(ws), 8 * 8, stream_ptr(DEV))
    assert st == -2


def test_ops_make_no_host_sync_and_launch_once():
    from paddle3d_amd import _lib
    from paddle3d_amd.ops import squeezeseg as ops

    xyz, feat = (_t(a) for a in cpu.block_inputs(2, 32, 3, 20, 1))
    dp = device_params(cpu.block_params(32, 1))
    pts, off = _t(cpu.scan(300, 1)), _t(np.array([0, 100, 300], np.int32))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with launch_ledger(_lib.lib(), _lib.symbols("test_memory_safety_squeezeseg_gpu")) as n:
            y = ops.sac_isk_forward(xyz, feat, *dp)
            image = ops.range_project(pts, off, 8, 64)[0]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert n == {"pd3_sac_isk_forward": 1, "pd3_range_project": 1}
    assert tuple(y.shape) == (2, 32, 3, 20) and tuple(image.shape) == (2, 5, 8, 64)


# ---- against the reference's golden results ---------------------------------------------------------------------------
NAMES = ("pd3_sac_isk_forward", "pd3_range_project")


@pytest.mark.parametrize("tag", list(mk.BLOCKS))
def test_sac_isk_on_the_golden_cases(golden, expf, tag):
    p, inp = cpu.golden_block_params(tag), mk.inputs(tag)
    got = run_kernel(inp["xyz"], inp["feature"], p)
    assert same_bits(got, restate(inp["xyz"], inp["feature"], p, expf))
    cpu.check_result(golden, tag, "y", got)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag", list(mk.BLOCKS))
def test_block_against_the_reference(golden, tag, fused):
    from paddle3d_amd import _lib

    with launch_ledger(_lib.lib(), NAMES) as n:
        y, out = cpu.block_outputs(tag, fused, DEV)
    assert n["pd3_sac_isk_forward"] == (2 if fused else 0)  # first_layer alone, then the whole block
    cpu.check_result(golden, tag, "y", y)
    cpu.check_result(golden, tag, "out", out)


@pytest.mark.parametrize("fused", ["force", True, False])
def test_network_against_the_reference(golden, fused):
    """The first stage with its downsample, the 21-layer network's last map, the head's logits within the reference's
    bounds; the argmax on every pixel and the per-point labels equal.  7 SAC blocks, each one launch, twice
    (export_forward and forward) when forced; by default the 4 blocks of up to 128 channels."""
    from paddle3d_amd import _lib

    with launch_ledger(_lib.lib(), NAMES) as n:
        out = cpu.net_outputs(fused, DEV)
    assert n["pd3_sac_isk_forward"] == {"force": 14, True: 8, False: 0}[fused]
    cpu.check_net(golden, out)


@pytest.mark.parametrize("kernel", ["direct", "winograd", "winograd43"])
def test_network_with_a_conv3x3_kernel_against_the_reference(golden, kernel):
    """The 3x3 stride-1 layers on a kernel of ops/conv.py where its predicate takes them (torch elsewhere)."""
    from paddle3d_amd import _lib
    from paddle3d_amd.squeezesegv3 import conv3x3_kernel_for

    assert conv3x3_kernel_for(kernel, 256, 256, 8, 4, DEV) == kernel and conv3x3_kernel_for(kernel, 256, 256, 8, 3, DEV) == "torch"
    symbol = {"direct": "pd3_conv3x3_bias_relu", "winograd": "pd3_conv3x3_winograd_bias_relu",
              "winograd43": "pd3_conv3x3_winograd43_bias_relu"}[kernel]
    with launch_ledger(_lib.lib(), (symbol,)) as n:
        out = cpu.net_outputs(True, DEV, conv3x3=kernel)
    assert n[symbol] > 0
    cpu.check_net(golden, out)


def test_range_project_on_the_golden_scans(golden):
    from paddle3d_amd.ops import squeezeseg as ops

    pts, off = mk.scans()
    image, idx, mask, py, px = (t.cpu().numpy() for t in ops.range_project(_t(pts), _t(off), mk.SCAN_H, mk.SCAN_W, 3.0,
                                                                            -25.0, mk.MEAN, mk.STD))
    for f, tag in enumerate(mk.SCANS):
        lo, hi = off[f], off[f + 1]
        assert np.array_equal(px[lo:hi], golden[f"{tag}_proj_x"]) and np.array_equal(py[lo:hi], golden[f"{tag}_proj_y"])
        assert np.array_equal(idx[f], golden[f"{tag}_proj_idx"]) and np.array_equal(mask[f], golden[f"{tag}_proj_mask"])
        cpu.check_result(golden, tag, "image", image[f])


def test_refused_shapes_fall_back(golden):
    """C = 24 (no multiple of 16): the fused block launches nothing and gives the unfused block's bits; fused=False never
    launches."""
    from paddle3d_amd import _lib
    from paddle3d_amd import squeezesegv3 as sq

    torch.manual_seed(3)
    xyz, feat = torch.randn(1, 3, 4, 9, device=DEV), torch.randn(1, 24, 4, 9, device=DEV)
    blocks = [sq.SACISKBlock(24, fused=f).to(DEV).eval() for f in (True, False)]
    blocks[1].load_state_dict(blocks[0].state_dict())
    with torch.no_grad(), launch_ledger(_lib.lib(), NAMES) as n:
        a, b = (blk(xyz, feat)[1] for blk in blocks)
    assert not any(n.values()) and torch.equal(a, b)
    assert not blocks[0].takes_kernel(feat) and blocks[0].takes_kernel(torch.zeros(1, 32, 4, 9, device=DEV))
    # C = 256 is opt-in
    wide = torch.zeros(1, 256, 2, 5, device=DEV)
    assert not sq.SACISKBlock(256).takes_kernel(wide) and sq.SACISKBlock(256, fused="force").takes_kernel(wide)
    assert sq.SACISKBlock(128).takes_kernel(wide[:, :128]) and not sq.SACISKBlock(128, fused=False).takes_kernel(wide[:, :128])


def test_model_forward_makes_no_host_sync(golden):
    from paddle3d_amd.ops import squeezeseg as ops

    model = cpu.build("net", True, DEV)
    pts, off = (_t(a) for a in mk.scans())
    inp = mk.inputs("net")
    image = _t(inp["image"])
    with torch.no_grad():
        model.export_forward(image)  # folds and packs once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            img, _, _, py, px = ops.range_project(pts, off, 8, 32, 3.0, -25.0, mk.MEAN, mk.STD)
            labels = model(img, py, px, off)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(labels.shape) == (pts.shape[0],) and labels.dtype == torch.int64
