"""pd3_aspp_forward and pd3_depth_softmax_split on the GPU: bit-equal to their NumPy restatement
(tests/golden/depthnet_numpy.py: per branch one fmaf chain over the in-range taps in ascending (ky, kx) and per tap over
ascending input channels; glibc's expf; a NaN matches any NaN) at the smallest shapes that reach each border.

ASPP: maps of 1 x 1 (only centre taps), 7 x 7 (dilation 6 just reaches one row and one column), 13 x 19, 19 x 37
(dilation 18 reaches) and 16 x 44; a single row of 15, 16, 17, 63, 64 and 65 pixels; a pixel tile that ends inside the
second image of a batch; Cin of 16 and 48; Cmid of 16, 48 and 512 (the last on a 2 x 3 map); dilations (1, 2, 3), with
which every tap is in range on a small map; a NaN and an Inf pixel; an Inf weight on a tap that is out of range
everywhere, which stays finite, and one on a tap that only some pixels of a tile have, which reaches those pixels alone.
The three launch forms (4, 2 and 1 channel tiles per wave, chosen from the pixel and channel counts) are reached with
many 8 x 16 frames and held to each other with torch.equal and, on one frame, to the restatement.
Tail: D of 1, 7, 64 and 118, C of 0, 1, 16 and 80, H W of 1, 63, 64 and 65, logits at which expf underflows to
subnormals and to 0, a NaN column.
A frame gives the same bits alone, elsewhere in the batch and on a side stream.  The modules of paddle3d_amd.bevdepth in
their three forms are held to the reference's golden results within the stored bounds, the view transformer's bev_feat
with both settings of accelerate; a fused ASPP is one call of its entry point, the tail one; a forward makes no host
synchronisation; a refused shape falls back to the torch composition; a forward in training mode is refused."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from guarded import launch_ledger  # noqa: E402

import depthnet_numpy as dn  # noqa: E402
import make_depthnet_golden as mk  # noqa: E402
import test_depthnet_cpu as cpu  # noqa: E402
from test_depthnet_cpu import expf, golden  # noqa: E402,F401

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
ASPP, TAIL = "pd3_aspp_forward", "pd3_depth_softmax_split"
GEO = ("rots", "trans", "cam2imgs", "post_rots", "post_trans", "bda")


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(got, want):
    """Bit equality of two float32 arrays, a NaN matching any NaN (the sign and payload of a NaN are not part of the
    arithmetic the header fixes)."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and
                np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def random_case(seed, N, ci, cm, H, W, dilations=(6, 12, 18)):
    """Seeded x and the unpacked parameter dict of tests/golden/depthnet_numpy.py, as float32 arrays."""
    rng = np.random.default_rng(seed)
    vec = lambda lo, hi, n: rng.uniform(lo, hi, n).astype(F32)  # noqa: E731
    p = dict(w=[(rng.standard_normal((cm, ci, k, k)) / np.sqrt(k * k * ci)).astype(F32) for k in (1, 3, 3, 3)],
             scale=vec(0.5, 1.5, 4 * cm), shift=vec(-0.5, 0.5, 4 * cm),
             wg=(rng.standard_normal((cm, ci)) / np.sqrt(ci)).astype(F32), gs=vec(0.5, 1.5, cm), gb=vec(-0.5, 0.5, cm),
             w1=(rng.standard_normal((cm, 5 * cm)) / np.sqrt(5 * cm)).astype(F32), s1=vec(0.5, 1.5, cm),
             b1=vec(-0.5, 0.5, cm))
    return dict(x=rng.standard_normal((N, ci, H, W)).astype(F32), p=p, dilations=tuple(dilations))


def packed(p):
    from paddle3d_amd.ops import depthnet as ops

    cm, ci = p["wg"].shape
    return ops.pack_aspp([_t(w) for w in p["w"]],
                         [(_t(p["scale"][b * cm:(b + 1) * cm]), _t(p["shift"][b * cm:(b + 1) * cm])) for b in range(4)],
                         _t(p["wg"].reshape(cm, ci, 1, 1)), (_t(p["gs"]), _t(p["gb"])),
                         _t(p["w1"].reshape(cm, 5 * cm, 1, 1)), (_t(p["s1"]), _t(p["b1"])))


def kernel(c, x=None, pk=None):
    from paddle3d_amd.ops import depthnet as ops

    y = ops.aspp_forward(_t(c["x"]) if x is None else x, packed(c["p"]) if pk is None else pk, c["dilations"])
    assert y is not None
    return y


def restated(c):
    return dn.aspp_forward(c["x"], c["p"], c["dilations"])


# (N, H, W): one pixel; 7 x 7: dilation 6 reaches one row and one column; 13 x 19: dilation 12; 19 x 37: dilation 18; the
# model's map; one row around 16 and around 64 pixels (the tile's end and one past it); 45 pixels an image: the first tile
# ends inside the second image
SIZES = ((1, 1, 1), (1, 7, 7), (1, 13, 19), (1, 19, 37), (1, 16, 44), (1, 1, 15), (1, 1, 16), (1, 1, 17), (1, 1, 63),
         (1, 1, 64), (1, 1, 65), (3, 5, 9))


@pytest.mark.parametrize("N,H,W", SIZES)
def test_aspp_map_sizes(N, H, W):
    c = random_case(100 + 7 * H + W, N, 16, 16, H, W)
    assert same_bits(kernel(c).cpu().numpy(), restated(c))


@pytest.mark.parametrize("ci,cm,H,W", [(48, 16, 5, 9), (16, 48, 5, 9), (48, 48, 7, 13), (16, 512, 2, 3)])
def test_aspp_channel_counts(ci, cm, H, W):
    c = random_case(ci + cm, 2, ci, cm, H, W)
    assert same_bits(kernel(c).cpu().numpy(), restated(c))


def test_aspp_small_dilations_every_tap_in_range():
    c = random_case(5, 2, 16, 16, 5, 7, dilations=(1, 2, 3))
    count = []
    dn.aspp_branches(c["x"], c["p"], c["dilations"], count=count)
    assert count == [35, (5 + 8) * (7 + 12), (5 + 6) * (7 + 10), (5 + 4) * (7 + 8)]  # every tap has pixels
    assert same_bits(kernel(c).cpu().numpy(), restated(c))


def test_aspp_hostile_data():
    """A NaN pixel in the first image and an Inf pixel in the second (the third stays finite); an Inf weight on a tap that
    no pixel of a 7 x 7 map has in range; an Inf weight on a tap that some pixels of a tile have and others lack."""
    c = random_case(77, 3, 16, 16, 7, 9)
    c["x"][0, 3, 2, 4], c["x"][1, 5, 0, 0] = np.nan, np.inf
    got, want = kernel(c).cpu().numpy(), restated(c)
    assert same_bits(got, want)
    assert np.isnan(want[0]).all() and not np.isfinite(want[1]).all() and np.isfinite(want[2]).all()
    c2 = random_case(78, 2, 16, 16, 7, 7)
    c2["p"]["w"][2][5, 0, 0, 0], c2["p"]["w"][3][7, 3, 2, 1] = np.inf, -np.inf  # dilations 12 and 18, off-centre taps
    got = kernel(c2).cpu().numpy()
    assert same_bits(got, restated(c2)) and np.isfinite(got).all()
    c3 = random_case(79, 1, 16, 16, 7, 7)
    c3["p"]["w"][1][5, 2, 0, 0] = np.inf  # dilation 6, tap (0, 0): in range for the pixel (6, 6) alone
    c3["x"][0, 2] = np.abs(c3["x"][0, 2]) + 1  # so that the product is Inf, not a NaN
    ws = dn.aspp_branches(c3["x"], c3["p"])
    assert np.isinf(ws[0, 16 + 5, 6, 6]) and np.isfinite(np.delete(ws[0, 16 + 5].reshape(-1), 48)).all()
    assert same_bits(kernel(c3).cpu().numpy(), restated(c3))


def test_aspp_three_launch_forms_agree():
    """8 x 16 frames, Cmid = 256: 256, 128 and 32 frames launch the forms with 4, 2 and 1 channel tiles per wave
    (ops.tiles_per_wave restates the choice).  Every frame's output is the same bits in each, and the last frame equals
    the restatement."""
    from paddle3d_amd.ops import depthnet as ops

    frames = (256, 128, 32)
    c = random_case(256, frames[0], 16, 256, 8, 16)
    assert [ops.tiles_per_wave(n * 128, 256) for n in frames] == [4, 2, 1]
    x, pk = _t(c["x"]), packed(c["p"])
    full = kernel(c, x, pk)
    for n in frames[1:]:
        assert torch.equal(kernel(c, x[-n:], pk), full[-n:])
    one = dict(c, x=c["x"][-1:])
    assert same_bits(full[-1:].cpu().numpy(), restated(one))


def test_aspp_frame_alone_in_a_batch_and_on_a_side_stream():
    c = random_case(31, 3, 48, 48, 5, 9)  # 45 pixels a frame: the tiles end inside the second and third frame
    x, pk = _t(c["x"]), packed(c["p"])
    full = kernel(c, x, pk)
    for i in range(3):
        assert torch.equal(kernel(c, x[i:i + 1], pk), full[i:i + 1])
    assert torch.equal(kernel(c, x[[2, 0, 1]], pk), full[[2, 0, 1]])
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        again = kernel(c, x, pk)
    side.synchronize()
    assert torch.equal(again, full)


# (N, D, C, H, W): H W of 1, 63, 64, 65 and more than one tile
TAILS = ((1, 1, 1, 1, 1), (2, 7, 16, 7, 9), (2, 64, 80, 8, 8), (1, 118, 80, 5, 13), (3, 118, 1, 1, 64), (2, 7, 80, 1, 65),
         (2, 4, 0, 3, 3), (2, 118, 80, 16, 44))


def tail(x, D):
    from paddle3d_amd.ops import depthnet as ops

    out = ops.depth_softmax_split(_t(x), D)
    assert out is not None
    return out


@pytest.mark.parametrize("N,D,C,H,W", TAILS)
def test_tail_sizes(expf, N, D, C, H, W):  # noqa: F811
    x = (np.random.default_rng(D + C + H * W).standard_normal((N, D + C, H, W)) * 3).astype(F32)
    depth, feat = tail(x, D)
    want_d, want_f = dn.depth_softmax_split(x, D, expf)
    assert tuple(feat.shape) == (N, H, W, C) and feat.is_contiguous()
    assert same_bits(depth.cpu().numpy(), want_d) and np.array_equal(feat.cpu().numpy(), want_f)


def test_tail_hostile_logits(expf):  # noqa: F811
    """Differences to the maximum at which expf gives subnormals (-88 .. -103.9) and 0 (below), logits of +-Inf, a column
    with a NaN first, one with a NaN later, and a column of equal logits."""
    rng = np.random.default_rng(11)
    x = rng.standard_normal((2, 7 + 3, 4, 5)).astype(F32)
    values = np.array([0, -87.5, -88.5, -95, -103.5, -103.97, -104.5, -200, -1e30, -np.inf], F32)
    x[0, :7] = values[rng.integers(0, values.size, (7, 4, 5))]
    x[0, 3, :, 0] = 0  # the maximum of those columns
    x[1, 0, 0, 0], x[1, 4, 1, 1], x[1, 2, 2, 2] = np.nan, np.nan, np.inf
    x[1, :7, 3, 3] = 1.5
    depth, feat = tail(x, 7)
    want_d, want_f = dn.depth_softmax_split(x, 7, expf)
    e = expf(np.array([-88.5, -103.5, -104.5], F32))
    assert 0 < e[0] < 2.0 ** -126 and 0 < e[1] < 2.0 ** -126 and e[2] == 0
    assert same_bits(depth.cpu().numpy(), want_d) and np.array_equal(feat.cpu().numpy(), want_f, equal_nan=True)
    assert np.isnan(want_d[1, :, 0, 0]).all() and np.isnan(want_d[1, :, 1, 1]).all() and np.isnan(want_d[1, :, 2, 2]).all()
    assert np.array_equal(want_d[1, :, 3, 3], np.full(7, F32(1) / F32(7)))
    assert np.isfinite(want_d[0]).all() and np.isfinite(want_d[1, :, 0, 1]).all()


def test_tail_frame_alone_in_a_batch_and_on_a_side_stream():
    x = (np.random.default_rng(3).standard_normal((3, 118 + 80, 5, 9)) * 2).astype(F32)
    depth, feat = tail(x, 118)
    for i in range(3):
        d1, f1 = tail(x[i:i + 1], 118)
        assert torch.equal(d1, depth[i:i + 1]) and torch.equal(f1, feat[i:i + 1])
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        d2, f2 = tail(x, 118)
    side.synchronize()
    assert torch.equal(d2, depth) and torch.equal(f2, feat)


@pytest.mark.parametrize("tag", [*mk.ASPPS, *mk.NETS])
def test_modules_in_three_forms_against_the_reference(golden, tag):  # noqa: F811
    """fused="force", the default and the torch composition within the stored bounds; the forced form calls the ASPP
    entry point once, the unfused form never; the default follows ops.depthnet.fused_by_default."""
    from paddle3d_amd import _lib
    from paddle3d_amd.ops import depthnet as ops

    xs = [_t(a) for a in mk.inputs(tag)]
    n_maps, _, h, w = xs[0].shape
    default = int(ops.fused_by_default("aspp", n_maps, 16, 16, h, w))  # these maps are below the measured border
    assert default == 0
    for fused, launches in (("force", 1), (True, default), (False, 0)):
        m = cpu.build(golden, tag, fused).to(DEV)
        with torch.no_grad(), launch_ledger(_lib.lib(), (ASPP,)) as n:
            y = m(*xs)
        assert n[ASPP] == launches, (fused, dict(n))
        assert tuple(y.shape) == golden[f"{tag}_y"].shape
        assert cpu.err(y.cpu().numpy(), golden[f"{tag}_y"]) <= float(golden[f"{tag}_y_bound"]), fused


def test_aspp_module_equals_the_restatement(golden):  # noqa: F811
    """The forced module is the entry point on the folded parameters: the restatement's bits."""
    for tag in mk.ASPPS:
        m = cpu.build(golden, tag, "force").to(DEV)
        with torch.no_grad():
            y = m(_t(mk.inputs(tag)[0]))
        st = mk.state(tag, mk.key_shapes(golden, tag))
        assert same_bits(y.cpu().numpy(), dn.aspp_forward(mk.inputs(tag)[0], dn.aspp_params(st))), tag


def _vt_input(golden):  # noqa: F811
    cams = {k: _t(v) for k, v in mk.rig("vt").items()}
    return [_t(mk.inputs("vt")[0]), *[cams[k] for k in GEO], _t(golden["vt_mlp_input"])]


@pytest.mark.parametrize("accelerate", [False, True])
def test_view_transformer_against_the_reference(golden, accelerate):  # noqa: F811
    from paddle3d_amd import _lib
    from paddle3d_amd.ops import depthnet as ops

    inp = _vt_input(golden)
    default = int(ops.fused_by_default("tail", 3, 15, 16, 4, 11))  # 132 pixels: inside the measured border
    assert default == 1
    for fused, tails in (("force", 1), (True, default), (False, 0)):
        m = cpu.build(golden, "vt", fused, accelerate).to(DEV)
        mlp = m.get_mlp_input(*inp[1:7])
        assert np.array_equal(mlp.cpu().numpy(), golden["vt_mlp_input"])
        for _ in range(2):  # with accelerate the second forward reuses the index sets
            with torch.no_grad(), launch_ledger(_lib.lib(), (ASPP, TAIL, "pd3_voxel_pooling_prepare")) as n:
                bev, depth = m(inp)
            assert n[TAIL] == tails, (fused, dict(n))
            assert tuple(bev.shape) == golden["vt_y"].shape and bool(bev.any())
            assert cpu.err(bev.cpu().numpy(), golden["vt_y"]) <= float(golden["vt_y_bound"]), (fused, accelerate)
            assert cpu.err(depth.cpu().numpy(), golden["vt_depth"]) <= float(golden["vt_depth_bound"]), fused
        assert n["pd3_voxel_pooling_prepare"] == (0 if accelerate else 1)


def test_no_host_synchronisation(golden):  # noqa: F811
    """DepthNet forced, and the whole view transformer with accelerate=True once its index sets exist."""
    from paddle3d_amd import _lib

    net = cpu.build(golden, "dn", "force").to(DEV)
    xs = [_t(a) for a in mk.inputs("dn")]
    vt = cpu.build(golden, "vt", "force", True).to(DEV)
    inp = _vt_input(golden)
    with torch.no_grad():
        net(*xs)  # folds and packs once
        vt(inp)   # prepares the index sets once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad(), launch_ledger(_lib.lib(), (ASPP, TAIL)) as n:
            y = net(*xs)
            bev, _ = vt(inp)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert n[ASPP] == 2 and n[TAIL] == 1
    assert cpu.err(y.cpu().numpy(), golden["dn_y"]) <= float(golden["dn_y_bound"])
    assert cpu.err(bev.cpu().numpy(), golden["vt_y"]) <= float(golden["vt_y_bound"])


def test_refused_shapes_fall_back_and_training_is_refused():
    """24 channels: the predicate refuses, the forced module runs the composition (the same operators as fused=False)."""
    from paddle3d_amd import _lib, bevdepth as bd

    torch.manual_seed(3)
    forced, plain = bd.ASPP(24, 24, fused="force").to(DEV).eval(), bd.ASPP(24, 24, fused=False).to(DEV).eval()
    plain.load_state_dict(forced.state_dict())
    x = torch.randn(2, 24, 5, 6, device=DEV)
    with torch.no_grad(), launch_ledger(_lib.lib(), (ASPP,)) as n:
        y = forced(x)
        assert n[ASPP] == 0 and not forced.takes_kernel(x) and torch.equal(y, plain(x)) and bool(y.any())
    m = bd.ASPP(16, 16, fused="force").to(DEV)
    x = torch.randn(1, 16, 4, 4, device=DEV)
    assert m.training and m.takes_kernel(x)
    with pytest.raises(RuntimeError, match="inference path only"):
        m(x)
    assert not m.takes_kernel(x.double()) and not m.takes_kernel(x.cpu())
