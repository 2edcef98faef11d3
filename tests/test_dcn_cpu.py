"""The modulated deformable convolution and the MMResNet modules on the CPU, against what the reference's own Python
computed around the stand-in op (tests/golden/python_dcn.npz, made by make_dcn_golden.py): the NumPy restatement of
pd3_deform_conv2d_forward (tests/golden/dcn_numpy.py) in float64 against the stand-in's float64 run to 1e-12 (two
independent formulations of one definition) and in float32 within the stored bounds; the modules of
paddle3d_amd.mm_resnet with fused=False (the torch composition, also what a refused shape runs) within the stored
bounds; zero offsets with a mask of ones against F.conv2d; the initial state against 0.5 * conv2d; the packer's round
trip; the state-dict keys against the reference's and a strict load of a synthetic .pdparams; MMResNet's stage shapes in
both styles; deform_conv2d_supported's borders; every refusal status of the entry point, none of which launches.

Bounds: the ones the maker stored, 4 x the largest error of the reference's own fp32 run against its fp64 run (one fp32
ulp of the largest output as a floor)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import dcn_numpy as dn  # noqa: E402
import make_dcn_golden as mk  # noqa: E402

F32 = np.float32
F64 = np.float64


@pytest.fixture(scope="module")
def golden():
    return mk.load()


@pytest.fixture(scope="module")
def expf():
    from oracle import pyoracle as O

    return lambda x: O.libm_eval(2, np.ascontiguousarray(x, F32).reshape(-1))


def build(g, tag, fused=False):
    """The module of case `tag` with the case's parameters, loaded strictly under the reference's keys."""
    from paddle3d_amd import mm_resnet as mr
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    if tag in mk.CASES:
        c = mk.CASES[tag]
        m = mr.DeformableConvV2(c["cin"], c["cout"], 3, stride=c["stride"], padding=c["dilation"], dilation=c["dilation"],
                                fused=fused)
    elif tag in mk.BLOCKS:
        c = mk.BLOCKS[tag]
        m = mr.Bottleneck(4 * c["planes"], c["planes"], style="caffe", dcn=mk.DCN, fused=fused)
    else:
        c = mk.STAGE[tag]
        m = mr.ResLayer(mr.Bottleneck, c["inplanes"], c["planes"], 2, stride=2, style="caffe", dcn=mk.DCN, fused=fused)
    assert load_paddle_state_dict(m, mk.state(tag, mk.key_shapes(g, tag)), strict=True) == []
    return m.eval()


def case_arrays(g, tag, dtype=F32):
    """x, conv_offset's output (torch's convolution in `dtype`; the stored float64 one for F64), the DCN weight and bias."""
    c, st = mk.CASES[tag], mk.state(tag, mk.key_shapes(g, tag))
    x = mk.inputs(tag)
    if dtype == F64:
        om = g[f"{tag}_offset_mask"]
    else:
        om = TF.conv2d(torch.from_numpy(x), torch.from_numpy(st["conv_offset.weight"]),
                       torch.from_numpy(st["conv_offset.bias"]), c["stride"], 1).numpy()
    return x.astype(dtype), om, st["conv_dcn.weight"].astype(dtype), st["conv_dcn.bias"].astype(dtype)


def restated(g, tag, expf):
    c = mk.CASES[tag]
    x, om, w, b = case_arrays(g, tag)
    return dn.deform_conv2d(x, om[:, :18], om[:, 18:], w, None, b, False, True, c["stride"], c["dilation"], c["dilation"],
                            expf)


def err(a, b):
    return float(np.abs(np.asarray(a, F64) - np.asarray(b, F64)).max())


@pytest.mark.parametrize("tag", list(mk.CASES))
def test_restatement_in_float64_is_the_stand_in(golden, tag):
    c = mk.CASES[tag]
    x, om, w, b = case_arrays(golden, tag, F64)
    y = dn.deform_conv2d_f64(x, om[:, :18], om[:, 18:], w, b, c["stride"], c["dilation"], c["dilation"], True)
    assert y.shape == golden[f"{tag}_y"].shape
    assert err(y, golden[f"{tag}_y"]) <= 1e-12


@pytest.mark.parametrize("tag", list(mk.CASES))
def test_restatement_in_float32_within_the_bounds(golden, expf, tag):
    y = restated(golden, tag, expf)
    assert y.dtype == F32 and err(y, golden[f"{tag}_y"]) <= float(golden[f"{tag}_y_bound"])


@pytest.mark.parametrize("tag", [*mk.CASES, *mk.BLOCKS, *mk.STAGE])
def test_modules_torch_form_within_the_bounds(golden, tag):
    m = build(golden, tag, fused=False)
    with torch.no_grad():
        y = m(torch.from_numpy(mk.inputs(tag))).numpy()
    assert y.shape == golden[f"{tag}_y"].shape
    assert err(y, golden[f"{tag}_y"]) <= float(golden[f"{tag}_y_bound"])


def test_zero_offsets_and_a_mask_of_ones_is_conv2d(golden, expf):
    from paddle3d_amd.mm_resnet import deform_conv2d_composition

    for tag in ("a", "b2", "e"):
        c = mk.CASES[tag]
        x, om, w, _ = case_arrays(golden, tag)
        want = TF.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), None, c["stride"], c["dilation"],
                         c["dilation"]).numpy()
        zeros, ones = np.zeros_like(om[:, :18]), np.ones_like(om[:, 18:])
        bound = float(golden[f"{tag}_y_bound"])
        got = dn.deform_conv2d(x, zeros, ones, w, stride=c["stride"], padding=c["dilation"], dilation=c["dilation"])
        assert err(got, want) <= bound
        assert np.array_equal(got, dn.deform_conv2d(x, zeros, None, w, stride=c["stride"], padding=c["dilation"],
                                                    dilation=c["dilation"]))  # DCNv1: m = 1
        t = torch.from_numpy
        got = deform_conv2d_composition(t(x), t(zeros), t(ones), t(w), None, c["stride"], c["dilation"], c["dilation"])
        assert err(got.numpy(), want) <= bound


def test_initial_state_is_half_the_convolution(golden, expf):
    x, om, w, b = case_arrays(golden, "d", F64)
    assert not om.any()
    want = 0.5 * TF.conv2d(torch.from_numpy(x), torch.from_numpy(w), None, 1, 1).numpy() + b[None, :, None, None]
    assert err(golden["d_y"], want) <= 1e-12
    assert err(restated(golden, "d", expf), want) <= float(golden["d_y_bound"])


def test_pinned_case_reaches_the_borders(golden):
    """The maker's conditions on the committed file: case c samples outside, on -1 and H, and on integers."""
    c, om = mk.CASES["c"], golden["c_offset_mask"]
    for tap, dy, dx in mk.PINNED:
        assert (om[:, 2 * tap] == dy).all() and (om[:, 2 * tap + 1] == dx).all()
    h0 = np.arange(c["H"]) - 1 + om[0, 0, :, 0]            # tap 0: row -1 at ho = 0, integers after it
    h8 = np.arange(c["H"]) - 1 + 2 + om[0, 16, :, 0]       # tap 8: + 3 reaches H and H + 1
    assert h0[0] == -1 and h0[1] == 0 and c["H"] in h8 and c["H"] + 1 in h8
    assert np.abs(om[:, :18]).max() > 8


def test_packer_round_trip():
    from paddle3d_amd.ops import deform_conv as ops

    for ci, co in ((16, 16), (48, 272), (32, 512)):
        rng = np.random.default_rng(ci + co)
        w = torch.from_numpy(rng.standard_normal((co, ci, 3, 3)).astype(F32))
        pw = ops.pack_deform_conv_weight(w)
        assert tuple(pw.shape) == (9 * ci // 16, co // 16, 64, 4) and pw.is_contiguous()
        assert torch.equal(ops.unpack_deform_conv_weight(pw, ci), w)
        t, nt, lane, ks = 9 * ci // 16 - 1, co // 16 - 1, 37, 2  # the lane order of the kernel's header
        assert pw[t, nt, lane, ks] == w.reshape(co, 9 * ci)[16 * nt + (lane & 15), 16 * t + 4 * ks + (lane >> 4)]
    for bad in ((16, 16, 1, 1), (16, 8, 3, 3), (24, 16, 3, 3), (16, 16, 3)):
        with pytest.raises(RuntimeError):
            ops.pack_deform_conv_weight(torch.zeros(bad))
    with pytest.raises(RuntimeError):
        ops.unpack_deform_conv_weight(torch.zeros(9, 1, 64, 4), 32)


def _reference_names(module):
    return {k.replace(".running_mean", "._mean").replace(".running_var", "._variance"): list(v.shape)
            for k, v in module.state_dict().items() if not k.endswith("num_batches_tracked")}


def test_state_dict_keys_are_the_references(golden, tmp_path):
    from paddle3d_amd import mm_resnet as mr
    from paddle3d_amd.checkpoint import load_paddle_state_dict, save_pdparams

    for tag in (*mk.CASES, *mk.BLOCKS, *mk.STAGE):
        assert _reference_names(build(golden, tag)) == mk.key_shapes(golden, tag), tag
    assert set(mk.key_shapes(golden, "a")) == {"conv_offset.weight", "conv_offset.bias", "conv_dcn.weight",
                                               "conv_dcn.bias"}
    shapes = mk.key_shapes(golden, "r50")
    net = mr.mm_resnet50_caffe_dcn()
    assert _reference_names(net) == shapes and net.out_indices == (2, 3)
    assert sum(k.endswith("conv_dcn.weight") for k in shapes) == 9 and "layer2.0.conv2.weight" in shapes
    assert not any(k.endswith("conv_dcn.bias") for k in shapes)  # the bottleneck's convolutions have no bias
    rng = np.random.default_rng(5)
    state = {k: rng.standard_normal(s).astype(F32) for k, s in shapes.items()}
    path = str(tmp_path / "r50.pdparams")
    save_pdparams(state, path)
    assert load_paddle_state_dict(net, path, strict=True) == []
    own = net.state_dict()
    for k in ("layer3.5.conv2.conv_offset.bias", "layer4.2.conv2.conv_dcn.weight", "bn1._mean", "layer4.0.downsample.1._variance"):
        name = k.replace("._mean", ".running_mean").replace("._variance", ".running_var")
        assert np.array_equal(own[name].numpy(), state[k]), k
    del state["layer3.0.conv2.conv_offset.weight"]
    save_pdparams(state, path)
    with pytest.raises(RuntimeError):
        load_paddle_state_dict(mr.mm_resnet50_caffe_dcn(), path, strict=True)


def test_fresh_module_is_the_references_initial_state():
    from paddle3d_amd.mm_resnet import DeformableConvV2

    m = DeformableConvV2(16, 32, 3)
    assert not m.conv_offset.weight.any() and not m.conv_offset.bias.any() and not m.conv_dcn.bias.any()
    assert tuple(m.conv_dcn.weight.shape) == (32, 16, 3, 3) and tuple(m.conv_offset.weight.shape) == (27, 16, 3, 3)
    assert DeformableConvV2(16, 32, 3, bias_attr=False).conv_dcn.bias is None
    with pytest.raises(ValueError):
        DeformableConvV2(16, 32, 3, fused="yes")


@pytest.mark.parametrize("style", ["caffe", "pytorch"])
def test_mm_resnet_stage_shapes_and_strides(style):
    from paddle3d_amd import mm_resnet as mr

    net = mr.MMResNet(50, base_channels=8, style=style, dcn=mk.DCN, stage_with_dcn=(False, False, True, True), fused=False)
    assert not net.training and [len(getattr(net, n)) for n in net.res_layers] == [3, 4, 6, 3]
    with torch.no_grad():
        outs = net(torch.zeros(1, 3, 64, 96))
    assert [tuple(o.shape) for o in outs] == [(1, 32, 16, 24), (1, 64, 8, 12), (1, 128, 4, 6), (1, 256, 2, 3)]
    first = net.layer2[0]
    assert (first.conv1.stride, first.conv2.stride) == (((2, 2), (1, 1)) if style == "caffe" else ((1, 1), (2, 2)))
    assert isinstance(net.layer2[1].conv2, torch.nn.Conv2d)
    assert all(isinstance(b.conv2, mr.DeformableConvV2) for b in (*net.layer3, *net.layer4))
    dcn0 = net.layer3[0].conv2  # the stage's stride is conv1's in caffe style, the DCN's in pytorch style
    assert dcn0.conv_dcn.stride == dcn0.conv_offset.stride[0] == (1 if style == "caffe" else 2)
    assert len(mr.MMResNet(101, base_channels=8, out_indices=(3,)).layer3) == 23
    net.train()  # norm_eval: the statistics stay frozen
    assert net.training and not any(m.training for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))
    for kwargs in (dict(depth=18), dict(depth=50, conv_cfg=dict(type_name="Conv2D")),
                   dict(depth=50, norm_cfg=dict(type_name="GroupNorm"))):
        with pytest.raises(NotImplementedError):
            mr.MMResNet(**kwargs)
    with pytest.raises(KeyError):
        mr.MMResNet(51)


def test_supported_borders():
    from paddle3d_amd.ops import deform_conv as ops

    def ok(ci, co, H=8, W=8, N=1, **kw):
        return ops.deform_conv2d_supported(ci, co, H, W, N, **kw)

    for c in (16, 32, 48, 256, 272, 496, 512):
        assert ok(c, 16) and ok(16, c) and ok(c, c, 32, 88, 6, stride=1, padding=1, dilation=1)
    for c in (0, 8, 15, 17, 24, 513, 528, 1024):
        assert not ok(c, 16) and not ok(16, c)
    assert ok(16, 16, stride=2) and not ok(16, 16, stride=3) and not ok(16, 16, stride=0)
    assert ok(16, 16, 5, 5, dilation=2) and not ok(16, 16, dilation=0) and not ok(16, 16, padding=-1)
    assert not ok(16, 16, kernel_size=1) and not ok(16, 16, kernel_size=(3, 5)) and ok(16, 16, kernel_size=(3, 3))
    assert not ok(16, 16, groups=2) and not ok(16, 16, deformable_groups=2)
    # the image against the dilated kernel: 3 rows without padding give one output row, 2 give none
    assert ok(16, 16, 3, 3) and not ok(16, 16, 2, 3) and ok(16, 16, 2, 3, padding=1) and not ok(16, 16, 4, 4, dilation=2)
    assert ok(16, 16, 1, 1, padding=1) and not ok(16, 16, 0, 1, padding=1) and not ops.deform_conv2d_supported(16, 16)
    # fewer than 2^30 tiles of 64 pixels: 8 x 8 outputs per image
    assert ops.PIXEL_TILE == 64 and ops.MAX_CHANNELS == 512
    assert ok(16, 16, 8, 8, 2 ** 30 - 1, padding=1) and not ok(16, 16, 8, 8, 2 ** 30, padding=1)
    assert ok(16, 16, 8, 8, 0) and not ok(16, 16, 8, 8, -1)
    assert not ok(16, 16, 2 ** 16, 2 ** 15, padding=1) and ok(16, 16, 2 ** 16, 2 ** 15 - 1, padding=1)  # H * W < 2^31


def test_every_refusal_returns_its_status_without_a_launch():
    """The entry point with NULL pointers: every refusal is decided before a pointer is read or a kernel launched (there
    is no GPU in this test)."""
    from paddle3d_amd import _lib

    fn = _lib.lib().pd3_deform_conv2d_forward
    null = C.c_void_p(0)

    def call(N=1, ci=16, co=16, H=8, W=8, s=1, p=1, d=1):
        return fn(null, null, 18 * 64, 8, null, 9 * 64, 8, 1, null, null, null, 1, N, ci, co, H, W, s, p, d, null, null)

    assert call(N=0) == 0                                    # nothing to do
    for kw in (dict(ci=8), dict(ci=24), dict(co=8), dict(co=528), dict(ci=528), dict(s=3), dict(s=0), dict(d=0),
               dict(p=-1), dict(H=2 ** 16, W=2 ** 15), dict(N=2 ** 30, H=130, W=130), dict(N=0, ci=24)):
        assert call(**kw) == -3, kw
    for kw in (dict(N=-1), dict(ci=0), dict(co=0), dict(H=0), dict(W=0), dict(H=2, p=0), dict(H=4, W=4, d=2, p=0), dict()):
        assert call(**kw) == -1, kw                          # the last: NULL tensors at a supported shape
    from paddle3d_amd.ops import deform_conv as ops

    with pytest.raises(RuntimeError, match="Unsupported device type"):
        ops.deform_conv2d(torch.zeros(1, 16, 4, 4), torch.zeros(1, 18, 4, 4), torch.zeros(16, 16, 3, 3), padding=1)
