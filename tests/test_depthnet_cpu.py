"""BEVDepth's depth network on the CPU, against what the reference's own Python computed
(tests/golden/python_depthnet.npz, made by make_depthnet_golden.py): the NumPy restatement of pd3_aspp_forward
(tests/golden/depthnet_numpy.py) in float64 against the reference's float64 run to 1e-12 and in float32 within the stored
bounds; the restated softmax / channels-last tail on the view transformer's case; the modules of paddle3d_amd.bevdepth
with fused=False (the torch composition, also what a refused shape runs) within the stored bounds; get_mlp_input bit for
bit; the state-dict keys against the reference's and a strict load at the config's arguments; the refused configurations;
the predicates' borders; every refusal status of the entry points, none of which launches; the packers' lane order; and
the count of in-range taps the restatement multiplies against the closed form at 16 x 44.

Bounds: the ones the maker stored, 4 x the largest error of the reference's own fp32 run against its fp64 run (one fp32
ulp of the largest output as a floor)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import depthnet_numpy as dn  # noqa: E402
import make_depthnet_golden as mk  # noqa: E402

F32 = np.float32
F64 = np.float64


@pytest.fixture(scope="module")
def golden():
    return mk.load()


@pytest.fixture(scope="module")
def expf():
    from oracle import pyoracle as O

    return lambda x: O.libm_eval(2, np.ascontiguousarray(x, F32).reshape(-1))


def build(g, tag, fused=False, accelerate=False):
    """The module of case `tag` with the case's parameters, loaded strictly under the reference's keys."""
    from paddle3d_amd import bevdepth as bd
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    c = mk._cfg(tag)
    if tag in mk.ASPPS:
        m = bd.ASPP(c["cin"], c["cmid"], fused=fused)
    elif tag in mk.SES:
        m = bd.SELayer(c["C"])
    elif tag in mk.MLPS:
        m = bd.Mlp(27, c["hidden"], c["out"])
    elif tag in mk.NETS:
        m = bd.DepthNet(c["cin"], c["mid"], c["ctx"], c["D"], fused=fused)
    else:
        m = bd.LSSViewTransformerBEVDepth(grid_config=c["grid"], input_size=c["input_size"], downsample=c["downsample"],
                                          in_channels=c["cin"], out_channels=c["cout"], depthnet_cfg=dict(use_dcn=False),
                                          accelerate=accelerate, fused=fused)
    assert load_paddle_state_dict(m, mk.state(tag, mk.key_shapes(g, tag)), strict=True) == []
    return m.eval()


def err(a, b):
    return float(np.abs(np.asarray(a, F64) - np.asarray(b, F64)).max())


@pytest.mark.parametrize("tag", list(mk.ASPPS))
def test_restatement_in_float64_is_the_reference(golden, tag):
    st = mk.state(tag, mk.key_shapes(golden, tag))
    y = dn.aspp_forward(mk.inputs(tag)[0], dn.aspp_params(st, F64), dtype=F64)
    assert y.shape == golden[f"{tag}_y"].shape and err(y, golden[f"{tag}_y"]) <= 1e-12


@pytest.mark.parametrize("tag", list(mk.ASPPS))
def test_restatement_in_float32_within_the_bounds(golden, tag):
    st = mk.state(tag, mk.key_shapes(golden, tag))
    y = dn.aspp_forward(mk.inputs(tag)[0], dn.aspp_params(st))
    assert y.dtype == F32 and err(y, golden[f"{tag}_y"]) <= float(golden[f"{tag}_y_bound"])


def test_restated_tail_on_the_view_transformers_case(golden, expf):
    """depth_net's output of the case (the torch modules in float64 and in float32) through the restated tail."""
    m = build(golden, "vt")
    x = torch.from_numpy(mk.inputs("vt")[0])
    mlp = torch.from_numpy(golden["vt_mlp_input"])
    with torch.no_grad():
        x32 = m.depth_net(x.reshape(-1, *x.shape[2:]), mlp)
        m.double()
        x64 = m.depth_net(x.double().reshape(-1, *x.shape[2:]), mlp.double())
    d64, f64 = dn.depth_softmax_split(x64.numpy(), m.D, dtype=F64)
    assert err(d64, golden["vt_depth"]) <= 1e-12
    assert np.array_equal(f64, x64[:, m.D:].permute(0, 2, 3, 1).numpy())
    d32, f32 = dn.depth_softmax_split(x32.numpy(), m.D, expf)
    assert d32.dtype == F32 and err(d32, golden["vt_depth"]) <= float(golden["vt_depth_bound"])
    assert f32.shape == (3, 4, 11, 16) and np.array_equal(f32, x32[:, m.D:].permute(0, 2, 3, 1).numpy())


@pytest.mark.parametrize("tag", [*mk.ASPPS, *mk.SES, *mk.MLPS, *mk.NETS])
def test_modules_torch_form_within_the_bounds(golden, tag):
    m = build(golden, tag, fused=False)
    with torch.no_grad():
        y = m(*[torch.from_numpy(a) for a in mk.inputs(tag)]).numpy()
    assert y.shape == golden[f"{tag}_y"].shape
    assert err(y, golden[f"{tag}_y"]) <= float(golden[f"{tag}_y_bound"])


def test_view_transformer_mlp_input_and_depth(golden):
    """What of the view transformer runs without the device ops: get_mlp_input bit for bit, depth within its bound."""
    m = build(golden, "vt")
    cams = {k: torch.from_numpy(v) for k, v in mk.rig("vt").items()}
    mlp = m.get_mlp_input(*[cams[k] for k in ("rots", "trans", "cam2imgs", "post_rots", "post_trans", "bda")])
    assert tuple(mlp.shape) == (1, 3, 27) and np.array_equal(mlp.numpy(), golden["vt_mlp_input"])
    x = torch.from_numpy(mk.inputs("vt")[0])
    with torch.no_grad():
        depth, feat = m._tail(m.depth_net(x.reshape(-1, *x.shape[2:]), mlp))
    assert err(depth.numpy(), golden["vt_depth"]) <= float(golden["vt_depth_bound"])
    assert tuple(feat.shape) == (3, 4, 11, 16) and feat.is_contiguous() and m.D == 15


def _reference_names(module):
    linear = {n + ".weight" for n, m in module.named_modules() if isinstance(m, torch.nn.Linear)}
    return {k.replace(".running_mean", "._mean").replace(".running_var", "._variance"):
            list(v.shape)[::-1] if k in linear else list(v.shape)
            for k, v in module.state_dict().items() if not k.endswith("num_batches_tracked")}


def test_state_dict_keys_are_the_references(golden):
    from paddle3d_amd import bevdepth as bd
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    for tag in mk.TAGS:
        assert _reference_names(build(golden, tag)) == mk.key_shapes(golden, tag), tag
    shapes = mk.key_shapes(golden, "r50")
    net = bd.bevdet4d_r50_depth_view_transformer()
    assert _reference_names(net) == shapes and len(shapes) == 90 and (net.D, net.out_channels) == (118, 80)
    assert shapes["depth_net.depth_conv.3.conv1.weight"] == [512, 2560, 1, 1]
    assert shapes["depth_net.depth_conv.3.aspp4.atrous_conv.weight"] == [512, 512, 3, 3]
    assert shapes["depth_net.depth_conv.4.weight"] == [118, 512, 1, 1] and shapes["depth_net.depth_mlp.fc1.weight"] == [27, 512]
    rng = np.random.default_rng(5)
    state = {k: rng.standard_normal(s, dtype=F32) for k, s in shapes.items()}
    assert load_paddle_state_dict(net, state, strict=True) == []
    own = net.state_dict()
    for k in ("depth_net.depth_conv.3.global_avg_pool.2._variance", "depth_net.bn._mean", "depth_net.context_conv.bias",
              "depth_net.depth_conv.1.conv2.weight"):
        name = k.replace("._mean", ".running_mean").replace("._variance", ".running_var")
        assert np.array_equal(own[name].numpy(), state[k]), k
    assert np.array_equal(own["depth_net.context_mlp.fc2.weight"].numpy(), state["depth_net.context_mlp.fc2.weight"].T)
    del state["depth_net.depth_conv.3.aspp2.bn.weight"]
    with pytest.raises(RuntimeError):
        load_paddle_state_dict(net, state, strict=True)


def test_refused_configurations():
    from paddle3d_amd import bevdepth as bd

    with pytest.raises(NotImplementedError):
        bd.DepthNet(16, 16, 8, 10, use_dcn=True)
    with pytest.raises(NotImplementedError):
        bd.LSSViewTransformerBEVDepth(in_channels=16, out_channels=8, depthnet_cfg=dict(use_dcn=True))
    with pytest.raises(NotImplementedError):
        bd.BasicBlock(16, 16, stride=2)
    for make in (lambda: bd.ASPP(16, 16, fused="yes"), lambda: bd.DepthNet(16, 16, 8, 10, fused=1.5),
                 lambda: bd.LSSViewTransformerBEVDepth(in_channels=16, out_channels=8, fused=None)):
        with pytest.raises(ValueError):
            make()
    net = bd.DepthNet(16, 16, 8, 10, use_aspp=False)
    assert len(net.depth_conv) == 4 and not any(isinstance(m, bd.ASPP) for m in net.modules())
    aspp = bd.ASPP(16, 16, fused="force").eval()
    x = torch.zeros(1, 16, 3, 3)
    assert not aspp.takes_kernel(x) and not aspp.takes_kernel(x.double())  # not on the device: the composition
    with torch.no_grad():
        assert tuple(aspp(x).shape) == (1, 16, 3, 3)


def test_supported_borders():
    from paddle3d_amd.ops import depthnet as ops

    for c in (16, 32, 48, 256, 496, 512):
        assert ops.aspp_supported(c, 16) and ops.aspp_supported(16, c) and ops.aspp_supported(c, c, 16, 44, 54)
    for c in (0, 8, 15, 17, 24, 513, 528, 1024):
        assert not ops.aspp_supported(c, 16) and not ops.aspp_supported(16, c)
    ok = lambda **kw: ops.aspp_supported(16, 16, **kw)  # noqa: E731
    assert ok(dilations=(1, 2, 3)) and ok(dilations=(65535,) * 3) and not ok(dilations=(6, 12, 65536))
    assert not ok(dilations=(0, 12, 18)) and not ok(dilations=(6, 12)) and not ok(h=0) and not ok(w=0) and not ok(n=-1)
    assert ok(n=0) and ok(h=2 ** 16, w=2 ** 15 - 1) and not ok(h=2 ** 16, w=2 ** 15)
    assert ok(h=8, w=8, n=2 ** 30 - 1) and not ok(h=8, w=8, n=2 ** 30 + 1)
    assert ops.PIXEL_TILE == 64 and ops.MAX_CHANNELS == 512
    assert ops.tail_supported(54, 118, 80, 16, 44) and ops.tail_supported(1, 1, 0, 1, 1)
    assert not ops.tail_supported(1, 0, 8, 4, 4) and not ops.tail_supported(65536, 4, 4, 4, 4)
    assert not ops.tail_supported(1, 4, 4, 2 ** 16, 2 ** 15)
    assert [ops.tiles_per_wave(n * 704, 512) for n in (54, 12, 1)] == [4, 2, 1] and ops.tiles_per_wave(54 * 704, 16) == 1
    with pytest.raises(ValueError):
        ops.fused_by_default("conv", 1, 16, 16, 4, 4)
    with pytest.raises(ValueError):
        ops.fused_by_default("aspp")
    # the measured borders: the ASPP from 54 maps of 16 x 44 on, the tail up to 6
    assert ops.fused_by_default("aspp", 54, 512, 512, 16, 44) and not ops.fused_by_default("aspp", 53, 512, 512, 16, 44)
    assert not ops.fused_by_default("aspp", 6, 512, 512, 16, 44)
    assert ops.fused_by_default("tail", 6, 118, 80, 16, 44) and not ops.fused_by_default("tail", 7, 118, 80, 16, 44)
    assert not ops.fused_by_default("tail", 54, 118, 80, 16, 44) and not ops.fused_by_default("tail", 0, 118, 80, 16, 44)


def test_every_refusal_returns_its_status_without_a_launch():
    """The entry points with NULL pointers: every refusal is decided before a pointer is read or a kernel launched (there
    is no GPU in this test)."""
    from paddle3d_amd import _lib
    from paddle3d_amd.ops import depthnet as ops

    L = _lib.lib()
    null = C.c_void_p(0)

    def aspp(N=1, ci=16, cm=16, H=8, W=8, d=(6, 12, 18), ws=null, nbytes=0):
        return L.pd3_aspp_forward(*[null] * 11, N, ci, cm, H, W, *d, null, ws, nbytes, null)

    assert aspp(N=0) == 0                                    # nothing to do
    for kw in (dict(ci=8), dict(ci=24), dict(cm=8), dict(cm=528), dict(ci=528), dict(d=(0, 12, 18)), dict(d=(6, 12, 65536)),
               dict(H=2 ** 16, W=2 ** 15), dict(N=2 ** 30, H=130, W=130), dict(N=0, ci=24)):
        assert aspp(**kw) == -3, kw
    for kw in (dict(N=-1), dict(ci=0), dict(cm=0), dict(H=0), dict(W=0), dict()):
        assert aspp(**kw) == -1, kw                          # the last: NULL tensors at a supported shape
    assert L.pd3_aspp_workspace(54, 512, 512, 16, 44) == 4 * (54 * 4 * 512 * 704 + 54 * 512)
    assert L.pd3_aspp_workspace(1, 16, 16, 1, 1) == 4 * (64 + 16)
    assert L.pd3_aspp_workspace(1, 24, 16, 4, 4) == 0 == L.pd3_aspp_workspace(0, 16, 16, 4, 4)

    def tail(N=1, D=4, Cc=4, H=4, W=4):
        return L.pd3_depth_softmax_split(null, N, D, Cc, H, W, null, null, null)

    assert tail(N=0) == 0
    for kw in (dict(N=65536), dict(H=2 ** 16, W=2 ** 15)):
        assert tail(**kw) == -3, kw
    for kw in (dict(N=-1), dict(D=0), dict(Cc=-1), dict(H=0), dict(W=0), dict()):
        assert tail(**kw) == -1, kw
    with pytest.raises(RuntimeError, match="Unsupported device type"):
        ops.depth_softmax_split(torch.zeros(1, 8, 4, 4), 4)
    with pytest.raises(RuntimeError, match="Unsupported device type"):
        ops.aspp_forward(torch.zeros(1, 16, 4, 4), {})


def test_packers_lane_order():
    from paddle3d_amd.ops import depthnet as ops

    rng = np.random.default_rng(9)
    ci, cm = 32, 48
    ws = [torch.from_numpy(rng.standard_normal((cm, ci, k, k)).astype(F32)) for k in (1, 3, 3, 3)]
    pw = ops.pack_aspp_branches(*ws)
    assert tuple(pw.shape) == (28, ci // 16, cm // 16, 64, 4) and pw.is_contiguous()
    t, nt, lane, ks = 1, 2, 37, 2  # the lane order of the kernel's header
    o, c = 16 * nt + (lane & 15), 16 * t + 4 * ks + (lane >> 4)
    assert pw[0, t, nt, lane, ks] == ws[0][o, c, 0, 0]
    for b in (1, 2, 3):
        for k in (0, 4, 8):
            assert pw[1 + 9 * (b - 1) + k, t, nt, lane, ks] == ws[b][o, c, k // 3, k % 3]
    w1 = torch.from_numpy(rng.standard_normal((cm, 5 * cm, 1, 1)).astype(F32))
    proj, pool_t = ops.pack_aspp_projection(w1)
    assert tuple(proj.shape) == (1, 4 * cm // 16, cm // 16, 64, 4) and tuple(pool_t.shape) == (cm, cm)
    t = 4 * cm // 16 - 1
    assert proj[0, t, nt, lane, ks] == w1[o, 16 * t + 4 * ks + (lane >> 4), 0, 0]
    assert pool_t[5, 7] == w1[7, 4 * cm + 5, 0, 0] and pool_t.is_contiguous()
    for bad in ([torch.zeros(16, 16, 3, 3)] * 4, [torch.zeros(24, 16, 1, 1)] + [torch.zeros(24, 16, 3, 3)] * 3):
        with pytest.raises(RuntimeError):
            ops.pack_aspp_branches(*bad)
    with pytest.raises(RuntimeError):
        ops.pack_aspp_projection(torch.zeros(16, 64, 1, 1))


def test_in_range_taps_at_the_models_map():
    """16 x 44: the restatement multiplies 1 + 6.14 + 3.68 + 2.18 = 13.0 of the nominal 28 taps per pixel."""
    from paddle3d_amd.ops import depthnet as ops

    rng = np.random.default_rng(2)
    p = dict(w=[rng.standard_normal((16, 16, k, k)).astype(F32) for k in (1, 3, 3, 3)], scale=np.ones(64, F32),
             shift=np.zeros(64, F32))
    count = []
    dn.aspp_branches(rng.standard_normal((1, 16, 16, 44)).astype(F32), p, count=count)
    closed = [16 * 44] + [(16 + 2 * max(16 - d, 0)) * (44 + 2 * max(44 - d, 0)) for d in (6, 12, 18)]
    assert count == closed == ops.in_range_taps(16, 44) == [704, 4320, 2592, 1536]
    assert sum(count) == 13 * 704 and [round(c / 704, 2) for c in count] == [1.0, 6.14, 3.68, 2.18]
    assert round(28 * 704 / sum(count), 2) == 2.15
