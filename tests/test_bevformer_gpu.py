"""BEVFormer's encoder attention on the device: the three entry points of csrc/bevformer.hip bit for bit against the
NumPy restatement (tests/golden/bevformer_numpy.py) on the golden cases and on seeded sweeps, and the ops and the
modules of paddle3d_amd.bevformer (fused and unfused; attention module, layer, 2-layer encoder) against what the
reference's own Python computed (tests/golden/python_bevformer.npz) within the bounds the maker stored: 4 x the
reference's own fp32 error.  Fused against unfused is held to the same bound.  Also: a frame alone, elsewhere in the
batch and on a side stream gives the same bits; refused shapes fall back; the encoder forward makes no host
synchronisation; a fused layer launches each attention kernel once and an encoder forward projects the anchors once."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from guarded import launch_ledger  # noqa: E402

import bevformer_numpy as bn  # noqa: E402
import make_bevformer_golden as mk  # noqa: E402
import test_bevformer_cpu as cpu  # noqa: E402
from test_bevformer_cpu import expf, golden  # noqa: E402,F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
TAGS = mk.TAGS


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.detach().cpu().numpy()


def same_bits(got, want):
    got = _n(got) if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    view = {4: np.uint32, 1: np.uint8}[got.dtype.itemsize]
    bad = got.view(view) != want.view(view)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}"


def _levels(shapes):
    sh, lsi, S = bn.md.level_layout(shapes)
    return sh, lsi, S


# ---- the ops against the restatement ---------------------------------------------------------------------------------


def device_ops(g, tag):
    """(point_sampling's outputs, sca, tsa) of the ops on the case's inputs (the CPU test's Linear rows, uploaded)."""
    from paddle3d_amd.ops import bevformer as ops

    c = mk.CASES[tag]
    sh, lsi, _ = mk.levels(tag)
    ref_3d = bn.get_reference_points(*c["bev"], cpu.Z_RANGE, c["D"])
    ps = ops.point_sampling(_t(ref_3d), _t(g[f"{tag}_lidar2img"]), mk.PC_RANGE, *mk.IMG_SHAPE[:2])
    value, off, logits = (_t(a) for a in cpu.sca_inputs(tag))
    sca = ops.spatial_cross_attention_sample(value, off, logits, ps[0], ps[2], _t(sh), _t(lsi), c["cams"])
    bev_sh, bev_lsi, _ = _levels([c["bev"]])
    value, off, logits = (_t(a) for a in cpu.tsa_inputs(tag))
    tsa = ops.temporal_self_attention_sample(value, off, logits, _t(cpu.ref_2d(tag)), _t(bev_sh), _t(bev_lsi))
    return ps, sca, tsa


@pytest.mark.parametrize("tag", TAGS)
def test_ops_on_the_golden_cases(golden, expf, tag):
    ps, sca, tsa = device_ops(golden, tag)
    want_ps, want_sca, want_tsa = cpu.restated(golden, tag, expf)
    for got, want in zip(ps, want_ps):
        same_bits(got, want.astype(F32) if want.dtype == np.float64 else want)
    same_bits(sca, want_sca)
    same_bits(tsa, want_tsa)
    cpu.check_point_sampling(golden, tag, *(_n(t) for t in ps))
    cpu.check_result(golden, tag, "sca_sample", _n(sca))
    cpu.check_result(golden, tag, "tsa_sample", _n(tsa))


def _odd_points(rng, ref):
    """NaN, Inf and 1e30 planted among the reference points."""
    flat = ref.reshape(-1)
    idx = rng.choice(flat.size, size=max(1, flat.size // 8), replace=False)
    flat[idx] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], F32), size=idx.size)
    return ref


# (Q, cams, C, M, levels, P, D, B): every value of the issue's lists occurs; the last has a level table past S
SCA_SWEEP = [
    (1, 1, 4, 1, [[3, 4]], 4, 1, 1), (31, 3, 16, 2, [[3, 4], [2, 2]], 4, 2, 1), (32, 6, 32, 2, [[6, 10]], 8, 4, 1),
    (33, 8, 64, 1, [[3, 4]], 8, 4, 1), (77, 3, 32, 2, [[6, 10], [3, 5]], 8, 4, 2), (77, 6, 4, 8, [[3, 4]], 4, 4, 1),
    (33, 1, 16, 8, [[4, 4], [3, 3], [2, 2], [1, 1]], 8, 2, 1), (31, 8, 32, 1, [[5, 3], [2, 7]], 8, 1, 2),
    (32, 3, 64, 2, [[4, 4], [3, 3], [2, 2], [1, 1]], 4, 4, 1), (1, 6, 32, 8, [[6, 10]], 8, 2, 1),
    (77, 8, 16, 1, [[3, 5], [2, 3]], 4, 1, 1), (33, 3, 4, 2, [[4, 4], [3, 3], [2, 2], [1, 1]], 8, 4, 1),
    (31, 6, 64, 8, [[3, 4]], 4, 2, 1), (32, 1, 32, 1, [[2, 3], [1, 2]], 8, 8, 1), (1, 8, 16, 2, [[3, 4], [2, 2]], 8, 4, 2),
    (77, 1, 64, 2, [[7, 9]], 4, 4, 1), (33, 6, 16, 1, [[3, 4], [2, 2]], 4, 4, 3), (31, 3, 32, 8, [[6, 10]], 8, 8, 1),
    (32, 8, 4, 2, [[3, 4], [2, 2]], 8, 2, 1), (77, 6, 32, 2, [[6, 10], [3, 5]], 8, 4, 1),
]


@pytest.mark.parametrize("i", range(len(SCA_SWEEP)))
def test_sca_sweep(expf, i):
    from paddle3d_amd.ops import bevformer as ops

    Q, cams, C, M, shapes, P, D, B = SCA_SWEEP[i]
    rng = np.random.default_rng(100 + i)
    sh, lsi, S = _levels(shapes)
    L = len(shapes)
    if i == len(SCA_SWEEP) - 1:  # a level table that points past S: such rows are never read
        lsi = lsi + S - 7
    value = rng.standard_normal((B * cams, S, M, C)).astype(F32)
    off = (rng.standard_normal((B, Q, M, L, P, 2)) * 1.5).astype(F32)
    logits = (rng.standard_normal((B, Q, M, L * P)) * 2).astype(F32)
    ref = _odd_points(rng, rng.uniform(-0.2, 1.2, (cams, B, Q, D, 2)).astype(F32))
    bits = rng.integers(0, 256, (B, Q)).astype(np.uint8)  # bits above `cams` are ignored
    bits[:, ::5] = 0  # all-miss queries
    want = bn.sca(value, off, logits, ref, bits, sh, lsi, cams, expf)
    got = ops.spatial_cross_attention_sample(_t(value), _t(off), _t(logits), _t(ref), _t(bits), _t(sh), _t(lsi), cams)
    same_bits(got, want)
    assert np.isfinite(want).all() and (Q < 5 or np.abs(want).max() > 0) and not want[:, ::5].any()


TSA_SWEEP = [(1, 4, 1, [[3, 4]], 4, 1), (31, 16, 2, [[3, 4], [2, 2]], 8, 1), (33, 32, 8, [[5, 6]], 4, 2),
             (77, 64, 2, [[7, 11]], 8, 1), (32, 32, 2, [[4, 4], [3, 3], [2, 2], [1, 1]], 8, 2), (77, 4, 1, [[7, 11]], 4, 1)]


@pytest.mark.parametrize("i", range(len(TSA_SWEEP)))
def test_tsa_sweep(expf, i):
    from paddle3d_amd.ops import bevformer as ops

    Q, C, M, shapes, P, B = TSA_SWEEP[i]
    rng = np.random.default_rng(200 + i)
    sh, lsi, S = _levels(shapes)
    L = len(shapes)
    if i == len(TSA_SWEEP) - 1:
        lsi = lsi + S - 5
    value = rng.standard_normal((B * 2, S, M, C)).astype(F32)
    off = (rng.standard_normal((B, Q, M, 2, L, P, 2)) * 1.5).astype(F32)
    logits = (rng.standard_normal((B, Q, M, 2, L * P)) * 2).astype(F32)
    ref = _odd_points(rng, rng.uniform(-0.2, 1.2, (B * 2, Q, L, 2)).astype(F32))
    want = bn.tsa(value, off, logits, ref, sh, lsi, expf)
    got = ops.temporal_self_attention_sample(_t(value), _t(off), _t(logits), _t(ref), _t(sh), _t(lsi))
    same_bits(got, want)
    assert np.isfinite(want).all() and (Q < 5 or np.abs(want).max() > 0)


@pytest.mark.parametrize("Q,cams,D,B", [(1, 1, 1, 1), (33, 8, 4, 2), (77, 3, 2, 1), (257, 6, 4, 3)])
def test_point_sampling_sweep(Q, cams, D, B):
    from paddle3d_amd.ops import bevformer as ops

    rng = np.random.default_rng(300 + Q)
    ref = rng.uniform(0, 1, (D, Q, 3)).astype(F32)
    mats = rng.standard_normal((B, cams, 4, 4)).astype(F32)
    mats[..., 0, :] = 40 * (mats[..., 0, :] + mats[..., 2, :])  # u, v = 0.5 + a ratio of two random depths
    mats[..., 1, :] = 24 * (mats[..., 1, :] + mats[..., 2, :])
    want = bn.point_sampling(ref, mats, mk.PC_RANGE, 48, 80)
    got = ops.point_sampling(_t(ref), _t(mats), mk.PC_RANGE, 48, 80)
    for a, b in zip(got, want):
        same_bits(a, b)
    assert Q == 1 or 0 < want[1].mean() < 1


def test_a_frame_alone_elsewhere_and_on_a_side_stream(golden):
    from paddle3d_amd.ops import bevformer as ops

    tag = "a"
    c = mk.CASES[tag]
    cams = c["cams"]
    sh, lsi, S = mk.levels(tag)
    sh, lsi = _t(sh), _t(lsi)
    ps, sca, tsa = device_ops(golden, tag)
    value, off, logits = (_t(a) for a in cpu.sca_inputs(tag))
    bev_sh, bev_lsi, _ = _levels([c["bev"]])
    bev_sh, bev_lsi = _t(bev_sh), _t(bev_lsi)
    tvalue, toff, tlogits = (_t(a) for a in cpu.tsa_inputs(tag))
    tref = _t(cpu.ref_2d(tag))
    rows = lambda t, b, n: t[b * n:(b + 1) * n]  # noqa: E731
    for b in range(c["B"]):  # alone
        got = ops.spatial_cross_attention_sample(rows(value, b, cams), off[b:b + 1], logits[b:b + 1], ps[0][:, b:b + 1],
                                                 ps[2][b:b + 1], sh, lsi, cams)
        assert torch.equal(got[0], sca[b])
        got = ops.temporal_self_attention_sample(rows(tvalue, b, 2), toff[b:b + 1], tlogits[b:b + 1], rows(tref, b, 2),
                                                 bev_sh, bev_lsi)
        assert torch.equal(got[0], tsa[b])
    flip = lambda t, n: torch.cat([rows(t, 1, n), rows(t, 0, n)])  # noqa: E731  (the two frames swapped)
    got = ops.spatial_cross_attention_sample(flip(value, cams), off.flip(0), logits.flip(0), ps[0].flip(1), ps[2].flip(0),
                                             sh, lsi, cams)
    assert torch.equal(got.flip(0), sca)
    got = ops.temporal_self_attention_sample(flip(tvalue, 2), toff.flip(0), tlogits.flip(0), flip(tref, 2), bev_sh, bev_lsi)
    assert torch.equal(got.flip(0), tsa)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        ref_3d = _t(bn.get_reference_points(*c["bev"], cpu.Z_RANGE, c["D"]))
        ps2 = ops.point_sampling(ref_3d, _t(golden[f"{tag}_lidar2img"]), mk.PC_RANGE, *mk.IMG_SHAPE[:2])
        sca2 = ops.spatial_cross_attention_sample(value, off, logits, ps2[0], ps2[2], sh, lsi, cams)
        tsa2 = ops.temporal_self_attention_sample(tvalue, toff, tlogits, tref, bev_sh, bev_lsi)
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ps2, ps)) and torch.equal(sca2, sca) and torch.equal(tsa2, tsa)


# ---- the modules against the reference -------------------------------------------------------------------------------


def encoder(tag, fused):
    from paddle3d_amd import bevformer
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    m = bevformer.BEVFormerEncoder(**mk.encoder_cfg(tag), fused=fused)
    load_paddle_state_dict(m, mk.state(tag))
    return m.eval().to(DEV)


def encoder_inputs(g, tag):
    c, inp = mk.CASES[tag], mk.inputs(tag)
    sh, lsi, _ = mk.levels(tag)
    seq = lambda a: _t(a.transpose(1, 0, 2))  # noqa: E731  [B, Q, E] -> [Q, B, E]
    mats = _t(g[f"{tag}_lidar2img"])
    metas = [dict(lidar2img=mats[b], img_shape=[mk.IMG_SHAPE] * c["cams"]) for b in range(c["B"])]
    feats = _t(inp["feats"])
    return (seq(inp["bev_query"]), feats, feats), dict(bev_h=c["bev"][0], bev_w=c["bev"][1], bev_pos=seq(inp["bev_pos"]),
                                                       spatial_shapes=_t(sh), level_start_index=_t(lsi),
                                                       prev_bev=seq(inp["prev_bev"]), shift=_t(inp["shift"]),
                                                       img_metas=metas)


_modules = {}


def module_outputs(g, tag, fused):
    """{sca_out, tsa_out, layer_out, encoder_out} of the modules, once per (case, fused)."""
    if (tag, fused) in _modules:
        return _modules[tag, fused]
    c, inp = mk.CASES[tag], mk.inputs(tag)
    enc = encoder(tag, fused)
    args, kw = encoder_inputs(g, tag)
    q, pos, prev = (_t(inp[k]) for k in ("bev_query", "bev_pos", "prev_bev"))
    ref_3d = enc.get_reference_points(*c["bev"], cpu.Z_RANGE, c["D"], "3d", c["B"], torch.float32, DEV)
    ref_cam, mask = enc.point_sampling(ref_3d, mk.PC_RANGE, kw["img_metas"])
    hybrid, queue = _t(cpu.ref_2d(tag)), torch.stack([prev, q], 1).reshape(c["B"] * 2, -1, mk.EMBED)
    bev_sh, bev_lsi, _ = _levels([c["bev"]])
    layer = enc.layers[0]
    out = {}
    with torch.no_grad():
        out["sca_out"] = layer.attentions[1](q, args[1], args[2], reference_points_cam=ref_cam, bev_mask=mask,
                                             spatial_shapes=kw["spatial_shapes"], level_start_index=kw["level_start_index"])
        out["tsa_out"] = layer.attentions[0](q, queue, queue, None, query_pos=pos, reference_points=hybrid,
                                             spatial_shapes=_t(bev_sh), level_start_index=_t(bev_lsi))
        out["layer_out"] = layer(q, args[1], args[2], bev_pos=pos, ref_2d=hybrid, ref_3d=ref_3d, bev_h=kw["bev_h"],
                                 bev_w=kw["bev_w"], spatial_shapes=kw["spatial_shapes"],
                                 level_start_index=kw["level_start_index"], reference_points_cam=ref_cam, bev_mask=mask,
                                 prev_bev=queue)
        out["encoder_out"] = enc(*args, **kw)
    _modules[tag, fused] = {k: _n(v) for k, v in out.items()}
    return _modules[tag, fused]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("tag", TAGS)
def test_modules_against_the_reference(golden, tag, fused):
    out = module_outputs(golden, tag, fused)
    errs = []
    for name, got in out.items():
        want, bound = golden[f"{tag}_{name}"], float(golden[f"{tag}_{name}_bound"])
        e = float(np.abs(got.astype(np.float64) - want).max())
        print(f"{tag} fused={fused} {name} err {e:.3e} bound {bound:.3e} (reference's own "
              f"{float(golden[f'{tag}_{name}_ref_err']):.3e})")
        assert got.shape == want.shape and got.dtype == F32
        errs.append((name, e, bound))
    assert all(e <= b for _, e, b in errs), errs


@pytest.mark.parametrize("tag", TAGS)
def test_fused_against_unfused(golden, tag):
    f, u = module_outputs(golden, tag, True), module_outputs(golden, tag, False)
    errs = []
    for name in f:
        e, bound = float(np.abs(f[name].astype(np.float64) - u[name]).max()), float(golden[f"{tag}_{name}_bound"])
        print(f"{tag} {name} fused against unfused {e:.3e} bound {bound:.3e}")
        errs.append((name, e, bound))
    assert all(e <= b for _, e, b in errs), errs


def test_refused_shapes_fall_back():
    """C = 6 (no multiple of 4) and L * P = 36: the ops return None, the fused modules take the unfused route."""
    from paddle3d_amd import _lib, bevformer
    from paddle3d_amd.ops import bevformer as ops

    with_msda = _lib.symbols("test_memory_safety_bevformer_gpu") + ("pd3_ms_deform_attn_forward",)
    torch.manual_seed(5)
    B, Q, cams, D = 1, 20, 2, 4
    sh, lsi, S = _levels([[3, 4]])
    sh, lsi = _t(sh), _t(lsi)
    ref_cam = torch.rand(cams, B, Q, D, 2, device=DEV)
    mask = torch.rand(cams, B, Q, D, device=DEV) > 0.5
    bev_sh, bev_lsi, _ = _levels([[4, 5]])
    ref_2d = torch.rand(B * 2, Q, 1, 2, device=DEV)
    for E, M, P in ((12, 2, 8), (16, 2, 36)):
        q = torch.randn(B, Q, E, device=DEV)
        feats = torch.randn(cams, S, B, E, device=DEV)
        queue = torch.randn(B * 2, Q, E, device=DEV)
        att = dict(type_name="MSDeformableAttention3D", embed_dims=E, num_heads=M, num_points=P, num_levels=1)
        outs = []
        for fused in (True, False):
            torch.manual_seed(6)
            sca = bevformer.SpatialCrossAttention(embed_dims=E, num_cams=cams, deformable_attention=att,
                                                  fused=fused).eval().to(DEV)
            tsa = bevformer.TemporalSelfAttention(embed_dims=E, num_heads=M, num_levels=1, num_points=P,
                                                  fused=fused).eval().to(DEV)
            with torch.no_grad(), launch_ledger(_lib.lib(), with_msda) as n:
                outs.append((sca(q, feats, feats, reference_points_cam=ref_cam, bev_mask=mask, spatial_shapes=sh,
                                 level_start_index=lsi),
                             tsa(q, queue, queue, reference_points=ref_2d, spatial_shapes=_t(bev_sh),
                                 level_start_index=_t(bev_lsi))))
            assert n["pd3_ms_deform_attn_forward"] == 2, dict(n)
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        assert outs[0][0].abs().max() > 0 and torch.isfinite(outs[0][0]).all()
        v = torch.randn(B * cams, S, M, E // M, device=DEV)
        assert ops.spatial_cross_attention_sample(v, torch.randn(B, Q, M, 1, P, 2, device=DEV),
                                                  torch.randn(B, Q, M, P, device=DEV), ref_cam,
                                                  bevformer.hit_bits_of(mask), sh, lsi, cams) is None
        assert ops.temporal_self_attention_sample(v, torch.randn(B, Q, M, 2, 1, P, 2, device=DEV),
                                                  torch.randn(B, Q, M, 2, P, device=DEV), ref_2d[:, :, :1],
                                                  sh, lsi) is None


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_encoder_forward_makes_no_host_sync(golden, fused):
    tag = "a"
    enc = encoder(tag, fused)  # a fresh module: its reference points are built and sent inside the forward
    args, kw = encoder_inputs(golden, tag)
    want = module_outputs(golden, tag, fused)["encoder_out"]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            out = enc(*args, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    err, bound = float(np.abs(_n(out).astype(np.float64) - want).max()), float(golden[f"{tag}_encoder_out_bound"])
    assert err <= bound, (err, bound)


def test_launch_counts(golden):
    from paddle3d_amd import _lib

    tag = "c"
    c, inp = mk.CASES[tag], mk.inputs(tag)
    enc = encoder(tag, True)
    args, kw = encoder_inputs(golden, tag)
    names = ("pd3_bevformer_point_sampling", "pd3_bevformer_sca", "pd3_bevformer_tsa")
    with_msda = _lib.symbols("test_memory_safety_bevformer_gpu") + ("pd3_ms_deform_attn_forward",)
    with torch.no_grad():
        with launch_ledger(_lib.lib(), _lib.symbols("test_memory_safety_bevformer_gpu")) as n:
            enc(*args, **kw)
        assert [n[k] for k in names] == [1, mk.LAYERS, mk.LAYERS], dict(n)
        q, pos, prev = (_t(inp[k]) for k in ("bev_query", "bev_pos", "prev_bev"))
        ref_3d = enc.get_reference_points(*c["bev"], cpu.Z_RANGE, c["D"], "3d", c["B"], torch.float32, DEV)
        ref_cam, mask = enc.point_sampling(ref_3d, mk.PC_RANGE, kw["img_metas"])
        queue = torch.stack([prev, q], 1).reshape(c["B"] * 2, -1, mk.EMBED)
        with launch_ledger(_lib.lib(), with_msda) as n:
            enc.layers[0](q, args[1], args[2], bev_pos=pos, ref_2d=_t(cpu.ref_2d(tag)), bev_h=kw["bev_h"], bev_w=kw["bev_w"],
                          spatial_shapes=kw["spatial_shapes"], level_start_index=kw["level_start_index"],
                          reference_points_cam=ref_cam, bev_mask=mask, prev_bev=queue)
        assert [n[k] for k in names] == [0, 1, 1] and n["pd3_ms_deform_attn_forward"] == 0, dict(n)
        with launch_ledger(_lib.lib(), with_msda) as n:
            encoder(tag, False)(*args, **kw)
        assert [n[k] for k in names] == [1, 0, 0] and n["pd3_ms_deform_attn_forward"] == 2 * mk.LAYERS, dict(n)
