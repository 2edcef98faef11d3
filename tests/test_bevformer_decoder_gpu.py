"""BEVFormer's decoder, head and NMS-free decode on the device: the three entry points of csrc/bevformer_decoder.hip bit
for bit against the NumPy restatement (tests/golden/bevformer_decoder_numpy.py) on the golden cases and on seeded
sweeps, and the ops and the modules of paddle3d_amd.bevformer_head (fused and unfused; attention modules, layer, 2-layer
decoder, head, decode) against what the reference's own Python computed (tests/golden/python_bevformer_decoder.npz)
within the bounds the maker stored: 4 x the reference's own fp32 error.  Fused against unfused is held to the same
bound.  Also: a frame alone, elsewhere in the batch and on a side stream gives the same bits; refused shapes return None
and the modules fall back; a decoder + head + decode forward makes no host synchronisation; a fused layer launches each
attention kernel once and a forward decodes the whole batch in one launch."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from guarded import launch_ledger  # noqa: E402

import bevformer_decoder_numpy as dn  # noqa: E402
import make_bevformer_decoder_golden as mk  # noqa: E402
import test_bevformer_decoder_cpu as cpu  # noqa: E402
from test_bevformer_decoder_cpu import atan2f, expf, golden  # noqa: E402,F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
TAGS = mk.TAGS
M = mk.HEADS


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.detach().cpu().numpy()


def same_bits(got, want, nan_ok=False):
    """Bit equality; with nan_ok a NaN must stand exactly where the restatement has one (its payload is free)."""
    got = _n(got) if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    view = {4: np.uint32, 1: np.uint8}[got.dtype.itemsize]
    bad = got.view(view) != want.view(view)
    if nan_ok:
        assert np.array_equal(np.isnan(got), np.isnan(want)), "NaNs stand elsewhere"
        bad &= ~np.isnan(want)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}"


# ---- the ops against the restatement ---------------------------------------------------------------------------------


def device_ops(tag):
    from paddle3d_amd.ops import bevformer_decoder as ops

    mha = ops.multihead_attention(*(_t(a) for a in cpu.mha_inputs(tag)), M)
    ca = ops.decoder_cross_attention_sample(*(_t(a) for a in cpu.ca_inputs(tag)))
    return mha, ca


def device_decode(g, tag, name, bottom_center=True):
    from paddle3d_amd.ops import bevformer_decoder as ops

    c = mk.CASES[tag]
    cls, bbox = (_t(a) for a in cpu.decode_case(g, tag, name))
    return ops.nms_free_decode(cls, bbox, c["post"], c["max_num"], c["thr"], bottom_center)


@pytest.mark.parametrize("tag", TAGS)
def test_ops_on_the_golden_cases(golden, expf, atan2f, tag):
    mha, ca = device_ops(tag)
    want_mha, want_ca = cpu.restated(tag, expf)
    same_bits(mha, want_mha)
    same_bits(ca, want_ca)
    if tag in ("a", "b"):
        cpu.check_result(golden, tag, "mha_sample", _n(mha))
        cpu.check_result(golden, tag, "ca_sample", _n(ca))
    for name in mk.DECODES[tag]:
        got = device_decode(golden, tag, name)
        want = cpu.restated_decode(golden, tag, name, expf, atan2f)
        for a, b in zip(got, want[:4]):
            same_bits(a, b)
        cpu.check_decode(golden, tag, name, *(_n(t) for t in got))


MHA_SWEEP = [(1, 1), (1, 17), (15, 16), (16, 15), (17, 33), (37, 37), (33, 130)]


def mha_case(Nq, Nk, d, heads, B):
    """(q, k, v, NaNs planted, an expf underflows to 0 somewhere, to a subnormal somewhere) of one sweep point."""
    rng = np.random.default_rng(1000 * Nq + 10 * Nk + d + heads + B)
    E = heads * d
    q, k, v = (rng.standard_normal((B, n, E)).astype(F32) for n in (Nq, Nk, Nk))
    q *= rng.choice(np.array([1, 6, 60], F32), size=(B, Nq, 1))  # rows whose expf underflows
    plant = Nq > 1 and Nk > 1
    if plant:
        q[B - 1, Nq // 2, E // 3] = np.nan
        v[0, Nk // 3, :] = np.nan
    qs = (q.reshape(B, Nq, heads, d) * F32(d ** -0.5)).astype(np.float64)
    s = np.einsum("bqmc,bkmc->bmqk", qs, k.reshape(B, Nk, heads, d).astype(np.float64))
    with np.errstate(invalid="ignore"):
        low = s - np.where(np.isnan(s), -np.inf, s).max(-1, keepdims=True)
        return q, k, v, plant, bool((low < -104.5).any()), bool(((low > -103) & (low < -88)).any())


@pytest.mark.parametrize("Nq,Nk", MHA_SWEEP)
def test_mha_sweep(expf, Nq, Nk):
    from paddle3d_amd.ops import bevformer_decoder as ops

    seen_zero = seen_sub = False
    for d in (16, 32, 64):
        for heads in (1, 3):
            for B in (1, 2):
                q, k, v, plant, zero, sub = mha_case(Nq, Nk, d, heads, B)
                seen_zero, seen_sub = seen_zero or zero, seen_sub or sub
                want = dn.mha(q, k, v, heads, expf)
                got = ops.multihead_attention(_t(q), _t(k), _t(v), heads)
                same_bits(got, want, nan_ok=True)
                if plant:  # the NaN of q takes its row of one head, the NaN of v every query of frame 0
                    nan = np.isnan(want)
                    assert nan[0].all() and nan[B - 1, Nq // 2].any() and (B == 1 or not nan[1].all())
                else:
                    assert np.isfinite(want).all()
    assert Nk < 16 or (seen_zero and seen_sub), (seen_zero, seen_sub)


def _odd_points(rng, ref):
    """NaN, Inf and 1e30 planted among the reference points."""
    flat = ref.reshape(-1)
    idx = rng.choice(flat.size, size=max(1, flat.size // 8), replace=False)
    flat[idx] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], F32), size=idx.size)
    return ref


# (Q, C, M, levels, P, one reference point for all levels, B); L * P = 32 in three of them, 33 in the last (refused)
CA_SWEEP = [(1, 4, 1, [[3, 4]], 4, True, 1), (17, 32, 2, [[7, 11]], 4, True, 2), (33, 16, 8, [[5, 6], [3, 3]], 8, False, 1),
            (31, 64, 2, [[4, 4], [3, 3], [2, 2], [1, 1]], 8, False, 1), (77, 32, 1, [[4, 4], [3, 3], [2, 2], [1, 1]], 8, True, 2),
            (16, 4, 3, [[6, 5]], 32, True, 1), (20, 32, 2, [[6, 5]], 33, True, 1)]


@pytest.mark.parametrize("i", range(len(CA_SWEEP)))
def test_cross_attention_sweep(expf, i):
    from paddle3d_amd.ops import bevformer_decoder as ops

    Q, C, heads, shapes, P, one, B = CA_SWEEP[i]
    rng = np.random.default_rng(400 + i)
    sh, lsi, S = dn.md.level_layout(shapes)
    L = len(shapes)
    value = rng.standard_normal((B, S, heads, C)).astype(F32)
    off = (rng.standard_normal((B, Q, heads, L, P, 2)) * 1.5).astype(F32)
    logits = (rng.standard_normal((B, Q, heads, L * P)) * 2).astype(F32)
    ref = _odd_points(rng, rng.uniform(-0.2, 1.2, (B, Q, 1 if one else L, 2)).astype(F32))
    got = ops.decoder_cross_attention_sample(_t(value), _t(off), _t(logits), _t(ref), _t(sh), _t(lsi))
    if L * P > 32:
        assert got is None and not ops.dec_ca_supported(C, L, P)
        return
    want = dn.dec_ca(value, off, logits, ref, sh, lsi, expf)
    same_bits(got, want)
    assert np.isfinite(want).all() and (Q < 5 or np.abs(want).max() > 0)


# (Q, K, code, max_num, score_threshold, bottom_center, what is planted)
DECODE_SWEEP = [(103, 10, 10, 300, None, True, "ties"), (341, 3, 8, 1, 0.3, False, "ties"), (128, 8, 10, 1024, None, True, "nan"),
                (205, 10, 8, 1024, 0.2, False, "ties"), (2047, 1, 10, 300, None, True, "nan"), (1025, 2, 8, 1024, 0.9, True, "ties"),
                (103, 10, 10, 300, 0.05, False, "outside"), (64, 16, 8, 1, None, True, "outside"), (7, 3, 10, 21, 0.0, False, "nan")]


@pytest.mark.parametrize("i", range(len(DECODE_SWEEP)))
def test_decode_sweep(expf, atan2f, i):
    from paddle3d_amd.ops import bevformer_decoder as ops

    Q, K, code, max_num, thr, bottom, plant = DECODE_SWEEP[i]
    B = 2
    rng = np.random.default_rng(500 + i)
    post = [-8.0, -8.0, -2.5, 8.0, 8.0, 4.0]
    cls = rng.uniform(-5.0, 3.0, (B, Q, K)).astype(F32)
    bbox = (rng.standard_normal((B, Q, code)) * 0.5).astype(F32)
    ctr = rng.uniform(-10, 10, (B, Q, 3)) * np.array([1, 1, 0.4])
    if plant == "outside":
        ctr = np.abs(ctr) + np.array([8.5, 0, 0])
    bbox[..., 0], bbox[..., 1], bbox[..., 4] = ctr[..., 0], ctr[..., 1], ctr[..., 2]
    if plant == "ties":  # equal logits in several classes and rows, among the best
        rows = rng.choice(Q, size=min(Q, 12), replace=False)
        cls[:, rows] = np.tile(np.array([2.5, 2.5, 2.75], F32), K)[:K]
        cls[0, rows[:3], 0] = 2.9
    if plant == "nan":
        cls.reshape(-1)[rng.choice(cls.size, size=max(2, cls.size // 9), replace=False)] = np.nan
        cls[1, 0, 0] = np.nan
        bbox[0, :, 3] = np.where(rng.random(Q) < 0.2, np.nan, bbox[0, :, 3])  # a NaN size does not touch the mask
        bbox[1, ::7, 1] = np.nan  # a NaN centre is outside
    want = dn.nms_free_decode(cls, bbox, post, max_num, thr, bottom, expf, atan2f)
    got = ops.nms_free_decode(_t(cls), _t(bbox), post, max_num, thr, bottom)
    for a, b in zip(got, want[:4]):
        same_bits(a, b, nan_ok=True)
    count = want[3]
    if plant == "outside":
        assert not count.any() and not want[0].any() and (want[2] == -1).all()
    elif max_num > 1:
        assert (count > 0).all() and (count < max_num).all()
    if plant == "ties":
        assert any(len(set(want[1][b, :count[b]].tolist())) < count[b] for b in range(B)) or max_num == 1


def test_decode_errors():
    from paddle3d_amd.ops import bevformer_decoder as ops

    cls, bbox = torch.zeros(1, 10, 3, device=DEV), torch.zeros(1, 10, 10, device=DEV)
    post = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
    with pytest.raises(RuntimeError, match="max_num"):
        ops.nms_free_decode(cls, bbox, post, 31)
    with pytest.raises(RuntimeError, match="max_num"):
        ops.nms_free_decode(torch.zeros(1, 600, 3, device=DEV), torch.zeros(1, 600, 10, device=DEV), post, 1025)
    with pytest.raises(RuntimeError, match="code size"):
        ops.nms_free_decode(cls, bbox[..., :9], post, 5)
    with pytest.raises(RuntimeError, match="score_threshold"):
        ops.nms_free_decode(cls, bbox, post, 5, score_threshold=float("inf"))
    with pytest.raises(RuntimeError, match="Unsupported device"):
        ops.nms_free_decode(cls.cpu(), bbox, post, 5)
    boxes, scores, labels, count = ops.nms_free_decode(cls, bbox, post, 30)  # max_num = Q * K, all scores tie
    assert count.tolist() == [30] and labels[0].tolist() == [i % 3 for i in range(30)] and (scores == 0.5).all()


def test_a_frame_alone_elsewhere_and_on_a_side_stream(golden):
    from paddle3d_amd.ops import bevformer_decoder as ops

    tag = "c"
    c = mk.CASES[tag]
    q, k, v = (_t(a) for a in cpu.mha_inputs(tag))
    value, off, logits, ref, sh, lsi = (_t(a) for a in cpu.ca_inputs(tag))
    cls, bbox = (_t(a) for a in cpu.decode_case(golden, tag, "dec"))
    dec = lambda cl, bb: ops.nms_free_decode(cl, bb, c["post"], c["max_num"], c["thr"], True)  # noqa: E731
    mha, ca, det = ops.multihead_attention(q, k, v, M), ops.decoder_cross_attention_sample(value, off, logits, ref, sh, lsi), dec(cls, bbox)
    for b in range(c["B"]):  # alone
        s = slice(b, b + 1)
        assert torch.equal(ops.multihead_attention(q[s], k[s], v[s], M)[0], mha[b])
        assert torch.equal(ops.decoder_cross_attention_sample(value[s], off[s], logits[s], ref[s], sh, lsi)[0], ca[b])
        assert all(torch.equal(x[0], y[b]) for x, y in zip(dec(cls[s], bbox[s]), det))
    f = lambda t: t.flip(0)  # noqa: E731  (the two frames swapped)
    assert torch.equal(f(ops.multihead_attention(f(q), f(k), f(v), M)), mha)
    assert torch.equal(f(ops.decoder_cross_attention_sample(f(value), f(off), f(logits), f(ref), sh, lsi)), ca)
    assert all(torch.equal(f(x), y) for x, y in zip(dec(f(cls), f(bbox)), det))
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        mha2, ca2 = ops.multihead_attention(q, k, v, M), ops.decoder_cross_attention_sample(value, off, logits, ref, sh, lsi)
        det2 = dec(cls, bbox)
    side.synchronize()
    assert torch.equal(mha2, mha) and torch.equal(ca2, ca) and all(torch.equal(x, y) for x, y in zip(det2, det))
    assert det[3].tolist() == golden[f"{tag}_dec_count"].tolist()


# ---- the modules against the reference -------------------------------------------------------------------------------

_modules = {}


def head(tag, fused):
    return cpu.build_head(tag, fused).to(DEV)


def module_outputs(tag, fused):
    """Every stored result of the modules, once per (case, fused); the decode runs on the head's own output."""
    if (tag, fused) not in _modules:
        h = head(tag, fused)
        out = dict(cpu.first_layer_outputs(h, tag, DEV)) if tag in ("a", "b") else {}
        model, outs = cpu.model_outputs(h, tag, DEV)
        out.update(model)
        with torch.no_grad():
            det = h.get_bboxes(outs)
        _modules[tag, fused] = ({k: _n(v) for k, v in out.items()}, tuple(_n(t) for t in det))
    return _modules[tag, fused]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("tag", TAGS)
def test_modules_against_the_reference(golden, tag, fused):
    out, det = module_outputs(tag, fused)
    assert set(out) == set(mk.results(tag)) - {"mha_sample", "ca_sample"}  # those two are the ops' (above)
    errs = []
    for name, got in out.items():
        want, bound = golden[f"{tag}_{name}"], float(golden[f"{tag}_{name}_bound"])
        e = float(np.abs(got.astype(np.float64) - want).max())
        print(f"{tag} fused={fused} {name} err {e:.3e} bound {bound:.3e} (reference's own "
              f"{float(golden[f'{tag}_{name}_ref_err']):.3e})")
        assert got.shape == want.shape and got.dtype == F32
        errs.append((name, e, bound))
    assert all(e <= b for _, e, b in errs), errs
    if "chain" in mk.DECODES[tag]:
        cpu.check_decode(golden, tag, "chain", *det)


@pytest.mark.parametrize("tag", TAGS)
def test_fused_against_unfused(golden, tag):
    (f, fd), (u, ud) = module_outputs(tag, True), module_outputs(tag, False)
    errs = []
    for name in f:
        e, bound = float(np.abs(f[name].astype(np.float64) - u[name]).max()), float(golden[f"{tag}_{name}_bound"])
        print(f"{tag} {name} fused against unfused {e:.3e} bound {bound:.3e}")
        errs.append((name, e, bound))
    assert all(e <= b for _, e, b in errs), errs
    if "chain" in mk.DECODES[tag]:  # the selection is the same, the rows agree within the decode's bounds
        assert np.array_equal(fd[3], ud[3]) and np.array_equal(fd[2], ud[2])
        assert np.abs(fd[0].astype(np.float64) - ud[0]).max() <= float(golden[f"{tag}_chain_boxes_bound"])
        assert np.abs(fd[1].astype(np.float64) - ud[1]).max() <= float(golden[f"{tag}_chain_scores_bound"])


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("tag", TAGS)
def test_coder_on_the_stand_alone_cases(golden, tag, fused):
    from paddle3d_amd import bevformer_head as bh

    c = mk.CASES[tag]
    coder = bh.NMSFreeCoder(mk.PC_RANGE, post_center_range=c["post"], max_num=c["max_num"], score_threshold=c["thr"],
                            num_classes=c["K"], fused=fused)
    cls, bbox = (_t(a)[None] for a in cpu.decode_case(golden, tag, "dec"))
    got = coder.decode(dict(all_cls_scores=cls, all_bbox_preds=bbox), bottom_center=True)
    cpu.check_decode(golden, tag, "dec", *(_n(t) for t in got))
    lst = coder.to_list(*got)
    assert [len(d["scores"]) for d in lst] == golden[f"{tag}_dec_count"].tolist()


def test_refused_shapes_fall_back():
    """d = 24 or 6 (no multiple of 16), Nk above the cap, C = 6 and L * P = 36: the ops return None, the fused modules
    take the unfused route and give the unfused modules' bits."""
    from paddle3d_amd import _lib, bevformer_head as bh
    from paddle3d_amd.ops import bevformer_decoder as ops

    names = _lib.symbols("test_memory_safety_bevformer_dec_gpu") + ("pd3_ms_deform_attn_forward",)
    B, Q = 1, 20
    sh, lsi, S = dn.md.level_layout([[3, 4]])
    sh, lsi = _t(sh), _t(lsi)
    ref = torch.rand(B, Q, 1, 2, device=DEV)
    for E, heads, P, mha_ok, ca_ok in ((48, 2, 4, False, True), (12, 2, 8, False, False), (16, 1, 36, True, False)):
        torch.manual_seed(5)
        q = torch.randn(Q, B, E, device=DEV)
        pos = torch.randn(Q, B, E, device=DEV)
        bev = torch.randn(S, B, E, device=DEV)
        outs = []
        for fused in (True, False):
            torch.manual_seed(6)
            mha = bh.MultiheadAttention(E, heads, fused=fused).eval().to(DEV)
            ca = bh.CustomMSDeformableAttention(E, heads, num_levels=1, num_points=P, fused=fused).eval().to(DEV)
            with torch.no_grad(), launch_ledger(_lib.lib(), names) as n:
                outs.append((mha(q, q, q, None, query_pos=pos, key_pos=pos),
                             ca(q, None, bev, None, query_pos=pos, reference_points=ref, spatial_shapes=sh,
                                level_start_index=lsi)))
            want = [int(fused and mha_ok), int(fused and ca_ok), int(not (fused and ca_ok)), 0]
            assert [n[k] for k in ("pd3_mha_forward", "pd3_bevformer_dec_ca", "pd3_ms_deform_attn_forward",
                                   "pd3_nms_free_decode")] == want, (E, heads, P, fused, dict(n))
        assert mha_ok or torch.equal(outs[0][0], outs[1][0])
        assert ca_ok or torch.equal(outs[0][1], outs[1][1])
        assert all(t.abs().max() > 0 and torch.isfinite(t).all() for pair in outs for t in pair)
        assert (outs[0][0] - outs[1][0]).abs().max() < 1e-4 and (outs[0][1] - outs[1][1]).abs().max() < 1e-4
        if not ca_ok:
            v = torch.randn(B, S, heads, E // heads, device=DEV)
            assert ops.decoder_cross_attention_sample(v, torch.randn(B, Q, heads, 1, P, 2, device=DEV),
                                                      torch.randn(B, Q, heads, P, device=DEV), ref, sh, lsi) is None
    x = torch.randn(1, 5, 48, device=DEV)
    assert ops.multihead_attention(x, x, x, 2) is None  # d = 24
    x = torch.randn(1, 5, 288, device=DEV)
    assert ops.multihead_attention(x, x, x, 2) is None  # d = 144
    k = torch.randn(1, ops.MAX_KEYS + 1, 32, device=DEV)
    assert ops.multihead_attention(k[:, :5], k, k, 2) is None
    got = ops.multihead_attention(k[:, :5], k[:, :ops.MAX_KEYS], k[:, :ops.MAX_KEYS], 2)  # the largest key count taken
    want = bh.MultiheadAttention(32, 2).core(k[:, :5], k[:, :ops.MAX_KEYS], k[:, :ops.MAX_KEYS])
    assert got is not None and (got - want).abs().max() < 1e-5
    # reference points of 4 are the torch route's
    ca = bh.CustomMSDeformableAttention(32, 2, num_levels=1, num_points=4).eval().to(DEV)
    with torch.no_grad(), launch_ledger(_lib.lib(), names) as n:
        out = ca(torch.randn(Q, B, 32, device=DEV), None, torch.randn(S, B, 32, device=DEV), None,
                 reference_points=torch.rand(B, Q, 1, 4, device=DEV), spatial_shapes=sh, level_start_index=lsi)
    assert n["pd3_bevformer_dec_ca"] == 0 and n["pd3_ms_deform_attn_forward"] == 1 and torch.isfinite(out).all()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_forward_makes_no_host_sync(golden, fused):
    tag = "a"
    h = head(tag, fused)
    bev = _t(mk.inputs(tag)["bev_embed"])
    want, want_det = module_outputs(tag, fused)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            outs = h.forward_from_bev(bev)
            det = h.get_bboxes(outs)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for name in ("all_cls_scores", "all_bbox_preds"):
        cpu.check_result(golden, tag, name, _n(outs[name]))
    assert np.array_equal(_n(det[3]), want_det[3]) and np.array_equal(_n(det[2]), want_det[2])
    cpu.check_decode(golden, tag, "chain", *(_n(t) for t in det))


def test_launch_counts(golden):
    from paddle3d_amd import _lib

    tag = "c"
    names = ("pd3_mha_forward", "pd3_bevformer_dec_ca", "pd3_nms_free_decode")
    symbols = _lib.symbols("test_memory_safety_bevformer_dec_gpu") + ("pd3_ms_deform_attn_forward",)
    bev = _t(mk.inputs(tag)["bev_embed"])
    h = head(tag, True)
    with torch.no_grad():
        with launch_ledger(_lib.lib(), symbols) as n:
            h.get_bboxes(h.forward_from_bev(bev))
        assert [n[k] for k in names] == [mk.LAYERS, mk.LAYERS, 1] and n["pd3_ms_deform_attn_forward"] == 0, dict(n)
        with launch_ledger(_lib.lib(), symbols) as n:
            cpu.first_layer_outputs(h, tag, DEV)  # each attention alone, then the layer
        assert [n[k] for k in names] == [2, 2, 0] and n["pd3_ms_deform_attn_forward"] == 0, dict(n)
        u = head(tag, False)
        with launch_ledger(_lib.lib(), symbols) as n:
            u.get_bboxes(u.forward_from_bev(bev))
        assert [n[k] for k in names] == [0, 0, 0] and n["pd3_ms_deform_attn_forward"] == mk.LAYERS, dict(n)
