"""PETR / PETRv2's head on the device: the two entry points of csrc/petr.hip against the NumPy restatement
(tests/golden/petr_numpy.py) -- the streamed attention bit for bit on the golden cases and on seeded sweeps, the
coordinates bit for bit where the clip makes them a constant and on coords_mask, and within one float32 ulp of
float32(log(float64(ratio))) of the restated ratio elsewhere (a double logarithm whose error is below one double ulp,
rounded once to float32, cannot be further from the correctly rounded value than that) -- and the ops and the modules
of paddle3d_amd.petr_head (fused and unfused; attention modules, layer, 2-layer decoder, head, decode) against what the
reference's own Python computed (tests/golden/python_petr.npz) within the bounds the maker stored: 4 x the
reference's own fp32 error.  Fused against unfused is held to the same bound.  Also: a frame alone, elsewhere in the
batch and on a side stream gives the same bits, as do the first 16 query rows whatever Nq is; refused shapes return
None and the modules fall back; a forward makes no host synchronisation; a fused forward launches the coordinate kernel
once and each attention kernel once per decoder layer."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from guarded import launch_ledger  # noqa: E402

import make_petr_golden as mk  # noqa: E402
import petr_numpy as pn  # noqa: E402
import test_petr_cpu as cpu  # noqa: E402
from test_bevformer_decoder_cpu import check_decode, check_result  # noqa: E402
from test_bevformer_decoder_gpu import MHA_SWEEP, same_bits  # noqa: E402
from test_petr_cpu import expf, golden  # noqa: E402,F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
TAGS = mk.TAGS
M = mk.HEADS
H, W = mk.FEAT
KC = 64  # the keys of one round of the kernel: four waves of one 16-key tile each


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.detach().cpu().numpy()


# ---- pd3_mha_stream_forward against the restatement ------------------------------------------------------------------


@pytest.mark.parametrize("tag", ["a", "b"])
def test_stream_attention_on_the_golden_cases(golden, expf, tag):
    from paddle3d_amd.ops import petr as ops

    q, k, v, km = cpu.ca_inputs(tag)
    got = ops.multihead_attention_stream(_t(q), _t(k), _t(v), M, _t(km))
    same_bits(got, cpu.restated(tag, expf)[4])
    check_result(golden, tag, "ca_core", _n(got))
    got3 = ops.multihead_attention_stream(_t(q), _t(k), _t(v), M, _t(km[:, None, :]).view(torch.uint8))  # [B, 1, Nk] uint8
    assert torch.equal(got3, got)


MASKS = ("none", "random", "all_but_one", "frame", "last_tile")


def key_mask(kind, rng, B, Nk):
    if kind == "none":
        return None
    m = np.zeros((B, Nk), bool)
    if kind == "random":
        m = rng.random((B, Nk)) < 0.3
    elif kind == "all_but_one":
        m[:] = True
        m[:, Nk // 2] = False
    elif kind == "frame":  # every key of the last frame
        m[B - 1] = True
    else:  # only keys of the last partial tile
        m[:, (Nk - 1) // 16 * 16:] = True
        m[:, Nk - 1] = Nk % 2 == 0
    return m


def stream_case(Nq, Nk, d, heads, B):
    """(q, k, v, a NaN row planted, an expf underflows to 0 somewhere, to a subnormal somewhere) of one sweep point."""
    rng = np.random.default_rng(7000 * Nq + 10 * Nk + d + heads + B)
    E = heads * d
    q, k, v = (rng.standard_normal((B, n, E)).astype(F32) for n in (Nq, Nk, Nk))
    q *= rng.choice(np.array([1, 6, 60], F32), size=(B, Nq, 1))  # rows whose expf underflows
    plant = Nq > 1 and Nk > 1
    if plant:
        q[B - 1, Nq // 2, E // 3] = np.nan
    qs = (q.reshape(B, Nq, heads, d) * F32(d ** -0.5)).astype(np.float64)
    s = np.einsum("bqmc,bkmc->bmqk", qs, k.reshape(B, Nk, heads, d).astype(np.float64))
    with np.errstate(invalid="ignore"):
        low = s - np.where(np.isnan(s), -np.inf, s).max(-1, keepdims=True)
        return q, k, v, plant, bool((low < -104.5).any()), bool(((low > -103) & (low < -88)).any())


def run_stream_point(expf, Nq, Nk, d, heads, B, kind):
    from paddle3d_amd.ops import petr as ops

    q, k, v, plant, zero, sub = stream_case(Nq, Nk, d, heads, B)
    km = key_mask(kind, np.random.default_rng(Nq + Nk), B, Nk)
    want = pn.mha_stream(q, k, v, heads, expf, km)
    got = ops.multihead_attention_stream(_t(q), _t(k), _t(v), heads, None if km is None else _t(km))
    same_bits(got, want, nan_ok=True)
    nan = np.isnan(want)
    if plant:  # the NaN of q takes its row of one head and nothing else
        assert nan[B - 1, Nq // 2].any() and int(nan.any(-1).sum()) == 1
    else:
        assert not nan.any()
    assert np.isfinite(want[~nan]).all()  # an all-padded row is a finite softmax
    return zero, sub


@pytest.mark.parametrize("Nq,Nk", MHA_SWEEP)
def test_stream_attention_sweep(expf, Nq, Nk):
    seen_zero = seen_sub = False
    for d in (16, 32, 128):
        for heads, B in ((1, 1), (3, 2)):
            for kind in MASKS:
                zero, sub = run_stream_point(expf, Nq, Nk, d, heads, B, kind)
                seen_zero, seen_sub = seen_zero or zero, seen_sub or sub
    assert Nk < 16 or (seen_zero and seen_sub), (seen_zero, seen_sub)


@pytest.mark.parametrize("Nk", [KC - 1, KC, KC + 1, 2 * KC + 1])
def test_stream_attention_at_the_key_chunk(expf, Nk):
    for d, heads, B in ((16, 3, 2), (32, 1, 1), (128, 1, 2)):
        for kind in MASKS:
            run_stream_point(expf, 17, Nk, d, heads, B, kind)


def test_stream_attention_beyond_the_lds_kernels_cap(expf):
    """Nk = 2049: one key more than pd3_mha_forward takes."""
    from paddle3d_amd.ops import bevformer_decoder as dec_ops

    for kind in ("none", "random"):
        run_stream_point(expf, 17, 2049, 16, 1, 1, kind)
    assert not dec_ops.mha_supported(16, 2049)


def test_stream_attention_alone_elsewhere_side_stream_and_query_tiling(expf):
    from paddle3d_amd.ops import petr as ops

    q, k, v, km = (_t(a) for a in cpu.ca_inputs("a"))
    run = lambda q, k, v, km: ops.multihead_attention_stream(q, k, v, M, km)  # noqa: E731
    out = run(q, k, v, km)
    for b in range(q.shape[0]):  # alone
        s = slice(b, b + 1)
        assert torch.equal(run(q[s], k[s], v[s], km[s])[0], out[b])
    f = lambda t: t.flip(0)  # noqa: E731  (the two frames swapped)
    assert torch.equal(f(run(f(q), f(k), f(v), f(km))), out)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        out2 = run(q, k, v, km)
    side.synchronize()
    assert torch.equal(out2, out)
    assert q.shape[1] == 37
    assert torch.equal(run(q[:, :16].contiguous(), k, v, km), out[:, :16])  # Nq = 16 and Nq = 37: the same first rows


def test_stream_attention_refusals_and_errors():
    from paddle3d_amd.ops import petr as ops

    x = torch.randn(1, 5, 48, device=DEV)
    assert ops.multihead_attention_stream(x, x, x, 2) is None and not ops.mha_stream_supported(24, 5)  # d = 24
    x = torch.randn(1, 5, 288, device=DEV)
    assert ops.multihead_attention_stream(x, x, x, 2) is None  # d = 144
    x = torch.randn(1, 6, 36, device=DEV)[:, :, 1:33]  # d = 16 at an address that is no multiple of 16: made contiguous
    assert ops.multihead_attention_stream(x, x, x, 2) is not None
    x = torch.randn(2, 5, 32, device=DEV)
    assert ops.multihead_attention_stream(x[:, :0], x, x, 2).shape == (2, 0, 32)
    with pytest.raises(RuntimeError, match="key_padding_mask"):
        ops.multihead_attention_stream(x, x, x, 2, torch.zeros(2, 6, dtype=torch.bool, device=DEV))
    with pytest.raises(RuntimeError, match="key_padding_mask"):
        ops.multihead_attention_stream(x, x, x, 2, torch.zeros(2, 5, device=DEV))
    with pytest.raises(RuntimeError, match="Unsupported device"):
        ops.multihead_attention_stream(x.cpu(), x, x, 2)
    with pytest.raises(RuntimeError, match="multiple of num_heads"):
        ops.multihead_attention_stream(x, x, x, 3)


# ---- pd3_petr_coords3d against the restatement -----------------------------------------------------------------------


def check_coords(got, got_mask, args, token_mask=None):
    """The kernel's output against the restated ratio: bit-equal where the clip decides, one ulp elsewhere."""
    ratio, mask, norm = pn.coords3d_ratio(*args, token_mask=token_mask)
    with np.errstate(all="ignore"):
        want = np.log(ratio.astype(np.float64)).astype(F32)
        const = (norm <= 0) | (norm >= 1)  # the ratio is eps / 1 or 1 / eps there
        ulp = np.spacing(np.abs(want))
    got = _n(got)
    assert got.shape == want.shape and got.dtype == F32
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[const & ~nan].view(np.uint32), want[const & ~nan].view(np.uint32))
    assert len(np.unique(want[const & ~nan])) <= 2
    ok = ~nan
    assert (np.abs(got[ok].astype(np.float64) - want[ok]) <= ulp[ok]).all()
    if got_mask is not None:
        assert got_mask.dtype == torch.bool and np.array_equal(_n(got_mask), mask)
    return want, mask, const


@pytest.mark.parametrize("tag", TAGS)
def test_coords3d_on_the_golden_cases(golden, tag):
    from paddle3d_amd.ops import petr as ops

    c = mk.CASES[tag]
    args = cpu.coords_args(tag)
    tm = cpu.token_masks(tag)
    got, got_mask = ops.petr_coords3d(_t(args[0]), (H, W), mk.PAD, mk.D, c["depth_start"], c["position_range"], c["LID"],
                                      token_mask=_t(tm), want_mask=True)
    want, mask, const = check_coords(got, got_mask, args, tm)
    assert const.any() and not const.all()
    check_result(golden, tag, "coords3d", _n(got))
    assert np.array_equal(_n(got_mask).reshape(c["B"], c["N"], H, W), golden[f"{tag}_coords_mask"])
    alone = ops.petr_coords3d(_t(args[0]), (H, W), mk.PAD, mk.D, c["depth_start"], c["position_range"], c["LID"])
    assert isinstance(alone, torch.Tensor) and torch.equal(alone, got)  # the optional pointers NULL


# (BN, H, W, D, LID, what is planted)
COORD_SWEEP = [(1, 1, 1, 1, True, None), (2, 3, 1, 5, False, None), (1, 1, 9, 1, True, None), (3, 2, 65, 3, True, None),
               (2, 4, 130, 9, False, "odd"), (1, 5, 7, 64, True, "odd"), (2, 5, 7, 6, False, "mask")]


@pytest.mark.parametrize("i", range(len(COORD_SWEEP)))
def test_coords3d_sweep(i):
    from paddle3d_amd.ops import petr as ops

    BN, h, w, D, LID, plant = COORD_SWEEP[i]
    rng = np.random.default_rng(900 + i)
    m = mk.inputs("a")["img2lidars"].reshape(-1, 4, 4)[rng.integers(0, 6, BN)].copy()
    m[:, :3, 3] += rng.uniform(-3, 3, (BN, 3)).astype(F32)
    if plant == "odd":  # NaN, Inf and 1e30 matrix entries
        m[0, 0, 1], m[0, 2, 3] = np.nan, 1e30
        m[BN - 1, 1, 0] = np.inf
        m[BN - 1, 2, 2] = -1e30
    tm = rng.random((BN, h, w)) < 0.4 if plant == "mask" else None
    r = [-20.0, -15.0, -6.0, 20.0, 25.0, 6.0]
    pad = (8 * h, 8 * w)
    got, got_mask = ops.petr_coords3d(_t(m), (h, w), pad, D, 1.0, r, LID, token_mask=None if tm is None else _t(tm),
                                      want_mask=True)
    want, mask, const = check_coords(got, got_mask, (m, h, w, D, pad[0], pad[1], 1.0, r, LID), tm)
    assert got.shape == (BN, 3 * D, h, w)
    if plant == "odd":
        assert np.isnan(want).any() and not np.isnan(want).all()
    if plant == "mask":
        assert (mask & ~tm).any() or (tm & mask).any()
    z = ops.petr_coords3d(_t(m), (h, 0), pad, D, 1.0, r, LID, want_mask=True)
    assert z[0].shape == (BN, 3 * D, h, 0) and z[1].shape == (BN, h, 0)
    with pytest.raises(RuntimeError, match="token_mask"):
        ops.petr_coords3d(_t(m), (h, w), pad, D, 1.0, r, LID, token_mask=torch.zeros(BN, h + 1, w, dtype=torch.bool, device=DEV))
    with pytest.raises(RuntimeError, match="img2lidars"):
        ops.petr_coords3d(_t(m[:, :3]), (h, w), pad, D, 1.0, r, LID)


# ---- the modules against the reference -------------------------------------------------------------------------------

_modules = {}


def head(tag, fused):
    return cpu.build_head(tag, fused).to(DEV)


def module_outputs(tag, fused):
    """Every stored result of the modules, once per (case, fused); the decode runs on the head's own output."""
    if (tag, fused) not in _modules:
        h = head(tag, fused)
        out = dict(cpu.piece_outputs(h, tag, DEV)) if tag != "c" else {}
        res, outs = cpu.chain_outputs(h, tag, DEV)
        out.update(res)
        with torch.no_grad():
            det = h.get_bboxes(outs)
        _modules[tag, fused] = ({k: _n(v) for k, v in out.items()}, tuple(_n(t) for t in det))
    return _modules[tag, fused]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("tag", TAGS)
def test_modules_against_the_reference(golden, tag, fused):
    out, det = module_outputs(tag, fused)
    assert set(out) == set(mk.results(tag)) - {"coords_norm", "coords3d", "ca_core"} | {"coords_mask"}  # those are the ops'
    errs = []
    for name, got in out.items():
        if name == "coords_mask":
            assert np.array_equal(got, golden[f"{tag}_coords_mask"])
            continue
        want, bound = golden[f"{tag}_{name}"], float(golden[f"{tag}_{name}_bound"])
        e = float(np.abs(got.astype(np.float64) - want).max())
        print(f"{tag} fused={fused} {name} err {e:.3e} bound {bound:.3e} (reference's own "
              f"{float(golden[f'{tag}_{name}_ref_err']):.3e})")
        assert got.shape == want.shape and got.dtype == F32
        errs.append((name, e, bound))
    assert all(e <= b for _, e, b in errs), errs
    check_decode(golden, tag, "chain", *det)


@pytest.mark.parametrize("tag", TAGS)
def test_fused_against_unfused(golden, tag):
    (f, fd), (u, ud) = module_outputs(tag, True), module_outputs(tag, False)
    errs = []
    for name in f:
        if name == "coords_mask":
            assert np.array_equal(f[name], u[name])
            continue
        e, bound = float(np.abs(f[name].astype(np.float64) - u[name]).max()), float(golden[f"{tag}_{name}_bound"])
        print(f"{tag} {name} fused against unfused {e:.3e} bound {bound:.3e}")
        errs.append((name, e, bound))
    assert all(e <= b for _, e, b in errs), errs
    assert np.array_equal(fd[3], ud[3]) and np.array_equal(fd[2], ud[2])  # the same selection
    assert np.abs(fd[0].astype(np.float64) - ud[0]).max() <= float(golden[f"{tag}_chain_boxes_bound"])
    assert np.abs(fd[1].astype(np.float64) - ud[1]).max() <= float(golden[f"{tag}_chain_scores_bound"])


NAMES = ("pd3_mha_forward", "pd3_mha_stream_forward", "pd3_petr_coords3d", "pd3_nms_free_decode")


def test_refused_shapes_fall_back():
    """d = 24 or 6 (no multiple of 16): the op returns None, the fused modules take the torch route and give the unfused
    modules' bits; with an attn_mask the cross-attention is the torch route's too."""
    from paddle3d_amd import _lib, petr_head as ph

    B, Q, Nk = 2, 20, 45
    for E, heads, ok in ((48, 2, False), (12, 2, False), (32, 2, True)):
        torch.manual_seed(5)
        q, pos = torch.randn(B, Q, E, device=DEV), torch.randn(B, Q, E, device=DEV)
        mem, kpos = torch.randn(B, Nk, E, device=DEV), torch.randn(B, Nk, E, device=DEV)
        km = torch.rand(B, 1, Nk, device=DEV) < 0.3
        outs = []
        for fused in (True, False):
            torch.manual_seed(6)
            sa = ph.MultiHeadAttention(E, heads, fused=fused).eval().to(DEV)
            ca = ph.PETRMultiheadAttention(E, heads, fused=fused).eval().to(DEV)
            with torch.no_grad(), launch_ledger(_lib.lib(), NAMES) as n:
                outs.append((sa(q, q, q, None, query_pos=pos, key_pos=pos),
                             ca(q, mem, mem, None, query_pos=pos, key_pos=kpos, key_padding_mask=km)))
            assert [n[k] for k in NAMES] == [int(fused and ok), int(fused and ok), 0, 0], (E, fused, dict(n))
        assert ok or (torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]))
        assert all(t.abs().max() > 0 and torch.isfinite(t).all() for pair in outs for t in pair)
        assert (outs[0][0] - outs[1][0]).abs().max() < 1e-4 and (outs[0][1] - outs[1][1]).abs().max() < 1e-4
    ca = ph.PETRMultiheadAttention(32, 2).eval().to(DEV)
    with torch.no_grad(), launch_ledger(_lib.lib(), NAMES) as n:
        out = ca(q, mem, mem, None, attn_mask=torch.rand(Q, Nk, device=DEV) < 0.2)
    assert n["pd3_mha_stream_forward"] == 0 and torch.isfinite(out).all()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_forward_makes_no_host_sync(golden, fused):
    tag = "b"
    h = head(tag, fused)
    args = cpu.forward_args(tag, DEV)
    want, want_det = module_outputs(tag, fused)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            outs = h(*args)
            det = h.get_bboxes(outs)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for name in ("all_cls_scores", "all_bbox_preds"):
        check_result(golden, tag, name, _n(outs[name]))
    assert np.array_equal(_n(det[3]), want_det[3]) and np.array_equal(_n(det[2]), want_det[2])
    check_decode(golden, tag, "chain", *(_n(t) for t in det))


def test_launch_counts(golden):
    from paddle3d_amd import _lib

    tag = "a"
    args = cpu.forward_args(tag, DEV)
    h = head(tag, True)
    with torch.no_grad():
        with launch_ledger(_lib.lib(), NAMES) as n:
            h.get_bboxes(h(*args))
        # one launch for the position embedding, two attention launches per decoder layer, one decode
        assert [n[k] for k in NAMES] == [mk.LAYERS, mk.LAYERS, 1, 1], dict(n)
        with launch_ledger(_lib.lib(), NAMES) as n:
            cpu.piece_outputs(h, tag, DEV)  # each attention alone, the layer, the 2-layer decoder
        assert [n[k] for k in NAMES] == [2 + mk.LAYERS, 2 + mk.LAYERS, 0, 0], dict(n)
        u = head(tag, False)
        with launch_ledger(_lib.lib(), NAMES) as n:
            u.get_bboxes(u(*args))
        assert [n[k] for k in NAMES] == [0, 0, 0, 0], dict(n)


def test_an_attention_can_opt_out_inside_a_layer():
    """`fused=False` in the attentions' own cfgs: a fused head launches the coordinate kernel and the decode only."""
    from paddle3d_amd import _lib, petr_head as ph
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    tag = "a"
    cfg = mk.head_cfg(tag, True)
    for a in cfg["transformer"]["decoder"]["transformerlayers"]["attns"]:
        a["fused"] = False
    h = ph.PETRHead(**cfg)
    assert load_paddle_state_dict(h, mk.state(tag)) == []
    h = h.eval().to(DEV)
    with torch.no_grad(), launch_ledger(_lib.lib(), NAMES) as n:
        det = h.get_bboxes(h(*cpu.forward_args(tag, DEV)))
    assert [n[k] for k in NAMES] == [0, 0, 1, 1], dict(n)
    want = module_outputs(tag, False)[1]
    assert np.array_equal(_n(det[3]), want[3]) and np.array_equal(_n(det[2]), want[2])
