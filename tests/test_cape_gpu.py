"""CAPE / CAPE-T's attention layers on the device: the two entry points of csrc/cape.hip against the NumPy restatement
(tests/golden/cape_numpy.py) bit for bit -- on the golden cases and on seeded sweeps over the tile, camera, query-block
and head-dim borders, every mask kind (the wholly masked NaN row included) and hostile data (zero and negative scales,
expf underflowing to subnormals and to 0, a NaN query row, an Inf in v under a masked key and under an unmasked key of
weight 0) -- and the ops and the modules of paddle3d_amd.cape (forced, default, unfused) against what the reference's
own Python computed (tests/golden/python_cape.npz) within the bounds the maker stored.  Also: the first 16 rows are the
same for 16 and 37 queries; a frame alone, elsewhere in the batch and on a side stream gives the same bits; refused
shapes return None and the modules fall back; nothing synchronises with the host; a layer launches each attention
kernel once, and the default takes each attention kernel up to its measured border only.  The 2-layer transformer in
both time settings and the head with its decode in the three forms against the reference; their launches, and the host
synchronisations of a forward and its decode pinned at zero."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from guarded import launch_ledger  # noqa: E402

import cape_numpy as cn  # noqa: E402
import make_cape_golden as mk  # noqa: E402
import test_cape_cpu as cpu  # noqa: E402
from test_bevformer_decoder_gpu import same_bits  # noqa: E402
from test_cape_cpu import check_result, expf, golden, sincos  # noqa: E402,F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
TAGS = mk.TAGS


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.detach().cpu().numpy()


def run_cva(q_a, q_g, k_a, k_g, v, sa, sg, heads, mask=None):
    from paddle3d_amd.ops import cape as ops

    return ops.cross_view_attention(_t(q_a), _t(q_g), _t(k_a), _t(k_g), _t(v), _t(sa), _t(sg), heads, _t(mask))


# ---- pd3_cape_cva_forward against the restatement ---------------------------------------------------------------------


@pytest.mark.parametrize("tag", TAGS)
def test_attention_on_the_golden_cases(golden, expf, tag):
    q_a, q_g, k_a, k_g, v, sa, sg, mask = cpu.ca_rows(golden, tag)
    heads = mk.CASES[tag]["heads"]
    got = run_cva(q_a, q_g, k_a, k_g, v, sa, sg, heads, mask)
    same_bits(got, cn.cva(q_a, q_g, k_a, k_g, v, sa, sg, heads, expf, mask))
    check_result(golden, tag, "ca_core", _n(got))
    got8 = run_cva(q_a, q_g, k_a, k_g, v, sa, sg, heads, mask.astype(np.uint8))
    assert torch.equal(got8, got)


MASKS = ("none", "random", "camera", "all_but_one", "last_tile", "every")
SCALES_A = np.array([0.25, -0.3, 0.0], F32)   # a negative and a zero scale
SCALES_G = np.array([-0.2, 0.0, 0.4], F32)


def key_mask(kind, rng, B, N, K):
    if kind == "none":
        return None
    m = np.zeros((B, N, K), bool)
    if kind == "random":
        m = rng.random((B, N, K)) < 0.3
        m[:, 0, 0] = False
    elif kind == "camera":  # one whole camera of the last frame (with one camera: every key of that frame)
        m[B - 1, N - 1] = True
    elif kind == "all_but_one":
        m[:] = True
        m[:, N // 2, K // 2] = False
    elif kind == "last_tile":  # the last, partial or whole, tile of camera 0 -- with one tile and one camera: every key
        m[:, 0, (K - 1) // 16 * 16:] = True
    else:
        m[:] = True
    return m


def cva_case(N, K, Q, d, heads, B):
    """(rows, a NaN planted at (b, q, head) or None, an expf underflows to 0 somewhere, to a subnormal somewhere)"""
    rng = np.random.default_rng(100000 * N + 100 * K + 7 * Q + d + heads + B)
    E = heads * d
    f = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    q_a, q_g, k_a, k_g, v = f(B, Q, E), f(B, N, Q, E), f(B, N, K, E), f(B, N, K, E), f(B, N, K, E)
    q_a *= rng.choice(np.array([1, 8, 80], F32), size=(B, Q, 1))  # rows whose expf underflows
    plant = None
    if Q > 1 and N * K > 1:
        plant = (B - 1, Q // 2, (E // 3) // d)
        q_a[B - 1, Q // 2, E // 3] = np.nan
    sa, sg = SCALES_A[:heads].copy(), SCALES_G[:heads].copy()
    a = np.einsum("bqmc,bnkmc->bmqnk", q_a.reshape(B, Q, heads, d).astype(np.float64),
                  k_a.reshape(B, N, K, heads, d).astype(np.float64)) * sa[None, :, None, None, None]
    g = np.einsum("bnqmc,bnkmc->bmqnk", q_g.reshape(B, N, Q, heads, d).astype(np.float64),
                  k_g.reshape(B, N, K, heads, d).astype(np.float64)) * sg[None, :, None, None, None]
    s = (a + g).reshape(B, heads, Q, N * K)
    with np.errstate(invalid="ignore"):
        low = s - np.where(np.isnan(s), -np.inf, s).max(-1, keepdims=True)
        return ((q_a, q_g, k_a, k_g, v, sa, sg), plant, bool((low < -104.5).any()),
                bool(((low > -103) & (low < -88)).any()))


def run_point(expf, N, K, Q, d, heads, B, kind):
    rows, plant, zero, sub = cva_case(N, K, Q, d, heads, B)
    mask = key_mask(kind, np.random.default_rng(N + K + Q), B, N, K)
    want = cn.cva(*rows, heads, expf, mask)
    got = run_cva(*rows, heads, mask)
    same_bits(got, want, nan_ok=True)
    nan = np.isnan(want).reshape(B, Q, heads, d)
    dead = np.zeros((B, Q, heads), bool)  # the rows the reference's softmax makes NaN: every key masked
    if mask is not None:
        dead[mask.reshape(B, -1).all(-1)] = True
    if plant is not None:
        dead[plant] = True
    assert np.array_equal(nan.all(-1), dead) and np.array_equal(nan.any(-1), dead)
    assert np.isfinite(want.reshape(B, Q, heads, d)[~dead]).all()
    return zero, sub


# (N, K): tiles per camera 1, 1, 1, 2, 3, 16; tiles in all 1, 1, 2, 6, 15, 32 and 5 -- multiples of the 4 waves and not
NK_SWEEP = [(1, 1), (1, 15), (2, 16), (3, 17), (5, 33), (2, 250), (5, 1)]
# (Q, d, heads, B)
SHAPES = [(1, 16, 1, 1), (15, 32, 2, 2), (16, 64, 3, 1), (17, 16, 3, 2), (37, 64, 2, 1)]


@pytest.mark.parametrize("N,K", NK_SWEEP)
def test_attention_sweep(expf, N, K):
    seen_zero = seen_sub = False
    for Q, d, heads, B in SHAPES:
        for kind in MASKS:
            zero, sub = run_point(expf, N, K, Q, d, heads, B, kind)
            seen_zero, seen_sub = seen_zero or zero, seen_sub or sub
    assert N * K < 16 or (seen_zero and seen_sub), (seen_zero, seen_sub)


@pytest.mark.parametrize("d", [48, 80, 96, 112, 128])
def test_attention_at_every_other_accepted_head_dim(expf, d):
    """cva_supported takes d = 16 .. 128 in steps of 16, one kernel instance each: the five the sweep above does not reach,
    at a camera border inside a wave's walk (3 cameras of 17 keys), a second query block of one row, a random mask."""
    from paddle3d_amd.ops import cape as ops

    assert ops.cva_supported(d) and not ops.cva_supported(d + 8)
    for heads, B, kind in ((1, 2, "random"), (2, 1, "none")):
        run_point(expf, 3, 17, 17, d, heads, B, kind)


def test_infinities_in_v_follow_the_reference(expf):
    """An Inf in v under a masked key, and under an unmasked key whose weight underflowed to 0, makes its channel NaN:
    the kernel keeps fmaf(+0, v, .) for both, as the reference multiplies the zero weight by v."""
    rng = np.random.default_rng(3)
    B, N, Q, K, M, d = 2, 2, 17, 33, 2, 16
    f = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    q_a, q_g, k_a, k_g, v = f(B, Q, M * d), f(B, N, Q, M * d), f(B, N, K, M * d), f(B, N, K, M * d), f(B, N, K, M * d)
    sa, sg = np.array([0.25, -0.3], F32), np.array([0.0, 0.2], F32)
    mask = np.zeros((B, N, K), bool)
    mask[1, 1] = True        # a wholly masked camera ...
    v[1, 1, 20, 19] = np.inf  # ... with an Inf: head 1, channel 3 of frame 1
    mask[0, 1, 4] = True
    v[0, 1, 4, 3] = -np.inf
    q_a[0, :, :d] = np.abs(q_a[0, :, :d]) * 30
    k_a[0, 0, 2, :d] = -40.0  # unmasked, weight exactly 0 in head 0 of frame 0
    v[0, 0, 2, 5] = np.inf
    want = cn.cva(q_a, q_g, k_a, k_g, v, sa, sg, M, expf, mask)
    nan = np.isnan(want)
    assert nan[0][:, [3, 5]].all() and nan[1][:, 19].all() and int(nan.sum()) == 3 * Q
    same_bits(run_cva(q_a, q_g, k_a, k_g, v, sa, sg, M, mask), want, nan_ok=True)


def test_attention_alone_elsewhere_side_stream_and_query_tiling(golden):
    rows = cpu.ca_rows(golden, "b")
    heads = mk.CASES["b"]["heads"]
    q_a, q_g, k_a, k_g, v, sa, sg, mask = (_t(a) for a in rows)
    from paddle3d_amd.ops import cape as ops

    run = lambda q_a, q_g, k_a, k_g, v, m: ops.cross_view_attention(q_a, q_g, k_a, k_g, v, sa, sg, heads, m)  # noqa: E731
    args = (q_a, q_g, k_a, k_g, v, mask)
    out = run(*args)
    for b in range(q_a.shape[0]):  # alone
        assert torch.equal(run(*(t[b:b + 1] for t in args))[0], out[b])
    assert torch.equal(run(*(t.flip(0) for t in args)).flip(0), out)  # the two frames swapped
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        out2 = run(*args)
    side.synchronize()
    assert torch.equal(out2, out)
    assert q_a.shape[1] == 37  # Q = 16 and Q = 37: the same first rows
    assert torch.equal(run(q_a[:, :16].contiguous(), q_g[:, :, :16].contiguous(), k_a, k_g, v, mask), out[:, :16])


def test_attention_refusals_and_errors():
    from paddle3d_amd.ops import cape as ops

    def rows(B, N, Q, K, E):
        x = lambda *s: torch.randn(*s, device=DEV)  # noqa: E731
        return x(B, Q, E), x(B, N, Q, E), x(B, N, K, E), x(B, N, K, E), x(B, N, K, E)

    s = torch.full((2,), 0.2, device=DEV)
    assert ops.cross_view_attention(*rows(1, 2, 5, 7, 48), s, s, 2) is None and not ops.cva_supported(24)   # d = 24
    assert ops.cross_view_attention(*rows(1, 2, 5, 7, 288), s, s, 2) is None                                # d = 144
    r = rows(2, 2, 5, 7, 32)
    assert ops.cross_view_attention(r[0][:, :0], r[1][:, :, :0], *r[2:], s, s, 2).shape == (2, 0, 32)
    x = torch.randn(2, 5, 36, device=DEV)[:, :, 1:33]  # a view at an address that is no multiple of 16: made contiguous
    assert ops.cross_view_attention(x, *r[1:], s, s, 2) is not None
    with pytest.raises(RuntimeError, match="mask must be"):
        ops.cross_view_attention(*r, s, s, 2, torch.zeros(2, 2, 8, dtype=torch.bool, device=DEV))
    with pytest.raises(RuntimeError, match="mask must be torch.bool"):
        ops.cross_view_attention(*r, s, s, 2, torch.zeros(2, 2, 7, device=DEV))
    with pytest.raises(RuntimeError, match="scale_a must be"):
        ops.cross_view_attention(*r, s[:1], s, 2)
    with pytest.raises(RuntimeError, match="k_g must be"):
        ops.cross_view_attention(r[0], r[1], r[2], r[3][:, :, :6], r[4], s, s, 2)
    with pytest.raises(RuntimeError, match="multiple of num_heads"):
        ops.cross_view_attention(*r, s, s, 3)
    with pytest.raises(RuntimeError, match="Unsupported device"):
        ops.cross_view_attention(r[0].cpu(), *r[1:], s, s, 2)


# ---- pd3_cape_posemb3d against the restatement ------------------------------------------------------------------------


@pytest.mark.parametrize("tag", TAGS)
def test_posemb3d_on_the_golden_cases(golden, sincos, tag):
    from paddle3d_amd.ops import cape as ops

    i = mk.inputs(tag)
    got = ops.posemb3d(_t(i["ref_points"]), mk.POS_FEATS)
    same_bits(got, cn.posemb3d(i["ref_points"], ops.dim_t(mk.POS_FEATS), *sincos))
    check_result(golden, tag, "posemb", _n(got))
    got = ops.posemb3d(_t(i["ref_points"]), 8, bound=mk.BOUND, rot=_t(i["R"]), trans=_t(i["t"]))
    same_bits(got, cn.posemb3d(i["ref_points"], ops.dim_t(8), *sincos, bound=mk.BOUND, rot=i["R"], trans=i["t"]))
    check_result(golden, tag, "posemb_world", _n(got))


# (B, N (0: no views), Q, F, bound, what is planted): Q = 300 is past a workgroup's 256 elements for every F
POS_SWEEP = [(1, 0, 1, 8, False, None), (2, 0, 300, 96, True, None), (2, 3, 37, 8, True, None), (1, 2, 300, 96, False, "odd"),
             (3, 1, 5, 128, True, "odd"), (1, 0, 7, 2, True, "odd")]


@pytest.mark.parametrize("i", range(len(POS_SWEEP)))
def test_posemb3d_sweep(sincos, i):
    from paddle3d_amd.ops import cape as ops

    B, N, Q, F, with_bound, plant = POS_SWEEP[i]
    rng = np.random.default_rng(700 + i)
    pts = rng.random((B, Q, 3)).astype(F32)
    if not with_bound:
        pts = (pts * 100 - 50).astype(F32)
    if plant == "odd":  # NaN, Inf and 1e30 points (sinf / cosf reduce a huge argument exactly)
        pts[0, 0, 0], pts[B - 1, Q // 2, 1], pts[0, Q - 1, 2] = np.nan, np.inf, 1e30
        pts[B - 1, Q // 3, 0] = -1e30
    R = t = None
    if N:
        R, t = rng.standard_normal((B, N, 3, 3)).astype(F32), rng.uniform(-2, 2, (B, N, 3)).astype(F32)
    bound = mk.BOUND if with_bound else None
    got = ops.posemb3d(_t(pts), F, bound=bound, rot=_t(R), trans=_t(t))
    want = cn.posemb3d(pts, ops.dim_t(F), *sincos, bound=bound, rot=R, trans=t)
    assert got.shape == ((B, N, Q, 3 * F) if N else (B, Q, 3 * F))
    same_bits(got, want, nan_ok=True)
    if plant == "odd":
        assert np.isnan(want).any() and not np.isnan(want).all()
        assert np.isfinite(want[~np.isnan(want)]).all() and np.abs(want[~np.isnan(want)]).max() <= 1
    else:
        assert np.isfinite(want).all()


def test_posemb3d_refusals_and_errors():
    from paddle3d_amd.ops import cape as ops

    p = torch.rand(2, 5, 3, device=DEV)
    assert ops.posemb3d(p, 7) is None and ops.posemb3d(p, 130) is None
    assert ops.posemb3d(p[:, :0], 8).shape == (2, 0, 24)
    R, t = torch.randn(2, 3, 3, 3, device=DEV), torch.randn(2, 3, 3, device=DEV)
    assert ops.posemb3d(p, 8, rot=R, trans=t).shape == (2, 3, 5, 24)
    with pytest.raises(RuntimeError, match="come together"):
        ops.posemb3d(p, 8, rot=R)
    with pytest.raises(RuntimeError, match="trans must be"):
        ops.posemb3d(p, 8, rot=R, trans=t[:, :2])
    with pytest.raises(RuntimeError, match="points must be"):
        ops.posemb3d(p[..., :2], 8)
    with pytest.raises(ValueError, match="expected 6 floats"):
        ops.posemb3d(p, 8, bound=[0.0, 1.0])


# ---- the modules against the reference --------------------------------------------------------------------------------

_outputs = {}


def outputs(golden, tag, fused):
    if (tag, fused) not in _outputs:
        _outputs[tag, fused] = cpu.module_outputs(golden, tag, fused, DEV)
    return _outputs[tag, fused]


@pytest.mark.parametrize("fused", ["force", True, False], ids=["forced", "default", "unfused"])
@pytest.mark.parametrize("tag", TAGS)
def test_modules_against_the_reference(golden, tag, fused):
    out = outputs(golden, tag, fused)
    assert set(out) == set(mk.results(tag))
    for name, got in out.items():
        check_result(golden, tag, name, got)


@pytest.mark.parametrize("fused", ["force", True, False], ids=["forced", "default", "unfused"])
@pytest.mark.parametrize("tag", TAGS)
def test_transformer_against_the_reference(golden, tag, fused):
    """position_embeding through pd3_petr_coords3d (coords_mask equal to the reference's, the coordinates within their
    bound), the 2-layer transformer without and with time, MLP_Fusion with Ego_emb."""
    cpu.check_transformer(golden, tag, cpu.transformer_outputs(golden, tag, fused, DEV))


@pytest.mark.parametrize("fused", ["force", True, False], ids=["forced", "default", "unfused"])
@pytest.mark.parametrize("tag", sorted(mk.HEAD_CASES))
def test_head_and_decode_against_the_reference(golden, tag, fused):
    """CAPETemporalDNHead's forward (without time; with time, 2 x 6 cameras) and get_bboxes through pd3_nms_free_decode:
    labels, counts and row order equal to the reference's, everything else within the bounds."""
    cpu.check_head(golden, tag, *cpu.head_outputs(golden, tag, fused, DEV))


def test_head_launches_and_host_syncs(golden):
    """A forward with time and its decode: the transformer's launches and one pd3_nms_free_decode in the fused forms, none
    in the unfused one, and the host synchronisations of forward + get_bboxes pinned at ZERO in the three forms (the
    camera matrices are inverted on the device, once per forward)."""
    from paddle3d_amd import _lib

    tag = "b"
    args = cpu.head_args(tag, DEV)
    names = NAMES + ("pd3_petr_coords3d", "pd3_nms_free_decode")
    for fused, want in (("force", [2, 2, 2, 1, 1]), (True, [0, 2, 0, 1, 1]), (False, [0, 0, 0, 0, 0])):
        head = cpu.build_head(golden, tag, fused).to(DEV)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with torch.no_grad(), launch_ledger(_lib.lib(), names) as n:
                det = head.get_bboxes(head(*args))
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert [n[k] for k in names] == want, (fused, dict(n))
        from test_bevformer_decoder_cpu import check_decode

        check_decode(golden, tag, "head", *(_n(t) for t in det))


def test_transformer_launches_and_host_syncs(golden):
    """A forced 2-layer forward with time: one coordinate launch, two embedding launches (query_embedding's and
    bev_embed's), each attention kernel once per layer; and NO host synchronisation in any form -- the count is pinned at
    zero under torch's sync guard in its "error" mode."""
    from paddle3d_amd import _lib, cape

    tag = "b"
    ti = {k: torch.from_numpy(v).to(DEV) for k, v in mk.tr_inputs(tag).items()}
    ego = cape.curlidar2prevlidar(ti["ext_cur"].T, ti["ext_prev"].T)
    args = (ti["feature"], ti["mask"], ti["I_inv"], ti["R_inv"], ti["t"], mk.TR["image"])
    names = NAMES + ("pd3_petr_coords3d",)
    for fused, want in (("force", [2, 2, 2, 1]), (True, [2, 2, 0, 1]), (False, [0, 0, 0, 0])):
        tr = cpu.build_transformer(golden, tag, fused).to(DEV)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with torch.no_grad(), launch_ledger(_lib.lib(), names) as n:
                out = tr(*args, ego_matrix=ego)[0]
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert [n[k] for k in names] == want, (fused, dict(n))
        check_result(golden, tag, "tr_time", _n(out))


NAMES = ("pd3_cape_cva_forward", "pd3_cape_posemb3d", "pd3_mha_forward")


def layer_args(tag):
    i = cpu.tensors(tag, DEV)
    return (i["x"], i["bev_embed"], i["lidar_obj_pe"], i["feature"], i["camera_pe"], i["mask"], i["img_embed"],
            i["bev_embed"], None)


def test_launch_counts_and_the_default_border(golden, monkeypatch):
    """A layer launches each attention kernel once; fused=True takes the cross-view kernel up to CVA_FUSED_MAX_KEYS keys
    (N * K) and sl_layer's up to SL_FUSED_MAX_KEYS, and torch above; "force" takes both whatever the number of keys;
    fused=False takes no kernel.  The borders are the measured ones."""
    from paddle3d_amd import _lib, cape

    assert (cape.CVA_FUSED_MAX_KEYS, cape.SL_FUSED_MAX_KEYS) == (192, 0)
    tag = "a"
    keys, Q = mk.CASES[tag]["N"] * mk.K, mk.CASES[tag]["Q"]
    args = layer_args(tag)
    for cva_border, sl_border, fused, want in ((keys, Q, True, [1, 0, 1]), (keys - 1, Q, True, [0, 0, 1]),
                                               (keys, Q - 1, True, [1, 0, 0]), (keys - 1, Q - 1, "force", [1, 0, 1]),
                                               (keys, Q, False, [0, 0, 0])):
        monkeypatch.setattr(cape, "CVA_FUSED_MAX_KEYS", cva_border)
        monkeypatch.setattr(cape, "SL_FUSED_MAX_KEYS", sl_border)
        layer = cpu.build(golden, tag, "cva", fused).to(DEV)
        with torch.no_grad(), launch_ledger(_lib.lib(), NAMES) as n:
            out = layer(*args)
        assert torch.isfinite(out).all()
        assert [n[k] for k in NAMES] == want, (cva_border, sl_border, fused, dict(n))
    with torch.no_grad(), launch_ledger(_lib.lib(), NAMES) as n:
        i = cpu.tensors(tag, DEV)
        cape.pos2posemb3d(i["ref_points"], mk.POS_FEATS)
        cape.world_posemb3d(i["ref_points"], mk.BOUND, i["R"], i["t"], 8)
        cape.pos2posemb3d(i["ref_points"], mk.POS_FEATS, fused=False)
    assert [n[k] for k in NAMES] == [0, 2, 0], dict(n)


def test_refused_shapes_fall_back():
    """dim_head = 24: the op returns None, the forced module takes the torch route and gives the unfused module's bits."""
    from paddle3d_amd import _lib, cape

    B, N, Q, K, dim = 2, 2, 9, 11, 48
    x = lambda *s: torch.randn(*s, device=DEV)  # noqa: E731
    torch.manual_seed(5)
    args = (x(B, N, K, dim), x(B, N, Q, dim), x(B, N, K, dim), x(B, Q, dim), x(B, N, K, dim), torch.rand(B, N, K, device=DEV) < 0.3)
    outs = []
    for fused in ("force", False):
        torch.manual_seed(6)
        ca = cape.CrossAttention(dim, 2, 24, True, fused=fused).eval().to(DEV)
        with torch.no_grad(), launch_ledger(_lib.lib(), NAMES) as n:
            outs.append(ca(*args))
        assert [n[k] for k in NAMES] == [0, 0, 0]
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all() and outs[0].abs().max() > 0
    with pytest.raises(RuntimeError, match="stack expects"):  # an odd F: refused by the op, and the reference's stack fails
        cape.pos2posemb3d(x(3, 3), 7)
    p = torch.rand(2, 5, 3, device=DEV)
    assert torch.equal(cape.pos2posemb3d(p, 130), cape.pos2posemb3d(p, 130, fused=False))  # F = 130: the torch route


@pytest.mark.parametrize("fused", ["force", True, False], ids=["forced", "default", "unfused"])
def test_layer_makes_no_host_sync(golden, fused):
    from paddle3d_amd import cape

    tag = "a"
    layer = cpu.build(golden, tag, "cva", fused).to(DEV)
    args = layer_args(tag)
    i = cpu.tensors(tag, DEV)
    want = outputs(golden, tag, fused)
    qcr = _t(want["qcr"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            out = layer(*args[:1], qcr, *args[2:])
            pe = cape.world_posemb3d(i["ref_points"], mk.BOUND, i["R"], i["t"], 8, fused=fused)
            pe0 = cape.pos2posemb3d(i["ref_points"], mk.POS_FEATS, fused=fused)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for name, got in (("cva", out), ("posemb_world", pe), ("posemb", pe0)):
        check_result(golden, tag, name, _n(got))
