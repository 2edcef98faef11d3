"""BEV-LaneDet's lane head tail and lane post-processing on the device: both entry points (the lazy head and the
from-maps form) bit-equal to the NumPy restatement (tests/golden/lanedet_numpy.py) on the golden cases, on seeded shapes
-- 1 x 1, widths that are no multiple of 4, several workgroups of the pixel kernels, the full 200 x 48, nd 1, 2 and 4, B
up to 3 -- and on border cases built from integer-valued embeddings (lanedet_numpy.border_cases): a frame without a
selected pixel, one selected pixel, all of them, 127 / 128 / 129 centres, 32 / 33 canvas ids, clusters of
min_cluster_size - 1 and min_cluster_size pixels, an exact distance tie, a distance equal to the gap, lanes of 1 to 4
rows, NaN and Inf in seg and emb, a selected pixel in every map corner; the lazy form from dense maps and from one
stacked, pitched map; the module in its three forms against the reference's golden file under the tolerance rule; no
host synchronisation in lanes_padded, exactly one in forward; refusals; and the module's host-side branches on a stub
network that serves border-case maps: the np.polyfit finish of lanes of 2 and 3 rows, the redo of flagged frames by
the transcription, the transcription for a shape the kernels refuse."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from guarded import launch_ledger  # noqa: E402

import lanedet_numpy as ln  # noqa: E402
import test_lanedet_cpu as cpu  # noqa: E402
from test_lanedet_cpu import golden  # noqa: E402,F401  (fixture)

from paddle3d_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
FIELDS = ("labels", "num_lanes", "lane_id", "lane_rows", "fit_ok", "points", "fit", "flags", "num_selected")
WATCHED = _lib.symbols("test_memory_safety_lanedet_gpu") + _lib.symbols("test_memory_safety_gpu")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.detach().cpu().numpy()


def same_bits(got, want, what=""):
    """Bit equality; a NaN must stand exactly where the restatement has one (its payload is free)."""
    got = _n(got) if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == "f":
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaNs stand elsewhere"
        bad = (got.view(np.uint32) != want.view(np.uint32)) & ~np.isnan(want)
    else:
        bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}"


def same_pack(got, want, what=""):
    assert got is not None, f"{what}: the op refused the shape"
    for k in FIELDS:
        same_bits(getattr(got, k), want[k], f"{what} {k}")


def _cfg(cfg):
    return dict(conf=cfg["conf"], emb_margin=cfg["emb_margin"], min_cluster_size=cfg["min_cluster_size"],
                max_x=cfg["max_x"], meter_per_pixel=tuple(cfg["meter_per_pixel"]))


def from_maps(seg, emb, off, z, cfg, logit=False):
    from paddle3d_amd.ops import lanedet as A

    return A.lanedet_post_process(_t(seg), _t(emb), _t(off), _t(z), offset_is_logit=logit, **_cfg(cfg))


def lazy(feats, state, cfg, stacked=False):
    """ops.lanedet.lanedet_head_forward on numpy inputs; stacked: the four branches as views of one
    [B, 4C, H, pitch4(W)] map."""
    from paddle3d_amd.ops import lanedet as A
    from paddle3d_amd.ops.conv import pitch4

    B, C, H, W = feats[0].shape
    if stacked:
        buf = torch.zeros((B, 4 * C, H, pitch4(W)), dtype=torch.float32, device=DEV)
        views = []
        for i, f in enumerate(feats):
            buf[:, i * C:(i + 1) * C, :, :W] = _t(f)
            views.append(buf[:, i * C:(i + 1) * C, :, :W])
    else:
        views = [_t(f) for f in feats]
    wb = [_t(state[f"{k}.{p}"]) for k in ln.BRANCHES for p in ("weight", "bias")]
    return A.lanedet_head_forward(*views, *wb, **_cfg(cfg))


@pytest.fixture(scope="module")
def borders():
    return {name: (case, ln.post_process(case[0], case[1], ln.sigmoid(case[2]), case[3], case[4]))
            for name, case in ln.border_cases().items()}


def test_border_cases_from_maps(borders):
    seen = set()
    for name, ((seg, emb, off, z, cfg), want) in borders.items():
        same_pack(from_maps(seg, emb, off, z, cfg, logit=True), want, name + " logit")
        same_pack(from_maps(seg, emb, ln.sigmoid(off), z, cfg), want, name)
        seen.update(int(f) for f in want["flags"])
    assert seen == {0, 1, 2}
    # what the cases are there for, stated on the restatement's results
    w = {k: v[1] for k, v in borders.items()}
    assert w["empty_frame"]["num_selected"].tolist() == [18, 0] and w["empty_frame"]["num_lanes"].tolist() == [2, 0]
    assert w["one_pixel"]["labels"].sum() == 1 and w["one_pixel"]["num_lanes"][0] == 0
    assert w["all_selected"]["num_selected"][0] == 30
    assert [int(w[f"centres_{k}"]["flags"][0]) for k in (127, 128, 129)] == [0, 0, 1]
    assert w["centres_129"]["num_lanes"].tolist() == [0, 1] and not w["centres_129"]["labels"][0].any()
    assert w["lanes_32"]["num_lanes"][0] == 32 and w["lanes_33"]["flags"][0] == 2
    assert w["min_cluster_size"]["lane_id"][0, :2].tolist() == [2, 0]
    for nd in (1, 2):
        assert w[f"tie_nd{nd}"]["labels"][0, 0].tolist() == [1, 2, 1]       # the lower id wins the tie
        assert w[f"gap_nd{nd}"]["labels"][0, :2, :2].tolist() == [[1, 2], [1, 2]]  # distance == gap founds a centre
    assert w["rows_1_to_4"]["lane_rows"][0, :4].tolist() == [2, 3, 4, 0]
    assert w["rows_1_to_4"]["fit_ok"][0, :4].tolist() == [0, 0, 1, 0]


def test_border_cases_lazy(borders):
    """The same cases through the lazy form: branch maps and weights whose convolutions reproduce the maps exactly
    (finite maps), from dense maps and from one stacked, pitched map.  The NaN / Inf case takes the restatement of
    the convolution as its reference, since 0 x Inf spreads there."""
    for name, ((seg, emb, off, z, cfg), want) in borders.items():
        feats, state = ln.identity_head(seg, emb, off, z)
        if name == "nan_inf":
            want = ln.head_forward(feats, state, cfg)
        same_pack(lazy(feats, state, cfg), want, name + " lazy")
        same_pack(lazy(feats, state, cfg, stacked=True), want, name + " lazy stacked")


@pytest.mark.parametrize("H,W,B", ln.SWEEP)
def test_seeded_shapes(H, W, B):
    """Synthetic lanes from maps, and a seeded head through the lazy form, at nd 1, 2 and 4; the full size runs the
    head's 64 channels at nd 2 and 16 channels at nd 1 and 4 (the restatement's convolution is the slow part)."""
    for nd in (1, 2, 4):
        rng = np.random.default_rng(1000 * H + 10 * W + nd)
        cfg = ln.sweep_cfg(H, W)
        seg, emb, off, z = ln.synthetic_lanes(rng, B, H, W, nd, lanes=min(5, max(1, W // 4)))
        want = ln.post_process(seg, emb, off, z, cfg)
        same_pack(from_maps(seg, emb, off, z, cfg), want, f"{H}x{W} nd{nd} maps")
        if H * W >= 2000:
            assert want["num_lanes"].min() >= 4 and want["fit_ok"].sum() >= 8 and not want["flags"].any()
        C = 64 if H * W >= 2000 and nd == 2 else 16  # the head's width once; 16 elsewhere (the NumPy convolution's cost)
        feats, state, conf = ln.random_head(rng, B, C, H, W, nd)
        for c in (conf, -1e30):  # about a third of the pixels; all of them (every border pixel's padding)
            if c < 0 and H * W >= 2000:
                continue
            cfg2 = dict(cfg, conf=c)
            want = ln.head_forward(feats, state, cfg2)
            same_pack(lazy(feats, state, cfg2), want, f"{H}x{W} nd{nd} lazy conf {c}")
            same_pack(lazy(feats, state, cfg2, stacked=True), want, f"{H}x{W} nd{nd} lazy stacked conf {c}")
            same_pack(from_maps(*ln.head_maps(feats, state), cfg2), want, f"{H}x{W} nd{nd} head maps conf {c}")


def _golden_maps(golden):
    """(tag, seg, emb, offset, z, cfg) of every golden case: the post-processing cases' maps and the head cases' fp32
    maps from the reference."""
    for tag in cpu.POST_TAGS:
        yield (tag, *cpu.post_inputs(golden, tag))
    for tag in cpu.HEAD_TAGS:
        m = golden[f"{tag}_maps32"]
        yield tag, m[:, :1], m[:, 1:3], m[:, 3:4], m[:, 4:5], cpu.mk.HEAD_POST


def test_golden_cases_bit_equal(golden):
    """Both entry points on every golden case.  The from-maps form takes the maps as they are.  The lazy form takes
    branch maps whose final convolutions reproduce seg, emb and z exactly and the offset's logit (its sigmoid is within
    a rounding or two of the golden offset, so the restatement of the lazy form is the reference there): dense maps and
    one stacked, pitched map; labels, ids and counts equal those of the from-maps form."""
    for tag, seg, emb, off, z, cfg in _golden_maps(golden):
        want = ln.post_process(seg, emb, off, z, cfg)
        same_pack(from_maps(seg, emb, off, z, cfg), want, tag)
        logit = np.log(off.astype(np.float64) / (1 - off.astype(np.float64))).astype(F32)
        feats, state = ln.identity_head(seg, emb, logit, z)
        lazy_want = ln.head_forward(feats, state, cfg)
        for k in ("labels", "num_lanes", "lane_id", "lane_rows", "fit_ok", "flags", "num_selected"):
            assert np.array_equal(lazy_want[k], want[k]), (tag, k)
        same_pack(lazy(feats, state, cfg), lazy_want, tag + " lazy")
        same_pack(lazy(feats, state, cfg, stacked=True), lazy_want, tag + " lazy stacked")
        same_pack(from_maps(seg, emb, logit, z, cfg, logit=True), lazy_want, tag + " from maps, offset logit")


def test_refusals():
    from paddle3d_amd.ops import lanedet as A

    z = torch.zeros((1, 1, 4, 4), device=DEV)
    assert A.lanedet_post_process(z, torch.zeros((1, 5, 4, 4), device=DEV), z, z) is None        # nd 5
    assert A.lanedet_post_process(torch.zeros((1, 1, 1025, 1), device=DEV), torch.zeros((1, 2, 1025, 1), device=DEV),
                                  torch.zeros((1, 1, 1025, 1), device=DEV), torch.zeros((1, 1, 1025, 1), device=DEV)) is None
    with pytest.raises(RuntimeError, match="offset must be"):
        A.lanedet_post_process(z, torch.zeros((1, 2, 4, 4), device=DEV), torch.zeros((1, 1, 4, 5), device=DEV), z)
    with pytest.raises(_lib.Paddle3DAmdError, match="invalid argument"):
        A.lanedet_post_process(z, torch.zeros((1, 2, 4, 4), device=DEV), z, z, meter_per_pixel=0.0)


# ---- the module ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", ["lazy", "dense", False])
def test_module_forms_meet_the_tolerance_rule(golden, fused):
    for tag in cpu.HEAD_TAGS:
        cpu.check_head_case(golden, tag, DEV, fused)


def _sync_calls(fn):
    """The host synchronisations torch sees while fn runs (the way tests/test_smoke_gpu.py counts them): device-to-host
    copies and explicit synchronisations raise under set_sync_debug_mode("error"); here they are counted."""
    import warnings

    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return out, [x for x in w if "synchroniz" in str(x.message).lower()]


def test_lanes_padded_makes_no_host_synchronisation_and_forward_one(golden):
    tag = cpu.HEAD_TAGS[0]
    m = cpu.build_model(golden, tag).to(DEV)
    x = _t(cpu.head_input(golden, tag))
    for fused in ("lazy", "dense"):
        with torch.no_grad():
            m.lanes_padded(x, fused=fused)  # warm: weights derived, kernels loaded
            with launch_ledger(_lib.lib(), WATCHED) as calls:
                out, syncs = _sync_calls(lambda: m.lanes_padded(x, fused=fused))
        assert out is not None and not syncs, [str(s.message) for s in syncs]
        assert calls["pd3_lanedet_head_forward" if fused == "lazy" else "pd3_lanedet_post_process"] == 1
    with torch.no_grad():
        lanes, syncs = _sync_calls(lambda: m.forward(dict(img=x)))
    assert len(syncs) == 1, [str(s.message) for s in syncs]
    assert len(lanes) == x.shape[0]


# ---- the module's host-side branches ---------------------------------------------------------------------------------
def stub_model(case, nd_head=None):
    """A BEVLaneDet whose network is replaced by fixed maps: `images` are frame numbers [B], the head's branch maps
    are those of lanedet_numpy.identity_head (64 channels) for those frames and its final convolutions the matching
    weights, so that every path of the module sees the border case's maps.  nd_head: a head of another embedding
    width (zero-padded emb), for the shapes the kernels refuse."""
    from paddle3d_amd import bev_lanedet as M

    seg, emb, logit, z, cfg = case
    B, nd, H, W = emb.shape
    if nd_head is not None:
        emb = np.concatenate([emb, np.zeros((B, nd_head - nd, H, W), F32)], 1)
        nd = nd_head
    feats, state = ln.identity_head(seg, emb, logit, z, C=64)

    class Head(M.InstanceEmbeddingOffsetYZ):
        def branch_maps(self, x, winograd=False):
            return [f[x.long()] for f in self.fixed]

        def forward(self, x):
            return tuple(b[6](m) for b, m in zip(self.branches(), self.branch_maps(x)))

    m = M.BEVLaneDet(None, bev_shape=(H, W), train=False, s32=(8, 2, 2), s64=(8, 1, 1), bev=(8, 2, 2),
                     x_range=(3, cfg["max_x"]), meter_per_pixel=cfg["meter_per_pixel"][0], post_conf=cfg["conf"],
                     post_emb_margin=cfg["emb_margin"], post_min_cluster_size=cfg["min_cluster_size"])
    head = Head(64, nd)
    with torch.no_grad():
        for k in ln.BRANCHES:
            getattr(head, k)[6].weight.copy_(torch.from_numpy(state[k + ".weight"]))
            getattr(head, k)[6].bias.copy_(torch.from_numpy(state[k + ".bias"]))
    m.lane_head.head = head
    m = m.eval().to(DEV)
    head.fixed = [_t(f) for f in feats]
    m.bev_feat = lambda images, fused=False: images
    return m, torch.arange(B, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("fused", ["lazy", "dense", False])
def test_forward_finishes_short_lanes_with_polyfit(borders, fused):
    """Lanes of 2 and 3 rows come back with fit_ok == 0 and are finished on the host from the device's points; the lane
    of 4 rows is the device's fit.  All three equal what the restatement's outputs give under the same finish."""
    case, want = borders["rows_1_to_4"]
    m, frames = stub_model(case)
    with torch.no_grad():
        pack = m.lanes_padded(frames, fused=fused)
        lanes = m.forward(dict(img=frames), fused=fused)
    assert _n(pack.fit_ok)[0, :3].tolist() == [0, 0, 1] and _n(pack.lane_rows)[0, :3].tolist() == [2, 3, 4]
    ref = ln.lanes_of(want, 0)
    assert len(lanes) == 1 and len(lanes[0]) == len(ref) == 3
    for got, exp in zip(lanes[0], ref):
        assert got.shape == (40, 3) and np.allclose(got, exp, rtol=0, atol=1e-4)
    if fused == "lazy":  # no torch layer on this path: the same points, the same host arithmetic
        for got, exp in zip(lanes[0], ref):
            assert np.array_equal(got, exp)


def test_forward_redoes_flagged_frames_by_the_transcription(borders):
    from paddle3d_amd import bev_lanedet as M

    for name, flag in (("centres_129", 1), ("lanes_33", 2)):
        case, want = borders[name]
        m, frames = stub_model(case)
        with torch.no_grad():
            for fused in ("lazy", "dense", False):
                pack = m.lanes_padded(frames, fused=fused)
                assert int(pack.flags[0]) == flag and int(pack.num_lanes[0]) == 0 and not bool(pack.labels[0].any()), fused
                lanes = m.forward(dict(img=frames), fused=fused)
                maps = np.concatenate([case[0], case[1], ln.sigmoid(case[2]), case[3]], 1)
                ref = [f for _, _, f in M.lanes_numpy(maps[0], **m.post)[1]]
                assert len(lanes[0]) == len(ref) > 0 and all(np.allclose(a, b, rtol=0, atol=1e-4) for a, b in zip(lanes[0], ref)), (name, fused)
                if len(frames) > 1:  # the frame beside it comes from the device as usual
                    assert len(lanes[1]) == int(want["num_lanes"][1])


def test_refused_shapes_take_the_transcription(borders):
    """A head with five embedding channels is outside the kernels' predicate: lanes_padded answers from the
    transcription, with the same canvas and lanes, and calls no entry point."""
    case, want = borders["all_selected"]
    m, frames = stub_model(case, nd_head=5)
    with torch.no_grad(), launch_ledger(_lib.lib(), WATCHED) as calls:
        packs = {fused: m.lanes_padded(frames, fused=fused) for fused in ("lazy", "dense", True)}
    assert not any(calls.values()), {k: v for k, v in calls.items() if v}
    for fused, pack in packs.items():
        assert np.array_equal(_n(pack.labels), want["labels"]) and np.array_equal(_n(pack.lane_id), want["lane_id"])
        assert np.array_equal(_n(pack.lane_rows), want["lane_rows"]) and np.array_equal(_n(pack.fit_ok), want["fit_ok"])
        assert np.allclose(_n(pack.points), want["points"], atol=1e-6) and np.allclose(_n(pack.fit), want["fit"], atol=1e-4)

