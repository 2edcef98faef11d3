"""DD3D's FCOS heads and post-processing on the device: both entry points (the lazy form and the from-maps form) bit-equal
to the NumPy restatement (tests/golden/dd3d_numpy.py) on the golden cases and on seeded sweeps -- selected pixels on all
four corners and edges, a 1 x 1 level, rows of padded pitch in one stacked map, count = pre_nms_topk exactly and one
more, all scores equal (the tie order), identical boxes of one class and of two classes, NaN and Inf in the logits and
in the 3D maps, a tie at the post_nms_topk cut (counts > R) -- the lazy form bit-equal to the from-maps form fed the
restatement's dense maps; a frame alone and elsewhere in the batch; refusals; no host synchronisation; the module in
its three forms against the reference's golden file within its stored bounds."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from guarded import launch_ledger  # noqa: E402

import dd3d_numpy as dn  # noqa: E402
import test_dd3d_cpu as cpu  # noqa: E402
from test_dd3d_cpu import golden  # noqa: E402,F401  (fixture)

from paddle3d_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
MODULE = "test_memory_safety_dd3d_gpu"


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
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}: "
                           f"{got[tuple(np.argwhere(bad)[0])]!r} for {want[tuple(np.argwhere(bad)[0])]!r}")


def same_results(got, want, what=""):
    assert got is not None, f"{what}: the op refused the shape"
    same_bits(got[1], want[1], what + " counts")
    same_bits(got[0], want[0], what + " rows")


def sweep_camera(B):
    Ks = np.zeros((B, 3, 3), F32)
    for b in range(B):
        f = 70.0 + 3.0 * b
        Ks[b] = [[f, 0, 41.0 - b], [0, f, 23.0 + 0.5 * b], [0, 0, 1]]
    return Ks


def sweep_packed(rng, C, nc, L, strides, ncp=None, wl=1, has3d=True):
    ncp = nc if ncp is None else ncp
    scales = np.ones((L, 6), F32)
    scales[:, 0] = np.asarray(strides, F32) * F32(0.75)
    p = dict(w2d=(rng.standard_normal((4, C, 3, 3)) / np.sqrt(9 * C)).astype(F32),
             b2d=(rng.standard_normal(4) * 0.1 + 1.0).astype(F32), scales=scales)
    if has3d:
        scales[:, 1] = np.asarray(strides, F32)
        scales[:, 2:4] = rng.uniform(0.8, 1.2, (L, 2))
        scales[:, 4] = rng.uniform(2.0, 5.0, L)
        scales[:, 5] = rng.uniform(5.0, 30.0, L)
        p["w3d"] = (rng.standard_normal((wl, 11 * ncp, C, 3, 3)) * 2.0 / np.sqrt(9 * C)).astype(F32)
        p["b3d"] = (rng.standard_normal((wl, 11 * ncp)) * 0.1).astype(F32)
    return p


def sweep_levels(rng, B, C, nc, shapes, has3d=True, bias=0.0):
    out = []
    for h, w in shapes:
        lv = dict(logits=(rng.standard_normal((B, nc, h, w)) * 1.5 + bias).astype(F32),
                  centerness=(rng.standard_normal((B, 1, h, w)) + 1.0).astype(F32),
                  f2d=rng.standard_normal((B, C, h, w)).astype(F32))
        if has3d:
            lv["f3d"] = rng.standard_normal((B, C, h, w)).astype(F32)
        out.append(lv)
    return out


def lazy(levels, strides, packed, K, canon, cfg, stacked=False):
    """ops.dd3d.dd3d_head_forward on numpy inputs; stacked: both towers' outputs as views of one [B, 2C, H, pitch4(W)]
    map per level."""
    from paddle3d_amd.ops import dd3d as A
    from paddle3d_amd.ops.conv import pitch4

    has3d = "f3d" in levels[0]
    f2d, f3d = [], []
    for lv in levels:
        B, C, H, W = lv["f2d"].shape
        if stacked and has3d:
            buf = torch.zeros((B, 2 * C, H, pitch4(W) + 4), dtype=torch.float32, device=DEV)
            buf[:, :C, :, :W], buf[:, C:, :, :W] = _t(lv["f2d"]), _t(lv["f3d"])
            f2d.append(buf[:, :C, :, :W]), f3d.append(buf[:, C:, :, :W])
        else:
            f2d.append(_t(lv["f2d"]))
            if has3d:
                f3d.append(_t(lv["f3d"]))
    p = {k: _t(v) for k, v in packed.items()}
    return A.dd3d_head_forward([_t(lv["logits"]) for lv in levels], [_t(lv["centerness"]) for lv in levels], f2d,
                               f3d if has3d else None, strides, p["w2d"], p["b2d"], p.get("w3d"), p.get("b3d"),
                               p["scales"], _t(K) if has3d else None, _t(np.asarray(canon, F32)) if has3d else None, **cfg)


def from_maps(dense, strides, K, canon, cfg):
    from paddle3d_amd.ops import dd3d as A

    has3d = "quat" in dense[0]
    box3d = [[_t(lv[k]) for lv in dense] for k in ("quat", "ctr", "depth", "size", "conf")] if has3d else None
    return A.dd3d_post_process([_t(lv["logits"]) for lv in dense], [_t(lv["centerness"]) for lv in dense],
                               [_t(lv["box2d_reg"]) for lv in dense], box3d, strides, _t(K) if has3d else None,
                               _t(np.asarray(canon, F32)) if has3d else None, **cfg)


def check_both(levels, strides, packed, K, canon, cfg, what, stacked=False, details=None):
    """Both entry points against the restatement: the lazy form from the towers' outputs, the from-maps form from the
    restatement's dense maps (so the two device forms are bit-equal to each other too).  Returns (rows, counts)."""
    want, dense = dn.head_forward(levels, strides, packed, K, canon, cfg, details)
    same_results(lazy(levels, strides, packed, K, canon, cfg, stacked), want, what + " lazy")
    same_results(from_maps(dense, strides, K, canon, cfg), want, what + " from maps")
    return want


CFG = dict(pre_nms_thresh=0.3, pre_nms_topk=20, post_nms_topk=8, nms_thresh=0.6)


# ---- golden cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", dn.TAGS)
def test_entry_points_on_the_golden_cases(tag, golden):  # noqa: F811
    c = dn.CASES[tag]
    levels, packed = cpu.tower_outputs(tag)
    rows, counts = check_both(levels, c["strides"], packed, dn.golden_camera(tag), dn.CANON, cpu.op_cfg(tag), tag,
                              stacked=True)
    cpu.check_against_golden(tag, rows, counts, golden, "device (= restatement)")


@pytest.mark.parametrize("tag", dn.TAGS)
@pytest.mark.parametrize("fused", ("lazy", "dense", False))
def test_module_on_the_golden_cases(tag, fused, golden):  # noqa: F811
    model = cpu.build_model(tag).to(DEV)
    rows, counts = cpu.run_model(model, tag, DEV, fused=fused)
    cpu.check_against_golden(tag, _n(rows), _n(counts), golden, f"module fused={fused}")


# ---- seeded sweeps --------------------------------------------------------------------------------------------------
# (shapes, strides, C, nc, ncp, wl, B, cfg): every pixel of the small maps is a candidate somewhere, so the selected entries
# stand on all four corners and edges; a 1 x 1 level; widths 7 and 5 (stacked maps of padded pitch)
SWEEP = (
    (((1, 1),), (8,), 16, 1, 1, 1, 1, dict(CFG, pre_nms_thresh=0.01)),
    (((3, 4), (1, 1)), (8, 16), 16, 3, 3, 1, 2, dict(CFG, offset="half", pre_nms_thresh=0.05, pre_nms_topk=64)),
    (((5, 7), (3, 4), (2, 2)), (8, 16, 32), 32, 5, 5, 3, 3, dict(CFG, thresh_with_ctr=False)),
    (((6, 10), (3, 5), (2, 3), (1, 2), (1, 1)), (8, 16, 32, 64, 128), 16, 6, 1, 1, 1, dict(CFG, predict_distance=True)),
    (((9, 13), (5, 7)), (4, 8), 64, 16, 16, 2, 2, dict(CFG, pre_nms_topk=1024, post_nms_topk=0, pre_nms_thresh=0.01,
                                                       nms_categories=16)),
    (((17, 31),), (8,), 16, 2, 2, 1, 1, dict(CFG, pre_nms_topk=300, post_nms_topk=100, pre_nms_thresh=0.2,
                                             predict_allocentric_rot=False, scale_depth_by_focal_lengths=False)),
)


@pytest.mark.parametrize("point", SWEEP, ids=lambda p: "-".join("x".join(map(str, s)) for s in p[0]) + f"-c{p[2]}n{p[3]}")
def test_sweep_is_bit_equal_to_the_restatement(point):
    shapes, strides, C, nc, ncp, wl, B, cfg = point
    rng = np.random.default_rng(sum(h * 131 + w for h, w in shapes) * 1009 + C * 7 + nc)
    levels = sweep_levels(rng, B, C, nc, shapes)
    packed = sweep_packed(rng, C, nc, len(shapes), strides, ncp, wl)
    rows, counts = check_both(levels, strides, packed, sweep_camera(B), dn.CANON + dn.CANON, cfg, str(point[:4]),
                              stacked=True)
    assert counts.max() > 0


def test_only_box2d_sweep():
    rng = np.random.default_rng(77)
    shapes, strides = ((5, 7), (2, 3)), (8, 16)
    levels = sweep_levels(rng, 2, 16, 3, shapes, has3d=False)
    packed = sweep_packed(rng, 16, 3, 2, strides, has3d=False)
    rows, counts = check_both(levels, strides, packed, None, None, dict(CFG), "only_box2d")
    assert counts.max() > 0 and not rows[..., 5].any() and not rows[..., 10:].any()


def crafted(B, nc, shapes, logit=-20.0):
    """From-maps levels with no candidate anywhere, boxes of 6 x 6 pixels around every location and plain 3D maps."""
    out = []
    for h, w in shapes:
        z = lambda k, v=0.0: np.full((B, k, h, w), v, F32)  # noqa: E731
        out.append(dict(logits=z(nc, logit), centerness=z(1, 3.0), box2d_reg=z(4, 3.0), quat=z(4 * nc, 0.5),
                        ctr=z(2 * nc), depth=z(nc, 10.0), size=z(3 * nc), conf=z(nc, 1.0)))
    return out


def run_maps(dense, strides, cfg, what, B=1):
    K = sweep_camera(B)
    want = dn.post_process(dense, strides, K, dn.CANON, cfg)
    same_results(from_maps(dense, strides, K, dn.CANON, cfg), want, what)
    return want


def test_count_at_pre_nms_topk_and_one_more():
    """Exactly pre_nms_topk candidates (every one is taken, the n <= K path) and one more (the radix select drops the
    lowest); the locations are far apart, so nothing is suppressed."""
    shapes, strides = ((6, 10),), (8,)
    for extra in (0, 1):
        dense = crafted(1, 2, shapes)
        flat = dense[0]["logits"].reshape(2, -1)
        rng = np.random.default_rng(5 + extra)
        take = rng.permutation(60)[:20 + extra]
        flat[take % 2, take] = np.linspace(1.0, 3.0, len(take)).astype(F32)
        cfg = dict(CFG, post_nms_topk=0, nms_thresh=0.99)
        rows, counts = run_maps(dense, strides, cfg, f"K + {extra}")
        assert counts[0] == 20
        if extra:
            assert rows[0, :, 4].min() > np.sqrt(dn.sigmoid(F32(1.0)) * dn.sigmoid(F32(3.0)))


def test_all_scores_equal_take_the_lower_flat_index():
    shapes, strides = ((6, 10), (3, 5)), (8, 16)
    dense = crafted(1, 3, shapes, logit=2.0)
    dense[0]["box2d_reg"][:] = 1.0  # 2 x 2 boxes on an 8-pixel grid: disjoint
    dense[1]["box2d_reg"][:] = 0.5  # 1 x 1 boxes on the 16-pixel grid: an IoU of 0.25 with level 0's at the same place
    rows, counts = run_maps(dense, strides, dict(CFG, post_nms_topk=0), "all equal")
    assert counts[0] == 40
    # level 0 first, then level 1, each by ascending flat index pixel * nc + class: 20 entries = pixels 0 .. 6
    assert np.array_equal(rows[0, :20, 7], np.zeros(20)) and np.array_equal(rows[0, :20, 6], np.arange(20) % 3)
    assert np.array_equal(rows[0, :20, 8], (np.arange(20) // 3) * 8.0)


def test_identical_boxes_of_one_class_and_of_two_classes():
    shapes, strides = ((2, 3),), (8,)
    dense = crafted(1, 2, shapes)
    lv = dense[0]
    lx, ly = np.meshgrid(np.arange(3) * 8.0, np.arange(2) * 8.0)
    lv["box2d_reg"][0] = np.stack([lx + 2, ly + 2, 30 - lx, 30 - ly]).astype(F32)  # every location: (-2, -2, 30, 30)
    lv["logits"][0, 0] = np.array([[1.0, 2.0, 3.0], [-20, -20, -20]], F32)         # class 0 at three pixels
    lv["logits"][0, 1, 0, 0] = 2.5                                                 # class 1 at one of them
    rows, counts = run_maps(dense, strides, dict(CFG), "identical boxes")
    assert counts[0] == 2 and sorted(rows[0, :2, 6]) == [0.0, 1.0]
    assert (rows[0, :2, :4] == np.array([-2, -2, 30, 30], F32)).all()


def test_nan_and_inf_never_become_candidates_and_corrupt_nothing():
    rng = np.random.default_rng(91)
    shapes, strides, B, C, nc = ((5, 7), (2, 3)), (8, 16), 2, 16, 3
    levels = sweep_levels(rng, B, C, nc, shapes, bias=1.0)
    packed = sweep_packed(rng, C, nc, 2, strides)
    levels[0]["logits"][0, 1, 2, 3] = np.nan
    levels[0]["logits"][1, 0, 0, 0] = np.inf
    levels[0]["logits"][1, 2, 4, 6] = -np.inf
    levels[1]["centerness"][0, 0, 1, 1] = np.nan
    levels[0]["f3d"][0, 3, 1, 1] = np.nan      # the 3D predictors of nine pixels become NaN
    levels[0]["f3d"][1, 5, 3, 5] = np.inf
    levels[1]["f2d"][1, 2, 0, 2] = np.nan
    for twc in (True, False):
        cfg = dict(CFG, thresh_with_ctr=twc, pre_nms_topk=64, post_nms_topk=0)
        det = {}
        rows, counts = check_both(levels, strides, packed, sweep_camera(B), dn.CANON, cfg, f"nan / inf twc={twc}", details=det)
        assert not np.isnan(rows[..., 4]).any() and np.isnan(rows[..., 10:]).any()
        flat = (2 * 7 + 3) * nc + 1
        assert flat not in det["levels"][0][0][0]  # the NaN logit's entry is no candidate


def test_tie_at_the_post_nms_cut_keeps_more_than_R_rows():
    shapes, strides = ((6, 10),), (8,)
    dense = crafted(1, 1, shapes, logit=2.0)
    dense[0]["box2d_reg"][:] = 1.0
    dense[0]["logits"][0, 0, 0, :4] = 4.0  # four rows above the tie
    rows, counts = run_maps(dense, strides, dict(CFG, pre_nms_topk=30, post_nms_topk=8), "tie at the cut")
    assert counts[0] == 30 and rows.shape[1] == 8 and (rows[0, :, 4] > 0).all()
    assert (rows[0, :4, 4] > rows[0, 4:, 4].max()).all() and np.unique(rows[0, 4:, 4]).size == 1


def test_frame_alone_and_elsewhere_in_the_batch():
    rng = np.random.default_rng(31)
    shapes, strides, B, C, nc = ((5, 7), (3, 4)), (8, 16), 3, 16, 3
    levels = sweep_levels(rng, B, C, nc, shapes)
    packed = sweep_packed(rng, C, nc, 2, strides)
    K = sweep_camera(B)
    rows, counts = lazy(levels, strides, packed, K, dn.CANON, CFG)
    pick = lambda idx: [{k: v[idx] for k, v in lv.items()} for lv in levels]  # noqa: E731
    alone = lazy(pick([1]), strides, packed, K[[1]], dn.CANON, CFG)
    assert torch.equal(alone[0][0], rows[1]) and torch.equal(alone[1][0], counts[1])
    perm = [2, 1, 0]
    moved = lazy(pick(perm), strides, packed, K[perm], dn.CANON, CFG)
    assert torch.equal(moved[0][0], rows[2]) and torch.equal(moved[0][2], rows[0]) and torch.equal(moved[1], counts[perm])


def test_refused_shapes_return_none():
    rng = np.random.default_rng(41)
    shapes, strides = ((3, 4),), (8,)
    levels = sweep_levels(rng, 1, 16, 3, shapes)
    packed = sweep_packed(rng, 16, 3, 1, strides)
    K = sweep_camera(1)
    assert lazy(levels, strides, packed, K, dn.CANON, dict(CFG, pre_nms_topk=1025)) is None
    assert lazy(levels, strides, packed, K, dn.CANON, dict(CFG, nms_thresh=0.0)) is None
    lv17 = sweep_levels(rng, 1, 16, 17, shapes)
    assert lazy(lv17, strides, sweep_packed(rng, 16, 17, 1, strides), K, dn.CANON * 3, CFG) is None
    nine = sweep_levels(rng, 1, 16, 3, shapes * 9)
    assert lazy(nine, strides * 9, sweep_packed(rng, 16, 3, 9, strides * 9), K, dn.CANON, CFG) is None


def test_no_host_synchronisation_and_launch_counts():
    tag = "v2_l5"
    model = cpu.build_model(tag).to(DEV)
    feats = [torch.from_numpy(f).to(DEV) for f in dn.golden_inputs(tag)]
    K = torch.from_numpy(dn.golden_camera(tag)).to(DEV)
    L = _lib.lib()
    with torch.no_grad():
        model.head_padded(feats, K, fused="lazy")  # packs the weights
        for fused, op in (("lazy", "pd3_dd3d_head_forward"), ("dense", "pd3_dd3d_post_process")):
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                with launch_ledger(L, _lib.symbols(MODULE)) as calls:
                    model.head_padded(feats, K, fused=fused)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            ran = {k: v for k, v in calls.items() if v}
            assert ran == {"pd3_dd3d_workspace": 1, op: 1}, (fused, ran)


def test_winograd_towers_on_request():
    """conv_kernel="winograd43" runs the towers' convolutions on the F(4x4, 3x3) kernel (one launch per convolution and
    level, a width of 7 through a row-padded copy).  The bound is reasoned, not measured: a direct fp32 convolution of
    9 * C = 288 terms carries about sqrt(288) * 2^-24 = 1e-6 of the outputs' scale, the F(4x4, 3x3) transforms amplify
    rounding by about ten, and the second layer sees the first one's error once more: 1e-4 of the largest output."""
    from paddle3d_amd import dd3d as D

    torch.manual_seed(5)
    shapes, strides, C = ((12, 40), (5, 7)), (8, 16), 32
    ref = D.FCOS2DHead(list(strides), [C] * 2, num_classes=3, norm="FrozenBN", num_cls_convs=2, num_box_convs=2).to(DEV).eval()
    win = D.FCOS2DHead(list(strides), [C] * 2, num_classes=3, norm="FrozenBN", num_cls_convs=2, num_box_convs=2,
                       conv_kernel="winograd43").to(DEV).eval()
    win.load_state_dict(ref.state_dict())
    feats = [torch.randn(2, C, h, w, device=DEV) for h, w in shapes]
    with torch.no_grad(), launch_ledger(_lib.lib(), ("pd3_conv3x3_winograd43_bias_relu",)) as calls:
        want, got = ref.towers(feats), win.towers(feats)
    assert calls["pd3_conv3x3_winograd43_bias_relu"] == 2 * 2 * len(shapes)
    for a, b in zip(want[0] + want[1], got[0] + got[1]):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-4 * float(a.abs().max())
