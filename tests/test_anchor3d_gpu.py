"""BEVFusion's Anchor3DHead on the device: both entry points (the lazy head and the from-maps form) bit-equal to the NumPy
restatement (tests/golden/anchor3d_numpy.py) on the golden cases and on seeded sweeps -- map sizes around the dense
kernel's 16-pixel wave tile and 128-pixel workgroup, channel counts, anchors per cell (up to three chunks of the dense
kernel), class counts, both code sizes, selection sizes around N and the 64-box NMS tile, output sizes, thresholds that
empty a class or a frame, and hostile data (tied scores, saturated sigmoids, a NaN cell, infinite deltas, exp overflow);
the two paths on torch's convolutions and the module (fused, forced, unfused) against the reference's golden file
within its stored bounds; a frame alone, elsewhere in the batch and on a side stream; refusals; no host
synchronisation; launch counts."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from guarded import launch_ledger  # noqa: E402

import anchor3d_numpy as an  # noqa: E402
import make_anchor3d_golden as mk  # noqa: E402
import test_anchor3d_cpu as cpu  # noqa: E402
from test_anchor3d_cpu import golden  # noqa: E402,F401  (fixture)

from paddle3d_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
# the table's first block (patch convolution, per-class NMS, ...): what the head runs besides its own entry points
FIRST_BLOCK = _lib.symbols("test_memory_safety_gpu")


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


def same_results(got, want, what=""):
    for name, g, w in zip(("boxes", "scores", "labels", "counts"), got, want):
        same_bits(g, w, f"{what} {name}")


def lazy(feat, st, anchors, cfg):
    from paddle3d_amd.ops import anchor3d_head as ops

    return ops.anchor3d_head_forward(
        _t(feat), ops.pack_cls_weight(_t(st["conv_cls.weight"]), cfg["num_classes"]), _t(st["conv_cls.bias"]),
        _t(st["conv_reg.weight"]), _t(st["conv_reg.bias"]), _t(st["conv_dir_cls.weight"]), _t(st["conv_dir_cls.bias"]),
        _t(anchors), cfg["num_classes"], cfg["nms_pre"], cfg["max_num"], cfg["score_thr"], cfg["nms_thr"],
        cfg["dir_offset"], cfg["dir_limit_offset"])


def from_maps(maps, anchors, cfg):
    from paddle3d_amd.ops import anchor3d_head as ops

    return ops.anchor3d_get_bboxes(*(m if isinstance(m, torch.Tensor) else _t(m) for m in maps), _t(anchors),
                                   cfg["num_classes"], cfg["nms_pre"], cfg["max_num"], cfg["score_thr"], cfg["nms_thr"],
                                   cfg["dir_offset"], cfg["dir_limit_offset"])


# ---- the golden cases ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", an.TAGS)
def test_both_entry_points_on_the_golden_cases(golden, tag):  # noqa: F811
    feat, st, anchors, cfg = an.golden_inputs(tag), an.golden_state(tag), mk.anchors_of(tag), an.cfg_of(tag)
    want = cpu.restated(tag)
    got = lazy(feat, st, anchors, cfg)
    same_results(got, want, f"{tag} lazy")
    same_results(from_maps(an.head_maps(feat, st), anchors, cfg), want, f"{tag} from maps")
    cpu.check_padded(golden, tag, [_n(t) for t in got])


@pytest.mark.parametrize("tag", an.TAGS)
def test_paths_on_torch_convolutions_and_the_module(golden, tag):  # noqa: F811
    """The from-maps path on maps made by torch's convolutions, and the module fused / forced / unfused, against the
    reference: labels, counts and rows equal, values within the stored bounds."""
    feat, st, anchors, cfg = an.golden_inputs(tag), an.golden_state(tag), mk.anchors_of(tag), an.cfg_of(tag)
    x = _t(feat)
    maps = [torch.nn.functional.conv2d(x, _t(st[k + ".weight"]), _t(st[k + ".bias"]))
            for k in ("conv_cls", "conv_reg", "conv_dir_cls")]
    cpu.check_padded(golden, tag, [_n(t) for t in from_maps(maps, anchors, cfg)])
    head = cpu.build_head(tag).to(DEV)
    metas = [{}] * an.CASES[tag]["B"]
    with torch.no_grad():
        for fused in (True, "force", False):
            res = head.forward_get_bboxes([x], metas, fused=fused)
            for b, (bx, sc, lb) in enumerate(res):
                assert lb.dtype == torch.int64 and bx.is_cuda
                cpu.check_frame(golden, tag, b, _n(bx), _n(sc), _n(lb))
        hmaps = head([x])
        for fused in (True, False):
            for b, (bx, sc, lb) in enumerate(head.get_bboxes(*hmaps, metas, fused=fused)):
                cpu.check_frame(golden, tag, b, _n(bx), _n(sc), _n(lb))
        padded = head.forward_get_bboxes([x], metas, fused="force", return_padded=True)
    same_results(padded, cpu.restated(tag), f"{tag} module")


# ---- seeded sweeps ---------------------------------------------------------------------------------------------------
def sweep_anchors(rng, H, W, A, cs):
    """An anchor table by the generator (A = sizes x rotations) with random custom columns."""
    from paddle3d_amd.ops.anchor3d_head import aligned_anchor3d_grid

    rots = [0, 1.57] if A % 2 == 0 else [0.3]
    sizes = rng.uniform(0.5, 6.0, (A // len(rots), 3)).round(2).tolist()
    a = aligned_anchor3d_grid([[-30.0, -30.0, -1.0, 30.0, 30.0, -1.0]], sizes, rots, (0,) * (cs - 7), (H, W)).numpy()
    a[:, 7:] = rng.standard_normal((len(a), cs - 7)).astype(F32)
    return a


def sweep_state(rng, C, A, nc, cs, reg_scale=0.3):
    st = {}
    for name, rows, scale in (("conv_cls", A * nc, 1.5), ("conv_reg", A * cs, reg_scale), ("conv_dir_cls", A * 2, 1.0)):
        st[name + ".weight"] = (rng.standard_normal((rows, C, 1, 1)) * scale / np.sqrt(C)).astype(F32)
        st[name + ".bias"] = (rng.standard_normal(rows) * 0.1).astype(F32)
    return st


def run_point(seed, B, H, W, C, A, nc, cs, nms_pre, max_num, score_thr=0.3, nms_thr=0.2, feat_edit=None, st_edit=None):
    rng = np.random.default_rng(seed)
    anchors, st = sweep_anchors(rng, H, W, A, cs), sweep_state(rng, C, A, nc, cs)
    feat = rng.standard_normal((B, C, H, W)).astype(F32)
    if feat_edit is not None:
        feat_edit(feat)
    if st_edit is not None:
        st_edit(st)
    cfg = dict(nms_pre=nms_pre, max_num=max_num, score_thr=score_thr, nms_thr=nms_thr, dir_offset=0.7854,
               dir_limit_offset=0, num_classes=nc)
    maps = an.head_maps(feat, st)
    want = an.get_bboxes(*maps, anchors, cfg)
    what = f"{(B, H, W, C, A, nc, cs, nms_pre, max_num, score_thr)}"
    same_results(lazy(feat, st, anchors, cfg), want, what + " lazy")
    same_results(from_maps(maps, anchors, cfg), want, what + " from maps")
    return want


SHAPES = [  # H, W, C, A, nc, cs, nms_pre, max_num
    (1, 1, 16, 1, 1, 7, 1000, 1),        # one anchor: K = 1
    (1, 1, 48, 6, 3, 9, 1, 5),           # K = 1 of 6
    (5, 7, 48, 6, 3, 7, 8, 5),
    (5, 7, 16, 14, 10, 9, 1000, 500),    # nms_pre above the 490 anchors
    (16, 16, 16, 14, 10, 9, 64, 500),    # whole 16-pixel tiles, K = 64
    (17, 15, 384, 14, 10, 9, 65, 5),     # a second workgroup with one partial wave tile, the flagship's channels
    (4, 33, 16, 6, 3, 9, 4 * 33 * 6 - 1, 500),   # N - 1
    (4, 33, 48, 1, 10, 7, 4 * 33, 1),            # N
    (5, 7, 16, 6, 1, 7, 5 * 7 * 6 + 1, 5),       # N + 1
    (5, 7, 16, 6, 3, 7, -1, 500),                # no pre-selection
    (3, 5, 16, 32, 16, 7, 200, 500),     # 512 class rows: three chunks of the dense kernel
    (3, 23, 32, 28, 7, 9, 300, 500),     # 196 class rows: a second chunk of one anchor
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_sweep(shape):
    H, W, C, A, nc, cs, nms_pre, max_num = shape
    want = run_point(11 + H * W + A, 2, H, W, C, A, nc, cs, nms_pre, max_num)
    assert want[3].max() > 0


def test_thresholds_that_empty_a_class_and_a_frame():
    def no_class_1(st):
        st["conv_cls.bias"].reshape(6, 3)[:, 1] = F32(-9.0)

    def frame_1_flat(feat):
        feat[1] = 0.0

    want = run_point(5, 2, 5, 7, 16, 6, 3, 7, 50, 500, score_thr=0.3, st_edit=no_class_1)
    assert want[3].min() > 0 and not (want[2] == 1).any()
    want = run_point(6, 2, 5, 7, 16, 6, 3, 7, 50, 500, score_thr=0.7, feat_edit=frame_1_flat)
    assert want[3][0] > 0 and want[3][1] == 0 and not want[0][1].any()
    want = run_point(7, 2, 5, 7, 16, 6, 3, 7, 50, 500, score_thr=1.0)  # nothing anywhere
    assert not want[3].any()


@pytest.mark.parametrize("n", [63, 64, 65])
def test_candidate_counts_at_the_nms_tile(n):
    """Class 0 has exactly n candidates (the others none): far apart, all kept, and packed, most suppressed."""
    rng = np.random.default_rng(n)
    H, W, A, nc, cs = 9, 11, 2, 3, 7
    N = H * W * A
    for spread in (True, False):
        anchors = sweep_anchors(rng, H, W, A, cs)
        anchors[:, :2] *= F32(10.0 if spread else 0.05)
        cls = np.full((1, A * nc, H, W), -5.0, F32)
        hot = rng.choice(H * W, n, replace=False) * A + rng.integers(0, A, n)  # one anchor per cell
        rows = cls.reshape(A, nc, H * W)
        rows[hot % A, 0, hot // A] = rng.uniform(0.0, 4.0, n).astype(F32)
        reg = (rng.standard_normal((1, A * cs, H, W)) * 0.05).astype(F32)
        dirs = rng.standard_normal((1, A * 2, H, W)).astype(F32)
        cfg = dict(nms_pre=100, max_num=500, score_thr=0.3, nms_thr=0.2, dir_offset=0.0, dir_limit_offset=1.0, num_classes=nc)
        trace = {}
        an.frame_bboxes(cls[0], reg[0], dirs[0], anchors, cfg, trace=trace)
        assert [(c, len(cand)) for c, cand, _ in trace["sets"]] == [(0, n)]
        want = an.get_bboxes(cls, reg, dirs, anchors, cfg)
        assert want[3][0] == n if spread else 0 < want[3][0] < n
        same_results(from_maps((cls, reg, dirs), anchors, cfg), want, f"{n} candidates, spread {spread}")


import topk_lattice as TL  # noqa: E402


def _far_apart(rng, H, W, A):
    anchors = sweep_anchors(rng, H, W, A, TL.A3D_CS)
    anchors[:, :2] *= F32(10.0)   # no two boxes overlap: the NMS keeps every candidate
    return anchors


@pytest.mark.parametrize("grid", list(TL.A3D_GRIDS))
@pytest.mark.parametrize("nms_pre", TL.A3D_NMS_PRE)
def test_selection_lattice_nms_pre(grid, nms_pre):
    """a3d_topk_kernel at nms_pre 63 / 64 / 65 / 129 / 1024 with N & 3 both ways (the float4 and the scalar walk): the
    cut lies inside ten equal scores, five taken, the other five in the next wave of block_topk_compact
    (tests/test_topk_lattice_cpu.py::test_anchor3d_call_site_labels).  Bit for bit against the restatement."""
    H, W, A = TL.A3D_GRIDS[grid]
    x, cluster = TL.a3d_select_case(grid, nms_pre)
    rng = np.random.default_rng(nms_pre)
    anchors = _far_apart(rng, H, W, A)
    cls, reg, dirs = TL.a3d_maps(H, W, A, x, nms_pre)
    cfg = dict(nms_pre=nms_pre, max_num=500, score_thr=0.05, nms_thr=0.2, dir_offset=0.0, dir_limit_offset=1.0,
               num_classes=TL.A3D_NC)
    trace = {}
    an.frame_bboxes(cls[0], reg[0], dirs[0], anchors, cfg, trace=trace)
    sel = trace["sel"]
    assert len(sel) == nms_pre and np.array_equal(np.intersect1d(sel, cluster), cluster[:5])
    want = an.get_bboxes(cls, reg, dirs, anchors, cfg)
    assert 0 < want[3][0] <= min(nms_pre, 500)      # (the two rotations of a pixel overlap: the NMS drops a few)
    same_results(from_maps((cls, reg, dirs), anchors, cfg), want, f"{grid} nms_pre {nms_pre}")


@pytest.mark.parametrize("n", TL.A3D_SET_SIZES)
def test_selection_lattice_class_sets_and_max_num(n):
    """A class set of exactly 64, 65 and 129 candidates (a3d_class_sets_kernel's block_topk_sort alone: n2 = 64, 128 and
    256, the last with block barriers inside the network), tied scores inside; then two classes whose kept candidates
    number max_num + 1 (a3d_output_kernel's cut over the concatenated keys takes all but one)."""
    for total_cut in (False, True):
        (H, W, A), x = TL.a3d_set_case(n, total_cut)
        rng = np.random.default_rng(n)
        anchors = _far_apart(rng, H, W, A)
        cls, reg, dirs = TL.a3d_maps(H, W, A, x, n)
        total = n + (n // 2 if total_cut else 0)
        cfg = dict(nms_pre=1000, max_num=total - 1 if total_cut else 500, score_thr=0.3, nms_thr=0.2, dir_offset=0.0,
                   dir_limit_offset=1.0, num_classes=TL.A3D_NC)
        trace = {}
        an.frame_bboxes(cls[0], reg[0], dirs[0], anchors, cfg, trace=trace)
        sizes = [(c, len(cand), len(keep)) for c, cand, keep in trace["sets"]]
        assert sizes == ([(0, n, n), (1, n // 2, n // 2)] if total_cut else [(0, n, n)]) and trace["total"] == total
        want = an.get_bboxes(cls, reg, dirs, anchors, cfg)
        assert want[3][0] == (total - 1 if total_cut else n)
        same_results(from_maps((cls, reg, dirs), anchors, cfg), want, f"class set of {n}, total cut {total_cut}")


def test_hostile_data():
    rng = np.random.default_rng(77)
    H, W, A, nc, cs = 6, 9, 6, 3, 9
    N = H * W * A
    anchors = sweep_anchors(rng, H, W, A, cs)
    cfg = dict(nms_pre=40, max_num=12, score_thr=0.3, nms_thr=0.2, dir_offset=0.7854, dir_limit_offset=0.0, num_classes=nc)
    reg = (rng.standard_normal((2, A * cs, H, W)) * 0.3).astype(F32)
    dirs = rng.standard_normal((2, A * 2, H, W)).round().astype(F32)  # tied direction logits: the first maximum wins
    # tied scores everywhere: at the nms_pre cut, inside the class sets and at the max_num cut
    cls = (rng.standard_normal((2, A * nc, H, W)) * 2).round().astype(F32) * F32(0.5)
    want = an.get_bboxes(cls, reg, dirs, anchors, cfg)
    assert (want[3] == 12).all()
    same_results(from_maps((cls, reg, dirs), anchors, cfg), want, "tied scores")
    # sigmoids saturated to 1.0 and to 0.0
    cls2 = cls.copy()
    cls2[:, :, :2] = 40.0
    cls2[:, :, 2:4] = -120.0
    want = an.get_bboxes(cls2, reg, dirs, anchors, cfg)
    assert (want[1][:, 0] == 1.0).all()
    same_results(from_maps((cls2, reg, dirs), anchors, cfg), want, "saturated")
    # a NaN logit, +-Inf deltas, exp overflow in the sizes, among the selected anchors of frame 0
    cfg_all = dict(cfg, nms_pre=N, max_num=500)
    cls3, reg3 = cls.copy(), reg.copy()
    r = reg3.reshape(2, A, cs, H * W)
    cls3.reshape(2, A, nc, H * W)[0, 1, 0, 3] = np.nan
    r[0, 0, 0, 5] = np.inf      # x
    r[0, 2, 3, 7] = -np.inf     # w: exp(-inf) = 0
    r[0, 3, 4, 9] = 100.0       # l: exp overflows
    r[0, 4, 5, 11] = np.inf     # h
    for a, pix in ((0, 5), (2, 7), (3, 9), (4, 11)):
        cls3.reshape(2, A, nc, H * W)[0, a, 2, pix] = 3.0  # candidates of class 2
    with np.errstate(all="ignore"):
        want = an.get_bboxes(cls3, reg3, dirs, anchors, cfg_all)
    assert np.isinf(want[0]).any()
    same_results(from_maps((cls3, reg3, dirs), anchors, cfg_all), want, "non-finite")
    # the lazy path: a NaN feature cell (every logit of the cell is a NaN) and huge regression weights
    def nan_cell(feat):
        feat[0, :, 2, 3] = np.nan

    def big_sizes(st):
        st["conv_reg.weight"].reshape(A, cs, -1)[:, 3:6] *= F32(200.0)

    with np.errstate(all="ignore"):
        run_point(78, 2, H, W, 16, A, nc, cs, N, 500, feat_edit=nan_cell)
        want = run_point(79, 2, H, W, 16, A, nc, cs, 60, 500, st_edit=big_sizes)
    assert np.isinf(want[0]).any()


def test_module_forward_runs_the_patch_convolution():
    """forward(feats) on a map the 1x1 patch-GEMM kernel takes: three launches, torch's convolution within fp32 noise."""
    from paddle3d_amd import bevfusion_head as bh

    torch.manual_seed(0)
    head = bh.Anchor3DHead(3, 32, 32, anchor_generator=dict(ranges=[[0.0, -40.0, -0.6, 70.0, 40.0, -0.6]],
                                                            sizes=[[0.6, 0.8, 1.73], [1.6, 3.9, 1.56]], scales=[1]),
                           bbox_coder=dict(code_size=7), test_cfg=dict(nms_pre=50, max_num=20, score_thr=0.3, nms_thr=0.1))
    head = head.to(DEV).eval()
    x = torch.randn(2, 32, 4, 10, device=DEV)
    with launch_ledger(_lib.lib(), FIRST_BLOCK) as base, torch.no_grad():
        maps = head([x])
    assert base["pd3_patch_conv_bias_relu"] == 3
    for m, conv in zip(maps, (head.conv_cls, head.conv_reg, head.conv_dir_cls)):
        with torch.no_grad():
            want = conv(x)
        assert m[0].shape == want.shape and float((m[0] - want).abs().max()) < 1e-5
    with torch.no_grad():
        a = head.get_bboxes(*maps, [{}] * 2, return_padded=True)
        b = head.get_bboxes(*maps, [{}] * 2, fused=False, return_padded=True)
    assert torch.equal(a[3], b[3]) and torch.equal(a[2], b[2]) and int(a[3].min()) > 0
    assert float((a[0] - b[0]).abs().max()) < 1e-4 and float((a[1] - b[1]).abs().max()) < 1e-6


# ---- placement -------------------------------------------------------------------------------------------------------
def test_alone_elsewhere_in_the_batch_and_on_a_side_stream():
    tag = "nus"
    feat, st, anchors, cfg = an.golden_inputs(tag), an.golden_state(tag), mk.anchors_of(tag), an.cfg_of(tag)
    want = cpu.restated(tag)
    for run in (lambda f: lazy(f, st, anchors, cfg), lambda f: from_maps(an.head_maps(f, st), anchors, cfg)):
        for b in range(2):
            same_results(run(feat[b:b + 1]), [w[b:b + 1] for w in want], f"frame {b} alone")
        got = run(feat[[1, 0, 1]])
        same_results(got, [w[[1, 0, 1]] for w in want], "frames 1, 0, 1")
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            got = run(feat)
        side.synchronize()
        same_results(got, want, "side stream")


def test_refused_shapes_return_none_and_the_module_falls_back(golden):  # noqa: F811
    from paddle3d_amd.ops import anchor3d_head as ops

    rng = np.random.default_rng(3)
    cfg = dict(nms_pre=20, max_num=10, score_thr=0.3, nms_thr=0.2, dir_offset=0.0, dir_limit_offset=1.0, num_classes=3)
    anchors = sweep_anchors(rng, 5, 7, 6, 7)
    for C in (24, 8, 528):  # channels the lazy kernels do not take
        st, feat = sweep_state(rng, C, 6, 3, 7), rng.standard_normal((1, C, 5, 7)).astype(F32)
        assert lazy(feat, st, anchors, cfg) is None
        assert from_maps(an.head_maps(feat, st), anchors, cfg) is not None
    st, feat = sweep_state(rng, 16, 6, 3, 7), rng.standard_normal((1, 16, 33, 7)).astype(F32)
    big = sweep_anchors(rng, 33, 7, 6, 7)  # 1386 anchors
    for bad in (dict(nms_pre=-1), dict(nms_pre=1025), dict(max_num=1025)):
        assert lazy(feat, st, big, dict(cfg, **bad)) is None and from_maps(an.head_maps(feat, st), big, dict(cfg, **bad)) is None
    with pytest.raises(RuntimeError, match="Unsupported device"):
        ops.anchor3d_get_bboxes(torch.zeros(1, 18, 5, 7), torch.zeros(1, 42, 5, 7), torch.zeros(1, 12, 5, 7),
                                torch.zeros(210, 7), 3, 20, 10, 0.3, 0.2)
    # the module: nms_pre above the candidate list's size -> the torch transcription, still the reference's results
    tag = "kitti"
    head = cpu.build_head(tag).to(DEV)
    x, metas = _t(an.golden_inputs(tag)), [{}] * 2
    with launch_ledger(_lib.lib(), FIRST_BLOCK) as base, torch.no_grad():
        with launch_ledger(_lib.lib(), _lib.symbols("test_memory_safety_anchor3d_gpu")) as calls:
            head.test_cfg = dict(head.test_cfg, nms_pre=-1)  # all 210 anchors: taken by the kernels
            n_all = [len(r[1]) for r in head.forward_get_bboxes([x], metas)]
            assert calls["pd3_anchor3d_head_forward"] == 1
            head.test_cfg = dict(an.CASES[tag]["test_cfg"], max_num=2000)  # refused
            res = head.forward_get_bboxes([x], metas)
            assert calls["pd3_anchor3d_head_forward"] == 1 and calls["pd3_anchor3d_get_bboxes"] == 0
        assert base["pd3_nms_bev"] >= 2  # ops.iou3d_nms.nms_gpu per class
    assert all(n > 0 for n in n_all)
    for b, (bx, sc, lb) in enumerate(res):  # max_num = 2000 keeps every survivor: the golden's 10 rows are its best 10
        top = torch.argsort(sc, descending=True, stable=True)[:10]
        assert len(sc) > 10
        cpu.check_frame(golden, tag, b, _n(bx[top]), _n(sc[top]), _n(lb[top]))


def test_no_host_synchronisation_and_launch_counts(golden):  # noqa: F811
    tag = "nus"
    head = cpu.build_head(tag).to(DEV)
    x, metas = _t(an.golden_inputs(tag)), [{}] * 2
    with torch.no_grad():
        head.forward_get_bboxes([x], metas, fused="force", return_padded=True)  # packs the weights, builds the anchors
        maps = head([x])
        head.get_bboxes(*maps, metas, return_padded=True)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with launch_ledger(_lib.lib(), _lib.symbols("test_memory_safety_anchor3d_gpu")) as calls:
                a = head.forward_get_bboxes([x], metas, fused="force", return_padded=True)
                b = head.get_bboxes(*maps, metas, return_padded=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert calls == {"pd3_anchor3d_head_workspace": 2, "pd3_anchor3d_head_forward": 1, "pd3_anchor3d_get_bboxes": 1}
    same_results(a, cpu.restated(tag), "lazy")
    cpu.check_padded(golden, tag, [_n(t) for t in b])
    # the lazy path runs no convolution and no per-class NMS call
    with launch_ledger(_lib.lib(), FIRST_BLOCK) as base, torch.no_grad():
        head.forward_get_bboxes([x], metas, fused="force", return_padded=True)
    assert not any(base.values()), {k: v for k, v in base.items() if v}
