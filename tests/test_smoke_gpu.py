"""SMOKE's head and post-processing on the device: both entry points (the lazy head and the from-maps form) bit-equal to
the NumPy restatement (tests/golden/smoke_numpy.py) on the golden cases and on seeded sweeps -- map sizes around the
wave, the 64-pixel workgroup of the class kernel and the top-K's 1024-key walk, head widths and group counts, class
counts, selection sizes 1, 2, 50, H * W and 1024, more rows than peaks, B = 1 .. 3, rows of padded pitch in one stacked
map -- and on hostile data (saturated logits, a NaN and an Inf pixel, expf overflow, a zero orientation vector,
z = -1e-7, a singular K, thresholds that empty a frame and a batch); both entry points and the module in its three forms
against the reference's golden file within its stored bounds; the norm tables on a constant map and on one whose mean is
far above its spread; a frame alone, elsewhere in the batch and on a side stream; refusals; no host synchronisation;
launch counts."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from guarded import launch_ledger  # noqa: E402

import smoke_numpy as sn  # noqa: E402
import test_smoke_cpu as cpu  # noqa: E402
from test_smoke_cpu import golden  # noqa: E402,F401  (fixture)

from paddle3d_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
WATCHED = _lib.symbols("test_memory_safety_smoke_gpu") + _lib.symbols("test_memory_safety_gpu")


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
    assert got is not None, f"{what}: the op refused the shape"
    same_bits(got[0], want[0], what + " rows")
    same_bits(got[1], want[1], what + " counts")


def sweep_state(rng, C, nc, cls_scale=2.0):
    st = {}
    for head, rows, scale in (("class_head", nc, cls_scale), ("regression_head", 10, 0.5)):
        st[f"{head}.1.weight"] = rng.uniform(0.5, 1.5, C).astype(F32)
        st[f"{head}.1.bias"] = (rng.standard_normal(C) * 0.1).astype(F32)
        st[f"{head}.3.weight"] = (rng.standard_normal((rows, C, 1, 1)) * scale / np.sqrt(C)).astype(F32)
        st[f"{head}.3.bias"] = (rng.standard_normal(rows) * 0.1).astype(F32)
    st["class_head.3.bias"] = (st["class_head.3.bias"] - F32(1.0)).astype(F32)
    return st


def sweep_camera(B, H, W, nc):
    Ks, Ts = np.zeros((B, 3, 3), F32), np.zeros((B, 3, 3), F32)
    for b in range(B):
        f = 700.0 + 11.0 * b
        Ks[b] = [[f, 0, 600.0 - 3.0 * b], [0, f, 180.0 + b], [0, 0, 1]]
        s = W / (1200.0 + 8 * b)
        Ts[b] = [[s, 0, 0.25 * b], [0, s, -0.5 * b], [0, 0, 1]]
    dim_ref = (np.array(sn.DIM_REF, F32)[np.arange(nc) % 3] + np.arange(nc, dtype=F32)[:, None] * F32(0.125)).astype(F32)
    return dict(K=Ks, trans_mat=Ts, down_ratios=np.array([[1200.0 / W, 360.0 / H]], F32),
                image_size=np.array([[1200.0, 360.0]], F32), depth_ref=np.array([28.01, 16.32], F32), dim_ref=dim_ref)


def lazy(cf, rf, st, cam, cfg, groups, tables=None, stacked=False):
    """ops.smoke.smoke_head_forward on numpy inputs; stacked: both branches as views of one [B, 2C, H, pitch4(W)] map."""
    from paddle3d_amd.ops import smoke as A
    from paddle3d_amd.ops.conv import pitch4

    B, C, H, W = cf.shape
    if stacked:
        buf = torch.zeros((B, 2 * C, H, pitch4(W)), dtype=torch.float32, device=DEV)
        buf[:, :C, :, :W], buf[:, C:, :, :W] = _t(cf), _t(rf)
        tc, tr = buf[:, :C, :, :W], buf[:, C:, :, :W]
    else:
        tc, tr = _t(cf), _t(rf)
    s = {k: _t(v) for k, v in st.items()}
    fwd = cfg["mode"] == "forward"
    tabs = (None, None) if tables is None else tuple(_t(t) for t in tables)
    return A.smoke_head_forward(tc, tr, (s["class_head.1.weight"], s["class_head.1.bias"]),
                                (s["regression_head.1.weight"], s["regression_head.1.bias"]), s["class_head.3.weight"],
                                s["class_head.3.bias"], s["regression_head.3.weight"], s["regression_head.3.bias"],
                                _t(cam["K"]), _t(cam["trans_mat"] if fwd else cam["down_ratios"]),
                                _t(cam["image_size"]) if fwd else None, _t(cam["depth_ref"]), _t(cam["dim_ref"]), groups,
                                cfg["max_detection"], cfg["det_threshold"], A.FORWARD if fwd else A.EXPORT, *tabs)


def from_maps(heat, reg, cam, cfg):
    from paddle3d_amd.ops import smoke as A

    fwd = cfg["mode"] == "forward"
    return A.smoke_post_process(_t(heat), _t(reg), _t(cam["K"]), _t(cam["trans_mat"] if fwd else cam["down_ratios"]),
                                _t(cam["image_size"]) if fwd else None, _t(cam["depth_ref"]), _t(cam["dim_ref"]),
                                cfg["max_detection"], cfg["det_threshold"], A.FORWARD if fwd else A.EXPORT)


def check_both(cf, rf, st, cam, cfg, groups, what, tables=None, stacked=False):
    """Both entry points against the restatement: the lazy head from the 3x3 outputs, the from-maps form from the
    restatement's heat map and activated regression map.  Returns the restatement's (rows, counts)."""
    want, heat = sn.head_forward(cf, rf, st, cam, cfg, groups, tables)
    same_results(lazy(cf, rf, st, cam, cfg, groups, tables, stacked), want, what + " lazy")
    rt = tables[1] if tables is not None else sn.stats_tables(rf, groups)
    reg = sn.activate(sn.regression_raw(rf, rt, st["regression_head.1.weight"], st["regression_head.1.bias"],
                                        st["regression_head.3.weight"], st["regression_head.3.bias"]))
    same_results(from_maps(heat, reg, cam, cfg), sn.post_process(heat, reg, cam, cfg), what + " from maps")
    return want


# ---- golden cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sn.TAGS)
def test_entry_points_on_the_golden_cases(tag, golden):  # noqa: F811
    c, st = sn.CASES[tag], sn.golden_state(tag)
    cf, rf = cpu.conv3x3_outputs(tag)
    tables = None
    if c["norm"] == "bn":
        tables = tuple(sn.bn_tables(st, f"{h}.1", c["B"]) for h in ("class_head", "regression_head"))
    rows, counts = check_both(cf, rf, st, sn.golden_camera(tag), sn.cfg_of(tag), sn.groups_of(tag), tag, tables,
                              stacked=c["W"] % 4 != 0)
    cpu.check_against_golden(tag, rows, counts, golden, "device (= restatement)")


@pytest.mark.parametrize("tag", sn.TAGS)
@pytest.mark.parametrize("fused", ("lazy", "dense", False))
def test_module_on_the_golden_cases(tag, fused, golden):  # noqa: F811
    """The three forms.  The two head cases of width 256 run their 3x3 convolutions as the stacked Winograd launch
    (smoke.WINOGRAD_MIN_WIDTH), the narrower ones through torch's convolution."""
    model = cpu.build_model(tag).to(DEV)
    rows, counts = cpu.run_model(model, tag, DEV, fused=fused)
    cpu.check_against_golden(tag, _n(rows), _n(counts), golden, f"module fused={fused}")


# ---- seeded sweeps ------------------------------------------------------------------------------------------------------
# (H, W, C, groups, nc, K, B, mode)
SWEEP = ((1, 1, 16, 16, 1, 1, 1, "forward"), (1, 2, 32, 32, 3, 2, 2, "export"), (3, 4, 48, 16, 4, 12, 3, "forward"),
         (5, 7, 64, 32, 16, 35, 1, "forward"), (17, 15, 256, 32, 3, 50, 2, "forward"), (4, 33, 512, 32, 4, 2, 1, "export"),
         (2, 65, 16, 16, 1, 50, 3, "forward"), (9, 129, 32, 32, 3, 1024, 1, "forward"), (9, 129, 16, 4, 16, 50, 2, "export"),
         (17, 15, 48, 16, 1, 255, 1, "export"), (4, 33, 64, 64, 3, 132, 2, "forward"))


@pytest.mark.parametrize("point", SWEEP, ids=lambda p: "x".join(str(v) for v in p))
def test_sweep_is_bit_equal_to_the_restatement(point):
    H, W, C, G, nc, K, B, mode = point
    rng = np.random.default_rng(H * 1000003 + W * 10007 + C * 101 + nc * 7 + K)
    cf, rf = (rng.standard_normal((B, C, H, W)).astype(F32) + F32(0.5) for _ in range(2))
    cfg = dict(max_detection=K, det_threshold=0.3, mode=mode)
    rows, counts = check_both(cf, rf, sweep_state(rng, C, nc), sweep_camera(B, H, W, nc), cfg, G, str(point),
                              stacked=W % 4 != 0)
    if K == H * W and mode == "export" and H * W > 9:  # more rows than peaks: rows of score 0, lowest index first
        assert (rows[..., 13] == 0).any()


# ---- hostile data ---------------------------------------------------------------------------------------------------------
def hostile_base(seed=9):
    rng = np.random.default_rng(seed)
    B, C, H, W, nc = 3, 32, 5, 7, 3
    cf, rf = (rng.standard_normal((B, C, H, W)).astype(F32) for _ in range(2))
    return rng, cf, rf, sweep_state(rng, C, nc), sweep_camera(B, H, W, nc)


@pytest.mark.parametrize("mode", ("forward", "export"))
def test_hostile_head_inputs(mode):
    cfg = dict(max_detection=20, det_threshold=0.3, mode=mode)
    # saturated logits: the scores tie on both ends of the clip
    rng, cf, rf, st, cam = hostile_base()
    st["class_head.3.weight"] = (st["class_head.3.weight"] * F32(500)).astype(F32)
    rows, _ = check_both(cf, rf, st, cam, cfg, 32, "saturated")
    assert np.unique(rows[..., 13]).size < rows[..., 13].size
    # a NaN and an Inf pixel, under GroupNorm (the frame's groups go) and under given tables (the pixel goes)
    rng, cf, rf, st, cam = hostile_base()
    cf[0, 3, 2, 2], cf[1, 5, 1, 1], rf[2, 7, 0, 0], rf[1, 9, 4, 6] = np.nan, np.inf, np.nan, -np.inf
    check_both(cf, rf, st, cam, cfg, 32, "nan / inf, gn")
    tables = tuple(np.stack([rng.standard_normal((3, 32)) * 0.1, rng.uniform(0.8, 1.2, (3, 32))], 1).astype(F32)
                   for _ in range(2))
    check_both(cf, rf, st, cam, cfg, 32, "nan / inf, tables", tables)
    # a zero orientation vector: the 1e-12 floor
    rng, cf, rf, st, cam = hostile_base()
    st["regression_head.3.weight"][6:8] = 0
    st["regression_head.3.bias"][6:8] = 0
    check_both(cf, rf, st, cam, cfg, 32, "zero orientation")
    # a singular K: whatever the restatement gives, no fault
    rng, cf, rf, st, cam = hostile_base()
    cam["K"][1] = 0
    cam["K"][2, 1] = cam["K"][2, 0]
    check_both(cf, rf, st, cam, cfg, 32, "singular K")
    # thresholds that empty a frame and a batch
    rng, cf, rf, st, cam = hostile_base()
    heat = sn.head_forward(cf, rf, st, cam, cfg, 32)[1]
    for thr in (float(np.sort(sn.peak_scores(heat[0]).reshape(-1))[-1]), 2.0):
        rows, counts = check_both(cf, rf, st, cam, dict(cfg, det_threshold=thr), 32, f"thr {thr}")
        if mode == "forward":
            assert counts[0] == 0 and (thr < 2.0 or not counts.any())


def test_hostile_maps():
    """The from-maps form on maps SMOKEPredictor cannot give: expf overflow in the dimensions, z = -1e-7 (the ray's
    denominator is 0), infinite offsets, a NaN and an Inf heat."""
    rng = np.random.default_rng(21)
    B, nc, H, W, K = 2, 3, 5, 7, 35
    heat = rng.uniform(1e-4, 1 - 1e-4, (B, nc, H, W)).astype(F32)
    heat[0, 1, 2, 3], heat[1, 0, 0, 0], heat[1, 2, 4, 6] = np.nan, np.inf, -1.0
    reg = rng.standard_normal((B, 10, H, W)).astype(F32)
    reg[0, 3:6] = 100.0      # expf overflows
    reg[1, 0] = 0.0          # depth = depth_ref[0] = -1e-7 below
    reg[1, 8, 1] = np.inf
    reg[0, 1, 0] = -np.inf
    cam = sweep_camera(B, H, W, nc)
    cam["K"][1] = [[700, 0, 0], [0, 700, 0], [0, 0, 1]]
    cam["depth_ref"] = np.array([-1e-7, 1.0], F32)
    for mode in ("forward", "export"):
        cfg = dict(max_detection=K, det_threshold=0.1, mode=mode)
        want = sn.post_process(heat, reg, cam, cfg)
        same_results(from_maps(heat, reg, cam, cfg), want, f"hostile maps {mode}")
    assert np.isinf(want[0][0, :, 6:9]).any() and (want[0][1, :, 11] == F32(-1e-7)).all()


# ---- further checks -----------------------------------------------------------------------------------------------------
def test_norm_tables():
    """The tables through the lazy head's own outputs are covered by the sweeps; here the statistics alone, through a
    head whose class branch passes the normalised value on: a constant map (variance 0) and a map with mean >> spread
    against the restatement (whose double accumulation tests/test_smoke_cpu.py holds to a float64 two-pass reference)."""
    rng = np.random.default_rng(5)
    B, C, H, W, G = 2, 32, 9, 11, 8
    cf = (1000.0 + rng.standard_normal((B, C, H, W))).astype(F32)
    cf[1, :4] = 3.25
    rf = np.full((B, C, H, W), -7.5, F32)
    cam, cfg = sweep_camera(B, H, W, 3), dict(max_detection=50, det_threshold=0.2, mode="export")
    check_both(cf, rf, sweep_state(rng, C, 3), cam, cfg, G, "tables")
    t = sn.stats_tables(rf, G)
    assert (t[:, 0] == F32(-7.5)).all() and (t[:, 1] == F32(1.0 / np.sqrt(1e-5))).all()


def test_frame_alone_elsewhere_and_on_a_side_stream():
    rng = np.random.default_rng(31)
    B, C, H, W, nc = 3, 48, 6, 10, 3
    cf, rf = (rng.standard_normal((B, C, H, W)).astype(F32) for _ in range(2))
    st, cam = sweep_state(rng, C, nc), sweep_camera(B, H, W, nc)
    cfg = dict(max_detection=20, det_threshold=0.3, mode="forward")
    rows, counts = lazy(cf, rf, st, cam, cfg, 16)
    one = {k: (v[1:2] if k in ("K", "trans_mat") else v) for k, v in cam.items()}
    alone = lazy(cf[1:2], rf[1:2], st, one, cfg, 16)
    assert torch.equal(alone[0][0], rows[1]) and torch.equal(alone[1][0], counts[1])
    perm = [2, 1, 0]
    moved = lazy(cf[perm], rf[perm], st, {k: (v[perm] if k in ("K", "trans_mat") else v) for k, v in cam.items()}, cfg, 16)
    assert torch.equal(moved[0][1], rows[1]) and torch.equal(moved[0][0], rows[2])
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        on_side = lazy(cf, rf, st, cam, cfg, 16)
    side.synchronize()
    assert torch.equal(on_side[0], rows) and torch.equal(on_side[1], counts)


def test_refused_shapes_return_none_and_the_module_falls_back():
    from paddle3d_amd import smoke as S

    rng = np.random.default_rng(41)
    B, C, H, W = 1, 32, 5, 7
    cf, rf = (rng.standard_normal((B, C, H, W)).astype(F32) for _ in range(2))
    cfg = dict(max_detection=6, det_threshold=0.3, mode="forward")
    assert lazy(cf, rf, sweep_state(rng, C, 17), sweep_camera(B, H, W, 17), cfg, 32) is None          # 17 classes
    assert lazy(cf, rf, sweep_state(rng, C, 3), sweep_camera(B, H, W, 3), dict(cfg, max_detection=36), 32) is None
    assert lazy(cf, rf, sweep_state(rng, C, 3), sweep_camera(B, H, W, 3), cfg, 5) is None              # 32 % 5
    heat = rng.uniform(0.1, 0.9, (B, 17, H, W)).astype(F32)
    assert from_maps(heat, rng.standard_normal((B, 10, H, W)).astype(F32), sweep_camera(B, H, W, 17), cfg) is None
    # the module with 17 classes runs the torch transcription on the device: the same rows as on the CPU
    torch.manual_seed(3)
    head = S.SMOKEPredictor(num_classes=17, num_channels=32, in_channels=8)
    model = S.SMOKE(torch.nn.Identity(), head, (28.01, 16.32), [sn.DIM_REF[i % 3] for i in range(17)], max_detection=6).eval()
    x = torch.from_numpy(rng.standard_normal((B, 8, H, W)).astype(F32))
    cam = sweep_camera(B, H, W, 17)
    tg = {k: torch.from_numpy(cam[k]) for k in ("K", "trans_mat", "image_size")}
    with torch.no_grad(), launch_ledger(_lib.lib(), _lib.symbols("test_memory_safety_smoke_gpu")) as calls:
        want = model.head_padded(x, targets=tg)
        got = model.to(DEV).head_padded(x.to(DEV), targets={k: v.to(DEV) for k, v in tg.items()})
    assert not calls["pd3_smoke_head_forward"] and not calls["pd3_smoke_post_process"]
    assert torch.equal(got[1].cpu(), want[1]) and torch.equal(got[0][..., 0].cpu(), want[0][..., 0])
    assert torch.allclose(got[0].cpu(), want[0], rtol=1e-4, atol=1e-3)


def test_no_host_synchronisation_and_launch_counts():
    tag = "gn256"  # 64 -> 2 x 256 at 12 x 40: the stacked Winograd launch
    model, cam = cpu.build_model(tag).to(DEV), cpu.camera_tensors(tag, DEV)
    x = torch.from_numpy(sn.golden_inputs(tag)).to(DEV)
    tg = dict(K=cam["K"], trans_mat=cam["trans_mat"], image_size=cam["image_size"])
    L = _lib.lib()
    with torch.no_grad():
        model.head_padded(x, targets=tg, fused="lazy")  # packs the weights
        for fused, op in (("lazy", "pd3_smoke_head_forward"), ("dense", "pd3_smoke_post_process")):
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                with launch_ledger(L, WATCHED) as calls:
                    model.head_padded(x, targets=tg, fused=fused)
                    model.head_padded(x, cam_info=[cam["K"], cam["down_ratios"]], fused=fused)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            ran = {k: v for k, v in calls.items() if v}
            assert ran == {"pd3_smoke_head_workspace": 2, op: 2, "pd3_conv3x3_winograd43_bias_relu": 2}, (fused, ran)


def test_forward_synchronises_exactly_once():
    tag = "gn32"
    model, cam = cpu.build_model(tag).to(DEV), cpu.camera_tensors(tag, DEV)
    x = torch.from_numpy(sn.golden_inputs(tag)).to(DEV)
    tg = dict(K=cam["K"], trans_mat=cam["trans_mat"], image_size=cam["image_size"])
    with torch.no_grad():
        pred = model.heads(x)
        model.post_process(pred, tg)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                res = model.post_process(pred, tg)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in seen if "synchroniz" in str(w.message)]
    assert len(syncs) == 1, [str(w.message) for w in seen]
    assert res.dim() == 2 and res.shape[1] == 15 and res.shape[0] > 0
