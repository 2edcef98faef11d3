"""IA-SSD on the device (csrc/iassd.hip, paddle3d_amd/ops/iassd.py, paddle3d_amd/iassd.py) against the NumPy restatement
tests/golden/iassd_numpy.py: pd3_sa_msg_pool and pd3_iassd_decode bit for bit (a NaN equals a NaN), on seeded sweeps of
the smallest shapes that can break them (the tile of 16 slots, the pass of 64 rows = 4 / 2 / 1 queries, the 64-point
scan step, the narrow / wide split of the layers at 64 columns), and the modules over them."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import iassd_numpy as ia  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
RADIUS = 0.8


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def weights(rng, c0, widths):
    """The scale's parameters in the kernel's form: (w_pos, scale1, shift1, w2, scale2, shift2, w3, scale3, shift3)."""
    c1, c2, c3 = widths
    out = [rng.standard_normal((c1, 3)).astype(F32)]
    for cin, cout in ((None, c1), (c1, c2), (c2, c3)):
        if cin is not None:
            out.append((rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(F32))
        out += [rng.uniform(0.5, 1.5, cout).astype(F32), rng.normal(0, 0.3, cout).astype(F32)]
    return out


def scene(rng, B, m, n, nsample, hits=None, radius=RADIUS):
    """Queries 10 apart on a line; query q of a frame gets hits[q % len(hits)] points within the radius while points
    last, the rest lie far away; the point order is shuffled (the first nsample hits in INDEX order are taken)."""
    S = nsample
    hits = [0, 1, S - 1, S, S + 1] if hits is None else hits
    q = np.zeros((B, m, 3), F32)
    q[:, :, 0] = 10.0 * np.arange(m)
    q += rng.uniform(-0.5, 0.5, q.shape).astype(F32)
    p = np.zeros((B, n, 3), F32)
    for b in range(B):
        rows, k = [], 0
        for i in range(m):
            h = min(max(hits[(i + b) % len(hits)], 0), n - k)
            v = rng.standard_normal((h, 3))
            v *= (radius * 0.9 * rng.uniform(0.05, 1.0, (h, 1)) / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-6))
            rows.append(q[b, i] + v.astype(F32))
            k += h
        far = rng.uniform(-1, 1, (n - k, 3)).astype(F32) + np.array([0, 500.0, 0], F32)
        p[b] = np.concatenate(rows + [far])[rng.permutation(n)]
    return q, p


def run(q, p, f, w, nsample, radius=RADIUS, **kw):
    from paddle3d_amd.ops import iassd as ops

    return ops.sa_msg_pool(_t(q), _t(p), _t(f), *[_t(x) for x in w], radius, nsample, **kw)


def check(q, p, f, w, nsample, radius=RADIUS):
    got = run(q, p, f, w, nsample, radius).cpu().numpy()
    want = ia.sa_msg_pool(q, p, f, *w, radius, nsample)
    bad = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])
    return got


WIDTHS = [(16, 16, 16), (16, 256, 16), (256, 16, 256), (64, 96, 128), (128, 256, 256), (48, 48, 48)]


@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "x".join(map(str, w)))
def test_sa_msg_pool_widths(widths):
    rng = np.random.default_rng(sum(widths))
    q, p = scene(rng, 2, 9, 129, 16)
    f = rng.standard_normal((2, 129, widths[0])).astype(F32)
    got = check(q, p, f, weights(rng, 0, widths), 16)
    assert np.isfinite(got).all() and (got > 0).any()


@pytest.mark.parametrize("nsample", [1, 15, 16, 17, 32, 33, 64])
@pytest.mark.parametrize("m", [1, 5])
def test_sa_msg_pool_nsample_and_pass_borders(nsample, m):
    """m = 1 and m = 5 leave a partial pass at every queries-per-pass (4, 2, 1); the hit counts 0, 1, nsample - 1,
    nsample, nsample + 1 rotate over the queries and the frames."""
    rng = np.random.default_rng(100 * nsample + m)
    B = 1 + nsample % 3
    widths = (16, 64, 48)  # layer 2 wide (a wave per column tile), layer 3 narrow (a wave per row tile)
    q, p = scene(rng, B, m, 200, nsample)
    f = rng.standard_normal((B, 200, 16)).astype(F32)
    check(q, p, f, weights(rng, 0, widths), nsample)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_sa_msg_pool_scan_borders(n):
    """The 64-point scan step; every point of the frame a hit (radius 1e3), with and without features."""
    rng = np.random.default_rng(n)
    w = weights(rng, 0, (32, 16, 64))
    for m, S in ((3, 16), (4, 32), (2, 64)):
        q, p = scene(rng, 2, m, n, S)
        f = rng.standard_normal((2, n, 32)).astype(F32)
        check(q, p, f, w, S)
        check(q, p, None, w, S)
        check(q, p, f, w, S, radius=1e3)


def test_sa_msg_pool_nonfinite():
    rng = np.random.default_rng(7)
    w = weights(rng, 0, (16, 32, 64))
    q, p = scene(rng, 2, 6, 100, 16, hits=[5, 16, 20])
    f = rng.standard_normal((2, 100, 16)).astype(F32)
    idx = ia.pn.ball_query(q, p, RADIUS, 16)
    p2, f2, q2 = p.copy(), f.copy(), q.copy()
    p2[0, idx[0, 0, 1]] = np.nan       # a NaN point is no hit: the row shifts
    f2[0, idx[0, 1, 2], 3] = np.nan    # a NaN feature reaches the pooled row
    f2[1, idx[1, 2, 0], 0] = np.inf
    q2[1, 4] = np.inf                  # an infinite query has no hit: point 0 with d = -inf
    got = check(q2, p2, f2, w, 16)
    assert np.isnan(got[0, 1]).any() and np.isfinite(got[0, 0]).all()
    assert not same_bits(got[0, 0], check(q, p, f, w, 16)[0, 0])


def test_sa_msg_pool_two_scales_into_one_buffer():
    """ld_out > c3 with a column offset: both scales of a layer into one [B, m, c3a + 5 + c3b] buffer; the five
    columns between them and nothing else keep their pattern."""
    rng = np.random.default_rng(11)
    q, p = scene(rng, 2, 7, 150, 16, hits=[3, 0, 16, 40])
    f = rng.standard_normal((2, 150, 16)).astype(F32)
    wa, wb = weights(rng, 0, (16, 16, 32)), weights(rng, 0, (16, 32, 48))
    out = torch.full((2, 7, 32 + 5 + 48), -7.0, device=DEV)
    assert run(q, p, f, wa, 16, out=out) is out
    run(q, p, f, wb, 32, radius=2 * RADIUS, out=out, col=37)
    got = out.cpu().numpy()
    assert same_bits(got[..., :32], ia.sa_msg_pool(q, p, f, *wa, RADIUS, 16))
    assert same_bits(got[..., 37:], ia.sa_msg_pool(q, p, f, *wb, 2 * RADIUS, 32))
    assert (got[..., 32:37] == -7.0).all()


def test_sa_msg_pool_position_in_the_launch():
    """A frame alone, elsewhere in the batch and on a side stream gives the same bits."""
    rng = np.random.default_rng(13)
    w = weights(rng, 0, (64, 96, 128))
    q, p = scene(rng, 3, 5, 90, 32)
    f = rng.standard_normal((3, 90, 64)).astype(F32)
    whole = run(q, p, f, w, 32).cpu().numpy()
    alone = run(q[1:2], p[1:2], f[1:2], w, 32).cpu().numpy()
    assert same_bits(whole[1:2], alone)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        side = run(q[::-1].copy(), p[::-1].copy(), f[::-1].copy(), w, 32)
    s.synchronize()
    assert same_bits(whole[::-1], side.cpu().numpy())


def test_sa_msg_pool_refusals_and_empty():
    from paddle3d_amd._lib import Paddle3DAmdError
    from paddle3d_amd.ops import iassd as ops

    rng = np.random.default_rng(3)
    q, p = scene(rng, 1, 2, 10, 4)
    for widths in ((32, 32, 272), (16, 8, 16), (24, 16, 16)):
        assert not ops.sa_msg_pool_supported(*widths, 4)
        with pytest.raises(Paddle3DAmdError, match="unsupported"):
            run(q, p, None, weights(rng, 0, widths), 4)
    w = weights(rng, 0, (16, 16, 16))
    with pytest.raises(Paddle3DAmdError, match="unsupported"):
        run(q, p, None, w, 65)
    with pytest.raises(RuntimeError, match="nsample"):
        run(q, p, None, w, 0)
    with pytest.raises(RuntimeError, match="columns"):
        run(q, p, None, w, 4, out=torch.zeros((1, 2, 20), device=DEV), col=8)
    assert tuple(run(q[:, :0], p, None, w, 4).shape) == (1, 0, 16)
    assert tuple(run(q[:0], p[:0], None, w, 4).shape) == (0, 2, 16)


# ---- iassd_decode -------------------------------------------------------------------------------------------------
MEAN_SIZE = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], F32)


def decode_case(rng, M, bins, K=3):
    cls = rng.standard_normal((M, K)).astype(F32)
    box = rng.standard_normal((M, 6 + 2 * bins)).astype(F32)
    ctr = rng.uniform(-40, 40, (M, 4)).astype(F32)
    return cls, box, ctr


def check_decode(cls, box, ctr4, mean_size, bins):
    from paddle3d_amd.ops import iassd as ops

    got = ops.iassd_decode(_t(cls), _t(box), _t(ctr4)[:, 1:4], _t(mean_size), bins).cpu().numpy()
    want = ia.iassd_decode(cls, box, ctr4[:, 1:4], mean_size, bins)
    assert same_bits(got, want), (got[~(got == want)][:4], want[~(got == want)][:4])
    return got


@pytest.mark.parametrize("bins", [1, 12])
@pytest.mark.parametrize("M", [1, 300])
@pytest.mark.parametrize("use_mean_size", [True, False])
def test_iassd_decode(bins, M, use_mean_size):
    rng = np.random.default_rng(1000 * bins + M)
    cls, box, ctr = decode_case(rng, M, bins)
    got = check_decode(cls, box, ctr, MEAN_SIZE if use_mean_size else None, bins)
    assert np.isfinite(got).all()


def test_iassd_decode_special_rows():
    rng = np.random.default_rng(5)
    bins = 12
    cls, box, ctr = decode_case(rng, 16, bins)
    cls[0] = (1.5, 1.5, 0.0)               # tied logits: the first maximum
    cls[1] = (0.0, 2.0, 2.0)
    cls[2] = (40.0, 50.0, 30.0)            # saturated: sigmoid is 1 for 0 and 1, the label is 0, the class here 1
    cls[3] = (0.0, np.nan, 9.0)            # a NaN counts as the maximum
    cls[4] = (np.nan, np.nan, 1.0)
    cls[5] = (-np.inf, -np.inf, -np.inf)
    box[6, 6:6 + bins] = 0.25              # tied bins: bin 0
    box[7, 6 + 3] = np.nan                 # a NaN bin logit: bin 3
    box[8, 3:6] = (100.0, 88.8, -200.0)    # exp overflow and underflow
    box[9, 3:6] = (np.nan, np.inf, -np.inf)
    box[10, 6 + bins + 4] = np.inf         # an infinite residual that is not selected ...
    box[10, 6 + 4] = -50.0
    box[11, 6 + 5], box[11, 6 + bins + 5] = 50.0, np.inf  # ... and one that is
    got = check_decode(cls, box, ctr, MEAN_SIZE, bins)
    check_decode(cls, box, ctr, None, bins)
    sig = 1 / (1 + np.exp(-cls[2].astype(np.float64))).astype(F32)
    assert int(np.argmax(sig)) == 0 and same_bits(got[2, 3:6], ia.expf(box[2, 3:6]) * MEAN_SIZE[1])
    assert same_bits(got[3, 3:6], ia.expf(box[3, 3:6]) * MEAN_SIZE[1]) and same_bits(got[4, 3:6], ia.expf(box[4, 3:6]) * MEAN_SIZE[0])
    assert np.isinf(got[8, 3]) and np.isinf(got[8, 4]) and got[8, 5] == 0 and np.isfinite(got[10, 6]) and np.isinf(got[11, 6])


def test_iassd_decode_refusals_and_empty():
    from paddle3d_amd.ops import iassd as ops

    cls, box, ctr = decode_case(np.random.default_rng(1), 4, 12)
    with pytest.raises(RuntimeError, match="box_preds"):
        ops.iassd_decode(_t(cls), _t(box), _t(ctr)[:, 1:4], None, 11)
    with pytest.raises(RuntimeError, match="mean_size"):
        ops.iassd_decode(_t(cls), _t(box), _t(ctr)[:, 1:4], _t(MEAN_SIZE[:2]), 12)
    assert tuple(ops.iassd_decode(_t(cls[:0]), _t(box[:0]), _t(ctr[:0, 1:4]), None, 12).shape) == (0, 7)


# ---- the golden cases and the modules -------------------------------------------------------------------------------
import make_iassd_golden as mk  # noqa: E402
import test_iassd_cpu as tc  # noqa: E402
from guarded import launch_ledger  # noqa: E402

_GOLDEN = {}


def golden():
    if not _GOLDEN:
        g = mk.load()
        _GOLDEN.update(g=g, backbone=mk.state(g, "backbone"), head=mk.state(g, "head"))
    return _GOLDEN["g"], _GOLDEN["backbone"], _GOLDEN["head"]


def _err(t, a):
    return float(np.abs(t.detach().cpu().numpy() - a).max())


def model(fused):
    g, st_b, st_h = golden()
    return tc.build(g, st_b, st_h, fused=fused).to(DEV)


@pytest.mark.parametrize("i", tc.SA_LAYERS)
def test_sa_msg_pool_on_the_golden_layers(i):
    """Each scale of each recorded layer, features_in formed on the device as the module forms it: bit for bit."""
    g, st, _ = golden()
    xyz, new_xyz = g[f"l{i}_in_xyz"], g[f"l{i}_out_new_xyz"] if i != 5 else g["l5_in_ctr_xyz"]
    for k, (r, s) in enumerate(zip(mk.BACKBONE["radius_list"][i], mk.BACKBONE["nsample_list"][i])):
        w_pos, w_feat, rest = ia.scale_params(st, f"SA_modules.{i}", k)
        f_in = torch.matmul(_t(g[f"l{i}_in_features"]).transpose(1, 2), _t(w_feat).t()).contiguous().cpu().numpy()
        check(new_xyz, xyz, f_in, [w_pos] + rest, s, radius=r)


def test_iassd_decode_on_the_golden():
    g = golden()[0]
    check_decode(g["head_batch_cls_preds"], g["head_center_box_preds"], g["head_centers"], np.asarray(mk.MEAN_SIZE, F32), 12)
    check_decode(g["head_batch_cls_preds"], g["head_center_box_preds"], g["head_centers"], None, 12)


@pytest.mark.parametrize("fused", ["force", True, False], ids=str)
def test_modules_against_the_golden_layers(fused):
    """Every layer from its recorded inputs within 4 x the reference's own fp32 error, the head likewise."""
    g = golden()[0]
    m = model(fused)
    with torch.no_grad():
        for i, layer in enumerate(m.backbone.SA_modules):
            a = {k: _t(g[f"l{i}_in_{k}"]) for k in ("xyz", "features", "cls_features", "ctr_xyz") if f"l{i}_in_{k}" in g}
            if i == 4:
                vote, _, _, off = layer(a["xyz"], a["features"])
                assert _err(vote, g["l4_out_vote_xyz"]) <= float(g["l4_out_vote_xyz_bound"])
                assert _err(off, g["l4_out_ctr_offsets"]) <= float(g["l4_out_ctr_offsets_bound"])
                continue
            new_xyz, feats, cls = layer(**a)
            assert np.array_equal(new_xyz.cpu().numpy(), g[f"l{i}_out_new_xyz"] if i != 5 else g["l5_in_ctr_xyz"])
            err = _err(feats, g[f"l{i}_out_new_features"])
            print(fused, i, "error", err, "bound", float(g[f"l{i}_out_new_features_bound"]))
            assert err <= float(g[f"l{i}_out_new_features_bound"])
            if f"l{i}_out_cls_features" in g:
                assert _err(cls, g[f"l{i}_out_cls_features"]) <= float(g[f"l{i}_out_cls_features_bound"])
        bd = m.head({k: _t(g[f"head_{k}"]) for k in ("centers_features", "centers", "ctr_offsets", "centers_origin")}
                    | {"sa_ins_preds": []})
    for k in ("batch_cls_preds", "batch_box_preds"):
        assert _err(bd[k], g[f"head_{k}"]) <= float(g[f"head_{k}_bound"]), k


def _lists_equal(preds, g, tag, box_tol, score_tol):
    for b, d in enumerate(preds):
        want_l = g[f"{tag}_labels{b}"]
        assert d["pred_labels"].cpu().numpy().astype(np.float32).tolist() == want_l.tolist(), (tag, b)  # count and order too
        assert float(np.abs(d["pred_boxes"].cpu().numpy() - g[f"{tag}_boxes{b}"]).max()) <= box_tol, (tag, b)
        assert float(np.abs(d["pred_scores"].cpu().numpy() - g[f"{tag}_scores{b}"]).max()) <= score_tol, (tag, b)


@pytest.mark.parametrize("fused", ["force", False], ids=str)
def test_whole_model_on_the_golden_input(fused):
    """Labels, counts and row order equal; boxes within the end-to-end bound (4 x the reference's own fp32 error
    against its fp64 run from the points on); scores within the logits' end-to-end bound (a sigmoid's slope is at most
    1 / 4) plus one rounding of a value below 1."""
    g = golden()[0]
    m = model(fused)
    box_tol = float(g["e2e_batch_box_preds_bound"])
    score_tol = float(g["e2e_batch_cls_preds_bound"]) / 4 + 2.0 ** -24
    from paddle3d_amd import _lib

    with launch_ledger(_lib.lib(), _lib.symbols("test_memory_safety_iassd_gpu")) as calls:
        preds = m({"data": _t(g["data"]), "batch_size": mk.B}, as_list=True)
    _lists_equal(preds, g, "post", box_tol, score_tol)
    assert calls == {"pd3_sa_msg_pool": 8 if fused == "force" else 0, "pd3_iassd_decode": 1}
    boxes, scores, labels, count = m({"data": _t(g["data"]), "batch_size": mk.B})
    assert count.tolist() == [len(g[f"post_scores{b}"]) for b in range(mk.B)] and tuple(boxes.shape) == (mk.B, 500, 7)
    for b in range(mk.B):
        assert torch.equal(boxes[b, :count[b]], preds[b]["pred_boxes"]) and not boxes[b, count[b]:].any()
        assert labels.dtype == torch.int64 and not scores[b, count[b]:].any()


def test_empty_frame_gets_the_fake_row():
    g = golden()[0]
    m = model("force")
    bd = {"batch_size": mk.B, "batch_box_preds": _t(g["head_batch_box_preds"]), "batch_index": _t(g["head_batch_index"]),
          "batch_cls_preds": _t(g["empty_batch_cls_preds"]), "cls_preds_normalized": False}
    preds = m.post_process(bd, as_list=True)
    _lists_equal(preds, g, "empty", 0.0, 2.0 ** -24)
    assert preds[1]["pred_labels"].tolist() == [-1.0] and preds[1]["pred_scores"].tolist() == [0.0]
    assert not preds[1]["pred_boxes"].any() and tuple(preds[1]["pred_boxes"].shape) == (1, 7)
    assert m.post_process(bd)[3].tolist() == [len(g["empty_scores0"]), 0]


def test_no_host_sync():
    g = golden()[0]
    m = model("force")
    data = _t(g["data"])
    with torch.no_grad():
        m({"data": data, "batch_size": mk.B})  # folds the BatchNorms, loads the library
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            bd = m.head(m.backbone({"data": data, "batch_size": mk.B}))
            out = m.post_process(bd)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert int(out[3].sum()) > 0


def test_refused_shapes_take_the_composition():
    """A scale the kernel refuses (width 24, nsample 65) under fused="force": the composition, equal to fused=False's."""
    from paddle3d_amd import iassd

    torch.manual_seed(3)
    kw = dict(npoint=16, sample_range=-1, sample_type="D-FPS", radii=[0.9, 1.5, 1.5], nsamples=[16, 16, 65],
              aggregation_mlp=[32], confidence_mlp=[16], num_classes=3)
    mlps = [[2, 16, 16, 32], [2, 16, 24, 32], [2, 16, 16, 16]]
    a = iassd.SAModuleMSG_WithSampling(mlps=[list(x) for x in mlps], fused="force", **kw).to(DEV).eval()
    b = iassd.SAModuleMSG_WithSampling(mlps=[list(x) for x in mlps], fused=False, **kw).to(DEV).eval()
    for mod in a.modules():
        if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
            mod.running_mean.normal_(0, 0.1)
            mod.running_var.uniform_(0.5, 1.5)
    b.load_state_dict(a.state_dict())
    assert [a.scale_is_fused(i) for i in range(3)] == [True, False, False]
    xyz, feats = torch.rand(2, 100, 3, device=DEV) * 4, torch.randn(2, 2, 100, device=DEV)
    from paddle3d_amd import _lib
    with torch.no_grad(), launch_ledger(_lib.lib(), _lib.symbols("test_memory_safety_iassd_gpu")) as calls:
        ra, rb = a(xyz, feats), b(xyz, feats)
    assert calls["pd3_sa_msg_pool"] == 1 and torch.equal(ra[0], rb[0])
    for x, y in zip(ra[1:], rb[1:]):
        assert x.shape == y.shape and float((x - y).abs().max()) <= 1e-5 * float(y.abs().max())
    a.train()
    assert a(xyz, feats)[1].shape == ra[1].shape  # training mode: the composition, batch statistics
