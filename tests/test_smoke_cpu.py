"""SMOKE's head and post-processing without a GPU: the NumPy restatement of csrc/smoke.hip (tests/golden/smoke_numpy.py)
and the module's torch fall-back against the reference's own Python (tests/golden/python_smoke.npz, written by
tests/golden/make_smoke_golden.py) within the stored per-column bounds, with classes, counts and row order equal; the
single exact top-K against the reference's two topk stages on maps with heavy ties; state-dict keys and a strict load of
a synthetic .pdparams; the predicate's borders; the C ABI's statuses."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import smoke_numpy as sn  # noqa: E402

F32 = np.float32
GOLDEN = os.path.join(HERE, "golden", "python_smoke.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def conv3x3_outputs(tag):
    """The two branches' 3x3 convolution outputs of the golden case by torch's convolution on the CPU (float32)."""
    st, x = sn.golden_state(tag), torch.from_numpy(sn.golden_inputs(tag))
    return tuple(torch.nn.functional.conv2d(x, torch.from_numpy(st[f"{h}.0.weight"]), torch.from_numpy(st[f"{h}.0.bias"]),
                                            padding=1).numpy() for h in ("class_head", "regression_head"))


def restated(tag):
    """(rows, counts) of the restatement on a golden case, from the conv outputs above."""
    c, st = sn.CASES[tag], sn.golden_state(tag)
    cf, rf = conv3x3_outputs(tag)
    tables = None
    if c["norm"] == "bn":
        tables = tuple(sn.bn_tables(st, f"{h}.1", c["B"]) for h in ("class_head", "regression_head"))
    (rows, counts), _ = sn.head_forward(cf, rf, st, sn.golden_camera(tag), sn.cfg_of(tag), sn.groups_of(tag), tables)
    return rows, counts


def build_model(tag, fused=True):
    """paddle3d_amd.smoke.SMOKE with an identity backbone and the golden case's state, loaded under the reference's names."""
    from paddle3d_amd import smoke as S
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    c = sn.CASES[tag]
    head = S.SMOKEPredictor(num_classes=c["nc"], num_channels=c["C"], norm_type=c["norm"], in_channels=c["Cin"])
    model = S.SMOKE(torch.nn.Identity(), head, depth_ref=(28.01, 16.32), dim_ref=sn.DIM_REF[:c["nc"]],
                    max_detection=c["K"], fused=fused)
    model.post_process.det_threshold = c["thr"]
    load_paddle_state_dict(model, {"heads." + k: v for k, v in sn.golden_state(tag).items()}, strict=True)
    return model.eval()


def camera_tensors(tag, device="cpu"):
    cam = sn.golden_camera(tag)
    return {k: torch.from_numpy(v).to(device) for k, v in cam.items()}


def run_model(model, tag, device="cpu", fused=None):
    """(rows [B, K, 14], counts) of the module on a golden case."""
    cam = camera_tensors(tag, device)
    x = torch.from_numpy(sn.golden_inputs(tag)).to(device)
    with torch.no_grad():
        if sn.CASES[tag]["mode"] == "forward":
            return model.head_padded(x, targets=dict(K=cam["K"], trans_mat=cam["trans_mat"], image_size=cam["image_size"]),
                                     fused=fused)
        return model.head_padded(x, cam_info=[cam["K"], cam["down_ratios"]], fused=fused)


def check_against_golden(tag, rows, counts, G, what):
    """rows [B, K, 14] / counts against the reference's result: the same rows in the same order, class column equal,
    every other column within its stored bound; prints the largest difference per column in units of the bound."""
    c = sn.CASES[tag]
    rows, counts = np.asarray(rows, F32), np.asarray(counts)
    ref = G[f"{tag}_rows"]
    if c["mode"] == "forward":
        got = np.concatenate([np.concatenate([rows[b, :counts[b]], np.full((counts[b], 1), b, F32)], 1)
                              for b in range(c["B"])])
        want_counts = [int((ref[:, 14] == b).sum()) for b in range(c["B"])]
        assert (rows[np.arange(c["K"])[None] >= counts[:, None]] == 0).all(), f"{what} {tag}: rows past the count"
    else:
        got, want_counts = rows.reshape(-1, 14), [c["K"]] * c["B"]
    assert list(counts) == want_counts, (what, tag, list(counts), want_counts)
    assert got.shape == ref.shape, (what, tag, got.shape, ref.shape)
    assert np.array_equal(got[:, 0], ref[:, 0]), f"{what} {tag}: classes / row order differ"
    if c["mode"] == "forward":
        assert np.array_equal(got[:, 14], ref[:, 14])
    err = np.abs(got[:, :14].astype(np.float64) - ref[:, :14]).max(0) if len(ref) else np.zeros(14)
    print(f"{what} {tag}: err / bound per column", np.array2string(err / G[f"{tag}_bound"], precision=2))
    assert (err <= G[f"{tag}_bound"]).all(), (what, tag, err, G[f"{tag}_bound"])


@pytest.mark.parametrize("tag", sn.TAGS)
def test_restatement_within_the_references_bounds(tag, golden):
    rows, counts = restated(tag)
    check_against_golden(tag, rows, counts, golden, "restatement")


@pytest.mark.parametrize("tag", sn.TAGS)
def test_module_torch_fallback_within_the_references_bounds(tag, golden):
    rows, counts = run_model(build_model(tag), tag)
    check_against_golden(tag, rows.numpy(), counts.numpy(), golden, "torch fall-back")


@pytest.mark.parametrize("tag", ("gn32", "bn256"))
def test_module_forward_returns_the_references_tensor(tag, golden):
    """PostProcessor.forward on CPU tensors: [n, 15] with the batch id, and an empty tensor when nothing passes."""
    model, cam = build_model(tag), camera_tensors(tag)
    x = torch.from_numpy(sn.golden_inputs(tag))
    with torch.no_grad():
        res = model.post_process(model.heads(x), dict(K=cam["K"], trans_mat=cam["trans_mat"], image_size=cam["image_size"]))
        assert tuple(res.shape) == golden[f"{tag}_rows"].shape
        assert np.array_equal(res[:, 14].numpy(), golden[f"{tag}_rows"][:, 14])
        model.post_process.det_threshold = 2.0
        none = model.post_process(model.heads(x), dict(K=cam["K"], trans_mat=cam["trans_mat"], image_size=cam["image_size"]))
        assert none.numel() == 0
        preds = model.test_forward(dict(data=x, target=dict(K=cam["K"], trans_mat=cam["trans_mat"],
                                                            image_size=cam["image_size"])))["preds"]
        assert len(preds) == x.shape[0] and all("labels" not in p for p in preds)


def tie_maps():
    """Seeded heat maps with heavy ties: saturated plateaus, an all-equal map, fewer than K peaks, a NaN pixel."""
    rng = np.random.default_rng(77)
    out = []
    for nc, H, W in ((3, 6, 9), (1, 4, 4), (4, 5, 7), (2, 1, 13)):
        h = rng.choice(np.array([1e-4, 0.25, 0.5, 1 - 1e-4], F32), size=(nc, H, W))
        out.append(("plateaus", h.copy()))
        out.append(("all equal", np.full((nc, H, W), 0.5, F32)))
        few = np.full((nc, H, W), 1e-4, F32)
        few[0, H // 2, W // 2] = 0.9
        few[-1, 0, 0] = 0.9
        out.append(("few peaks", few))
        h[0, 0, 0] = np.nan
        out.append(("nan", h))
    return out


def test_single_topk_equals_the_two_stage_topk_on_ties():
    for name, h in tie_maps():
        hw = h.shape[1] * h.shape[2]
        for K in sorted({1, 2, 5, hw}):
            i1, s1 = sn.select(h, K)
            i2, s2 = sn.select_two_stage(h, K)
            assert np.array_equal(i1, i2) and np.array_equal(s1, s2), (name, h.shape, K, i1, i2)


def test_restated_tables_against_float64_two_pass():
    """The double accumulation in the kernel's order on a map whose mean is far above its spread, and on a constant map:
    mean and rstd within one float32 ulp of a float64 two-pass reference (they are rounded once from double)."""
    rng = np.random.default_rng(5)
    x = (1000.0 + rng.standard_normal((2, 32, 9, 11))).astype(F32)
    x[1, :4] = 3.25  # a constant group: variance 0
    t = sn.stats_tables(x, 8)
    g = x.astype(np.float64).reshape(2, 8, -1)
    mean = g.mean(-1)
    rstd = 1.0 / np.sqrt(((g - mean[..., None]) ** 2).mean(-1) + 1e-5)
    assert (np.abs(t[:, 0] - mean) <= np.spacing(np.abs(mean).astype(F32))).all()
    assert (np.abs(t[:, 1] - rstd) <= np.spacing(rstd.astype(F32))).all()
    assert t[1, 0, 0] == F32(3.25) and t[1, 1, 0] == F32(1.0 / np.sqrt(1e-5))
    # a float32 running sum would not: its mean is off by far more than an ulp at this size
    from paddle3d_amd.ops.smoke import group_norm_tables

    assert torch.equal(group_norm_tables(torch.from_numpy(x), 8), torch.from_numpy(t))


def test_state_dict_keys_and_strict_load(tmp_path):
    from paddle3d_amd import smoke as S
    from paddle3d_amd.checkpoint import load_paddle_state_dict, save_pdparams

    for norm in ("gn", "bn"):
        model = S.SMOKE(torch.nn.Identity(), S.SMOKEPredictor(num_channels=32, norm_type=norm, in_channels=8),
                        depth_ref=(28.01, 16.32), dim_ref=sn.DIM_REF)
        keys = {k for k in model.state_dict() if not k.endswith("num_batches_tracked")}
        want = {f"heads.{h}.{i}.{p}" for h in ("class_head", "regression_head") for i in (0, 1, 3) for p in ("weight", "bias")}
        if norm == "bn":
            want |= {f"heads.{h}.1.running_{s}" for h in ("class_head", "regression_head") for s in ("mean", "var")}
        assert keys == want
        rng = np.random.default_rng(3)
        state = {k.replace("running_mean", "_mean").replace("running_var", "_variance"):
                 rng.uniform(0.5, 1.5, tuple(v.shape)).astype(F32) for k, v in model.state_dict().items()
                 if not k.endswith("num_batches_tracked")}
        path = str(tmp_path / f"smoke_{norm}.pdparams")
        save_pdparams(state, path)
        assert load_paddle_state_dict(model, path, strict=True) == []
        assert np.array_equal(model.heads.class_head[3].weight.detach().numpy(), state["heads.class_head.3.weight"])
        assert model.heads.class_head[1].num_groups == 32 if norm == "gn" else True
    assert S.group_norm(48).num_groups == 16
    m = S.smoke_dla34_no_dcn_kitti(torch.nn.Identity())
    assert (m.heads.in_channels, m.heads.num_channels, m.max_detection, m.post_process.det_threshold) == (64, 256, 50, 0.25)
    assert S.smoke_hrnet18_no_dcn_kitti(torch.nn.Identity()).heads.in_channels == 270
    assert float(m.heads.class_head[3].bias[0]) == pytest.approx(-2.19)


def test_predicate_borders():
    from paddle3d_amd.ops.smoke import smoke_supported as ok

    assert ok(256, 32, 3, 96, 320, 50)
    assert ok(512, 64, 16, 1, 1, 1) and not ok(513, 1, 3, 8, 8, 4) and not ok(48, 32, 3, 8, 8, 4) and ok(48, 16, 3, 8, 8, 4)
    assert ok(16, 16, 1, 32, 32, 1024) and not ok(16, 16, 1, 32, 32, 1025) and not ok(16, 16, 1, 4, 4, 17)
    assert not ok(16, 16, 1, 4, 4, 0) and not ok(16, 16, 0, 4, 4, 1) and not ok(16, 16, 17, 4, 4, 1)
    assert not ok(16, 16, 3, 4, 4, 4, reg_channels=(1, 2, 3, 2)) and not ok(16, 16, 3, 4, 4, 4, reg_channels=(1, 2, 3, 2, 3))
    assert not ok(16, 16, 3, 4, 4, 4, pred_2d=False)
    assert ok(None, None, 4, 16384, 16383, 50) and not ok(None, None, 4, 16384, 16384, 50)


def test_statuses_without_a_gpu():
    from paddle3d_amd import _lib

    L = _lib.lib()
    reg, bad = (C.c_int * 5)(1, 2, 3, 2, 2), (C.c_int * 5)(1, 2, 3, 2, 3)
    buf = np.zeros(64, F32)
    p = C.c_void_p(buf.ctypes.data)
    assert L.pd3_smoke_head_workspace(2, 5, 7, 3, 6) > 0
    assert L.pd3_smoke_head_workspace(2, 5, 7, 3, 36) == 0 and L.pd3_smoke_head_workspace(2, 5, 7, 17, 6) == 0

    def post(nc=3, h=5, w=7, k=6, regs=reg, mode=0, pred_2d=1, ptrs=p, ws=0, batch=2):
        return L.pd3_smoke_post_process(ptrs, ptrs, ptrs, ptrs, ptrs, ptrs, ptrs, batch, h, w, nc, regs, k, 0.25, mode,
                                        pred_2d, ptrs, ptrs, ptrs, ws, None)

    def head(c=32, g=32, nc=3, h=5, w=7, k=6, regs=reg, pred_2d=1, ptrs=p, ws=0, pitch=None):
        pitch = w if pitch is None else pitch
        return L.pd3_smoke_head_forward(ptrs, ptrs, c * h * pitch, pitch, *([ptrs] * 15), 2, c, g, h, w, nc, regs, k, 0.25,
                                        0, pred_2d, ptrs, ptrs, ptrs, ws, None)

    for f in (post, head):
        assert f(k=0) == -3 and f(k=1025, h=40, w=40) == -3 and f(k=36) == -3 and f(nc=17) == -3 and f(regs=bad) == -3
        assert f(pred_2d=0) == -3
        assert f(ptrs=None) == -1 and f(h=0) == -1
        assert f() == -2  # a workspace of 0 bytes
    assert post(nc=4, h=16384, w=16384, k=50) == -3 and post(mode=2) == -1 and post(batch=0) == 0
    assert head(c=48, g=32) == -3 and head(c=520, g=8) == -3 and head(c=48, g=16) == -2 and head(pitch=6) == -1
