"""SqueezeSegV3 on the CPU, against what the reference's own Python computed (tests/golden/python_squeezeseg.npz, made
by make_squeezeseg_golden.py): the NumPy restatement of pd3_sac_isk_forward (tests/golden/squeezeseg_numpy.py) and the
modules of paddle3d_amd.squeezesegv3 with fused=False (the torch composition, also what a refused shape runs) within the
stored bounds; the modules' state-dict keys against the reference's; the restated range projection against the
reference's pixels, range image and proj_idx exactly, and against a direct transcription of the reader's scatter; the
packers' round trip, the folded BatchNorm against the unfolded one, `sac_isk_supported`'s borders
and the maker's conditions on the committed file.

Bounds: the ones the maker stored, 4 x the largest error of the reference's own fp32 run against its fp64 run (one fp32
ulp of the largest output as a floor).  Predictions, labels, pixels and proj_idx are compared exactly: the maker keeps
every logit gap and pixel coordinate further from a decision than those bounds."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import make_squeezeseg_golden as mk  # noqa: E402
import squeezeseg_numpy as sn  # noqa: E402
from make_squeezeseg_golden import scan  # noqa: E402,F401

F32 = np.float32
EPS32 = float(np.finfo(F32).eps)


@pytest.fixture(scope="module")
def golden():
    return mk.load()


@pytest.fixture(scope="module")
def expf():
    from oracle import pyoracle as O

    return lambda x: O.libm_eval(2, np.ascontiguousarray(x, F32).reshape(-1))


def block_params(C, seed, big_z=False):
    """Seeded weights of one SAC block up to its 1x1 layer: dict(w [9C, 3, 7, 7], s_a, t_a [9C], v [C, 9C], s_m, t_m [C]).
    With big_z a few attention channels get shifts of +-100 and +-200, where expf(-z) overflows and underflows."""
    rng = np.random.default_rng(seed)
    p = dict(w=(rng.standard_normal((9 * C, 3, 7, 7)) / 12.0).astype(F32),
             s_a=rng.uniform(0.5, 1.5, 9 * C).astype(F32), t_a=rng.uniform(-1, 1, 9 * C).astype(F32),
             v=(rng.standard_normal((C, 9 * C)) / np.sqrt(9 * C)).astype(F32),
             s_m=rng.uniform(0.5, 1.5, C).astype(F32), t_m=rng.uniform(-0.5, 0.5, C).astype(F32))
    if big_z:
        p["t_a"][:8] = np.array([100, -100, 200, -200, 88.5, -88.5, 104, -104], F32)
    return p


def block_inputs(N, C, H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, 3, H, W)).astype(F32), rng.standard_normal((N, C, H, W)).astype(F32)


def composition(xyz, feature, p):
    """The block as torch operators on whatever device the inputs are on (float32 or float64 by the inputs' dtype)."""
    from paddle3d_amd.squeezesegv3 import sac_isk_composition

    t = lambda a: torch.as_tensor(a).to(xyz.device, xyz.dtype)  # noqa: E731
    return sac_isk_composition(xyz, feature, t(p["w"]), t(p["s_a"]), t(p["t_a"]), t(p["v"]), t(p["s_m"]), t(p["t_m"]))


def test_packers_round_trip():
    from paddle3d_amd.ops import squeezeseg as ops

    for C in (16, 48, 256):
        rng = np.random.default_rng(C)
        w = torch.from_numpy(rng.standard_normal((9 * C, 3, 7, 7)).astype(F32))
        v = torch.from_numpy(rng.standard_normal((C, 9 * C)).astype(F32))
        pw, pv = ops.pack_sac_attention_weight(w), ops.pack_sac_mlp_weight(v.reshape(C, 9 * C, 1, 1))
        assert tuple(pw.shape) == (9 * C // 16, 37, 64) and tuple(pv.shape) == (9 * C // 16, 4, C // 16, 64)
        assert torch.equal(ops.unpack_sac_attention_weight(pw, C), w)
        assert torch.equal(ops.unpack_sac_mlp_weight(pv, C), v)
        # every weight once, the 148th tap zero; the lane order of the kernel's header
        assert int((pw != 0).sum()) == int((w != 0).sum()) and int((pv != 0).sum()) == int((v != 0).sum())
        T, s, lane = 3, 5, 37
        m, k = lane & 15, lane >> 4
        assert pw[T, s, lane] == w.reshape(9 * C, 147)[16 * T + 4 * (m & 3) + (m >> 2), 4 * s + k]
        assert torch.equal(pw[:, 36, 48:], torch.zeros(9 * C // 16, 16))
        r, ot = 2, C // 16 - 1
        assert pv[T, r, ot, lane] == v[16 * ot + (lane & 15), 16 * T + 4 * r + (lane >> 4)]
    with pytest.raises(RuntimeError):
        ops.pack_sac_attention_weight(torch.zeros(9 * 8, 3, 7, 7))
    with pytest.raises(RuntimeError):
        ops.pack_sac_mlp_weight(torch.zeros(16, 9 * 16 + 1))


def test_supported_borders():
    from paddle3d_amd.ops import squeezeseg as ops

    for C in (16, 32, 48, 64, 128, 240, 256):
        assert ops.sac_isk_supported(C) and ops.sac_isk_supported(C, 1, 1) and ops.sac_isk_supported(C, 64, 1024, 8)
    for C in (0, 8, 15, 17, 24, 255, 257, 272, 512):
        assert not ops.sac_isk_supported(C)
    assert not ops.sac_isk_supported(32, 0, 5) and not ops.sac_isk_supported(32, 5, 0)
    assert ops.sac_isk_supported(32, 1, 16 * (2 ** 30 - 1)) and not ops.sac_isk_supported(32, 1, 16 * (2 ** 30 - 1) + 1)
    assert ops.MAX_CHANNELS == 256


def test_folded_batch_norm_equals_the_unfolded_one():
    from paddle3d_amd.ops.squeezeseg import fold_batch_norm

    rng = np.random.default_rng(3)
    n = 96
    g, b, m = (torch.from_numpy(rng.standard_normal(n).astype(F32)) for _ in range(3))
    var = torch.from_numpy(rng.uniform(0.2, 3.0, n).astype(F32))
    bias = torch.from_numpy(rng.standard_normal(n).astype(F32))
    x = torch.from_numpy(rng.standard_normal((2, n, 3, 5)).astype(F32))
    for bs in (bias, None):
        s, t = fold_batch_norm(g, b, m, var, 1e-5, bs)
        assert s.dtype == torch.float32 and t.dtype == torch.float32
        folded = x * s[None, :, None, None] + t[None, :, None, None]
        xb = x.double() + (bs.double()[None, :, None, None] if bs is not None else 0)
        want = torch.nn.functional.batch_norm(xb, m.double(), var.double(), g.double(), b.double(), False, 0.0, 1e-5)
        # x s + t in float32 with s, t rounded once: 4 roundings of values bounded by |x s| + |t|
        bound = 4 * EPS32 * float((x.double().abs() * s.double().abs()[None, :, None, None] +
                                   t.double().abs()[None, :, None, None]).max())
        assert float((folded.double() - want).abs().max()) <= bound


def reader_transcription(points, H, W, fov_up, fov_down, px, py):
    """The reader's scatter for one frame, given the pixels: a descending stable sort by depth (ties: the larger index
    first, so the smaller index writes last) and last write wins."""
    pts = np.asarray(points, F32)
    depth = np.linalg.norm(pts[:, :3], 2, axis=1)
    order = np.lexsort((-np.arange(len(pts)), -depth.astype(np.float64)))
    rng_img = np.full((H, W), -1, F32)
    xyz = np.full((H, W, 3), -1, F32)
    rem = np.full((H, W), -1, F32)
    idx = np.full((H, W), -1, np.int32)
    for i in order:
        rng_img[py[i], px[i]] = depth[i]
        xyz[py[i], px[i]] = pts[i, :3]
        rem[py[i], px[i]] = pts[i, 3]
        idx[py[i], px[i]] = i
    return np.concatenate([rng_img[None], xyz.transpose(2, 0, 1), rem[None]]), idx


def test_restated_projection_against_the_readers_scatter():
    H, W = 8, 64
    a, b = scan(1500, 1), scan(700, 2)
    a[10] = a[3]  # equal depths in one pixel: the smaller index wins
    mean, std = (12.12, 10.88, 0.23, -1.04, 0.21), (12.32, 11.47, 6.91, 0.86, 0.16)
    out = sn.range_project(np.concatenate([a, b]), [0, 1500, 2200], H, W, 3.0, -25.0, mean, std)
    assert out["proj_x"].min() >= 0 and out["proj_x"].max() == W - 1 and out["proj_y"].max() == H - 1
    for f, (pts, lo, hi) in enumerate(((a, 0, 1500), (b, 1500, 2200))):
        raw, idx = reader_transcription(pts, H, W, 3.0, -25.0, out["proj_x"][lo:hi], out["proj_y"][lo:hi])
        assert np.array_equal(out["raw"][f], raw) and np.array_equal(out["proj_idx"][f], idx)
        img = raw.copy()
        img -= np.array(mean)[:, None, None]  # NumPy's in-place float64 operand on a float32 image
        img /= np.array(std)[:, None, None]
        assert np.array_equal(out["image"][f], img)
        assert np.array_equal(out["proj_mask"][f], idx > 0)
    assert out["proj_idx"][0][out["proj_y"][3], out["proj_x"][3]] != 10


def test_restated_projection_edge_points():
    pts = np.array([[0, 0, 0, 0.5], [np.nan, 1, 1, 0.5], [1, np.inf, 0, 0.5], [5, 0, 0, 0.25], [5, 0, 0, 0.75]], F32)
    out = sn.range_project(pts, [0, 5], 4, 8)
    assert out["proj_x"].tolist() == [-1, -1, -1, 4, 4] and out["proj_y"][:3].tolist() == [-1, -1, -1]
    assert out["proj_idx"].max() == 3 and (out["proj_idx"] >= 0).sum() == 1
    assert out["image"][0, 4, out["proj_y"][3], 4] == F32(0.25)
    empty = sn.range_project(np.zeros((0, 4), F32), [0, 0], 2, 3, mean=(1,) * 5, std=(2,) * 5)
    assert np.array_equal(empty["image"], np.full((1, 5, 2, 3), -1.0, F32)) and (empty["proj_idx"] == -1).all()


# ---- against the reference's golden results ---------------------------------------------------------------------------


def check_result(golden, tag, key, got):
    """`got` within the stored bound of the reference's float64 result; prints the figure first."""
    want, bound = golden[f"{tag}_{key}"], float(golden[f"{tag}_{key}_bound"])
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == F32, (tag, key, got.shape, want.shape, got.dtype)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{tag} {key}: error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (tag, key, err, bound)


def build(tag, fused=False, device="cpu", **kw):
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    m = mk.build(tag, fused, **kw)
    assert load_paddle_state_dict(m, mk.state(tag)) == []
    return m.to(device).eval()


def golden_block_params(tag):
    """The case's weights as the kernel takes them (unpacked): the BatchNorms folded by ops.squeezeseg.fold_batch_norm."""
    from paddle3d_amd.ops.squeezeseg import fold_batch_norm

    st = {k: torch.from_numpy(v) for k, v in mk.state(tag).items()}
    C = mk.BLOCKS[tag]["C"]

    def fold(prefix):
        bn = prefix + "._batch_norm."
        return fold_batch_norm(st[bn + "weight"], st[bn + "bias"], st[bn + "_mean"], st[bn + "_variance"], 1e-5,
                               st[prefix + "._conv.bias"])

    (s_a, t_a), (s_m, t_m) = fold("attention_layer"), fold("position_mlp.0")
    return dict(w=st["attention_layer._conv.weight"].numpy(), s_a=s_a.numpy(), t_a=t_a.numpy(),
                v=st["position_mlp.0._conv.weight"].numpy().reshape(C, 9 * C), s_m=s_m.numpy(), t_m=t_m.numpy())


def block_outputs(tag, fused, device="cpu"):
    """(y, out) of our SACISKBlock on the case's inputs."""
    block, inp = build(tag, fused, device), mk.inputs(tag)
    xyz, feat = (torch.from_numpy(inp[k]).to(device) for k in ("xyz", "feature"))
    with torch.no_grad():
        return block.first_layer(xyz, feat).cpu().numpy(), block(xyz, feat)[1].cpu().numpy()


def net_outputs(fused, device="cpu", **kw):
    """dict(stage0, feat, logits, pred, labels) of our SqueezeSegV3 on the case's inputs."""
    model, inp = build("net", fused, device, **kw), mk.inputs("net")
    image, py, px, off = (torch.from_numpy(inp[k]).to(device) for k in ("image", "proj_y", "proj_x", "offsets"))
    tap = {}
    hooks = [model.backbone.encoder.encoder_stages[0].register_forward_hook(lambda m, i, o: tap.update(stage0=o[1])),
             model.heads[-1].register_forward_hook(lambda m, i, o: tap.update(feat=i[0], logits=o))]
    with torch.no_grad():
        pred = model.export_forward(image)
        labels = model(image, py, px, off)
    for h in hooks:
        h.remove()
    out = {k: v.cpu().numpy() for k, v in tap.items()}
    out.update(pred=pred.cpu().numpy(), labels=labels.cpu().numpy())
    return out


def check_net(golden, out):
    for k in ("stage0", "feat", "logits"):
        check_result(golden, "net", k, out[k])
    assert np.array_equal(out["pred"], golden["net_pred"])
    assert np.array_equal(out["labels"], golden["net_labels"])


@pytest.mark.parametrize("tag", list(mk.BLOCKS))
def test_restatement_against_the_reference(golden, expf, tag):
    p, inp = golden_block_params(tag), mk.inputs(tag)
    check_result(golden, tag, "y", sn.sac_isk(inp["xyz"], inp["feature"], p["w"], p["s_a"], p["t_a"], p["v"], p["s_m"],
                                              p["t_m"], expf))


@pytest.mark.parametrize("tag", list(mk.BLOCKS))
def test_unfused_block_against_the_reference(golden, tag):
    y, out = block_outputs(tag, False)
    check_result(golden, tag, "y", y)
    check_result(golden, tag, "out", out)


def test_unfused_network_against_the_reference(golden):
    check_net(golden, net_outputs(False))


def test_labels_of_points_without_a_pixel_are_zero():
    model, inp = build("net"), mk.inputs("net")
    py = torch.from_numpy(inp["proj_y"]).clone()
    py[::3] = -1
    with torch.no_grad():
        labels = model(torch.from_numpy(inp["image"]), py, torch.from_numpy(inp["proj_x"]), torch.from_numpy(inp["offsets"]))
        pred = model.export_forward(torch.from_numpy(inp["image"]))
    assert labels.dtype == torch.int64 and bool((labels[::3] == 0).all())
    frame = np.repeat(np.arange(mk.NET["N"]), mk.NET["points"])
    want = pred.numpy()[frame, inp["proj_y"], inp["proj_x"]]
    keep = np.arange(len(want)) % 3 != 0
    assert np.array_equal(labels.numpy()[keep], want[keep])


@pytest.mark.parametrize("tag", mk.TAGS)
def test_state_dict_keys_are_the_references(golden, tag):
    ours = sorted(mk.ref_key(k) for k in mk.build(tag).state_dict() if not k.endswith("num_batches_tracked"))
    assert ours == [str(k) for k in golden[f"{tag}_state_keys"]]
    if tag == "net":
        for k in ("backbone.encoder.encoder_stages.2.layers.0.attention_layer._conv.weight",
                  "backbone.encoder.encoder_stages.2.layers.0.attention_layer._batch_norm._mean", "heads.4.weight",
                  "backbone.decoder.decoder_stages.2.layers.0._deconv.weight"):
            assert k in ours


def test_range_net_53_has_the_references_depth():
    from paddle3d_amd import squeezesegv3 as sq

    n21 = sum(isinstance(m, sq.SACISKBlock) for m in sq.SACRangeNet21(in_channels=5).modules())
    n53 = sum(isinstance(m, sq.SACISKBlock) for m in sq.SACRangeNet53(in_channels=5).modules())
    assert (n21, n53) == (7, 23)
    with pytest.raises(ValueError):
        sq.SACRangeNet(5, num_layers=34)


def test_restated_projection_against_the_reference(golden):
    pts, off = mk.scans()
    out = sn.range_project(pts, off, mk.SCAN_H, mk.SCAN_W, 3.0, -25.0, mk.MEAN, mk.STD)
    for f, tag in enumerate(mk.SCANS):
        lo, hi = off[f], off[f + 1]
        assert np.array_equal(out["proj_x"][lo:hi], golden[f"{tag}_proj_x"])
        assert np.array_equal(out["proj_y"][lo:hi], golden[f"{tag}_proj_y"])
        assert np.array_equal(out["raw"][f], golden[f"{tag}_raw"])  # the float32 run's range image, xyz and remission
        assert np.array_equal(out["proj_idx"][f], golden[f"{tag}_proj_idx"])
        assert np.array_equal(out["proj_mask"][f], golden[f"{tag}_proj_mask"])
        check_result(golden, tag, "image", out["image"][f])
        # the float64 pixel coordinates against the reference's float64 run (whose depth is a float64 norm, ours the
        # float32 one): inside the margin the maker keeps every coordinate away from an integer by
        for k in ("fx", "fy"):
            assert np.abs(out[k][lo:hi] - golden[f"{tag}_{k}"]).max() < float(golden["scan_margin"])


def test_the_committed_file_meets_the_makers_conditions(golden):
    seen = mk.check_discrete(golden)
    assert seen["gap"] > 2 * seen["logits_bound"] and seen["scan_margin"] > 0
    assert os.path.getsize(mk.OUT) < 1 << 20
