"""BEV-LaneDet without a GPU: the NumPy restatement of csrc/lanedet.hip (tests/golden/lanedet_numpy.py) against the
reference's golden file (tests/golden/python_lanedet.npz, made by make_lanedet_golden.py from the reference's own
Python), the module's torch / NumPy transcription against the reference's maps and lanes on the head cases, the
state-dict keys, the shim's refusals by name, the workspace query and the shape predicate.

The tolerance rule.  Labels, lane ids and row counts have no tolerance.  For a float output q (a column of `points` or
of `fit`, or one kind of map) of a case, with ref32 and ref64 the reference's own fp32 and fp64 runs:

    max |ours - ref64|  <=  4 * max(max |ref32 - ref64|, ulp32(max |ref64|))

the project's "4 x the reference's own fp32 error" with one fp32 ulp as floor (the reference's column means are
float64 in both runs, so its own error can be exactly 0).  The maxima run over the quantity, as in every golden file
here (make_bevformer_golden.bound): element by element the reference's two runs agree to the last bit on some elements
by chance, and no other operation order can promise that of the same elements.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import lanedet_numpy as ln  # noqa: E402
import make_lanedet_golden as mk  # noqa: E402

F32 = np.float32
POST_TAGS, HEAD_TAGS = tuple(mk.POST_CASES), tuple(mk.HEAD_CASES)
RATIOS = {}  # (what, quantity) -> the largest observed ratio to the bound (printed; DESIGN.md quotes them)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "python_lanedet.npz")))


def within(ours, ref32, ref64, what):
    """The tolerance rule for one quantity; returns the ratio of the error to the bound."""
    ours, ref32, ref64 = (np.asarray(a, np.float64) for a in (ours, ref32, ref64))
    assert ours.shape == ref64.shape == ref32.shape, (what, ours.shape, ref32.shape, ref64.shape)
    if not ours.size:
        return 0.0
    err = float(np.abs(ref32 - ref64).max())
    ulp = float(np.spacing(F32(np.abs(ref64).max())))
    bound = 4.0 * max(err, ulp)
    got = float(np.abs(ours - ref64).max())
    ratio = got / bound
    RATIOS[what] = max(RATIOS.get(what, 0.0), ratio)
    print(f"[lanedet tolerance] {what}: error {got:.3e}, reference's own {err:.3e}, ulp {ulp:.3e}, ratio {ratio:.3f}")
    assert got <= bound, f"{what}: |ours - ref64| = {got:.3e} > 4 * max({err:.3e}, {ulp:.3e})"
    return ratio


def post_inputs(golden, tag):
    maps, c = golden[f"{tag}_maps"], golden[f"{tag}_cfg"]
    nd = maps.shape[1] - 3
    cfg = dict(conf=float(c[0]), emb_margin=float(c[1]), min_cluster_size=int(c[2]), max_x=float(c[3]),
               meter_per_pixel=(float(c[4]), float(c[5])))
    return maps[:, :1], maps[:, 1:1 + nd], maps[:, 1 + nd:2 + nd], maps[:, 2 + nd:], cfg


def check_lanes(golden, key, out, b, what, fit_of=None):
    """Frame b of padded outputs `out` (arrays) against the golden frame `key`."""
    canvas, ids, rows = golden[f"{key}_canvas"], golden[f"{key}_lane_id"], golden[f"{key}_lane_rows"]
    assert int(out["flags"][b]) == 0, what
    assert np.array_equal(out["labels"][b], canvas), f"{what}: the canvas differs"
    n = len(ids)
    assert int(out["num_lanes"][b]) == n, (what, int(out["num_lanes"][b]), n)
    assert np.array_equal(out["lane_id"][b, :n], ids) and np.array_equal(out["lane_rows"][b, :n], rows), what
    assert not out["lane_id"][b, n:].any() and not out["lane_rows"][b, n:].any()
    assert out["fit_ok"][b, :n].all(), f"{what}: a lane of at least 4 rows was not fitted"
    pts = np.concatenate([out["points"][b, l, :rows[l]] for l in range(n)])
    for j, col in enumerate(("x", "y", "z")):
        within(pts[:, j], golden[f"{key}_points32"][:, j], golden[f"{key}_points64"][:, j], f"{what} points.{col}")
        within(out["fit"][b, :n, :, j], golden[f"{key}_fit32"][:, :, j], golden[f"{key}_fit64"][:, :, j],
               f"{what} fit.{'XYZ'[j]}")
    for l in range(n):
        assert not out["points"][b, l, rows[l]:].any()
    assert not out["points"][b, n:].any() and not out["fit"][b, n:].any()


def test_restatement_equals_the_goldens(golden):
    for tag in POST_TAGS:
        seg, emb, off, z, cfg = post_inputs(golden, tag)
        out = ln.post_process(seg, emb, off, z, cfg)
        assert min(golden[f"{tag}_margins"]) >= mk.MARGIN
        check_lanes(golden, tag, out, 0, f"restatement {tag}")
        lanes = ln.lanes_of(out, 0)
        assert len(lanes) == len(golden[f"{tag}_lane_id"]) and all(l.shape == (40, 3) for l in lanes)
    for tag in HEAD_TAGS:
        maps = golden[f"{tag}_maps32"]
        out = ln.post_process(maps[:, :1], maps[:, 1:3], maps[:, 3:4], maps[:, 4:5], mk.HEAD_POST)
        for b in range(maps.shape[0]):
            # from the reference's fp32 maps: the fp64 fixture of the frame is the reference on its fp64 maps, so
            # the fp32 run's own error includes the head's
            check_lanes(golden, f"{tag}_f{b}", out, b, f"restatement {tag} frame {b}")


def test_restatement_border_cases():
    """The decisions the border cases are built for, on the restatement alone.  This runs test-side code only and says
    nothing about the kernels: tests/test_lanedet_gpu.py holds the device to these results bit for bit."""
    w = {k: ln.post_process(c[0], c[1], ln.sigmoid(c[2]), c[3], c[4]) for k, c in ln.border_cases().items()}
    assert [int(w[f"centres_{k}"]["flags"][0]) for k in (127, 128, 129)] == [0, 0, 1]
    assert w["lanes_32"]["num_lanes"][0] == 32 and w["lanes_33"]["flags"][0] == 2 and not w["lanes_33"]["labels"].any()
    assert w["tie_nd1"]["labels"][0, 0].tolist() == [1, 2, 1] and w["gap_nd2"]["labels"][0, 0, :2].tolist() == [1, 2]
    assert w["rows_1_to_4"]["fit_ok"][0, :3].tolist() == [0, 0, 1]
    # the lane of 4 rows is exact: x + 0.5 columns, heights y^2 / 8 -- the cubic through four points reproduces them
    o = w["rows_1_to_4"]
    assert np.allclose(o["fit"][0, 2, [0, 39], 2], o["points"][0, 2, [0, 3], 2], atol=1e-6)
    # the identity head reproduces the maps, so the lazy form's restatement gives the same lanes
    for name, c in ln.border_cases().items():
        if name == "nan_inf":
            continue
        lazy = ln.head_forward(*ln.identity_head(*c[:4]), c[4])
        assert all(np.array_equal(lazy[k], w[name][k]) for k in lazy), name


# ---- the module -------------------------------------------------------------------------------------------------------
def head_input(golden, tag):
    return golden[f"{tag}_x"]


def build_model(golden, tag, fused=True, conv_kernel="auto"):
    from paddle3d_amd import bev_lanedet as M
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    seed, B, s32, c64, bev, size = mk.HEAD_CASES[tag]
    shapes = {k: [int(s) for s in v.split(",")] for k, v in zip(golden[f"{tag}_keys"], golden[f"{tag}_shapes"])}
    state = mk.head_state(shapes, int(golden[f"{tag}_seed"][0]), tuple(golden[f"{tag}_scales"]))
    p = mk.HEAD_POST
    m = M.BEVLaneDet(None, bev_shape=size, train=False, fused=fused, conv_kernel=conv_kernel, s32=s32,
                     s64=(c64, (s32[1] + 1) // 2, (s32[2] + 1) // 2), bev=bev, x_range=(3, p["max_x"]),
                     meter_per_pixel=p["meter_per_pixel"][0], post_conf=p["conf"], post_emb_margin=p["emb_margin"],
                     post_min_cluster_size=p["min_cluster_size"])
    load_paddle_state_dict(m, state, strict=True)
    return m.eval()


def check_head_case(golden, tag, dev, fused, conv_kernel="auto"):
    """The module in one form on a head case: the maps and the lanes under the tolerance rule, labels exactly."""
    m = build_model(golden, tag, conv_kernel=conv_kernel).to(dev)
    x = torch.from_numpy(head_input(golden, tag)).to(dev)
    what = f"module {tag} fused={fused}" + ("" if conv_kernel == "auto" else f" {conv_kernel}")
    with torch.no_grad():
        maps = m.raw_maps(x, fused=fused).cpu().numpy()
        pack = m.lanes_padded(x, fused=fused)
        lanes = m.forward(dict(img=x), fused=fused)
    m32, m64 = golden[f"{tag}_maps32"], golden[f"{tag}_maps64"]
    for name, sl in (("seg", slice(0, 1)), ("emb", slice(1, 3)), ("offset", slice(3, 4)), ("z", slice(4, 5))):
        within(maps[:, sl], m32[:, sl], m64[:, sl], f"{what} maps.{name}")
    out = {k: getattr(pack, k).cpu().numpy() for k in pack._fields}
    for b in range(x.shape[0]):
        check_lanes(golden, f"{tag}_f{b}", out, b, f"{what} frame {b}")
        # forward evaluates the network again: torch's convolution library may take another algorithm per call, so its
        # lanes are held to the reference like the padded ones, not to the bits of the call before
        key = f"{tag}_f{b}"
        assert len(lanes[b]) == int(out["num_lanes"][b]) and all(lane.shape == (40, 3) for lane in lanes[b])
        for j in range(3):
            within(np.stack(lanes[b])[:, :, j], golden[f"{key}_fit32"][:, :, j], golden[f"{key}_fit64"][:, :, j],
                   f"{what} frame {b} forward.{'XYZ'[j]}")


def test_transcription_equals_the_reference(golden):
    for tag in HEAD_TAGS:
        check_head_case(golden, tag, torch.device("cpu"), False)


def test_state_dict_keys_are_the_references(golden):
    from paddle3d_amd import bev_lanedet as M

    m = M.bev_lanedet_apollo_576x1024(None)
    ours = sorted(k.replace(".running_mean", "._mean").replace(".running_var", "._variance")
                  for k in m.state_dict() if not k.endswith("num_batches_tracked"))
    assert ours == [str(k) for k in golden["state_keys"]]
    assert any(k.startswith("lane_head_2d.") for k in ours)
    assert m.bev_shape == (200, 48) and m.post == dict(conf=0.9, emb_margin=6.0, min_cluster_size=15, max_x=103.0,
                                                       meter_per_pixel=(0.5, 0.5))
    # the [in, out] Linear weights load transposed
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    small = build_model(golden, HEAD_TAGS[0])
    lin = small.s32transformer.fc_transform[0]
    assert tuple(lin.weight.shape) == (6, 24)
    state = {k: v.detach().numpy() for k, v in small.state_dict().items() if not k.endswith("num_batches_tracked")}
    state = {k.replace(".running_mean", "._mean").replace(".running_var", "._variance"):
             (v.T if k.endswith("fc_transform.0.weight") or k.endswith("fc_transform.2.weight") else v)
             for k, v in state.items()}
    assert load_paddle_state_dict(small, state, strict=True) == []


def test_shim_refuses_by_name():
    from paddle3d_amd.ops import lanedet as A

    z = torch.zeros((1, 1, 4, 4))
    with pytest.raises(RuntimeError, match="Unsupported device type for lanedet operator"):
        A.lanedet_post_process(z, torch.zeros((1, 2, 4, 4)), z, z)
    with pytest.raises(RuntimeError, match="Unsupported device type for lanedet operator"):
        A.lanedet_head_forward(*[torch.zeros((1, 64, 4, 4))] * 4, *[None] * 8)
    with pytest.raises(RuntimeError, match="Unsupported device type for lanedet operator"):
        A.lanedet_post_process(np.zeros((1, 1, 4, 4), F32), z, z, z)
    if torch.cuda.is_available():
        dev = torch.device("cuda", 0)
        g = torch.zeros((1, 1, 4, 4), device=dev)
        e = torch.zeros((1, 2, 4, 4), device=dev)
        with pytest.raises(RuntimeError, match="seg must be torch.float32"):
            A.lanedet_post_process(g.double(), e, g, g)
        with pytest.raises(RuntimeError, match="seg must be \\[B, 1, H, W\\]"):
            A.lanedet_post_process(e, e, g, g)
        with pytest.raises(RuntimeError, match="emb must be"):
            A.lanedet_post_process(g, torch.zeros((1, 2, 4, 5), device=dev), g, g)
        with pytest.raises(RuntimeError, match="z must be"):
            A.lanedet_post_process(g, e, g, torch.zeros((1, 1, 5, 4), device=dev))
        with pytest.raises(RuntimeError, match="Unsupported device type"):
            A.lanedet_post_process(g, e, g.cpu(), g)
        f = torch.zeros((1, 64, 4, 4), device=dev)
        with pytest.raises(RuntimeError, match="z_feat must be"):
            A.lanedet_head_forward(f, f, f, torch.zeros((1, 64, 4, 5), device=dev), *[None] * 8)
        with pytest.raises(RuntimeError, match="seg_feat must be float32"):
            A.lanedet_head_forward(f.half(), f, f, f, *[None] * 8)


def test_workspace_and_predicate_need_no_gpu():
    from paddle3d_amd import _lib
    from paddle3d_amd.ops import lanedet as A

    L = _lib.lib()
    full = L.pd3_lanedet_workspace(1, 200, 48, 2)
    assert 200 * 48 * 4 * 8 <= full < 4 * 2 ** 20 and L.pd3_lanedet_workspace(2, 200, 48, 2) > full
    assert L.pd3_lanedet_workspace(1, 1, 1, 1) > 0
    for bad in ((1, 0, 4, 2), (1, 4, 4, 5), (1, 4, 4, 0), (1, 1025, 1, 2), (1, 1024, 1025, 2), (0, 4, 4, 2)):
        assert L.pd3_lanedet_workspace(*bad) == 0, bad
    assert A.lanedet_supported(1, 1, 1) and A.lanedet_supported(200, 48, 2) and A.lanedet_supported(200, 48, 2, 64)
    assert all(A.lanedet_supported(5, w, nd) for w in (1, 7, 33, 129) for nd in (1, 2, 3, 4))
    assert not A.lanedet_supported(4, 4, 5) and not A.lanedet_supported(4, 4, 0) and not A.lanedet_supported(1025, 1, 2)
    assert not A.lanedet_supported(4, 4, 2, 129) and not A.lanedet_supported(1024, 1025, 2)
    assert A.lanedet_supported(4, 4, 2, batch=65535) and not A.lanedet_supported(4, 4, 2, batch=65536)
    assert A.lanedet_supported(4, 5, 2, 128, pitch=8) and not A.lanedet_supported(1024, 1024, 2, 128, pitch=2 ** 14)
    for h, w, nd in ((1, 1, 1), (5, 7, 4), (200, 48, 2), (1025, 1, 2), (4, 4, 5)):
        assert A.lanedet_supported(h, w, nd) == (L.pd3_lanedet_workspace(1, h, w, nd) > 0), (h, w, nd)
    assert (A.MAX_CENTRES, A.MAX_LANES, A.FIT_SAMPLES) == (ln.MAX_CENTRES, ln.MAX_LANES, ln.FIT_SAMPLES) == (128, 32, 40)


def test_constructor_asks_for_the_2d_shape_when_it_builds_the_2d_head():
    from paddle3d_amd import bev_lanedet as M

    with pytest.raises(ValueError, match="output_2d_shape"):
        M.BEVLaneDet(None, bev_shape=(4, 4), s32=(8, 2, 2), s64=(8, 1, 1), bev=(8, 2, 2))
    M.BEVLaneDet(None, bev_shape=(4, 4), train=False, s32=(8, 2, 2), s64=(8, 1, 1), bev=(8, 2, 2))


def test_transcription_pack_has_the_kernels_definitions():
    """lanes_padded_torch on border-case maps: the flags, the all-zero flagged frame and fit_ok as the restatement
    (and with it the device) has them."""
    from paddle3d_amd import bev_lanedet as M

    cases = ln.border_cases()
    for name in ("centres_128", "centres_129", "lanes_32", "lanes_33", "rows_1_to_4", "empty_frame"):
        seg, emb, logit, z, cfg = cases[name]
        want = ln.post_process(seg, emb, ln.sigmoid(logit), z, cfg)
        m = M.BEVLaneDet(None, bev_shape=seg.shape[2:], train=False, s32=(8, 2, 2), s64=(8, 1, 1), bev=(8, 2, 2),
                         x_range=(3, cfg["max_x"]), meter_per_pixel=cfg["meter_per_pixel"][0], post_conf=cfg["conf"],
                         post_emb_margin=cfg["emb_margin"], post_min_cluster_size=cfg["min_cluster_size"])
        pack = m.lanes_padded_torch(torch.from_numpy(np.concatenate([seg, emb, ln.sigmoid(logit), z], 1)))
        for k in ("labels", "num_lanes", "lane_id", "lane_rows", "fit_ok", "flags", "num_selected"):
            assert np.array_equal(getattr(pack, k).numpy(), want[k]), (name, k)
        assert np.allclose(pack.points.numpy(), want["points"], atol=1e-6), name
        assert np.allclose(pack.fit.numpy(), want["fit"], atol=1e-5), name

