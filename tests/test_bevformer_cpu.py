"""BEVFormer's encoder attention on the CPU: the NumPy restatement of the three entry points
(tests/golden/bevformer_numpy.py) against what the reference's own Python computed (tests/golden/python_bevformer.npz),
the fused spatial cross-attention against the reference's rebatch / scatter algorithm,
the refusal statuses, and the maker's conditions on the committed file.

Bounds: the ones the maker stored, 4 x the largest error of the reference's own fp32 run against its fp64 run (one fp32
ulp of the largest output as a floor).  reference_points_cam: that bound over the points in front of the camera, and the
same rule on a relative scale for the components behind it (u = x / 1e-5, about 1e5 in size).  The masks are compared
bit for bit: the maker keeps every u, v 1e-4 and every depth a factor of 10 away from the comparisons' edges."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import bevformer_numpy as bn  # noqa: E402
import make_bevformer_golden as mk  # noqa: E402

F32 = np.float32
TAGS = mk.TAGS
Z_RANGE = mk.PC_RANGE[5] - mk.PC_RANGE[2]


@pytest.fixture(scope="module")
def golden():
    return mk.load()


@pytest.fixture(scope="module")
def expf():
    from oracle import pyoracle as O

    return lambda x: O.libm_eval(2, x)


def _linear(st, key, x):
    """Paddle's Linear on the CPU in float32: x W + b with W [in, out]."""
    return (torch.from_numpy(x) @ torch.from_numpy(st[key + ".weight"]) + torch.from_numpy(st[key + ".bias"])).numpy()


def ref_2d(tag):
    """The hybrid BEV points [B*2, Q, 1, 2] the encoder hands TSA: both queue entries shifted."""
    c = mk.CASES[tag]
    pts = bn.get_reference_points(*c["bev"], dim="2d")[None] + mk.inputs(tag)["shift"][:, None, None, :]
    return np.repeat(pts.astype(F32), 2, 0)


def sca_inputs(tag, layer=0):
    """(value [B*cams, S, M, C], offsets [B, Q, M, L, P, 2], logits [B, Q, M, L*P]) of the layer's SCA on bev_query."""
    c, st, inp = mk.CASES[tag], mk.state(tag), mk.inputs(tag)
    k = f"layers.{layer}.attentions.1.deformable_attention."
    B, Q, L = c["B"], c["bev"][0] * c["bev"][1], len(c["levels"])
    feats = np.ascontiguousarray(inp["feats"].transpose(2, 0, 1, 3)).reshape(B * c["cams"], -1, mk.EMBED)
    value = _linear(st, k + "value_proj", feats).reshape(B * c["cams"], -1, mk.HEADS, mk.EMBED // mk.HEADS)
    off = _linear(st, k + "sampling_offsets", inp["bev_query"]).reshape(B, Q, mk.HEADS, L, c["P"], 2)
    logits = _linear(st, k + "attention_weights", inp["bev_query"]).reshape(B, Q, mk.HEADS, L * c["P"])
    return value, off, logits


def tsa_inputs(tag, layer=0):
    """(value [B*2, Q, M, C], offsets [B, Q, M, 2, 1, P, 2], logits [B, Q, M, 2, P]) of the layer's TSA."""
    c, st, inp = mk.CASES[tag], mk.state(tag), mk.inputs(tag)
    k = f"layers.{layer}.attentions.0."
    B, Q, P = c["B"], c["bev"][0] * c["bev"][1], c["tsa_P"]
    queue = np.stack([inp["prev_bev"], inp["bev_query"]], 1).reshape(B * 2, Q, mk.EMBED)
    query = np.concatenate([queue[0::2], inp["bev_query"] + inp["bev_pos"]], -1)
    value = _linear(st, k + "value_proj", queue).reshape(B * 2, Q, mk.HEADS, mk.EMBED // mk.HEADS)
    off = _linear(st, k + "sampling_offsets", query).reshape(B, Q, mk.HEADS, 2, 1, P, 2)
    logits = _linear(st, k + "attention_weights", query).reshape(B, Q, mk.HEADS, 2, P)
    return value, off, logits


_cache = {}


def restated(g, tag, expf):
    """(point_sampling's four outputs, sca, tsa) of the restatement, computed once per case."""
    if tag not in _cache:
        c = mk.CASES[tag]
        sh, lsi, _ = mk.levels(tag)
        ps = bn.point_sampling(bn.get_reference_points(*c["bev"], Z_RANGE, c["D"]), g[f"{tag}_lidar2img"], mk.PC_RANGE,
                               *mk.IMG_SHAPE[:2])
        sca = bn.sca(*sca_inputs(tag), ps[0], ps[2], sh, lsi, c["cams"], expf)
        bev_sh, bev_lsi, _ = bn.md.level_layout([c["bev"]])
        tsa = bn.tsa(*tsa_inputs(tag), ref_2d(tag), bev_sh, bev_lsi, expf)
        _cache[tag] = (ps, sca, tsa)
    return _cache[tag]


def check_point_sampling(g, tag, ref_cam, mask, bits, count):
    want, front = g[f"{tag}_reference_points_cam"], g[f"{tag}_depth"] > mk.EPS
    assert ref_cam.shape == want.shape and ref_cam.dtype == F32
    diff = np.abs(ref_cam.astype(np.float64) - want)
    err, bound = float(diff[front].max()), float(g[f"{tag}_reference_points_cam_bound"])
    rel, rel_bound = float((diff[~front] / np.abs(want[~front])).max()), float(g[f"{tag}_reference_points_cam_rel_bound"])
    print(f"{tag} reference_points_cam err {err:.3e} bound {bound:.3e}; behind the camera {rel:.3e} bound {rel_bound:.3e}")
    assert err <= bound and rel <= rel_bound
    assert mask.dtype == np.uint8 and np.array_equal(mask, g[f"{tag}_bev_mask"])
    hit = g[f"{tag}_bev_mask"].astype(bool).any(-1)
    assert np.array_equal(count, hit.sum(0)) and count.dtype == np.uint8 and bits.dtype == np.uint8
    for cam in range(hit.shape[0]):
        assert np.array_equal((bits >> cam) & 1, hit[cam])
    assert not (bits >> hit.shape[0]).any()


def check_result(g, tag, name, got):
    want, bound = g[f"{tag}_{name}"], float(g[f"{tag}_{name}_bound"])
    assert got.shape == want.shape and got.dtype == F32, (tag, name, got.shape, got.dtype)
    e = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{tag} {name} err {e:.3e} bound {bound:.3e} (reference's own {float(g[f'{tag}_{name}_ref_err']):.3e})")
    assert e <= bound, (tag, name, e, bound)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_against_reference(golden, expf, tag):
    ps, sca, tsa = restated(golden, tag, expf)
    check_point_sampling(golden, tag, *ps)
    check_result(golden, tag, "sca_sample", sca)
    check_result(golden, tag, "tsa_sample", tsa)


@pytest.mark.parametrize("tag", TAGS)
def test_fused_sca_equals_the_rebatch_form(golden, expf, tag):
    """One pass over the hit cameras of each query against gather / pad / sample / scatter_nd_add / divide: the same
    bits, because a rebatched row's Linear outputs are the BEV query's and padded rows are never scattered back."""
    c = mk.CASES[tag]
    sh, lsi, _ = mk.levels(tag)
    ps, sca, _ = restated(golden, tag, expf)
    got = bn.sca_rebatch(*sca_inputs(tag), ps[0], ps[1], sh, lsi, c["cams"], expf)
    assert np.array_equal(got.view(np.uint32), sca.view(np.uint32))
    seen = ps[3] > 0
    assert np.abs(sca[seen]).min(-1).max() > 0 and not sca[~seen].any()  # misses are exactly zero


def test_refusals_need_no_gpu():
    from paddle3d_amd import _lib, build

    build.build()
    L = _lib.lib()
    sca = lambda cams, C, Lv, P, D: L.pd3_bevformer_sca(None, None, None, None, None, None, None, 1, cams, 10, 2, C, Lv,  # noqa: E731
                                                        5, P, D, None, None)
    tsa = lambda C, Lv, P: L.pd3_bevformer_tsa(None, None, None, None, None, None, 1, 10, 2, C, Lv, 5, P, None, None)  # noqa: E731
    for args in ((3, 30, 1, 8, 4), (9, 32, 1, 8, 4), (3, 32, 5, 8, 4), (3, 32, 1, 33, 1), (3, 32, 1, 8, 3), (3, 2, 1, 8, 4)):
        assert sca(*args) == -3, args
    for args in ((30, 1, 4), (32, 9, 4), (32, 1, 33), (2, 1, 4)):
        assert tsa(*args) == -3, args
    # a supported shape with null pointers, and sizes that are no sizes
    assert sca(3, 32, 4, 8, 4) == -1 and tsa(32, 1, 32) == -1
    assert sca(0, 32, 1, 8, 4) == -1 and sca(3, 32, 1, 8, 0) == -1 and tsa(32, 0, 4) == -1
    pc = np.asarray(mk.PC_RANGE, F32)
    ps = lambda pcp, cams, h: L.pd3_bevformer_point_sampling(None, None, pcp, h, 80, 1, cams, 5, 4, None, None, None,  # noqa: E731
                                                             None, None)
    assert ps(pc.ctypes.data, 9, 48) == -3
    assert ps(None, 3, 48) == -1 and ps(pc.ctypes.data, 3, 0) == -1 and ps(pc.ctypes.data, 3, 48) == -1
    # nothing to do is no error
    assert L.pd3_bevformer_point_sampling(None, None, pc.ctypes.data, 48, 80, 0, 3, 5, 4, None, None, None, None, None) == 0


@pytest.mark.parametrize("tag", TAGS)
def test_maker_conditions_hold_on_the_committed_file(golden, tag):
    seen = mk.check_conditions(golden, tag)
    print(tag, seen)
    assert os.path.getsize(mk.OUT) < 1_000_000
    c = mk.CASES[tag]
    Q = c["bev"][0] * c["bev"][1]
    assert np.array_equal(golden[f"{tag}_lidar2img"], mk.calibrations(tag))
    assert golden[f"{tag}_reference_points_cam"].shape == (c["cams"], c["B"], Q, c["D"], 2)
    for name in mk.RESULTS:
        assert golden[f"{tag}_{name}"].shape == (c["B"], Q, mk.EMBED)
    if c["B"] > 1:  # the frames' calibrations differ
        assert not np.array_equal(golden[f"{tag}_lidar2img"][0], golden[f"{tag}_lidar2img"][1])
    # the restatement's own locations: some fall outside every level
    sh, _, _ = mk.levels(tag)
    _, off, _ = sca_inputs(tag)
    loc = bn.sca_locations(off, golden[f"{tag}_reference_points_cam"][0].astype(F32), sh)
    assert (~((loc >= 0) & (loc <= 1)).all(-1)).any()
