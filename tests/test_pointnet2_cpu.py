"""The NumPy restatement of the pointnet2 batch ops and points_in_boxes (tests/golden/pointnet2_numpy.py) against what
the reference's IA-SSD Python hands the ops and gets back (tests/golden/python_pointnet2.npz), and the contract points
the reference leaves implicit: the FPS tie rule (against a literal run of the reference's scan and tree), fminf and
the 1e10 clamp, rows with an empty ball, and the double-precision box faces."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_pointnet2_golden as mk  # noqa: E402
import pointnet2_numpy as pn  # noqa: E402

F32 = np.float32


@pytest.fixture(scope="module")
def golden():
    return mk.load()


@pytest.fixture(scope="module")
def libm():
    from oracle import pyoracle as O

    return O.libm_eval


def _scalar(a):
    return float(np.asarray(a).reshape(-1)[0])


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_fps_restatement_equals_golden(golden):
    g = golden
    assert np.array_equal(pn.farthest_point_sample(g["fps0_arg0"], int(_scalar(g["fps0_arg1"]))), g["fps0_out"])
    # the callers hand FPS (B, N, 3) and gather the flipped (B, 3, N)
    assert g["fps0_arg0"].shape == (1, 2048, 3) and tuple(g["gather0_src_shape"]) == (1, 3, 2048)
    assert np.array_equal(g["gather0_arg1"], g["fps0_out"])


def test_ball_query_restatement_equals_golden(golden):
    g = golden
    for i in range(4):
        out = pn.ball_query(g[f"ball_query{i}_arg0"], g[f"ball_query{i}_arg1"], _scalar(g[f"ball_query{i}_arg2"]),
                            int(_scalar(g[f"ball_query{i}_arg3"])))
        assert np.array_equal(out, g[f"ball_query{i}_out"]), i
    # radii 0.2 / 0.8, nsample 16 / 32; rows with fewer hits than nsample exist (filled with the first hit)
    assert [_scalar(g[f"ball_query{i}_arg2"]) for i in range(4)] == [0.2, 0.8, 0.8, 0.8]
    o = g["ball_query0_out"]
    assert (o == o[..., :1]).all(-1).any() and not (o == o[..., :1]).all()


def test_sa_layer_outputs_from_restatement(golden):
    g = golden
    xyz, feat = g["xyz"], g["features"]
    idx = pn.farthest_point_sample(xyz, 512)
    new_xyz = pn.group(xyz.transpose(0, 2, 1), idx).transpose(0, 2, 1)
    assert np.array_equal(_bits(new_xyz), _bits(g["sa1_new_xyz"]))
    pooled = []
    for r, s in ((0.2, 16), (0.8, 32)):
        bi = pn.ball_query(new_xyz, xyz, r, s)
        gx = pn.group(xyz.transpose(0, 2, 1), bi) - new_xyz.transpose(0, 2, 1)[..., None]
        gf = pn.group(feat, bi)
        pooled.append(np.concatenate([gx, gf], 1).max(-1))
    assert np.array_equal(_bits(np.concatenate(pooled, 1)), _bits(g["sa1_new_features"]))
    # ctr_aware: sigmoid of the class maximum, top-k
    score = 1.0 / (1.0 + np.exp(-g["sa2_cls_features"].astype(np.float64).max(-1)))
    top = np.argsort(-score, axis=-1, kind="stable")[:, :128]
    assert np.array_equal(_bits(pn.group(new_xyz.transpose(0, 2, 1), top).transpose(0, 2, 1)),
                          _bits(g["sa2_new_xyz"]))


def test_query_and_group_layout(golden):
    g = golden
    new_xyz, q, feat = g["sa1_new_xyz"], g["sa2_new_xyz"], g["sa1_new_features"]
    bi = pn.ball_query(q, new_xyz, 0.8, 16)
    gx = pn.group(new_xyz.transpose(0, 2, 1), bi) - q.transpose(0, 2, 1)[..., None]
    want = np.concatenate([gx, pn.group(feat, bi)], 1)  # use_xyz: xyz first
    assert g["qag_out"].shape == (1, 13, 128, 16)
    assert np.array_equal(_bits(want), _bits(g["qag_out"]))


def test_points_in_boxes_restatement_equals_golden(golden, libm):
    g = golden
    for k in range(2):
        boxes = g[f"points_in_boxes{k}_arg1"]
        assert boxes.shape == (1, 6, 7) and np.array_equal(boxes[0], g["gt_boxes"][k, :, :7])
        out = pn.points_in_boxes(g[f"points_in_boxes{k}_arg0"], boxes, libm)
        assert np.array_equal(out, g[f"points_in_boxes{k}_out"]), k
        assert (out >= 0).any() and (out < 0).any()


def _ties(n, pts):
    xyz = np.zeros((1, n, 3), F32)
    for k, v in pts.items():
        xyz[0, k] = v
    return xyz


@pytest.mark.parametrize("n, a, b, winner", [(2048, 3, 1025, 1025), (1024, 1, 512, 512), (4, 1, 2, 2), (5, 1, 2, 2),
                                              (1500, 7, 1031, 7), (16, 5, 9, 9)])
def test_fps_tie_rule(n, a, b, winner):
    xyz = _ties(n, {a: (1, 0, 0), b: (0, 1, 0)})
    sim = pn.fps_reference_sim(xyz, 2)
    assert sim[0, 1] == winner
    assert pn.farthest_point_sample(xyz, 2)[0, 1] == winner
    assert winner != min(a, b) or (a % (1 << pn.fps_bs_log2(n))) == (b % (1 << pn.fps_bs_log2(n)))


def test_fps_tie_rule_random_tie_heavy():
    rng = np.random.default_rng(3)
    for _ in range(40):
        n = int(rng.integers(1, 3000))
        xyz = rng.integers(0, 3, (1, n, 3)).astype(F32)  # quantised grid: many equal distances
        m = int(rng.integers(1, 12))
        assert np.array_equal(pn.farthest_point_sample(xyz, m), pn.fps_reference_sim(xyz, m))


def test_fps_fminf_and_clamp():
    # far points: distances above 1e10 are clamped, so 5 and 9 tie at 1e10 and the tie rule picks 9 (bs = 16)
    xyz = _ties(16, {5: (1e6, 0, 0), 9: (0, -1e6, 0), 3: (1, 1, 1)})
    assert pn.farthest_point_sample(xyz, 3)[0].tolist() == pn.fps_reference_sim(xyz, 3)[0].tolist()
    assert pn.farthest_point_sample(xyz, 2)[0, 1] == 9
    # a NaN point: its distance never replaces temp; from a NaN centre nothing changes
    xyz = _ties(8, {2: (np.nan, 0, 0), 6: (3, 0, 0)})
    out = pn.farthest_point_sample(xyz, 6)
    assert np.array_equal(out, pn.fps_reference_sim(xyz, 6))
    assert 2 in out[0].tolist()
    # m <= 0 -> nothing; m > n repeats
    assert pn.farthest_point_sample(xyz, 0).shape == (1, 0)
    assert np.array_equal(pn.farthest_point_sample(xyz, 20), pn.fps_reference_sim(xyz, 20))


def test_ball_query_empty_rows():
    xyz = np.zeros((1, 10, 3), F32)
    q = np.array([[[5, 5, 5], [0, 0, 0]]], F32)
    out = pn.ball_query(q, xyz, 0.5, 4)
    assert out[0, 0].tolist() == [0, 0, 0, 0] and out[0, 1].tolist() == [0, 1, 2, 3]
    # strict <: a point at exactly the radius is outside
    xyz[0, 0] = (0.5, 0, 0)
    out = pn.ball_query(np.zeros((1, 1, 3), F32), xyz, 0.5, 3)
    assert out[0, 0].tolist() == [1, 2, 3]


def test_group_out_of_range_indices():
    pts = np.arange(12, dtype=F32).reshape(1, 2, 6) + 1
    idx = np.array([[[0, 5, 6, -1]]], np.int32)
    out = pn.group(pts, idx)
    assert out[0, :, 0].tolist() == [[1, 6, 0, 0], [7, 12, 0, 0]]
    g = pn.group_grad(np.ones((1, 2, 1, 4)), idx, 6)
    assert g[0, 0].tolist() == [1, 0, 0, 0, 0, 1]


def test_points_in_boxes_double_faces(libm):
    v = 0.5 + np.float64(F32(1e-5))  # dx / 2.0 + MARGIN in double, dx = 1
    inside_x = np.nextafter(F32(v), F32(0)) if F32(v) >= v else F32(v)
    outside_x = np.nextafter(inside_x, F32(1))
    box = np.array([[[0, 0, 0, 1, 1, 2, 0]]], F32)
    pts = np.array([[[inside_x, 0, 0], [outside_x, 0, 0], [0, 0, 1], [0, 0, np.nextafter(F32(1), F32(2))],
                     [-inside_x, 0, -1]]], F32)
    out = pn.points_in_boxes(pts, box, libm)
    assert out[0].tolist() == [0, -1, 0, -1, 0]
    # zero boxes: everything -1; first box in index order wins
    assert pn.points_in_boxes(pts, np.zeros((1, 0, 7), F32), libm)[0].tolist() == [-1] * 5
    two = np.concatenate([box, box], 1)
    assert pn.points_in_boxes(pts, two, libm)[0].tolist() == [0, -1, 0, -1, 0]
