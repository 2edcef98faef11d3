"""What tests/box_families.py is for, pinned on the oracle port (no GPU): the cluster families fill every polygon size
of box_overlap's LDS path (9 ... 16 vertices), no pair of any family exceeds 16 vertices (beyond that the reference
writes past its array and the device bounds the append: nothing to compare, so the GPU tests filter nothing out), IoU
reaches and exceeds 1.0, and the NMS threshold decides how many boxes of a mixture survive.  If a generator change
breaks one of these, the generator is what gets fixed."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import box_families as bf  # noqa: E402

N = 129


def _upper(m):
    return m[np.triu_indices(m.shape[0], 1)]


@pytest.fixture(scope="module")
def census(oracle):
    """family -> [(vertex histogram, upper-triangle IoU) per pinned seed] at n = 129."""
    out = {}
    for name, gen in bf.FAMILIES.items():
        rows = []
        for seed in bf.SEEDS[name]:
            b = gen(seed, N)
            assert b.dtype == np.float32 and b.shape == (N, 7)
            np.testing.assert_array_equal(b.view(np.uint32), gen(seed, N).view(np.uint32))  # deterministic
            hist = np.bincount(_upper(oracle.overlap_vertices(b, b)), minlength=25)
            rows.append((hist, _upper(oracle.boxes_iou_bev(b, b))))
        out[name] = rows
    return out


@pytest.mark.parametrize("name", list(bf.CLUSTERS))
def test_clusters_fill_the_lds_path(census, name):
    hist = sum(h for h, _ in census[name])
    print(name, "vertex histogram 0..16:", hist[:17].tolist(), "above 16:", int(hist[17:].sum()))
    assert (hist[9:17] > 0).all(), hist[:17]
    # and the first pinned seed does so on its own
    assert (census[name][0][0][9:17] > 0).all(), census[name][0][0][:17]
    for h, _ in census[name]:
        assert h[9:17].sum() > 1000, h[:17]  # no seed leaves the LDS path to a handful of its 8256 pairs


@pytest.mark.parametrize("name", list(bf.FAMILIES))
def test_no_pair_exceeds_16_vertices(oracle, census, name):
    for h, _ in census[name]:
        assert h[17:].sum() == 0, h
    # every set tests/test_iou_degenerate_gpu.py draws, not only n = 129; whole matrices: both argument orders
    for seed in bf.SEEDS[name]:
        for n in bf.NMS_SIZES + bf.POOL_SIZES:
            b = bf.FAMILIES[name](seed, n)
            assert oracle.overlap_vertices(b, b).max() <= 16, (name, seed, n)


@pytest.mark.parametrize("fams", bf.PAIRWISE, ids=lambda f: f"{f[0]}-{f[1]}")
def test_pairwise_cases_stay_comparable_and_reach_the_lds_path(oracle, fams):
    for sizes in bf.PAIRWISE_SIZES:
        a, b = bf.pairwise_case(*fams, *sizes)
        assert a.shape == (sizes[0], 7) and b.shape == (sizes[1], 7) and a.dtype == b.dtype == np.float32
        v = oracle.overlap_vertices(a, b)
        assert v.max() <= 16, (fams, sizes)
        assert sizes == (1, 1) or (v >= 9).any(), (fams, sizes)


@pytest.mark.parametrize("name", list(bf.CLUSTERS))
def test_clusters_reach_and_exceed_iou_one(census, name):
    ious = [iou for _, iou in census[name]]
    for iou in ious:
        assert (iou > 1.0).any()
    assert any((iou == 1.0).any() for iou in ious)
    print(name, "largest IoU", max(float(iou.max()) for iou in ious))


def test_lattice_and_specials_hold_their_cases(oracle):
    b = bf.axis_aligned_lattice(0, 28)  # two whole cells
    v = oracle.overlap_vertices(b, b)
    hist = np.bincount(_upper(v), minlength=17)
    assert hist[4] > 0 and hist[8] > 0 and hist[0] > 0, hist  # nested, turned squares / coincident, apart
    assert set(np.unique(b[:14 * 2, 6])) >= {np.float32(0), np.float32(np.pi / 2), np.float32(np.pi),
                                            np.float32(-np.pi / 2)}
    s = bf.specials(0, 12)
    assert np.isnan(s[:, 0]).sum() == 1 and np.isinf(s[:, 3]).sum() == 1 and (s[:, 3] < 0).sum() == 2
    assert (s[:, 3] == 0).sum() == 2 and (s[:, 4] == 0).sum() == 2 and (s[:, 0] == 1e4).sum() >= 1
    iou = oracle.boxes_iou_bev(s, s)
    assert np.nanmax(iou) > 1e8  # negative extents: the eps clamp of the union


def test_mixture_threshold_matters(oracle):
    for seed in bf.SEEDS["mixture"]:
        b = bf.mixture(seed, 300)
        kept = [len(oracle.nms(b, thr)) for thr in (0.1, 0.5, 0.999)]
        assert kept[0] < kept[1] < kept[2] < 300, kept
        assert kept[0] > 4  # several kept boxes per set
