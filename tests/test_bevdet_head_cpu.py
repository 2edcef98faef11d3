"""BEVDet4D CenterHead post-processing without a GPU: the C ABI is declared and exported, and the NumPy restatement
the GPU tests compare the device operator with bit for bit reproduces the reference's own outputs
(tests/golden/python_bevdet_head.npz, made by tests/golden/make_bevdet_head_golden.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import bevdet_head_numpy as bh  # noqa: E402

SYMBOLS = ("pd3_bevdet_postprocess_workspace", "pd3_bevdet_postprocess", "pd3_circle_nms_workspace", "pd3_circle_nms")


@pytest.fixture(scope="module")
def built():
    from paddle3d_amd import build

    return build.build()


def test_header_declares_and_library_exports(built):
    hdr = open(os.path.join(ROOT, "include", "paddle3d_amd.h")).read()
    declared = set(re.findall(r"\b(pd3_\w+)\s*\(", hdr))
    out = subprocess.check_output(["nm", "-D", "--defined-only", built], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for s in SYMBOLS:
        assert s in declared, s
        assert s in exported, s
    from paddle3d_amd import _lib

    L = _lib.lib()
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None


def test_python_layers_import():
    from paddle3d_amd import bevdet_head, ops

    assert ops.bevdet_postprocess.circle_nms is not None
    cfg = bevdet_head.BEVDET4D_TEST_CFG
    assert cfg["nms_type"][3] == "circle" and cfg["post_max_size"] == 83 and cfg["pre_max_size"] == 1000
    assert cfg["nms_rescale_factor"] == [1.0, [0.7, 0.7], [0.4, 0.55], 1.1, [1.0, 1.0], [4.5, 9.0]]
    assert bevdet_head.BEVDET4D_BBOX_CODER["max_num"] == 500


def test_workspace_query_needs_no_gpu(built):
    from paddle3d_amd import _lib
    from paddle3d_amd.ops._common import ptr

    L = _lib.lib()
    ncls = np.array([1, 2, 2, 1, 2, 2], np.int32)
    ws = L.pd3_bevdet_postprocess_workspace(8, 6, ptr(ncls), 128, 128, 500)
    assert 48 * 2 * 128 * 128 * 4 <= ws < 256 * 2**20
    assert L.pd3_bevdet_postprocess_workspace(8, 6, ptr(ncls), 128, 128, 2000) == 0  # max_num beyond the list
    assert L.pd3_bevdet_postprocess_workspace(1, 1, ptr(ncls), 8192, 4096, 500) == 0  # H*W > 2^24
    assert L.pd3_circle_nms_workspace(1000) > 1000 * 16 * 8
    assert L.pd3_circle_nms_workspace(0) == 0


def test_numpy_restatement_reproduces_reference_golden(oracle):
    gold = np.load(os.path.join(HERE, "golden", "python_bevdet_head.npz"))
    res = bh.get_bboxes(oracle, bh.golden_inputs(), bh.GOLDEN_TEST_CFG, bh.GOLDEN_CODER, bh.GOLDEN_TASKS)
    assert len(res) == bh.GOLDEN_BATCH
    for i, (b, s, l) in enumerate(res):
        assert b.shape == gold[f"bboxes_{i}"].shape
        np.testing.assert_array_equal(l, gold[f"labels_{i}"])
        np.testing.assert_allclose(s, gold[f"scores_{i}"], rtol=0, atol=2e-7)
        np.testing.assert_allclose(b, gold[f"bboxes_{i}"], rtol=2e-6, atol=2e-6)
    # the golden exercises what it is meant to: the circle task hits post_max_size, the rotate tasks remove boxes
    labels = gold["labels_0"]
    post = bh.GOLDEN_TEST_CFG["post_max_size"]
    assert int((labels == 3).sum()) == post
    assert all(0 < int(((labels == a) | (labels == b)).sum()) < post for a, b in ((0, 0), (1, 2), (4, 5)))


def test_circle_keep_matches_plain_loop():
    rng = np.random.default_rng(5)
    xy = rng.uniform(-5, 5, (300, 2)).astype(np.float32)
    keep = bh.circle_keep(xy, 0.85)
    supp = np.zeros(300, bool)
    ref = []
    for i in range(300):
        if supp[i]:
            continue
        ref.append(i)
        for j in range(i + 1, 300):
            d = (xy[i, 0] - xy[j, 0]) ** 2 + (xy[i, 1] - xy[j, 1]) ** 2
            if float(d) <= 0.85:
                supp[j] = True
    np.testing.assert_array_equal(keep, ref)
