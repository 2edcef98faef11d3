"""Anchor3DHead's entry points (the rows of paddle3d_amd._lib.ENTRY_POINTS that name this module) under guarded
allocations: tests/guarded.py's Protocol.  Each scenario builds seeded inputs and returns `(inputs, call)`; it runs plain,
guarded with fill 0x00 and guarded with fill 0xFF (tests/guarded.py), and the test asserts: no guard band damaged (no
store outside an output or the workspace), every input bit-equal to its clone, every output bit-equal across the three
runs (nothing depends on what an output or the workspace held before: the rows past a frame's count, the unused ends of
the candidate lists, the NMS matrix and the pool included) and not trivial.  The model scenario constructs the head
inside the run, so its packed weights and anchor table are allocated under the guard too.

The last test asserts that the scenarios reach every one of them."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from guarded import Protocol  # noqa: E402

import anchor3d_numpy as an  # noqa: E402
import make_anchor3d_golden as mk  # noqa: E402
import test_anchor3d_cpu as cpu  # noqa: E402
import test_anchor3d_gpu as gpu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32

P = Protocol("test_memory_safety_anchor3d_gpu", "memory-safety-anchor3d", DEV)
scenario = P.scenario


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# (H, W, C, A, nc, cs, nms_pre, max_num): a partial wave tile and a second workgroup, K = 1, K = N, three chunks
POINTS = ((17, 15, 48, 14, 10, 9, 65, 5), (1, 1, 16, 1, 1, 7, 1000, 1), (4, 33, 16, 6, 3, 9, 4 * 33 * 6, 500),
          (3, 5, 16, 32, 16, 7, 200, 500))


@scenario
def ops():
    """Both entry points at the tile borders (POINTS) and on the two golden cases; frame 1 of the first point has no
    detection (rows of zeros) and its score_thr empties most classes."""
    from paddle3d_amd.ops import anchor3d_head as A

    inputs, jobs = {}, []
    for i, (H, W, C, na, nc, cs, pre, mx) in enumerate(POINTS):
        rng = np.random.default_rng(40 + i)
        anchors, st = gpu.sweep_anchors(rng, H, W, na, cs), gpu.sweep_state(rng, C, na, nc, cs)
        feat = rng.standard_normal((2, C, H, W)).astype(F32)
        if i == 0:
            feat[1] = 0.0
        cfg = dict(nms_pre=pre, max_num=mx, score_thr=0.6 if i == 0 else 0.3, nms_thr=0.2, dir_offset=0.7854,
                   dir_limit_offset=0.0, num_classes=nc)
        jobs.append((f"p{i}", feat, st, anchors, cfg))
    for tag in an.TAGS:
        jobs.append((tag, an.golden_inputs(tag), an.golden_state(tag), mk.anchors_of(tag), an.cfg_of(tag)))
    for name, feat, st, anchors, cfg in jobs:
        inputs[name + "_feat"], inputs[name + "_anchors"] = _t(feat), _t(anchors)
        for k, v in st.items():
            inputs[f"{name}_{k}"] = _t(v)
        for k, m in zip(("cls", "reg", "dir"), an.head_maps(feat, st)):
            inputs[f"{name}_{k}_map"] = _t(m)

    def call():
        outs = {}
        for name, _, _, _, cfg in jobs:
            i = lambda k: inputs[f"{name}_{k}"]  # noqa: E731
            c = (cfg["num_classes"], cfg["nms_pre"], cfg["max_num"], cfg["score_thr"], cfg["nms_thr"], cfg["dir_offset"],
                 cfg["dir_limit_offset"])
            packed = A.pack_cls_weight(i("conv_cls.weight"), cfg["num_classes"])
            lazy = A.anchor3d_head_forward(i("feat"), packed, i("conv_cls.bias"), i("conv_reg.weight"), i("conv_reg.bias"),
                                           i("conv_dir_cls.weight"), i("conv_dir_cls.bias"), i("anchors"), *c)
            maps = A.anchor3d_get_bboxes(i("cls_map"), i("reg_map"), i("dir_map"), i("anchors"), *c)
            for kind, res in (("lazy", lazy), ("maps", maps)):
                outs.update({f"{name}_{kind}_{k}": v for k, v in zip(("boxes", "scores", "labels", "counts"), res)})
        # p1 is a single anchor of a single class: label 0
        outs["__trivial_ok__"] = {k for k in outs if k.startswith("p1_") and k.endswith("labels")}
        return outs

    return inputs, call


@scenario
def model():
    """The module on the nuScenes-like golden case, built inside the run: the lazy path, forward + the from-maps path,
    and the unfused transcription."""
    x = _t(an.golden_inputs("nus"))

    def call():
        head = cpu.build_head("nus").to(DEV)
        outs = {}
        with torch.no_grad():
            for name, fused in (("lazy", "force"), ("unfused", False)):
                res = head.forward_get_bboxes([x], [{}] * 2, fused=fused, return_padded=True)
                outs.update({f"{name}_{k}": v for k, v in zip(("boxes", "scores", "labels", "counts"), res)})
            res = head.get_bboxes(*head([x]), [{}] * 2, return_padded=True)
            outs.update({f"maps_{k}": v for k, v in zip(("boxes", "scores", "labels", "counts"), res)})
        return outs

    return dict(feat=x), call


@pytest.mark.parametrize("name", list(P.scenarios))
def test_scenario(name):
    P.check_scenario(name)


def test_every_launching_entry_point_is_exercised():
    """Runs last; scenarios that did not run in this process are run here in their plain form."""
    from paddle3d_amd import _lib

    P.check_complete(_lib.symbols("test_memory_safety_anchor3d_gpu"), 3)
