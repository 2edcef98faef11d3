"""DD3D's entry points (the rows of paddle3d_amd._lib.ENTRY_POINTS that name this module) under guarded allocations:
tests/guarded.py's Protocol.  Each scenario builds seeded inputs and returns `(inputs, call)`; it runs plain, guarded
with fill 0x00 and guarded with fill 0xFF, and the test asserts: no guard band damaged (no store outside an output or
the workspace), every input bit-equal to its clone, every output bit-equal across the three runs (nothing depends on
what an output or the workspace held before: the rows past an image's count, the keys, the selection lists, the
candidates, the bit matrix and the keep lists included) and not trivial.  The points include maps whose width is no
multiple of 4 (dense rows and rows of padded pitch in one stacked map), a 1 x 1 level, an image without a candidate,
pre_nms_topk = 1024 and post_nms_topk = 0 (the row capacity is levels * pre_nms_topk).  The model scenario constructs
the model inside the run, so its packed weights are allocated under the guard too.

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

import dd3d_numpy as dn  # noqa: E402
import test_dd3d_cpu as cpu  # noqa: E402
import test_dd3d_gpu as gpu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32

P = Protocol("test_memory_safety_dd3d_gpu", "memory-safety-dd3d", DEV)
scenario = P.scenario

# (shapes, strides, C, nc, ncp, wl, B, cfg)
POINTS = (
    (((5, 7), (3, 4), (1, 1)), (8, 16, 32), 16, 3, 3, 1, 2, dict(gpu.CFG)),
    (((6, 10), (3, 5), (2, 3), (1, 2), (1, 1)), (8, 16, 32, 64, 128), 32, 5, 1, 5, 3, dict(gpu.CFG, offset="half")),
    (((9, 33),), (8,), 16, 4, 4, 1, 1, dict(gpu.CFG, pre_nms_topk=1024, post_nms_topk=0, pre_nms_thresh=0.02)),
)


@scenario
def ops():
    """Both entry points at POINTS: the lazy form from dense tower outputs and from one stacked map of padded pitch, the
    from-maps form from the restatement's maps, and the lazy form without a 3D head.  Image 1 of the first point has no
    candidate."""
    jobs = []
    for i, (shapes, strides, C, nc, ncp, wl, B, cfg) in enumerate(POINTS):
        rng = np.random.default_rng(60 + i)
        levels = gpu.sweep_levels(rng, B, C, nc, shapes)
        if i == 0:
            for lv in levels:
                lv["logits"][1] = -20.0
        packed = gpu.sweep_packed(rng, C, nc, len(shapes), strides, ncp, wl)
        jobs.append((f"p{i}", levels, strides, packed, gpu.sweep_camera(B), cfg, dn.dense_levels(levels, packed)))
    inputs = {}
    for name, levels, strides, packed, K, cfg, dense in jobs:
        for l, (lv, dv) in enumerate(zip(levels, dense)):
            inputs.update({f"{name}_{l}_{k}": gpu._t(v) for k, v in lv.items()})
            inputs.update({f"{name}_{l}_dense_{k}": gpu._t(v) for k, v in dv.items() if k not in lv})

    def call():
        outs = {}
        for name, levels, strides, packed, K, cfg, dense in jobs:
            flat = [{k: v for k, v in lv.items() if k != "f3d"} for lv in levels]
            p2d = {k: v for k, v in packed.items() if k in ("w2d", "b2d", "scales")}
            for kind, res in (("lazy", gpu.lazy(levels, strides, packed, K, dn.CANON, cfg)),
                              ("stacked", gpu.lazy(levels, strides, packed, K, dn.CANON, cfg, stacked=True)),
                              ("maps", gpu.from_maps(dense, strides, K, dn.CANON, cfg)),
                              ("box2d", gpu.lazy(flat, strides, p2d, None, None, cfg))):
                outs[f"{name}_{kind}_rows"], outs[f"{name}_{kind}_counts"] = res
        return outs

    return inputs, call


@scenario
def model():
    """The module on two golden cases, built inside the run: the lazy path, the dense path and the torch transcription."""
    x = {f"{tag}_{l}": gpu._t(f) for tag in ("v2_l5", "v1_l3") for l, f in enumerate(dn.golden_inputs(tag))}

    def call():
        outs = {}
        for tag in ("v2_l5", "v1_l3"):
            m = cpu.build_model(tag).to(DEV)
            for fused in ("lazy", "dense", False):
                outs[f"{tag}_{fused}_rows"], outs[f"{tag}_{fused}_counts"] = cpu.run_model(m, tag, DEV, fused=fused)
        return outs

    return x, call


@pytest.mark.parametrize("name", list(P.scenarios))
def test_scenario(name):
    P.check_scenario(name)


def test_every_launching_entry_point_is_exercised():
    """Runs last; scenarios that did not run in this process are run here in their plain form."""
    from paddle3d_amd import _lib

    P.check_complete(_lib.symbols("test_memory_safety_dd3d_gpu"), 3)
