"""SMOKE's entry points (the rows of paddle3d_amd._lib.ENTRY_POINTS that name this module) under guarded allocations:
tests/guarded.py's Protocol.  Each scenario builds seeded inputs and returns `(inputs, call)`; it runs plain, guarded
with fill 0x00 and guarded with fill 0xFF, and the test asserts: no guard band damaged (no store outside an output or
the workspace), every input bit-equal to its clone, every output bit-equal across the three runs (nothing depends on
what an output or the workspace held before: the rows past a frame's count, the tables, the heat map, the keys and the
regression values included) and not trivial.  The points include maps whose width is not a multiple of 4 (dense rows
and rows of padded pitch in one stacked map) and K = H * W.  The model scenario constructs the model inside the run, so
its packed weights are allocated under the guard too.

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

import smoke_numpy as sn  # noqa: E402
import test_smoke_cpu as cpu  # noqa: E402
import test_smoke_gpu as gpu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32

P = Protocol("test_memory_safety_smoke_gpu", "memory-safety-smoke", DEV)
scenario = P.scenario

# (H, W, C, groups, nc, K, B, mode): widths 7, 33 and 129 (no multiple of 4), K = H * W, K = 1024, one pixel
POINTS = ((5, 7, 48, 16, 3, 35, 2, "forward"), (1, 1, 16, 16, 1, 1, 1, "export"), (4, 33, 64, 32, 16, 132, 3, "export"),
          (9, 129, 32, 32, 2, 1024, 1, "forward"), (17, 15, 256, 32, 3, 50, 2, "forward"))


@scenario
def ops():
    """Both entry points at POINTS: the lazy head from dense maps and from one stacked map of padded pitch (GroupNorm
    and given tables), the from-maps form from the restatement's maps.  Frame 1 of the first point has no detection."""
    jobs = []
    for i, (H, W, C, G, nc, K, B, mode) in enumerate(POINTS):
        rng = np.random.default_rng(60 + i)
        cf, rf = (rng.standard_normal((B, C, H, W)).astype(F32) + F32(0.5) for _ in range(2))
        st, cam = gpu.sweep_state(rng, C, nc), gpu.sweep_camera(B, H, W, nc)
        if i == 0:
            cf[1] = 0.0
            st["class_head.1.bias"][:] = 0
        cfg = dict(max_detection=K, det_threshold=0.3, mode=mode)
        tables = tuple(np.stack([rng.standard_normal((B, G)) * 0.1, rng.uniform(0.8, 1.2, (B, G))], 1).astype(F32)
                       for _ in range(2))
        heat = sn.class_heat(cf, tables[0], st["class_head.1.weight"], st["class_head.1.bias"], st["class_head.3.weight"],
                             st["class_head.3.bias"])
        reg = sn.activate(sn.regression_raw(rf, tables[1], st["regression_head.1.weight"], st["regression_head.1.bias"],
                                            st["regression_head.3.weight"], st["regression_head.3.bias"]))
        jobs.append((f"p{i}", cf, rf, st, cam, cfg, G, tables, heat, reg))
    inputs = {}
    for name, cf, rf, st, cam, cfg, G, tables, heat, reg in jobs:
        inputs.update({f"{name}_cf": gpu._t(cf), f"{name}_rf": gpu._t(rf), f"{name}_heat": gpu._t(heat),
                       f"{name}_reg": gpu._t(reg)})

    def call():
        outs = {}
        for name, cf, rf, st, cam, cfg, G, tables, heat, reg in jobs:
            for kind, res in (("gn", gpu.lazy(cf, rf, st, cam, cfg, G)),
                              ("stacked", gpu.lazy(cf, rf, st, cam, cfg, G, stacked=True)),
                              ("tables", gpu.lazy(cf, rf, st, cam, cfg, G, tables, stacked=True)),
                              ("maps", gpu.from_maps(heat, reg, cam, cfg))):
                outs[f"{name}_{kind}_rows"], outs[f"{name}_{kind}_counts"] = res
        return outs

    return inputs, call


@scenario
def model():
    """The module on two golden cases, built inside the run: the lazy path (one stacked Winograd launch), the dense
    path, the torch transcription, and PostProcessor.forward's [n, 15] tensor."""
    x = {tag: gpu._t(sn.golden_inputs(tag)) for tag in ("gn256", "bn256")}

    def call():
        outs = {}
        for tag in x:
            m = cpu.build_model(tag).to(DEV)
            for fused in ("lazy", "dense", False):
                outs[f"{tag}_{fused}_rows"], outs[f"{tag}_{fused}_counts"] = cpu.run_model(m, tag, DEV, fused=fused)
            cam = cpu.camera_tensors(tag, DEV)
            with torch.no_grad():
                outs[f"{tag}_result"] = m.post_process(m.heads(x[tag]), dict(K=cam["K"], trans_mat=cam["trans_mat"],
                                                                             image_size=cam["image_size"]))
        return outs

    return dict(x), call


@pytest.mark.parametrize("name", list(P.scenarios))
def test_scenario(name):
    P.check_scenario(name)


def test_every_launching_entry_point_is_exercised():
    """Runs last; scenarios that did not run in this process are run here in their plain form."""
    from paddle3d_amd import _lib

    P.check_complete(_lib.symbols("test_memory_safety_smoke_gpu"), 3)
