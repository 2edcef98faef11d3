"""The DepthNet entry points (paddle3d_amd._lib.DEPTHNET_ENTRY_POINTS, whose rows name this module) under guarded
allocations: tests/guarded.py's Protocol.  Each scenario builds seeded inputs and returns `(inputs, call)`; it runs plain,
guarded with fill 0x00 and guarded with fill 0xFF, and the test asserts: no guard band damaged (no store outside an
output or the workspace -- the padded pixels of a last tile and the channel tiles past Cmid included), every input
bit-equal to its clone, every output bit-equal across the three runs (nothing depends on what a buffer held before: the
workspace's branch maps and bias are written before they are read) and not trivial.  The model scenario constructs the
modules inside the run, so their tensors, the packed weights and the folded statistics are allocated under the guard too.

The last test asserts that the scenarios reach every row of the table."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from guarded import Protocol  # noqa: E402

import make_depthnet_golden as mk  # noqa: E402
import test_depthnet_cpu as cpu  # noqa: E402
import test_depthnet_gpu as gpu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32

P = Protocol("test_memory_safety_depthnet_gpu", "memory-safety-depthnet", DEV)
scenario = P.scenario

# (N, Cin, Cmid, H, W): one pixel; an odd pixel count (single-float stores) whose first tile ends inside the second image;
# 17 pixels behind a full tile with three channel tiles (the fourth wave of the workgroup holds none); 272 channels: the
# last workgroup of grid.y holds one tile; the model's map
ASPP_SHAPES = ((1, 16, 16, 1, 1), (3, 16, 16, 5, 9), (1, 48, 48, 9, 9), (2, 16, 272, 3, 11), (1, 16, 16, 16, 44))
# (N, D, C, H, W): one pixel; 65 pixels and two channel chunks; no context channel; the model's channel counts
TAIL_SHAPES = ((1, 1, 1, 1, 1), (2, 7, 80, 5, 13), (2, 4, 0, 3, 3), (2, 118, 80, 4, 11))


@scenario
def aspp():
    """pd3_aspp_workspace and pd3_aspp_forward at the border shapes, a NaN and an Inf pixel at the second."""
    from paddle3d_amd.ops import depthnet as ops

    inputs, cases = {}, []
    for i, (N, ci, cm, H, W) in enumerate(ASPP_SHAPES):
        c = gpu.random_case(40 + i, N, ci, cm, H, W)
        if i == 1:
            c["x"][0, 3, 2, 4], c["x"][1, 5, 0, 0] = np.nan, np.inf
        cases.append(c)
        inputs[f"x{i}"] = gpu._t(c["x"])
        for k, v in c["p"].items():
            if k == "w":
                inputs.update({f"w{i}_{b}": gpu._t(w) for b, w in enumerate(v)})
            else:
                inputs[f"{k}{i}"] = gpu._t(v)

    def call():
        t, outs = inputs, {}
        for i, c in enumerate(cases):
            cm, ci = c["p"]["wg"].shape
            pk = ops.pack_aspp([t[f"w{i}_{b}"] for b in range(4)],
                               [(t[f"scale{i}"][b * cm:(b + 1) * cm], t[f"shift{i}"][b * cm:(b + 1) * cm]) for b in range(4)],
                               t[f"wg{i}"].reshape(cm, ci, 1, 1), (t[f"gs{i}"], t[f"gb{i}"]),
                               t[f"w1{i}"].reshape(cm, 5 * cm, 1, 1), (t[f"s1{i}"], t[f"b1{i}"]))
            outs[f"y{i}"] = ops.aspp_forward(t[f"x{i}"], pk, c["dilations"])
        return outs

    return inputs, call


@scenario
def tail():
    """pd3_depth_softmax_split at the border shapes."""
    from paddle3d_amd.ops import depthnet as ops

    inputs = {f"x{i}": gpu._t((np.random.default_rng(60 + i).standard_normal((N, D + C, H, W)) * 3).astype(F32))
              for i, (N, D, C, H, W) in enumerate(TAIL_SHAPES)}

    def call():
        outs = {"__trivial_ok__": set()}
        for i, (N, D, C, H, W) in enumerate(TAIL_SHAPES):
            outs[f"depth{i}"], feat = ops.depth_softmax_split(inputs[f"x{i}"], D)
            if C:
                outs[f"feat{i}"] = feat
        return outs

    return inputs, call


@scenario
def model():
    """ASPP, DepthNet and the view transformer of the golden cases, forced and unfused, built inside the run."""
    g = mk.load()
    inputs = {"aspp_b": gpu._t(mk.inputs("aspp_b")[0]), "dn_x": gpu._t(mk.inputs("dn")[0]),
              "dn_mlp": gpu._t(mk.inputs("dn")[1])}
    vt = gpu._vt_input(g)
    inputs.update({f"vt{i}": v for i, v in enumerate(vt)})

    def call():
        outs = {}
        for fused in ("force", False):
            with torch.no_grad():
                outs[f"aspp_{fused}"] = cpu.build(g, "aspp_b", fused).to(DEV)(inputs["aspp_b"])
                outs[f"dn_{fused}"] = cpu.build(g, "dn", fused).to(DEV)(inputs["dn_x"], inputs["dn_mlp"])
                outs[f"bev_{fused}"], outs[f"depth_{fused}"] = cpu.build(g, "vt", fused).to(DEV)(vt)
        return outs

    return inputs, call


@pytest.mark.parametrize("name", list(P.scenarios))
def test_scenario(name):
    P.check_scenario(name)


def test_every_launching_entry_point_is_exercised():
    """Runs last; scenarios that did not run in this process are run here in their plain form."""
    from paddle3d_amd import _lib

    P.check_complete(_lib.symbols("test_memory_safety_depthnet_gpu"), 3)
