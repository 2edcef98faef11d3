"""The deformable convolution's entry point (paddle3d_amd._lib.DCN_ENTRY_POINTS, whose row names this module) under
guarded allocations: tests/guarded.py's Protocol.  Each scenario builds seeded inputs and returns `(inputs, call)`; it
runs plain, guarded with fill 0x00 and guarded with fill 0xFF, and the test asserts: no guard band damaged (no store
outside an output -- the padded pixels of a last tile and the channel tiles past Cout included), every input bit-equal to
its clone, every output bit-equal across the three runs (nothing depends on what a buffer held before) and not trivial.
The kernel takes no workspace.  The model scenario constructs the modules inside the run, so their tensors, the packed
weights and the folded statistics are allocated under the guard too.

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

import make_dcn_golden as mk  # noqa: E402
import test_dcn_cpu as cpu  # noqa: E402
import test_dcn_gpu as gpu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32

P = Protocol("test_memory_safety_dcn_gpu", "memory-safety-dcn", DEV)
scenario = P.scenario

# (N, Cin, Cout, H, W, stride, padding, dilation): one pixel; a tile of two pixels behind a full one, 17 channel tiles (the
# last workgroup of grid.y holds one); an odd output count (single-float stores) across three images; stride 2 with
# dilation 2; 4096 pixels x 512 channels: the form with two channel tiles per wave
SHAPES = ((1, 16, 16, 1, 1, 1, 1, 1), (2, 16, 272, 3, 11, 1, 1, 1), (3, 48, 48, 5, 9, 1, 1, 1), (1, 16, 32, 9, 12, 2, 2, 2),
          (2, 16, 512, 64, 64, 1, 1, 1))


@scenario
def op():
    """The entry point at the border shapes of tests/test_dcn_gpu.py: without a mask, with one, with logits and every
    epilogue, offset and mask as views of one map; hostile offsets (out of range, Inf, NaN) at the second shape."""
    from paddle3d_amd.ops import deform_conv as ops

    inputs, cases = {}, []
    for i, (N, ci, co, H, W, s, p, d) in enumerate(SHAPES):
        c = gpu.random_case(40 + i, N, ci, co, H, W, s, p, d)
        if i == 1:
            rng = np.random.default_rng(41)
            values = np.array([0, -1, 0.5, 3, 1e30, -1e30, np.inf, -np.inf, np.nan], F32)
            c["offset"] = values[rng.integers(0, values.size, c["offset"].shape)]
        cases.append(c)
        inputs.update({f"x{i}": gpu._t(c["x"]), f"om{i}": gpu._t(np.concatenate([c["offset"], c["mask"]], 1)),
                       f"w{i}": gpu._t(c["w"]), f"scale{i}": gpu._t(c["scale"]), f"shift{i}": gpu._t(c["shift"])})

    def call():
        t, outs = inputs, {}
        for i, c in enumerate(cases):
            packed = ops.pack_deform_conv_weight(t[f"w{i}"])
            offset, mask = t[f"om{i}"][:, :18], t[f"om{i}"][:, 18:]
            geom = (c["stride"], c["padding"], c["dilation"])
            outs[f"v1_{i}"] = ops.deform_conv2d_packed(t[f"x{i}"], offset, None, packed, None, None, False, False, *geom)
            outs[f"given_{i}"] = ops.deform_conv2d_packed(t[f"x{i}"], offset, mask, packed, None, t[f"shift{i}"], False,
                                                          False, *geom)
            outs[f"logit_{i}"] = ops.deform_conv2d_packed(t[f"x{i}"], offset, mask, packed, t[f"scale{i}"],
                                                          t[f"shift{i}"], True, True, *geom)
        outs["paddle"] = ops.deform_conv2d(t["x2"], t["om2"][:, :18].contiguous(), t["w2"], t["shift2"], 1, 1, 1, 1, 1,
                                           torch.sigmoid(t["om2"][:, 18:]))
        return outs

    return inputs, call


@scenario
def model():
    """DeformableConvV2 of the golden cases b2 and c, the bottleneck bb and the two-block stage, forced and unfused, built
    inside the run."""
    g = mk.load()
    inputs = {tag: gpu._t(mk.inputs(tag)) for tag in ("b2", "c", "bb", "s")}

    def call():
        outs = {}
        for fused in ("force", False):
            for tag, x in inputs.items():
                m = cpu.build(g, tag, fused).to(DEV)
                with torch.no_grad():
                    outs[f"{tag}_{fused}"] = m(x)
        return outs

    return inputs, call


@pytest.mark.parametrize("name", list(P.scenarios))
def test_scenario(name):
    P.check_scenario(name)


def test_every_launching_entry_point_is_exercised():
    """Runs last; scenarios that did not run in this process are run here in their plain form."""
    from paddle3d_amd import _lib

    P.check_complete(_lib.symbols("test_memory_safety_dcn_gpu"), 1)
