"""SqueezeSegV3's entry points (the rows of paddle3d_amd._lib.ENTRY_POINTS that name this module) under guarded
allocations: tests/guarded.py's Protocol.  Each scenario builds seeded inputs and returns `(inputs, call)`; it runs plain,
guarded with fill 0x00 and guarded with fill 0xFF (tests/guarded.py), and the test asserts: no guard band damaged (no
store outside an output), every input bit-equal to its clone, every output bit-equal across the three runs (nothing
depends on what a buffer held before -- the masked pixels of a partial 16-pixel segment and the projection's workspace,
which the entry point fills itself, included) and not trivial.  The model scenario constructs the network inside the
run, so its tensors are allocated under the guard too.

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

import make_squeezeseg_golden as mk  # noqa: E402
import test_squeezeseg_cpu as cpu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32

P = Protocol("test_memory_safety_squeezeseg_gpu", "memory-safety-squeezeseg", DEV)
scenario = P.scenario


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@scenario
def ops():
    """The block kernel at the segment borders: W = 17 (a second segment of one pixel) with H = 2 and C = 16, W = 65 (a
    second workgroup of one pixel) with C = 48, W = 4 (the vector store) with C = 64, and the golden case b32; the
    projection on the golden scans, on frames of which two are empty with bad points, and with H = 1, W = 2 (every point
    of a frame in one of two pixels; proj_y, all zero there, is left out of the outputs)."""
    from paddle3d_amd.ops import squeezeseg

    inputs, shapes = {}, ((16, 2, 2, 17), (48, 1, 3, 65), (64, 2, 1, 4))
    for C, N, H, W in shapes:
        p = cpu.block_params(C, C, big_z=True)
        xyz, feat = cpu.block_inputs(N, C, H, W, C + 1)
        inputs.update({f"xyz{C}": _t(xyz), f"feat{C}": _t(feat)})
        for k, v in zip(("w1p", "s_a", "t_a", "w2p", "s_m", "t_m"),
                        (squeezeseg.pack_sac_attention_weight(_t(p["w"])), _t(p["s_a"]), _t(p["t_a"]),
                         squeezeseg.pack_sac_mlp_weight(_t(p["v"])), _t(p["s_m"]), _t(p["t_m"]))):
            inputs[f"{k}{C}"] = v
    pts, off = mk.scans()
    bad = mk.scan(400, 4)
    bad[5, 0], bad[6, 1], bad[8, :3] = np.nan, np.inf, 0
    inputs.update(pts=_t(pts), off=_t(off), bad=_t(bad), bad_off=_t(np.array([0, 0, 250, 250, 400], np.int32)))

    def call():
        i, outs = inputs, {}
        for C, _, _, _ in shapes:
            outs[f"y{C}"] = squeezeseg.sac_isk_forward(i[f"xyz{C}"], i[f"feat{C}"], *(i[f"{k}{C}"] for k in
                                                       ("w1p", "s_a", "t_a", "w2p", "s_m", "t_m")))
        for name, (p, o, H, W) in dict(scans=(i["pts"], i["off"], mk.SCAN_H, mk.SCAN_W), bad=(i["bad"], i["bad_off"], 5, 33),
                                       one=(i["pts"], i["off"], 1, 2)).items():
            res = squeezeseg.range_project(p, o, H, W, 3.0, -25.0, mk.MEAN, mk.STD)
            for k, v in zip(("image", "idx", "mask", "py", "px"), res):
                if (name, k) != ("one", "py"):
                    outs[f"{name}_{k}"] = v.to(torch.uint8) if v.dtype == torch.bool else v
        return outs

    return inputs, call


@scenario
def model():
    """SqueezeSegV3 on a SACRangeNet21 (the golden case), fused at every block and unfused, built inside the run, on the projection of
    the golden scans: the prediction and the per-point labels, and the first block's kernel output on the image.  The
    logits are not among the outputs: torch's own operators around the blocks are not bitwise reproducible from call to
    call on the device (the logits of the unfused network, torch operators only, differ between any two calls by an ulp
    or two in a quarter of the elements), which is no dependence on stale memory; the golden case keeps every
    prediction further from a tie than that."""
    from paddle3d_amd.ops import squeezeseg

    pts, off = mk.scans()
    rng = np.random.default_rng(8)
    inputs = dict(pts=_t(pts), off=_t(off), image=_t(mk.inputs("net")["image"]),
                  feat=_t(rng.standard_normal((2, 32, 8, 32)).astype(F32)))

    def call():
        outs = {}
        img, _, _, py, px = squeezeseg.range_project(inputs["pts"], inputs["off"], 8, 32, 3.0, -25.0, mk.MEAN, mk.STD)
        for fused in ("force", False):
            net = cpu.build("net", fused, DEV)
            with torch.no_grad():
                outs[f"pred_{fused}"] = net.export_forward(inputs["image"])
                outs[f"labels_{fused}"] = net(inputs["image"], py, px, inputs["off"])
                if fused:
                    block = net.backbone.encoder.encoder_stages[0].layers[0]
                    outs["block_y"] = block.first_layer(inputs["image"][:, 1:4].contiguous(), inputs["feat"])
        return outs

    return inputs, call


@pytest.mark.parametrize("name", list(P.scenarios))
def test_scenario(name):
    P.check_scenario(name)


def test_every_launching_entry_point_is_exercised():
    """Runs last; scenarios that did not run in this process are run here in their plain form."""
    from paddle3d_amd import _lib

    P.check_complete(_lib.symbols("test_memory_safety_squeezeseg_gpu"), 2)
