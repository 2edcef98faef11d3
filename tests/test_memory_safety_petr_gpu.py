"""PETR's entry points (the rows of paddle3d_amd._lib.ENTRY_POINTS that name this module) under guarded
allocations: tests/guarded.py's Protocol.  Each scenario builds seeded inputs and returns `(inputs, call)`; it runs
plain, guarded with fill 0x00 and guarded with fill 0xFF (tests/guarded.py), and the test asserts: no guard band damaged
(no store outside an output), every input bit-equal to its clone, every output bit-equal across the three runs (nothing
depends on what a buffer held before -- the padded key tiles and query rows of the streamed attention included, since
they end in the output) and not trivial.  The kernels take no workspace.  The model scenario constructs the head inside
the run, so its tensors are allocated under the guard too.

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

import make_petr_golden as mk  # noqa: E402
import test_petr_cpu as cpu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32

P = Protocol("test_memory_safety_petr_gpu", "memory-safety-petr", DEV)
scenario = P.scenario


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@scenario
def ops():
    """The two ops at the tile borders: attention with Nq = 17 (a second query block of one row) and Nk = 65 (a second
    round of one key) and Nk = 3 (three waves without a tile), d = 16 and 128, with and without a mask, and at the golden
    case a; the coordinates with W = 65 (a second workgroup of one column) and D = 5 (the four d-groups uneven), W = 1,
    with and without the mask outputs, both LID settings, and at the golden case c."""
    from paddle3d_amd.ops import petr

    rng = np.random.default_rng(23)
    f = lambda *s: _t(rng.standard_normal(s).astype(F32))  # noqa: E731
    inputs = {}
    for d, heads, Nk in ((16, 3, 65), (128, 1, 3)):
        inputs.update({f"q{d}": f(2, 17, heads * d), f"k{d}": f(2, Nk, heads * d), f"v{d}": f(2, Nk, heads * d),
                       f"m{d}": _t(rng.random((2, Nk)) < 0.4)})
    inputs.update(zip(("a_q", "a_k", "a_v", "a_m"), (_t(a) for a in cpu.ca_inputs("a"))))
    mats = mk.inputs("a")["img2lidars"].reshape(-1, 4, 4)
    inputs.update(mats=_t(mats[:3]), tm65=_t(rng.random((3, 2, 65)) < 0.3), c_mats=_t(mk.inputs("c")["img2lidars"]))
    r = [-20.0, -15.0, -6.0, 20.0, 25.0, 6.0]

    def call():
        i, outs = inputs, {}
        for d, heads in ((16, 3), (128, 1)):
            outs[f"mha{d}"] = petr.multihead_attention_stream(i[f"q{d}"], i[f"k{d}"], i[f"v{d}"], heads)
            outs[f"mha{d}_masked"] = petr.multihead_attention_stream(i[f"q{d}"], i[f"k{d}"], i[f"v{d}"], heads, i[f"m{d}"])
        outs["a_mha"] = petr.multihead_attention_stream(i["a_q"], i["a_k"], i["a_v"], mk.HEADS, i["a_m"])
        outs["co65"], m65 = petr.petr_coords3d(i["mats"], (2, 65), (16, 520), 5, 1.0, r, True, token_mask=i["tm65"],
                                               want_mask=True)
        outs["co1"] = petr.petr_coords3d(i["mats"], (3, 1), (24, 8), 2, 0.5, r, False)
        c = mk.CASES["c"]
        outs["c_co"], mc = petr.petr_coords3d(i["c_mats"], mk.FEAT, mk.PAD, mk.D, c["depth_start"], c["position_range"],
                                              c["LID"], want_mask=True)
        outs["m65"], outs["c_m"] = m65.to(torch.uint8), mc.to(torch.uint8)
        return outs

    return inputs, call


@scenario
def model():
    """The head and the decode of case b (every option on), fused and unfused, built inside the run."""
    args = cpu.forward_args("b", DEV)

    def call():
        outs = {}
        for fused in (True, False):
            head = cpu.build_head("b", fused).to(DEV)
            with torch.no_grad():
                preds = head(*args)
                det = head.get_bboxes(preds)
            outs.update({f"cls_{fused}": preds["all_cls_scores"], f"bbox_{fused}": preds["all_bbox_preds"]})
            outs.update({f"{k}_{fused}": v for k, v in zip(("boxes", "scores", "labels", "count"), det)})
        return outs

    return dict(feats=args[0][0], img2lidars=args[1], timestamp=args[4]), call


@pytest.mark.parametrize("name", list(P.scenarios))
def test_scenario(name):
    P.check_scenario(name)


def test_every_launching_entry_point_is_exercised():
    """Runs last; scenarios that did not run in this process are run here in their plain form."""
    from paddle3d_amd import _lib

    P.check_complete(_lib.symbols("test_memory_safety_petr_gpu"), 2)
