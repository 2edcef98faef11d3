"""The decoder's entry points (the rows of paddle3d_amd._lib.ENTRY_POINTS that name this module) under guarded
allocations: tests/guarded.py's Protocol.  Each scenario builds seeded inputs and returns `(inputs, call)`; it runs
plain, guarded with fill 0x00 and guarded with fill 0xFF (tests/guarded.py), and the test asserts: no guard band damaged
(no store outside an output), every input bit-equal to its clone, every output bit-equal across the three runs (nothing
depends on what a buffer held before -- the attention's LDS-backed score rows and padded tiles included, since they end
in the output) and not trivial.  The kernels take no workspace.  The model scenario constructs the head inside the run,
so its tensors are allocated under the guard too.

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

import bevformer_decoder_numpy as dn  # noqa: E402
import make_bevformer_decoder_golden as mk  # noqa: E402
import test_bevformer_decoder_cpu as cpu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32

P = Protocol("test_memory_safety_bevformer_dec_gpu", "memory-safety-bevformer-dec", DEV)
scenario = P.scenario


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@scenario
def ops():
    """The three ops at the tile borders: attention with Nq = 17 (a second query block of one row) and Nk = 33 (a third
    key tile of one key), d = 16 and 64, and at the golden case a; cross-attention with Q = 17 at C = 4 (one lane per
    group) and C = 32, one reference point and one per level; the decode with count 0 (every centre outside), with
    count = max_num = Q * K (every entry kept) and at the golden case c (the lowered threshold)."""
    from paddle3d_amd.ops import bevformer_decoder

    rng = np.random.default_rng(19)
    f = lambda *s: _t(rng.standard_normal(s).astype(F32))  # noqa: E731
    inputs = {}
    for d, heads in ((16, 3), (64, 1)):
        inputs.update({f"q{d}": f(2, 17, heads * d), f"k{d}": f(2, 33, heads * d), f"v{d}": f(2, 33, heads * d)})
    inputs.update(zip(("a_q", "a_k", "a_v"), (_t(a) for a in cpu.mha_inputs("a"))))
    sh, lsi, S = dn.md.level_layout([[3, 4], [2, 2]])
    inputs.update(sh=_t(sh), lsi=_t(lsi), value4=f(2, S, 3, 4), off4=f(2, 17, 3, 2, 4, 2), logits4=f(2, 17, 3, 8),
                  ref1=_t(rng.uniform(0, 1, (2, 17, 1, 2)).astype(F32)), value32=f(1, S, 2, 32), off32=f(1, 17, 2, 2, 16, 2),
                  logits32=f(1, 17, 2, 32), ref2=_t(rng.uniform(0, 1, (1, 17, 2, 2)).astype(F32)))
    cls, bbox = f(2, 13, 5), f(2, 13, 10) * 0.3
    inputs.update(cls=cls, bbox=bbox, far=bbox + 100.0)
    inputs.update(zip(("c_cls", "c_bbox"), (_t(a) for a in mk.decode_inputs("c"))))
    post = [-5.0, -5.0, -5.0, 5.0, 5.0, 5.0]

    def call():
        i, outs = inputs, {}
        for d, heads in ((16, 3), (64, 1)):
            outs[f"mha{d}"] = bevformer_decoder.multihead_attention(i[f"q{d}"], i[f"k{d}"], i[f"v{d}"], heads)
        outs["a_mha"] = bevformer_decoder.multihead_attention(i["a_q"], i["a_k"], i["a_v"], mk.HEADS)
        outs["ca4"] = bevformer_decoder.decoder_cross_attention_sample(i["value4"], i["off4"], i["logits4"], i["ref1"],
                                                                       i["sh"], i["lsi"])
        outs["ca32"] = bevformer_decoder.decoder_cross_attention_sample(i["value32"], i["off32"], i["logits32"], i["ref2"],
                                                                        i["sh"], i["lsi"])
        full = bevformer_decoder.nms_free_decode(i["cls"], i["bbox"], post, 65, None, True)
        none = bevformer_decoder.nms_free_decode(i["cls"], i["far"], post, 40, 0.2, False)
        c = mk.CASES["c"]
        low = bevformer_decoder.nms_free_decode(i["c_cls"], i["c_bbox"], c["post"], c["max_num"], c["thr"], True)
        # count 0 leaves zeros and -1 only, which the protocol takes for an output never written: shifted, the values
        # still are the kernel's (an element it left alone shows in the 0x00 or in the 0xFF run)
        none = (none[0] + 1.0, none[1] + 1.0, none[2] - 1, none[3] + 7)
        for name, det in (("full", full), ("none", none), ("low", low)):
            outs.update({f"{name}_{k}": v for k, v in zip(("boxes", "scores", "labels", "count"), det)})
        return outs

    return inputs, call


@scenario
def model():
    """Decoder, head and decode of case a, fused and unfused, built inside the run."""
    bev = _t(mk.inputs("a")["bev_embed"])

    def call():
        outs = {}
        for fused in (True, False):
            head = cpu.build_head("a", fused).to(DEV)
            with torch.no_grad():
                preds = head.forward_from_bev(bev)
                det = head.get_bboxes(preds)
            outs.update({f"cls_{fused}": preds["all_cls_scores"], f"bbox_{fused}": preds["all_bbox_preds"]})
            outs.update({f"{k}_{fused}": v for k, v in zip(("boxes", "scores", "labels", "count"), det)})
        return outs

    return dict(bev=bev), call


@pytest.mark.parametrize("name", list(P.scenarios))
def test_scenario(name):
    P.check_scenario(name)


def test_every_launching_entry_point_is_exercised():
    """Runs last; scenarios that did not run in this process are run here in their plain form."""
    from paddle3d_amd import _lib

    P.check_complete(_lib.symbols("test_memory_safety_bevformer_dec_gpu"), 3)
