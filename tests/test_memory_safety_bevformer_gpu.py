"""BEVFormer's entry points (the rows of paddle3d_amd._lib.ENTRY_POINTS that name this module) under guarded
allocations: tests/guarded.py's Protocol.  Each scenario builds seeded inputs and returns `(inputs, call)`; it runs plain,
guarded with fill 0x00 and guarded with fill 0xFF (tests/guarded.py), and the test asserts: no guard band damaged (no
store outside an output), every input bit-equal to its clone, every output bit-equal across the three runs (nothing
depends on what a buffer held before) and not trivial.  The kernels take no workspace.  The model scenario constructs
the encoder inside the run, so its tensors are allocated under the guard too.

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

import bevformer_numpy as bn  # noqa: E402
import make_bevformer_golden as mk  # noqa: E402
import test_bevformer_cpu as cpu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32

P = Protocol("test_memory_safety_bevformer_gpu", "memory-safety-bevformer", DEV)
scenario = P.scenario


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@scenario
def ops():
    """The three ops at every golden case (Q = 77, 30: the last workgroup is partly idle; 1 and 2 levels; a camera that
    sees nothing) and the attention ops at C = 4, one lane per group; every output is written whole."""
    from paddle3d_amd.ops import bevformer

    g = mk.load()
    inputs, lv = {}, {}
    for tag in mk.TAGS:
        c = mk.CASES[tag]
        sh, lsi, _ = mk.levels(tag)
        bev_sh, bev_lsi, _ = bn.md.level_layout([c["bev"]])
        arrays = dict(ref_3d=bn.get_reference_points(*c["bev"], cpu.Z_RANGE, c["D"]), lidar2img=g[f"{tag}_lidar2img"],
                      sh=sh, lsi=lsi, bev_sh=bev_sh, bev_lsi=bev_lsi, ref_2d=cpu.ref_2d(tag))
        arrays.update(zip(("sca_value", "sca_off", "sca_logits"), cpu.sca_inputs(tag)))
        arrays.update(zip(("tsa_value", "tsa_off", "tsa_logits"), cpu.tsa_inputs(tag)))
        inputs.update({f"{tag}_{k}": _t(v) for k, v in arrays.items()})
    rng = np.random.default_rng(9)
    sh, lsi, S = bn.md.level_layout([[3, 4], [2, 2]])
    thin = dict(value=rng.standard_normal((2, S, 3, 4)), sca_off=rng.standard_normal((1, 33, 3, 2, 4, 2)),
                sca_logits=rng.standard_normal((1, 33, 3, 8)), ref_cam=rng.uniform(0, 1, (2, 1, 33, 2, 2)),
                tsa_off=rng.standard_normal((1, 33, 3, 2, 2, 4, 2)), tsa_logits=rng.standard_normal((1, 33, 3, 2, 8)),
                ref_2d=rng.uniform(0, 1, (2, 33, 2, 2)))
    inputs.update({f"thin_{k}": _t(v.astype(F32)) for k, v in thin.items()})
    inputs.update(thin_bits=_t(rng.integers(0, 4, (1, 33)).astype(np.uint8)), thin_sh=_t(sh), thin_lsi=_t(lsi))

    def call():
        outs = {}
        for tag in mk.TAGS:
            i = lambda k: inputs[f"{tag}_{k}"]  # noqa: E731
            ps = bevformer.point_sampling(i("ref_3d"), i("lidar2img"), mk.PC_RANGE, *mk.IMG_SHAPE[:2])
            outs.update({f"{tag}_{k}": v for k, v in zip(("ref_cam", "mask", "bits", "count"), ps)})
            outs[f"{tag}_sca"] = bevformer.spatial_cross_attention_sample(
                i("sca_value"), i("sca_off"), i("sca_logits"), ps[0], ps[2], i("sh"), i("lsi"), mk.CASES[tag]["cams"])
            outs[f"{tag}_tsa"] = bevformer.temporal_self_attention_sample(
                i("tsa_value"), i("tsa_off"), i("tsa_logits"), i("ref_2d"), i("bev_sh"), i("bev_lsi"))
        i = lambda k: inputs[f"thin_{k}"]  # noqa: E731
        outs["thin_sca"] = bevformer.spatial_cross_attention_sample(i("value"), i("sca_off"), i("sca_logits"), i("ref_cam"),
                                                                    i("bits"), i("sh"), i("lsi"), 2)
        outs["thin_tsa"] = bevformer.temporal_self_attention_sample(i("value"), i("tsa_off"), i("tsa_logits"), i("ref_2d"),
                                                                    i("sh"), i("lsi"))
        return outs

    return inputs, call


@scenario
def model():
    """The 2-layer encoder fused and unfused, built inside the run."""
    from paddle3d_amd import bevformer
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    g, tag = mk.load(), "a"
    c, inp = mk.CASES[tag], mk.inputs(tag)
    sh, lsi, _ = mk.levels(tag)
    seq = lambda a: _t(a.transpose(1, 0, 2))  # noqa: E731
    inputs = dict(bev_query=seq(inp["bev_query"]), bev_pos=seq(inp["bev_pos"]), prev_bev=seq(inp["prev_bev"]),
                  feats=_t(inp["feats"]), shift=_t(inp["shift"]), lidar2img=_t(g[f"{tag}_lidar2img"]), sh=_t(sh), lsi=_t(lsi))

    def call():
        outs = {}
        metas = [dict(lidar2img=inputs["lidar2img"][b], img_shape=[mk.IMG_SHAPE] * c["cams"]) for b in range(c["B"])]
        for fused in (True, False):
            m = bevformer.BEVFormerEncoder(**mk.encoder_cfg(tag), fused=fused)
            load_paddle_state_dict(m, mk.state(tag))
            m = m.eval().to(DEV)
            with torch.no_grad():
                outs[f"encoder_{fused}"] = m(inputs["bev_query"], inputs["feats"], inputs["feats"], bev_h=c["bev"][0],
                                             bev_w=c["bev"][1], bev_pos=inputs["bev_pos"], spatial_shapes=inputs["sh"],
                                             level_start_index=inputs["lsi"], prev_bev=inputs["prev_bev"],
                                             shift=inputs["shift"], img_metas=metas)
        return outs

    return inputs, call


@pytest.mark.parametrize("name", list(P.scenarios))
def test_scenario(name):
    P.check_scenario(name)


def test_every_launching_entry_point_is_exercised():
    """Runs last; scenarios that did not run in this process are run here in their plain form."""
    from paddle3d_amd import _lib

    P.check_complete(_lib.symbols("test_memory_safety_bevformer_gpu"), 3)
