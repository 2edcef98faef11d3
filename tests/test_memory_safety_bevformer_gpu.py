"""BEVFormer's entry points (paddle3d_amd._lib.SYMBOLS_BEVFORMER) under guarded allocations: the protocol of
tests/test_memory_safety_caddn_gpu.py.  Each scenario builds seeded inputs and returns `(inputs, call)`; it runs plain,
guarded with fill 0x00 and guarded with fill 0xFF (tests/guarded.py), and the test asserts: no guard band damaged (no
store outside an output), every input bit-equal to its clone, every output bit-equal across the three runs (nothing
depends on what a buffer held before) and not trivial.  The kernels take no workspace.  The model scenario constructs
the encoder inside the run, so its tensors are allocated under the guard too.

The last test asserts that the scenarios reach every name of SYMBOLS_BEVFORMER."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from guarded import guarded, launch_ledger  # noqa: E402

import bevformer_numpy as bn  # noqa: E402
import make_bevformer_golden as mk  # noqa: E402
import test_bevformer_cpu as cpu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32

SCENARIOS = {}
_LEDGER = {}
_RAN = set()


def scenario(fn):
    SCENARIOS[fn.__name__] = fn
    return fn


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


def _host(v):
    return v.detach().contiguous().cpu()


def _bits(t):
    return t.reshape(-1).view(torch.uint8)


def _nontrivial(t):
    x = t.reshape(-1)
    x = x[~torch.isnan(x)].double() if x.dtype.is_floating_point else x.long()
    return int(((x != 0) & (x != -1)).sum())


def _run(name, mode):
    from paddle3d_amd import _lib

    print(f"[memory-safety-bevformer] {name}: {mode}", flush=True)
    ctx = contextlib.nullcontext(None) if mode == "plain" else guarded(int(mode, 16), DEV)
    with ctx as g, launch_ledger(_lib.lib(), _lib.SYMBOLS_BEVFORMER) as calls:
        inputs, call = SCENARIOS[name]()
        before = {k: v.clone() for k, v in inputs.items()}
        outs = call()
        torch.cuda.synchronize()
        damage = g.check() if g is not None else []
        host = {k: _host(v) for k, v in outs.items()}
        changed = [k for k, v in inputs.items() if not torch.equal(_bits(_host(v)), _bits(_host(before[k])))]
        if g is not None:
            assert len(g.blocks) > 0 and all(buf.data_ptr() % 512 == 0 for buf, _, _, _ in g.blocks)
    return host, damage, changed, {k: v for k, v in calls.items() if v}


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_scenario(name):
    ref, damage, changed, calls = _run(name, "plain")
    assert damage == [] and changed == [] and ref, (name, "plain", changed)
    for k, v in ref.items():
        assert v.numel() > 0 and _nontrivial(v) > 0, f"{name}: output {k} {tuple(v.shape)} is empty or all 0 / -1"
    for mode in ("0x00", "0xFF"):
        got, damage, changed, calls_g = _run(name, mode)
        assert damage == [], f"{name} [{mode}]: " + "; ".join(str(d) for d in damage)
        assert changed == [], f"{name} [{mode}]: inputs written: {changed}"
        assert set(got) == set(ref), (name, mode, set(got) ^ set(ref))
        for k, want in ref.items():
            have = got[k]
            assert have.shape == want.shape and have.dtype == want.dtype, (name, mode, k)
            if not torch.equal(_bits(have), _bits(want)):
                diff = (_bits(have) != _bits(want)).nonzero().reshape(-1)
                first = int(diff[0]) // have.element_size()
                pytest.fail(f"{name} [{mode}]: output {k} {tuple(have.shape)} depends on the previous contents of "
                            f"memory: {diff.numel()} bytes differ, first at element {first} "
                            f"(plain {want.reshape(-1)[first].item()!r}, guarded {have.reshape(-1)[first].item()!r})")
        assert set(calls_g) == set(calls), (name, mode, set(calls_g) ^ set(calls))
    for sym, n in calls_g.items():
        _LEDGER[sym] = _LEDGER.get(sym, 0) + n
    _RAN.add(name)


def test_every_launching_entry_point_is_exercised():
    """Runs last; scenarios that did not run in this process are run here in their plain form."""
    from paddle3d_amd import _lib

    for name in SCENARIOS:
        if name not in _RAN:
            for sym, n in _run(name, "plain")[3].items():
                _LEDGER[sym] = _LEDGER.get(sym, 0) + n
    missing = [s for s in _lib.SYMBOLS_BEVFORMER if not _LEDGER.get(s)]
    assert len(_lib.SYMBOLS_BEVFORMER) == 3 and not missing, f"entry points of SYMBOLS_BEVFORMER reached by no scenario: {missing}"
