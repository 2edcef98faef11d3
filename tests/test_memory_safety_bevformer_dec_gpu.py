"""The decoder's entry points (paddle3d_amd._lib.SYMBOLS_BEVFORMER_DEC) under guarded allocations: the protocol of
tests/test_memory_safety_bevformer_gpu.py.  Each scenario builds seeded inputs and returns `(inputs, call)`; it runs
plain, guarded with fill 0x00 and guarded with fill 0xFF (tests/guarded.py), and the test asserts: no guard band damaged
(no store outside an output), every input bit-equal to its clone, every output bit-equal across the three runs (nothing
depends on what a buffer held before -- the attention's LDS-backed score rows and padded tiles included, since they end
in the output) and not trivial.  The kernels take no workspace.  The model scenario constructs the head inside the run,
so its tensors are allocated under the guard too.

The last test asserts that the scenarios reach every name of SYMBOLS_BEVFORMER_DEC."""
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

import bevformer_decoder_numpy as dn  # noqa: E402
import make_bevformer_decoder_golden as mk  # noqa: E402
import test_bevformer_decoder_cpu as cpu  # noqa: E402

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

    print(f"[memory-safety-bevformer-dec] {name}: {mode}", flush=True)
    ctx = contextlib.nullcontext(None) if mode == "plain" else guarded(int(mode, 16), DEV)
    with ctx as g, launch_ledger(_lib.lib(), _lib.SYMBOLS_BEVFORMER_DEC) as calls:
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
    missing = [s for s in _lib.SYMBOLS_BEVFORMER_DEC if not _LEDGER.get(s)]
    assert len(_lib.SYMBOLS_BEVFORMER_DEC) == 3 and not missing, f"entry points of SYMBOLS_BEVFORMER_DEC reached by no scenario: {missing}"
