"""PETR's entry points (paddle3d_amd._lib.SYMBOLS_PETR) under guarded allocations: the protocol of
tests/test_memory_safety_bevformer_dec_gpu.py.  Each scenario builds seeded inputs and returns `(inputs, call)`; it runs
plain, guarded with fill 0x00 and guarded with fill 0xFF (tests/guarded.py), and the test asserts: no guard band damaged
(no store outside an output), every input bit-equal to its clone, every output bit-equal across the three runs (nothing
depends on what a buffer held before -- the padded key tiles and query rows of the streamed attention included, since
they end in the output) and not trivial.  The kernels take no workspace.  The model scenario constructs the head inside
the run, so its tensors are allocated under the guard too.

The last test asserts that the scenarios reach every name of SYMBOLS_PETR."""
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

import make_petr_golden as mk  # noqa: E402
import test_petr_cpu as cpu  # noqa: E402

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

    print(f"[memory-safety-petr] {name}: {mode}", flush=True)
    ctx = contextlib.nullcontext(None) if mode == "plain" else guarded(int(mode, 16), DEV)
    with ctx as g, launch_ledger(_lib.lib(), _lib.SYMBOLS_PETR) as calls:
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
    missing = [s for s in _lib.SYMBOLS_PETR if not _LEDGER.get(s)]
    assert len(_lib.SYMBOLS_PETR) == 2 and not missing, f"entry points of SYMBOLS_PETR reached by no scenario: {missing}"
