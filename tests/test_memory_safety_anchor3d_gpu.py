"""Anchor3DHead's entry points (paddle3d_amd._lib.SYMBOLS_ANCHOR3D) under guarded allocations: the protocol of
tests/test_memory_safety_petr_gpu.py.  Each scenario builds seeded inputs and returns `(inputs, call)`; it runs plain,
guarded with fill 0x00 and guarded with fill 0xFF (tests/guarded.py), and the test asserts: no guard band damaged (no
store outside an output or the workspace), every input bit-equal to its clone, every output bit-equal across the three
runs (nothing depends on what an output or the workspace held before: the rows past a frame's count, the unused ends of
the candidate lists, the NMS matrix and the pool included) and not trivial.  The model scenario constructs the head
inside the run, so its packed weights and anchor table are allocated under the guard too.

The last test asserts that the scenarios reach every name of SYMBOLS_ANCHOR3D."""
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

import anchor3d_numpy as an  # noqa: E402
import make_anchor3d_golden as mk  # noqa: E402
import test_anchor3d_cpu as cpu  # noqa: E402
import test_anchor3d_gpu as gpu  # noqa: E402

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


# (H, W, C, A, nc, cs, nms_pre, max_num): a partial wave tile and a second workgroup, K = 1, K = N, three chunks
POINTS = ((17, 15, 48, 14, 10, 9, 65, 5), (1, 1, 16, 1, 1, 7, 1000, 1), (4, 33, 16, 6, 3, 9, 4 * 33 * 6, 500),
          (3, 5, 16, 32, 16, 7, 200, 500))


@scenario
def ops():
    """Both entry points at the tile borders (POINTS) and on the two golden cases; frame 1 of the first point has no
    detection (rows of zeros) and its score_thr empties most classes."""
    from paddle3d_amd.ops import anchor3d_head as A

    inputs, jobs = {}, []
    for i, (H, W, C, na, nc, cs, pre, mx) in enumerate(POINTS):
        rng = np.random.default_rng(40 + i)
        anchors, st = gpu.sweep_anchors(rng, H, W, na, cs), gpu.sweep_state(rng, C, na, nc, cs)
        feat = rng.standard_normal((2, C, H, W)).astype(F32)
        if i == 0:
            feat[1] = 0.0
        cfg = dict(nms_pre=pre, max_num=mx, score_thr=0.6 if i == 0 else 0.3, nms_thr=0.2, dir_offset=0.7854,
                   dir_limit_offset=0.0, num_classes=nc)
        jobs.append((f"p{i}", feat, st, anchors, cfg))
    for tag in an.TAGS:
        jobs.append((tag, an.golden_inputs(tag), an.golden_state(tag), mk.anchors_of(tag), an.cfg_of(tag)))
    for name, feat, st, anchors, cfg in jobs:
        inputs[name + "_feat"], inputs[name + "_anchors"] = _t(feat), _t(anchors)
        for k, v in st.items():
            inputs[f"{name}_{k}"] = _t(v)
        for k, m in zip(("cls", "reg", "dir"), an.head_maps(feat, st)):
            inputs[f"{name}_{k}_map"] = _t(m)

    def call():
        outs = {}
        for name, _, _, _, cfg in jobs:
            i = lambda k: inputs[f"{name}_{k}"]  # noqa: E731
            c = (cfg["num_classes"], cfg["nms_pre"], cfg["max_num"], cfg["score_thr"], cfg["nms_thr"], cfg["dir_offset"],
                 cfg["dir_limit_offset"])
            packed = A.pack_cls_weight(i("conv_cls.weight"), cfg["num_classes"])
            lazy = A.anchor3d_head_forward(i("feat"), packed, i("conv_cls.bias"), i("conv_reg.weight"), i("conv_reg.bias"),
                                           i("conv_dir_cls.weight"), i("conv_dir_cls.bias"), i("anchors"), *c)
            maps = A.anchor3d_get_bboxes(i("cls_map"), i("reg_map"), i("dir_map"), i("anchors"), *c)
            for kind, res in (("lazy", lazy), ("maps", maps)):
                outs.update({f"{name}_{kind}_{k}": v for k, v in zip(("boxes", "scores", "labels", "counts"), res)})
        return outs

    return inputs, call


@scenario
def model():
    """The module on the nuScenes-like golden case, built inside the run: the lazy path, forward + the from-maps path,
    and the unfused transcription."""
    x = _t(an.golden_inputs("nus"))

    def call():
        head = cpu.build_head("nus").to(DEV)
        outs = {}
        with torch.no_grad():
            for name, fused in (("lazy", "force"), ("unfused", False)):
                res = head.forward_get_bboxes([x], [{}] * 2, fused=fused, return_padded=True)
                outs.update({f"{name}_{k}": v for k, v in zip(("boxes", "scores", "labels", "counts"), res)})
            res = head.get_bboxes(*head([x]), [{}] * 2, return_padded=True)
            outs.update({f"maps_{k}": v for k, v in zip(("boxes", "scores", "labels", "counts"), res)})
        return outs

    return dict(feat=x), call


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

    print(f"[memory-safety-anchor3d] {name}: {mode}", flush=True)
    ctx = contextlib.nullcontext(None) if mode == "plain" else guarded(int(mode, 16), DEV)
    with ctx as g, launch_ledger(_lib.lib(), _lib.SYMBOLS_ANCHOR3D) as calls:
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
        if k.startswith("p1_") and k.endswith("labels"):  # a single anchor of a single class: label 0
            continue
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
    missing = [s for s in _lib.SYMBOLS_ANCHOR3D if not _LEDGER.get(s)]
    assert len(_lib.SYMBOLS_ANCHOR3D) == 3 and not missing, f"entry points of SYMBOLS_ANCHOR3D reached by no scenario: {missing}"
