"""BEV-LaneDet's entry points (the rows of paddle3d_amd._lib.LANEDET_ENTRY_POINTS) under guarded allocations:
tests/guarded.py's Protocol.  Each scenario builds seeded inputs and returns `(inputs, call)`; it runs plain, guarded
with fill 0x00 and guarded with fill 0xFF, and the test asserts: no guard band damaged (no store outside an output or
the workspace), every input bit-equal to its clone, every output bit-equal across the three runs (nothing depends on
what an output or the workspace held before: the canvas, the rows past the lane counts, the lanes past num_lanes, the
pixel list, the centre table and the row table included) and not trivial.  The points include widths that are no
multiple of 4 (dense rows and rows of padded pitch in one stacked map), a frame without a selected pixel, and frames
with either flag set.  The model scenario constructs the model inside the run, so its derived weights are allocated
under the guard too; its float outputs compare within a tolerance, because torch's convolutions are not bit-reproducible
from pass to pass (the observation is in DESIGN.md 4.5zg), everything else bit for bit.

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

import lanedet_numpy as ln  # noqa: E402
import test_lanedet_cpu as cpu  # noqa: E402
import test_lanedet_gpu as gpu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32

# the model scenario runs torch's convolutions, whose library may take another algorithm (another summation order) in
# another pass: its float outputs compare within a few fp32 roundings of the layers' depth, its labels, ids and counts
# bit for bit (the golden cases keep every decision a margin away); the kernels' own scenarios compare bit for bit
# (observed: DESIGN.md 4.5zg, "torch's convolutions are not bit-reproducible from call to call here")
TOLERANT = {("model", key): {torch.float32: 1e-5} for key in ("_points", "_fit", "_maps")}
P = Protocol("test_memory_safety_lanedet_gpu", "memory-safety-lanedet", DEV, tolerant=TOLERANT)
scenario = P.scenario

# (H, W, B, nd, C): widths 7 and 33 (no multiple of 4), one pixel, the full size
POINTS = ((5, 7, 2, 2, 16), (1, 1, 1, 1, 4), (4, 33, 3, 4, 8), (200, 48, 2, 2, 64))


def _pack(outs, name, pack):
    for k in pack._fields:
        outs[f"{name}_{k}"] = getattr(pack, k)


@scenario
def ops():
    """Both entry points at POINTS: the from-maps form on synthetic lanes (frame 1 of the first point has no selected
    pixel), the lazy head from dense maps and from one stacked map of padded pitch."""
    jobs = []
    for i, (H, W, B, nd, C) in enumerate(POINTS):
        rng = np.random.default_rng(70 + i)
        cfg = ln.sweep_cfg(H, W)
        maps = ln.synthetic_lanes(rng, B, H, W, nd, lanes=min(5, max(1, W // 4)))
        if i == 0:
            maps[0][1] = -5.0
        feats, state, conf = ln.random_head(rng, B, C, H, W, nd)
        jobs.append((f"p{i}", maps, feats, state, cfg, dict(cfg, conf=conf)))
    inputs = {}
    for name, maps, feats, state, cfg, cfg2 in jobs:
        inputs.update({f"{name}_map{j}": gpu._t(m) for j, m in enumerate(maps)})
        inputs.update({f"{name}_feat{j}": gpu._t(f) for j, f in enumerate(feats)})

    def call():
        outs = {"__trivial_ok__": set()}
        for name, maps, feats, state, cfg, cfg2 in jobs:
            for kind, pack in (("maps", gpu.from_maps(*maps, cfg)), ("lazy", gpu.lazy(feats, state, cfg2)),
                               ("stacked", gpu.lazy(feats, state, cfg2, stacked=True))):
                _pack(outs, f"{name}_{kind}", pack)
                outs["__trivial_ok__"].add(f"{name}_{kind}_flags")
                if name == "p1":  # one pixel: at most one selected pixel, never a lane
                    outs["__trivial_ok__"].update(f"{name}_{kind}_{k}" for k in pack._fields)
                elif name != "p3" and kind != "maps":  # a seeded head on a small map: few rows, maybe no lane to fit
                    outs["__trivial_ok__"].update(f"{name}_{kind}_{k}" for k in pack._fields
                                                  if k not in ("labels", "num_selected"))
        return outs

    return inputs, call


@scenario
def flagged():
    """The border cases, among them 129 centres (flag bit 0) and 33 canvas ids (flag bit 1), through both forms: a
    flagged frame writes zeros and nothing out of bounds."""
    cases = ln.border_cases()
    names = ("centres_128", "centres_129", "lanes_32", "lanes_33", "empty_frame", "rows_1_to_4")
    inputs = {f"{n}_{j}": gpu._t(a) for n in names for j, a in enumerate(cases[n][:4])}

    def call():
        outs = {"__trivial_ok__": set()}
        for n in names:
            seg, emb, off, z, cfg = cases[n]
            _pack(outs, n + "_maps", gpu.from_maps(seg, emb, off, z, cfg, logit=True))
            _pack(outs, n + "_lazy", gpu.lazy(*ln.identity_head(seg, emb, off, z), cfg, stacked=True))
            for kind in ("maps", "lazy"):
                outs["__trivial_ok__"].update(f"{n}_{kind}_{k}" for k in ("flags", "fit_ok", "fit"))
                if n == "lanes_33":
                    outs["__trivial_ok__"].update(f"{n}_{kind}_{k}" for k in gpu.FIELDS if k != "flags")
        return outs

    return inputs, call


@scenario
def model():
    """The module on the golden head cases, built inside the run: the lazy path, the dense path and the
    transcription."""
    golden = dict(np.load(os.path.join(HERE, "golden", "python_lanedet.npz")))
    x = {tag: gpu._t(cpu.head_input(golden, tag)) for tag in cpu.HEAD_TAGS}

    def call():
        outs = {"__trivial_ok__": set()}
        for tag in x:
            m = cpu.build_model(golden, tag).to(DEV)
            with torch.no_grad():
                for fused in ("lazy", "dense", False):
                    _pack(outs, f"{tag}_{fused}", m.lanes_padded(x[tag], fused=fused))
                    outs["__trivial_ok__"].add(f"{tag}_{fused}_flags")
                outs[f"{tag}_maps"] = m.raw_maps(x[tag], fused="dense")
        return outs

    return dict(x), call


@pytest.mark.parametrize("name", list(P.scenarios))
def test_scenario(name):
    P.check_scenario(name)


def test_every_launching_entry_point_is_exercised():
    """Runs last; scenarios that did not run in this process are run here in their plain form."""
    from paddle3d_amd import _lib

    P.check_complete(_lib.symbols("test_memory_safety_lanedet_gpu"), 3)
