"""IA-SSD's entry points (the rows of paddle3d_amd._lib.ENTRY_POINTS that name this module) under guarded
allocations: tests/guarded.py's Protocol.  Each scenario builds seeded inputs and returns `(inputs, call)`; it runs plain,
guarded with fill 0x00 and guarded with fill 0xFF (tests/guarded.py), and the test asserts: no guard band damaged (no
store outside an output), every input bit-equal to its clone, every specified output bit-equal across the three runs
(nothing depends on what a buffer held before) and not trivial.  The model scenario constructs the modules inside the
run, so their tensors are allocated under the guard too.

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

import make_iassd_golden as mk  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32

P = Protocol("test_memory_safety_iassd_gpu", "memory-safety-iassd", DEV)
scenario = P.scenario


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _weights(rng, widths):
    c1, c2, c3 = widths
    w = {"w_pos": rng.standard_normal((c1, 3))}
    for k, (cin, cout) in enumerate(((None, c1), (c1, c2), (c2, c3)), 1):
        if cin is not None:
            w[f"w{k}"] = rng.standard_normal((cout, cin)) / np.sqrt(cin)
        w[f"scale{k}"], w[f"shift{k}"] = rng.uniform(0.5, 1.5, cout), rng.normal(0, 0.3, cout)
    return {k: _t(v.astype(F32)) for k, v in w.items()}


def _pool(ops, q, p, f, w, radius, nsample, **kw):
    return ops.sa_msg_pool(q, p, f, w["w_pos"], w["scale1"], w["shift1"], w["w2"], w["scale2"], w["shift2"], w["w3"],
                           w["scale3"], w["shift3"], radius, nsample, **kw)


@scenario
def sa_msg_pool():
    """Widths on both sides of the narrow / wide split and at the border, nsample on both sides of the 16-slot tile and
    of the queries-per-pass steps, with and without features, on the golden's second layer (rows without a neighbour
    but themselves, rows with more hits than nsample); pooled is written whole."""
    from paddle3d_amd.ops import iassd as ops

    g = mk.load()
    rng = np.random.default_rng(19)
    q, p = _t(g["l1_out_new_xyz"]), _t(g["l1_in_xyz"])
    n = int(p.shape[1])
    cases = [((16, 16, 16), 16, True), ((16, 48, 64), 21, False), ((64, 96, 128), 33, True), ((256, 16, 256), 9, True),
             ((128, 256, 256), 64, False)]
    inputs = {"new_xyz": q, "xyz": p}
    for widths, S, feats in cases:
        tag = "x".join(map(str, widths))
        inputs.update({f"{tag}_{k}": v for k, v in _weights(rng, widths).items()})
        if feats:
            inputs[f"{tag}_features_in"] = _t(rng.standard_normal((2, n, widths[0])).astype(F32))

    def call():
        outs = {}
        for widths, S, feats in cases:
            tag = "x".join(map(str, widths))
            w = {k[len(tag) + 1:]: v for k, v in inputs.items() if k.startswith(tag + "_")}
            outs[f"pooled_{tag}_{S}"] = _pool(ops, q, p, w.get("features_in"), w, 1.6, S)
        return outs

    return inputs, call


@scenario
def sa_msg_pool_columns():
    """ld_out > c3: two scales into columns 3 .. 19 and 24 .. 56 of one [B, m, 60] buffer that holds a pattern; the
    columns beside the slices keep it (the buffer is a specified output: bit-equal across the runs, pattern included)."""
    from paddle3d_amd.ops import iassd as ops

    g = mk.load()
    rng = np.random.default_rng(23)
    q, p = _t(g["l2_out_new_xyz"]), _t(g["l2_in_xyz"])
    wa, wb = _weights(rng, (16, 16, 16)), _weights(rng, (32, 48, 32))
    inputs = {"new_xyz": q, "xyz": p, **{f"a_{k}": v for k, v in wa.items()}, **{f"b_{k}": v for k, v in wb.items()}}

    def call():
        out = torch.full((2, int(q.shape[1]), 60), -3.5, dtype=torch.float32, device=DEV)
        _pool(ops, q, p, None, wa, 1.6, 16, out=out, col=3)
        _pool(ops, q, p, None, wb, 4.8, 32, out=out, col=24)
        beside = torch.cat([out[..., :3], out[..., 19:24], out[..., 56:]], dim=-1)
        assert bool((beside == -3.5).all()), "columns beside the slices were written"
        assert bool((out[..., 3:19] >= 0).all()) and bool((out[..., 24:56] >= 0).all())
        return {"out": out}

    return inputs, call


@scenario
def iassd_decode():
    """One row, a row count past one workgroup, bins 1 and 12, with and without mean sizes, the centres read in place
    from columns 1:4; boxes is written whole."""
    from paddle3d_amd.ops import iassd as ops

    rng = np.random.default_rng(29)
    inputs = {"mean_size": _t(np.asarray(mk.MEAN_SIZE, F32))}
    for M in (1, 300):
        inputs[f"cls{M}"] = _t(rng.standard_normal((M, 3)).astype(F32))
        inputs[f"ctr{M}"] = _t(rng.uniform(-40, 40, (M, 4)).astype(F32))
        for bins in (1, 12):
            inputs[f"box{M}_{bins}"] = _t(rng.standard_normal((M, 6 + 2 * bins)).astype(F32))

    def call():
        outs = {}
        for M in (1, 300):
            for bins in (1, 12):
                for ms in ("mean_size", None):
                    outs[f"boxes{M}_{bins}_{ms}"] = ops.iassd_decode(
                        inputs[f"cls{M}"], inputs[f"box{M}_{bins}"], inputs[f"ctr{M}"][:, 1:4],
                        inputs[ms] if ms else None, bins)
        return outs

    return inputs, call


@scenario
def model():
    """The golden model with every supported scale fused, built inside the run, through the padded post_process."""
    import test_iassd_cpu as tc

    g = mk.load()
    inputs = {"data": _t(g["data"])}

    def call():
        m = tc.build(g, mk.state(g, "backbone"), mk.state(g, "head"), fused="force").to(DEV)
        with torch.no_grad():
            bd = m.head(m.backbone({"data": inputs["data"], "batch_size": mk.B}))
            post = m.post_process(bd)
        outs = {k: bd[k] for k in ("centers", "centers_features", "ctr_offsets", "batch_cls_preds", "batch_box_preds")}
        outs.update({f"post_{k}": v for k, v in zip(("boxes", "scores", "labels", "count"), post)})
        return outs

    return inputs, call


@pytest.mark.parametrize("name", list(P.scenarios))
def test_scenario(name):
    P.check_scenario(name)


def test_every_launching_entry_point_is_exercised():
    """Runs last; scenarios that did not run in this process are run here in their plain form."""
    from paddle3d_amd import _lib

    P.check_complete(_lib.symbols("test_memory_safety_iassd_gpu"), 2)
