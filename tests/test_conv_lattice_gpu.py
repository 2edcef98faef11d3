"""Every dense convolution kernel across the border of what its predicate accepts (tests/conv_lattice.py has the
lattice, tests/test_conv_lattice_cpu.py its own checks).

test_accepts    predicate says yes -> the wrapper runs and matches the float64 reference on the exact class (bit for bit;
                F(4x4, 3x3): within 4 x the error of its float32 restatement) and on the random class (the bars
                conv_lattice.BARS names), inside guarded allocations with fill 0x00 and 0xFF: bands intact, the two runs
                the same bytes, the inputs untouched.
test_refuses    predicate says no -> the wrapper raises (status -3, or -1) and writes nothing.  A shape the predicate
                refuses and the kernel takes is printed as SLACK, not failed.
test_dispatchers_cover_every_kernel
                the layers that choose among the kernels, over the lattice's channel / map corners, against float64
                torch; every dense-convolution entry point of the C ABI has to be reached through one of them.

Figures of the run that set this file (MI355X): see the docstring of test_accepts.  Slack found (predicate refuses,
kernel takes): odd ny / nx on pd3_scatter_conv3x3_s2_f16_bias_relu, an output width that is no multiple of 4 on the
sparse first layer.
"""
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_lattice as L  # noqa: E402
from guarded import guarded, launch_ledger  # noqa: E402

from paddle3d_amd._lib import Paddle3DAmdError  # noqa: E402
from paddle3d_amd.ops import conv  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ACCEPTS = L.all_accepts()
REFUSALS = L.all_refusals()
# the fp32 kernel a bf16x3 kernel's error is measured against (BARS["x3"])
FP32_SIBLING = {"s2_x3": "direct_s2", "patch0_x3": "patch0", "patch1_x3": "patch1", "patch2_x3": "patch2"}


def _device_inputs(fam, c, x, w, b):
    """(kernel input, packed weight, bias, tensors that must come back unchanged) on the device, outside any guard."""
    if fam.kind == "scatter":
        from paddle3d_amd.ops import pointpillars_scatter as ps

        feats, coords = L.canvas_rows(x)
        xin = ps.SparseCanvas(feats.to(DEV), coords.to(DEV), c.n, c.h, c.wv)
        keep = [xin.features, xin.coords, xin.inv]
    else:
        xin = fam.lay_in(c, x).to(DEV)
        keep = [xin]
    packed = fam.pack(c, w).to(DEV)
    bias = None if b is None else b.to(DEV)
    keep += [packed] + ([bias] if bias is not None else [])
    return xin, packed, bias, keep


def _run_guarded(fam, c, xin, packed, bias, keep, fill):
    before = [t.clone() for t in keep]
    with guarded(fill, DEV) as g:
        out = None
        if fam.takes_out():
            out = torch.full(fam.out_shape(c), L.SENTINEL, dtype=fam.out_dtype(), device=DEV)
        outs = fam.call(c, xin, packed, bias, out)
        torch.cuda.synchronize()
        damage = g.check()
    assert not damage, (c.id, hex(fill), [str(d) for d in damage])
    for t, t0 in zip(keep, before):
        assert torch.equal(t, t0), (c.id, "an input was written")
    return [o.cpu() for o in outs]


def _valid(fam, c, t, ref):
    """The part of an output tensor (CPU) the reference speaks about, as float64 [n, ch, ho, wo]."""
    exp = fam.expected(c, torch.zeros_like(ref))      # zeros where the result lives, SENTINEL / zeros elsewhere
    live = fam.expected(c, torch.ones_like(ref)) != exp
    return t.double()[live], fam.expected(c, ref)[live], t.double()[~live], exp[~live]


def _err(fam, c, outs, ref):
    """max |kernel - reference| over the written values; everything else must hold zeros / SENTINEL exactly."""
    worst = 0.0
    for o, (exp, _) in zip(outs, fam.expected_all(c, ref)):
        if fam.opts.get("out") == "dual" or fam.kind in ("f16", "f16s2") or "f16" in fam.predicate and fam.kind == "scatter":
            worst = max(worst, float((o.double() - exp).abs().max()))
            continue
        got, want, rest, rest_want = _valid(fam, c, o, ref)
        assert torch.equal(rest, rest_want), (c.id, "padding columns / sentinel channels")
        worst = max(worst, float((got - want).abs().max()))
    return worst


@pytest.mark.parametrize("case", ACCEPTS, ids=lambda c: c.id)
def test_accepts(case):
    """Figures of the MI355X run that set this test (712 cases, 30 families): on the exact class every kernel but the
    F(4x4, 3x3) ones equals the float64 reference bit for bit; over the 110 F(4x4, 3x3) cases the largest error of the
    float32 restatement is 2.0e-3 and the largest kernel error 2.5e-3 (both on wino43_pp at cin 64, cout 448, an 8 x 20 map,
    outputs up to ~300), the largest kernel / restatement ratio 2.0 (wino43_pp, 7 x 64 map, cin 8) against the bar of 4."""
    fam = L.FAMILIES[case.family]
    assert fam.accepts(case)
    for kind in ("exact", "random"):
        x, w, b = L.make_data(fam, case, kind)
        ref = fam.reference(case, x, w, b)
        xin, packed, bias, keep = _device_inputs(fam, case, x, w, b)
        runs = [_run_guarded(fam, case, xin, packed, bias, keep, fill) for fill in (0x00, 0xFF)]
        for a, z in zip(*runs):  # no dependence on what an output or a workspace held before
            assert a.dtype == z.dtype and torch.equal(a.view(torch.uint8), z.view(torch.uint8)), (case.id, kind, "fill")
        outs = runs[0]
        exps = fam.expected_all(case, ref)
        assert [tuple(o.shape) for o in outs] == [tuple(e.shape) for e, _ in exps], case.id
        assert [o.dtype for o in outs] == [d for _, d in exps], case.id
        mag = float(ref.abs().max())
        if kind == "exact" and fam.exact == "bits":
            for o, (e, d) in zip(outs, exps):
                bad = (o != e.to(d)).nonzero()
                assert torch.equal(o, e.to(d)), (case.id, "first differing index", bad[0].tolist(), len(bad))
            continue
        err = _err(fam, case, outs, ref)
        if kind == "exact":  # F(4x4, 3x3): 4 x the error of the float32 restatement of the same case
            rest = float((L.winograd43_f32(x, w, b, case.relu).double() - ref).abs().max())
            bar = max(4 * rest, 2.0 ** -23 * max(mag, 1.0))  # (never below one fp32 ulp of the largest output)
            print(f"{case.id}: restatement {rest:.3e}, kernel {err:.3e}, outputs up to {mag:.0f}")
            assert 4 * rest < 0.25, (case.id, rest)  # the bar stays a factor 4 under a missing term
            assert err <= bar, (case.id, err, bar)
        elif fam.bar == "fp32":
            assert err < 2e-4, (case.id, err)
        elif fam.bar == "f16":
            bar = 2e-4 * max(1.0, mag) + (1e-3 * mag if fam.out_f16 else 0.0)
            assert err <= bar, (case.id, err, bar)
        elif fam.bar == "x3":
            sib = L.FAMILIES[FP32_SIBLING[fam.name]]
            sc = L.Case(sib.name, case.axis, case.n, case.cin, case.cout, case.h, case.wv, case.bias, case.relu, case.opt)
            err32 = None
            if sib.accepts(sc):  # the fp32 kernel on the same operands
                out32 = torch.full(sib.out_shape(sc), L.SENTINEL, device=DEV)
                o32 = sib.call(sc, xin, sib.pack(sc, w).to(DEV), bias, out32)
                err32 = _err(sib, sc, [o.cpu() for o in o32], ref)
            print(f"{case.id}: bf16x3 {err:.3e}, fp32 kernel {err32}, magnitude {mag:.1f}")
            assert err < 2e-6 * mag, (case.id, err, mag)
            if err32 is not None:
                assert err <= max(2 * err32, 2e-7 * mag), (case.id, err, err32, mag)
        else:  # the sparse first layer against the dense fp32 kernel on the written-out canvas
            dense = L.FAMILIES["direct_s2"]
            dc = L.Case("direct_s2", case.axis, case.n, case.cin, case.cout, case.h, case.wv, case.bias, case.relu)
            err_dense = None
            if dense.accepts(dc) and (case.h % 2 == 0 and case.wv % 2 == 0):
                od = dense.call(dc, dense.lay_in(dc, x).to(DEV), dense.pack(dc, w).to(DEV), bias, None)
                err_dense = _err(dense, dc, [o.cpu() for o in od], ref)
            print(f"{case.id}: sparse {err:.3e}, dense fp32 kernel {err_dense}, magnitude {mag:.1f}")
            assert err < 1e-3, (case.id, err)
            assert err <= max(2 * (err_dense or 0.0), 2e-6 * max(1.0, mag)), (case.id, err, err_dense, mag)


def _dummy_weight(fam, c):
    """A zero weight buffer in the shape the wrapper reads its tile from, with room to spare where the wrapper allows: a
    kernel that takes a shape its predicate refuses (slack) must stay inside it."""
    g, cin, cout = fam.groups(c), c.cin, c.cout
    up = lambda v, m: -(-v // m) + 1  # noqa: E731
    p = fam.packer
    if p == "pack_grouped_weight":
        return torch.zeros(g, cin, cout, 9)
    if p == "pack_grouped_weight_f16":
        return torch.zeros(g, 9, cout, cin, dtype=torch.float16)
    if p == "pack_conv3x3_f16_weight":
        t = fam.opts["tile"]
        return torch.zeros(up(cout, t), up(cin, 16), 9, 2, t, 8, dtype=torch.float16)
    if p == "pack_winograd43_weight":
        t = fam.opts["tile"]
        return torch.zeros(up(cout, t), up(cin, 4), t // 16, 4, 16, 36)
    if p == "pack_winograd43_lane_weight":
        return torch.zeros(cout * cin * 36)   # (the wrapper checks the element count)
    if p == "sparse":
        return torch.zeros(cout, cin, 3, 3)
    big = 4 * (cout + 128) * (cin + 32) * 40 + (1 << 20)
    return torch.zeros(big, dtype=torch.bfloat16 if "x3" in p else torch.float32)


@pytest.mark.parametrize("clause,case", REFUSALS, ids=lambda v: v.id if isinstance(v, L.Case) else None)
def test_refuses(clause, case):
    fam = L.FAMILIES[case.family]
    assert not fam.accepts(case)
    x = torch.zeros(case.n, fam.groups(case) * case.cin, case.h, case.wv)
    if fam.kind == "scatter":
        from paddle3d_amd.ops import pointpillars_scatter as ps

        feats, coords = L.canvas_rows(x)
        xin = ps.SparseCanvas(feats.to(DEV), coords.to(DEV), case.n, case.h, case.wv)
    else:
        xin = fam.lay_in(case, x).to(DEV)
    wd = _dummy_weight(fam, case).to(DEV)
    nb = (fam.groups(case) * case.cout + 127) // 128 * 128 + 128
    bias = torch.zeros(nb, device=DEV)
    raised = None
    with guarded(0xFF, DEV) as g:
        out = None
        if fam.takes_out():
            shape = tuple(max(1, s) for s in fam.out_shape(case))
            out = torch.full(shape, L.SENTINEL, dtype=fam.out_dtype(), device=DEV)
        try:
            fam.call(case, xin, wd, bias, out)
        except (Paddle3DAmdError, AssertionError, RuntimeError) as e:  # (RuntimeError / assert: refused by the wrapper itself)
            raised = e
        torch.cuda.synchronize()
        damage = g.check()
    assert not damage, [str(d) for d in damage]
    if raised is None:
        print(f"SLACK {fam.name}: the predicate refuses '{clause}' ({case.id}) and {fam.symbol} takes it")
        return
    if isinstance(raised, Paddle3DAmdError):
        m = re.search(r"status (-?\d+)", str(raised))
        assert m and int(m.group(1)) in (-3, -1), str(raised)
    if out is not None:
        assert bool((out == L.SENTINEL).all()), (case.id, "a refused call wrote to its output")


# ---- the dispatchers ----------------------------------------------------------------------------------------------------------
# Entry points of the C ABI that are dense convolutions.  Not reached through a layer of the package, each for a stated reason:
NOT_DISPATCHED = {
    "pd3_conv3x3_winograd_bias_relu": "F(2x2, 3x3) is kept as a library op; _Conv3x3 has preferred F(4x4, 3x3) since it exists",
    "pd3_conv3x3_winograd43_pp_trace": "the ping-pong kernel with cycle counters, for tools/prof only",
    "pd3_grouped_conv3x3_small": "the ABI's whole-tensor form; the wrapper calls the _slice form for both uses",
    "pd3_grouped_conv3x3_small_f16": "the NHWC-input form; CenterHead feeds the group-major form (_gm) in every slice",
}
DENSE_CONV = re.compile(r"pd3_(conv3x3|scatter_conv3x3|patch_conv|grouped_conv3x3|winograd43_input_transform$)")


def _bn_randomize(module, gen):
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=gen) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=gen) + 0.5)
                m.weight.copy_(torch.rand(m.weight.shape, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.1)


def _conv3x3_layer(cin, cout, stride, n, h, wv, gen):
    """One _Conv3x3 call against float64 torch; returns the error."""
    from paddle3d_amd import centerpoint as cpm

    w = torch.randn(cout, cin, 3, 3, generator=gen) / (cin * 9) ** 0.5
    b = torch.randn(cout, generator=gen)
    x = torch.randn(n, cin, h, wv, generator=gen)
    ref = torch.relu(F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=1))
    layer = cpm._Conv3x3(w.to(DEV), b.to(DEV), stride)
    xin = F.pad(x, (0, conv.pitch4(wv) - wv)).to(DEV)
    y, wo = layer(xin, wv if wv % 4 else None)
    assert wo == wv // stride and tuple(y.shape) == (n, cout, h // stride, conv.pitch4(wo))
    assert not y[..., wo:].any()
    return float((y[..., :wo].cpu().double() - ref).abs().max())


@torch.no_grad()
def test_dispatchers_cover_every_kernel():
    from paddle3d_amd import _lib
    from paddle3d_amd import centerpoint as cpm
    from paddle3d_amd.ops import pointpillars_scatter as ps

    gen = torch.Generator().manual_seed(20)
    torch.manual_seed(20)
    with launch_ledger(_lib.lib(), _lib.symbols("test_memory_safety_gpu")) as calls:
        # _Conv3x3: both strides, with and without w_valid, either side of WINOGRAD43_PP_MIN_CIN and of the pre-transformed
        # form's 8 blocks, the bf16x3 stride-2 kernel's cout <= 1024 bound (1152 falls back to the fp32 implicit GEMM)
        for cin, cout, stride, n, h, wv in [(8, 64, 1, 2, 9, 20), (60, 64, 1, 1, 5, 18), (64, 64, 1, 1, 9, 68), (64, 448, 1, 1, 3, 12),
                                            (64, 512, 1, 2, 9, 18), (4, 32, 1, 1, 1, 4), (16, 128, 2, 2, 18, 36), (16, 1024, 2, 1, 4, 8),
                                            (16, 1152, 2, 1, 4, 8), (8, 64, 2, 1, 10, 36), (8, 64, 2, 9, 2, 8)]:
            err = _conv3x3_layer(cin, cout, stride, n, h, wv, gen)
            assert err < (5e-4 if stride == 1 else 2e-4), (cin, cout, stride, h, wv, err)  # (F(4,3): test_conv_gpu's 5e-4)
        for cin, cout, stride in [(6, 64, 1), (8, 48, 1), (8, 64, 3)]:  # no kernel family takes these: the dispatcher raises
            assert not any(f.accepts(L._case(f.name, "c", 1, cin, cout, 8, 16, stride=stride)) for f in L.FAMILIES.values()
                           if f.kind == "nchw3" and f.stride == min(stride, 2) and f.name != "wino23")
            with pytest.raises(Paddle3DAmdError):
                cpm._Conv3x3(torch.zeros(cout, cin, 3, 3, device=DEV), torch.zeros(cout, device=DEV), stride)(
                    torch.zeros(1, cin, 8, 16, device=DEV))

        # SecondFPN.forward: every patch mode on the bf16x3 kernel and on the fp32 one, the cout = 1152 level (the bf16x3
        # kernel keeps its bias in LDS: cout <= 1024) that has to fall back to the fp32 patch kernel instead of raising
        for ins, outs, strides, maps, wvs in [
            ((32, 64, 64), (128, 128, 64), (0.5, 1, 2), ((8, 64), (4, 32), (2, 16)), None),       # bf16x3: modes 0, 1, 2
            ((16, 16, 16), (64, 24, 16), (0.5, 1, 2), ((8, 16), (4, 8), (2, 4)), None),           # fp32: modes 0, 1, 2
            ((32, 16), (1152, 8), (1, 4), ((4, 16), (1, 4)), None),                               # cout 1152, mode 3
            ((32, 32), (64, 64), (2, 4), ((6, 12), (3, 8)), (10, 5)),                             # rows of pitch 12 / 8, real 10 / 5
        ]:
            neck = cpm.SecondFPN(ins, outs, strides, use_conv_for_no_stride=True).eval()
            _bn_randomize(neck, gen)
            xs = [torch.randn(2, c, h, w, generator=gen) for c, (h, w) in zip(ins, maps)]
            if wvs is not None:
                for x, wv in zip(xs, wvs):
                    x[..., wv:] = 0
            want = []
            for blk, x, wv in zip(neck.deblocks, xs, wvs or [x.shape[3] for x in xs]):
                want.append(blk.double()(x[..., :wv].double()))
                blk.float()
            want = torch.cat(want, 1)
            neck = neck.to(DEV)
            xd = [cpm._tag_valid_w(x.to(DEV), wv) for x, wv in zip(xs, wvs or [x.shape[3] for x in xs])]
            got = neck(xd).cpu().double()
            assert got.shape == want.shape, (got.shape, want.shape)
            assert float((got - want).abs().max()) < 2e-4 * max(1.0, float(want.abs().max())), (ins, outs, strides)
        assert calls["pd3_patch_conv_x3_bias_relu"] >= 3 and calls["pd3_patch_conv_bias_relu"] >= 5

        # SecondFPN.forward_f16 (fp16 NHWC stages in, the concatenated fp16 NHWC map out) on fp16-rounded weights and inputs,
        # under the bar test_second_fpn_f16_levels_match_fp32_levels holds it to (3e-3 of the magnitude)
        neck = cpm.SecondFPN((32, 64, 64), (128, 128, 64), (0.5, 1, 2), use_conv_for_no_stride=True).eval()
        _bn_randomize(neck, gen)
        with torch.no_grad():
            for m in neck.modules():
                if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
                    m.weight.copy_(m.weight.half().float())
            xs = [torch.randn(2, c, h, w, generator=gen).half().float()
                  for c, (h, w) in zip((32, 64, 64), ((16, 20), (8, 10), (4, 5)))]   # all three meet at 8 x 10
            want = torch.cat([blk.double()(x.double()) for blk, x in zip(neck.deblocks, xs)], 1)
            neck = neck.float().to(DEV)
            assert neck.amp_ok(None)
            got = neck([x.half().permute(0, 2, 3, 1).contiguous().to(DEV) for x in xs])
        assert got.dtype == torch.float16 and tuple(got.shape) == (2, 8, 10, 320)
        err = float((got.cpu().double().permute(0, 3, 1, 2) - want).abs().max())
        assert err < 3e-3 * max(1.0, float(want.abs().max())), err

        # SecondBackbone on a SparseCanvas: the three scatter-fused first layers (fp32 dense, sparse, fp16) and, under AMP, the
        # fp16 stride-1 / stride-2 / dual-output kernels
        for amp, sparse_first, cin, widths in [(False, False, 8, (64, 64)), (False, True, 16, (64, 64)), (True, True, 16, (128, 128))]:
            bb = cpm.SecondBackbone(cin, widths, (1, 1), (2, 2)).eval()
            _bn_randomize(bb, gen)
            x = torch.randn(2, cin, 16, 24, generator=gen) * (torch.rand(2, 1, 16, 24, generator=gen) < 0.4)
            want, t = [], x.double()
            for blk in bb.blocks:
                t = blk.double()(t)
                want.append(t)
                blk.float()
            bb = bb.to(DEV)
            bb.sparse_first, bb.amp = sparse_first, amp
            feats, coords = L.canvas_rows(x)
            got = bb(ps.SparseCanvas(feats.to(DEV), coords.to(DEV), 2, 16, 24))
            for g_, w_ in zip(got, want):
                tol = (3e-3 if amp else 5e-4) * max(1.0, float(w_.abs().max()))
                assert float((g_.cpu().double()[..., : w_.shape[3]] - w_).abs().max()) < tol, (amp, sparse_first)

        # CenterHead's fused forward: fp32 and AMP, the branches in slices of one group, half and all of them
        tasks = [dict(class_names=["a"]), dict(class_names=["b", "c"]), dict(class_names=["d", "e"]), dict(class_names=["f"])]
        heads = dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2))
        head = cpm.CenterHead(64, tasks, heads).eval()
        _bn_randomize(head, gen)
        x = torch.randn(2, 64, 9, 20, generator=gen)
        hd = head.double()
        shared = torch.relu(hd.shared_conv.bn(hd.shared_conv.conv(x.double())))
        want = []
        for task in hd.tasks:
            d = {}
            for name in task.heads:
                seq = getattr(task, name)
                d[name] = seq[1](torch.relu(seq[0].bn(seq[0].conv(shared))))
            want.append(d)
        head = head.float().to(DEV)
        groups = sum(len(t.heads) for t in head.tasks)
        for amp in (False, True):
            for chunk in (1, groups // 2, groups):
                head.amp, head.head_chunk = amp, chunk
                rets, _ = head(x.to(DEV))
                for got, wd in zip(rets, want):
                    for name, wt in wd.items():
                        tol = (3e-3 if amp else 1e-3) * max(1.0, float(wt.abs().max()))
                        assert float((got[name].cpu().double() - wt).abs().max()) < tol, (amp, chunk, name)
        head.amp, head.head_chunk = False, 0
        with pytest.raises(Paddle3DAmdError):  # a map width no fp32 kernel takes: no family's predicate accepts a pitch of 18
            head(torch.zeros(1, 64, 8, 18, device=DEV))

        reached = {k for k, v in calls.items() if v}
    dense = sorted(s for s in _lib.symbols("test_memory_safety_gpu") if DENSE_CONV.match(s))
    assert {f.symbol for f in L.FAMILIES.values() if f.kind != "scatter" or f.name != "scatter_sparse"} <= set(dense)
    missing = [s for s in dense if s not in reached and s not in NOT_DISPATCHED]
    assert not missing, f"dense convolution entry points no dispatcher reached: {missing}"
    assert not [s for s in NOT_DISPATCHED if s in reached or s not in dense], "NOT_DISPATCHED is out of date"
    for name in ("pd3_pillar_conv_rulebook", "pd3_rows_to_dense_fill", "pd3_f32_nchw_to_f16_nhwc"):
        assert name in reached, name
