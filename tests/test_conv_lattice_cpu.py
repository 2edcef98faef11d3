"""The dense convolution lattice's own checks, on the CPU (tests/conv_lattice.py): every family yields its axes and
refusals, the exact class's precondition holds, the float64 reference builders lay their tensors out as the kernels do,
every packer round-trips, the F(4x4, 3x3) float32 restatement is what it claims to be, and the bf16x3 predicates
carry the byte-size clause of their launchers."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_lattice as L  # noqa: E402

from paddle3d_amd.ops import conv  # noqa: E402

FAMS = list(L.FAMILIES.values())
AXES = ("height", "width", "ptiles", "channels", "epilogue")


@pytest.mark.parametrize("fam", FAMS, ids=lambda f: f.name)
def test_every_family_yields_every_axis_and_refusal(fam):
    cases = L.accept_cases(fam)
    assert all(fam.accepts(c) for c in cases)
    for axis in AXES:
        assert any(c.axis == axis for c in cases), (fam.name, axis)
    assert len({c.id for c in cases}) == len(cases)
    # the launchers round pixel tiles up to a multiple of 8: one short of, on and one past a multiple, and two rounds + 1
    assert {c.n for c in cases if c.axis == "ptiles"} >= {7, 8, 9, 17}
    T, C = fam.tile[0], fam.tile[1]
    # heights below, on and past the tile: at least three different ones (a predicate may forbid odd heights)
    assert len({c.h for c in cases if c.axis == "height"}) >= 3
    refusals = L.refuse_cases(fam)
    for clause, base, bad in refusals:
        assert fam.accepts(base) and not fam.accepts(bad), (fam.name, clause, bad.id)
    assert len(refusals) >= 2
    assert len({clause for clause, _, _ in refusals}) == len(refusals)
    for _, base, bad in refusals:
        changed = [k for k in ("n", "cin", "cout", "h", "wv") if getattr(base, k) != getattr(bad, k)]
        assert 1 <= len(changed) + (base.opt != bad.opt) <= 3, (base, bad)
    assert T > 0 and C > 0


def test_the_sweep_stays_small():
    cases = L.all_accepts()
    assert 300 <= len(cases) <= 999
    for c in cases:
        fam = L.FAMILIES[c.family]
        out = 1
        for s in fam.out_shape(c):
            out *= s
        assert max(out, c.n * fam.groups(c) * c.cin * c.h * c.wv) * 4 < 64 << 20, c.id


@pytest.mark.parametrize("fam", FAMS, ids=lambda f: f.name)
def test_exact_class_precondition(fam):
    """K * max|x| * max|w| (+ bias) below 2^24, below 2^11 where the output is fp16; all operands exact in bf16 and fp16."""
    for c in L.accept_cases(fam):
        x, w, b = L.make_data(fam, c, "exact")  # (asserts the bound)
        xm, wm, bm, step = L.exact_limits(fam, c)
        assert L.exact_bound(fam, c, xm, wm, bm) < (2 ** 11 if fam.out_f16 else 2 ** 24)
        for t in (x, w):
            assert torch.equal(t.bfloat16().float(), t) and torch.equal(t.half().float(), t)
        if fam.name == "wino23":
            assert torch.equal(w % 4, torch.zeros_like(w))
        if fam.exact == "wino43":
            assert float(w.abs().max()) <= 2 and torch.equal(w, w.round())
        ref = fam.reference(c, x, w, b)
        assert float(ref.abs().max()) <= L.exact_bound(fam, c, xm, wm, bm)
        if fam.out_f16:
            assert torch.equal(ref.half().double(), ref)


def _logical_input(fam, c, xin):
    """The kernel's input tensor read back as [n, channels, h, wv], written out here independently of Family.lay_in."""
    if fam.kind in ("f16", "f16s2", "groupedf16"):
        if fam.opts.get("group_major_in"):
            n, g, h, w, _ = xin.shape
            return torch.stack([xin[:, i] for i in range(g)], 1).permute(0, 1, 4, 2, 3).reshape(n, g * 64, h, w).float()
        return torch.einsum("nhwc->nchw", xin.float())
    assert xin.shape[3] == c.o("pitch", conv.pitch4(c.wv)) and not xin[..., c.wv:].any()
    return xin[..., : c.wv]


def _valid_output(fam, c, t, ch):
    """The valid region of an output tensor as [n, ch, ho, wo], plus the rest of it (what must be zero / SENTINEL)."""
    ho, wo = fam.out_hw(c)
    mode = fam.opts.get("out", "nhwc")
    if fam.kind in ("f16", "f16s2") or fam.predicate == "scatter_conv_s2_f16_supported":
        if mode == "f32":
            return t, None
        if mode == "gm":
            return torch.cat([t[:, i].permute(0, 3, 1, 2) for i in range(t.shape[1])], 1), None
        return torch.einsum("nhwc->nchw", t), None
    c0 = c.o("off", 0) if fam.kind == "patch" else c.o("out_group0", 0) * c.cout
    rest = t.clone()
    rest[:, c0:c0 + ch, :, :wo] = 0
    rest[:, c0:c0 + ch, :, wo:] += 0  # (padding columns: must be zero already)
    return t[:, c0:c0 + ch, :, :wo], (rest, c0, ch)


@pytest.mark.parametrize("fam", FAMS, ids=lambda f: f.name)
def test_reference_builders_agree_with_torch_float32(fam):
    """The float64 reference in the kernel's output layout against torch.nn.functional in float32 on the kernel's INPUT
    layout: guards w_valid / pitch4 / channel offset / NHWC / group-major handling of the builders themselves."""
    for c in L.accept_cases(fam):
        x, w, b = L.make_data(fam, c, "random")
        if fam.kind == "scatter":
            feats, coords = L.canvas_rows(x)
            dense = torch.zeros_like(x)
            keep = coords[:, 0] >= 0
            dense[coords[keep, 0].long(), :, coords[keep, 2].long(), coords[keep, 3].long()] = feats[keep]
            assert torch.equal(dense, x)
            xl = dense
        else:
            xl = _logical_input(fam, c, fam.lay_in(c, x))
        g = fam.groups(c)
        if fam.kind == "patch":
            mode = fam.opts["mode"]
            y = (F.conv2d(xl, w, b, stride=2) if mode == 0 else F.conv2d(xl, w, b) if mode == 1
                 else F.conv_transpose2d(xl, w, b, stride=2 * (mode - 1)))
        else:
            y = F.conv2d(xl, w, b, stride=fam.stride, padding=1, groups=g)
        if c.relu:
            y = torch.relu(y)
        exp = fam.expected(c, fam.reference(c, x, w, b))
        assert tuple(exp.shape) == tuple(fam.out_shape(c)), c.id
        got, rest = _valid_output(fam, c, exp, y.shape[1])
        assert got.shape == y.shape, (c.id, got.shape, y.shape)
        mag = max(1.0, float(y.abs().max()))
        assert float((got - y.double()).abs().max()) <= 1e-5 * mag, c.id
        if rest is not None:
            r, c0, ch = rest
            assert not r[:, c0:c0 + ch].any(), c.id                       # padding columns of the written channels: zero
            assert (r[:, :c0] == L.SENTINEL).all() and (r[:, c0 + ch:] == L.SENTINEL).all(), c.id


@pytest.mark.parametrize("fam", [f for f in FAMS if f.packer != "sparse"], ids=lambda f: f.name)
def test_packers_round_trip(fam):
    for c in [c for c in L.accept_cases(fam) if c.axis == "channels"]:
        _, w, _ = L.make_data(fam, c, "exact")
        back = L.unpack(fam, c, fam.pack(c, w))
        assert back.shape == w.shape, c.id
        if fam.exact == "wino43":  # U carries 1/6 and 1/24 rounded to fp32: 36 such values of size <= 2 per weight
            assert float((back - w.double()).abs().max()) <= 36 * 2 * 2.0 ** -23, c.id
        else:
            assert torch.equal(back.float(), w), c.id
        _, wr, _ = L.make_data(fam, c, "random")
        if fam.packer in ("pack_patch_weight_x3", "pack_conv3x3_s2_x3_weight", "pack_conv3x3_weight", "pack_patch_weight",
                          "pack_grouped_weight"):  # fp32 survives exactly (three bf16 pieces sum back to it)
            assert torch.equal(L.unpack(fam, c, fam.pack(c, wr)).float(), wr), c.id


@pytest.mark.parametrize("cin", [4, 64, 384])
def test_winograd43_restatement_is_the_convolution(cin):
    """F(4x4, 3x3) in float32 against float64 conv2d on the exact class (8 x 16 maps, |x| <= 4, integer |w| <= 2, 32 output
    channels).  Measured here: 1.1e-4 / 1.2e-3 / 5.2e-3 at cin 4 / 64 / 384 (outputs up to 78 / 306 / 741; the figure at 384
    depends on the order in which the 384 products of a component are summed).  The GPU test allows a kernel 4 x this error,
    and a missing or doubled term moves a result by at least 1: the restatement has to stay below 1 / 16 for that bar to keep
    a factor 4 under a missing term, which is what is asserted."""
    fam = L.FAMILIES["wino43_t32"]
    c = L._case("wino43_t32", "channels", 1, cin, 32, 8, 16, relu=False)
    x, w, b = L.make_data(fam, c, "exact")
    ref = fam.reference(c, x, w, b)
    err = float((L.winograd43_f32(x, w, b, c.relu).double() - ref).abs().max())
    print(f"cin {cin}: restatement error {err:.3e}, outputs up to {float(ref.abs().max()):.0f}")
    assert err <= 1 / 16
    # and it does see one term changed by one
    w2 = w.clone()
    w2[0, 0, 0, 0] += 1
    assert float((L.winograd43_f32(x, w2, b, c.relu).double() - ref).abs().max()) >= 1 - 1 / 16


def test_bf16x3_predicates_carry_the_launchers_byte_clause():
    """The 2 GB operand clause (32-bit buffer offsets) of the two bf16x3 kernels cannot be exercised with real buffers:
    the predicates against a restatement of conv_patch_x3.hip:376-381 / conv_s2_x3.hip:269-275.  A predicate may be
    stricter than its launcher (it does not know w_valid), never looser."""
    seen_false = 0
    for batch in (1, 16, 84, 85, 86, 128, 341, 342, 1 << 20):
        for cin, cout, h, w in ((384, 128, 128, 128), (64, 128, 512, 512), (256, 128, 128, 128), (32, 1024, 64, 64),
                                (128, 256, 256, 256)):
            for mode in (0, 1, 2):
                for ctot in (cout, 3 * cout):
                    p = conv.patch_x3_supported(mode, cin, cout, h, w, batch, ctot)
                    r = L.patch_x3_bytes_ok(mode, batch, cin, cout, ctot, h, w, w)
                    assert not p or r, (mode, batch, cin, cout, ctot, h, w)
                    assert p == r, (mode, batch, cin, cout, ctot, h, w)  # (w_valid == w: the two agree exactly)
                    seen_false += not p
            p = conv.conv3x3_s2_x3_supported(cin, cout, h, w, batch)
            assert not p or L.s2_x3_bytes_ok(batch, cin, cout, h, w, w), (batch, cin, cout, h, w)
            seen_false += not p
    assert seen_false > 10
    # a 384 x 128 x 128 fp32 input: 85 frames stay below 2 GB (2 139 095 040 bytes), 86 do not
    assert conv.patch_x3_supported(1, 384, 128, 128, 128, 85, 128) and not conv.patch_x3_supported(1, 384, 128, 128, 128, 86, 128)
    assert not conv.patch_x3_supported(1, 32, 1152, 8, 8) and conv.patch_x3_supported(1, 32, 1024, 8, 8)
    assert conv.patch_supported(1, 32, 1152, 8, 8)  # (the fp32 patch kernel takes the level the bf16x3 one refuses)
