"""pd3_grouped_conv3x3_small_counts_slice (the final SeparateHead convolutions with every group's real channel count) against
pd3_grouped_conv3x3_small_slice on zero padded weights and bias: the same bytes, the padded channels' +0.0 included, every
byte of the slice written and nothing outside it.  The entry point's row in paddle3d_amd._lib.ENTRY_POINTS names this
module: its scenario under guarded allocations (tests/guarded.py: Protocol) and the completeness assertion over the rows
that name this module are at the end of this file."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import Protocol  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
# CenterHead on nuScenes: six tasks of reg 2, height 1, dim 3, rot 2, vel 2 and a heat map of 1 or 2 classes
HEAD = [c for hm in (1, 2, 2, 1, 2, 2) for c in (2, 1, 3, 2, 2, hm)]
COUNTS = {
    "head36": (3, HEAD),
    "head_second_half": (3, HEAD[18:]),
    "ones": (3, [1] * 5),
    "full3": (3, [3] * 4),
    "mixed4": (4, [4, 1, 3, 2, 2, 4, 1]),
    "cmax2": (2, [1, 2, 2, 1]),
    "cmax1": (1, [1, 1, 1]),
    "groups64": (3, [1 + (g * 7) % 3 for g in range(64)]),
}
# 128 x 128 and 180 x 180 (the head's maps), partial tiles in both directions (h % 8, h % 16, w % 128 != 0, w % 4 == 0:
# the padded form's tiles are 8 rows high, the counts form's 16), one row in a second tile, single rows and quads
MAPS = [(128, 128), (180, 180), (13, 36), (9, 132), (17, 36), (8, 256), (1, 4)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(name, h, w, n, cg, out_group0, extra_groups, with_bias=True):
    from paddle3d_amd.ops import conv

    co, counts = COUNTS[name]
    groups = len(counts)
    g = torch.Generator().manual_seed(h * 1000 + w + groups)
    x = torch.randn(n, groups * cg, h, w, generator=g).cuda()
    wt = torch.randn(groups * co, cg, 3, 3, generator=g) / (cg * 9) ** 0.5
    b = torch.randn(groups * co, generator=g)
    for gi, c in enumerate(counts):  # the padding: zero weights, zero bias
        wt[gi * co + c:(gi + 1) * co] = 0
        b[gi * co + c:(gi + 1) * co] = 0
    wp = conv.pack_grouped_weight(wt.cuda(), groups)
    bias = b.cuda() if with_bias else None
    total = out_group0 + groups + extra_groups
    old = torch.full((n, total * co, h, w), SENTINEL, device="cuda")
    new = torch.full((n, total * co, h, w), SENTINEL, device="cuda")
    conv.grouped_conv3x3_small(x, wp, bias, groups, out=old, out_groups=total, out_group0=out_group0)
    conv.grouped_conv3x3_small(x, wp, bias, groups, out=new, out_groups=total, out_group0=out_group0, group_couts=counts)
    torch.cuda.synchronize()
    assert torch.equal(new, old)
    assert torch.equal(_bits(new), _bits(old))  # (-0.0 == +0.0 for torch.equal: the bits as well)
    lo, hi = out_group0 * co, (out_group0 + groups) * co
    assert bool((new[:, :lo] == SENTINEL).all()) and bool((new[:, hi:] == SENTINEL).all())  # nothing outside the slice
    assert not bool((new[:, lo:hi] == SENTINEL).any())                                      # every byte of it
    for gi, c in enumerate(counts):  # the padded channels: +0.0
        pad = new[:, lo + gi * co + c:lo + (gi + 1) * co]
        assert not bool(_bits(pad).any()), (name, gi)
    return new


@pytest.mark.parametrize("h,w", MAPS)
@pytest.mark.parametrize("name", ["head36", "mixed4"])
def test_counts_form_equals_padded_form_on_maps(name, h, w):
    _run(name, h, w, n=1, cg=64, out_group0=0, extra_groups=0)


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_counts_form_equals_padded_form_in_a_slice(name):
    """out_group0 > 0 inside a wider output, two images, partial tiles"""
    _run(name, 20, 140, n=2, cg=16 if name == "groups64" else 64, out_group0=3, extra_groups=2)


def test_counts_form_short_channels_and_no_bias():
    _run("mixed4", 12, 24, n=3, cg=4, out_group0=1, extra_groups=0, with_bias=False)  # one trip: nothing is prefetched
    _run("head_second_half", 16, 128, n=1, cg=8, out_group0=18, extra_groups=0)


def test_counts_form_refuses_what_it_cannot_take():
    from paddle3d_amd._lib import Paddle3DAmdError
    from paddle3d_amd.ops import conv

    x = torch.zeros(1, 2 * 8, 8, 8, device="cuda")
    wp = torch.zeros(2, 8, 3, 9, device="cuda")
    out = torch.full((1, 6, 8, 8), SENTINEL, device="cuda")
    for counts in ([0, 1], [4, 1]):  # a count outside 1 .. cout_per_group
        with pytest.raises(Paddle3DAmdError):
            conv.grouped_conv3x3_small(x, wp, None, 2, out=out, group_couts=counts)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def test_center_head_slices_use_the_counts_form():
    """CenterHead's fp32 sliced path hands the real counts over and returns what the padded form returns."""
    from paddle3d_amd import centerpoint as cpm
    from paddle3d_amd.ops import conv

    torch.manual_seed(3)
    tasks = [dict(class_names=["a"]), dict(class_names=["b", "c"])]
    heads = dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2))
    head = cpm.CenterHead(64, tasks, heads).eval().cuda()
    x = torch.randn(2, 64, 16, 64, device="cuda")
    groups = sum(len(t.heads) for t in head.tasks)
    head.head_chunk = groups // 2
    seen = []
    real = conv.grouped_conv3x3_small

    def spy(*a, **k):
        seen.append(k.get("group_couts"))
        return real(*a, **k)

    def padded(*a, **k):
        k.pop("group_couts", None)
        return real(*a, **k)

    try:
        conv.grouped_conv3x3_small = spy
        got, _ = head(x)
        conv.grouped_conv3x3_small = padded
        want, _ = head(x)
    finally:
        conv.grouped_conv3x3_small = real
    f = head._plan()
    assert seen == [f["ncls"][:groups // 2], f["ncls"][groups // 2:]]
    for a, b in zip(got, want):
        for name in a:
            assert torch.equal(a[name], b[name]), name


P = Protocol("test_grouped_counts_gpu", "grouped-counts", "cuda")


@P.scenario
def counts_form():
    """Seeded inputs and a call whose outputs are allocated under the guard: a slice into a wider tensor that the caller
    cleared, and a whole tensor the wrapper allocates (torch.empty: stale bytes under the guard)."""
    from paddle3d_amd.ops import conv

    co, counts = COUNTS["mixed4"]
    groups, cg, n, h, w = len(counts), 8, 2, 11, 132
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, groups * cg, h, w, generator=g).cuda()
    wt = torch.randn(groups * co, cg, 3, 3, generator=g)
    b = torch.randn(groups * co, generator=g)
    for gi, c in enumerate(counts):
        wt[gi * co + c:(gi + 1) * co] = 0
        b[gi * co + c:(gi + 1) * co] = 0
    inputs = dict(x=x, wp=conv.pack_grouped_weight(wt.cuda(), groups), b=b.cuda())

    def call():
        wide = torch.zeros((n, (groups + 3) * co, h, w), dtype=torch.float32, device="cuda")
        conv.grouped_conv3x3_small(inputs["x"], inputs["wp"], inputs["b"], groups, out=wide, out_groups=groups + 3,
                                   out_group0=2, group_couts=counts)
        auto = conv.grouped_conv3x3_small(inputs["x"], inputs["wp"], inputs["b"], groups, group_couts=counts)
        return dict(wide=wide, auto=auto)

    return inputs, call


def test_counts_form_under_guarded_allocations():
    P.check_scenario("counts_form")


def test_every_entry_point_of_symbols_head_is_exercised():
    """Runs last; runs the scenario itself when it was not selected."""
    from paddle3d_amd import _lib

    P.check_complete(_lib.symbols("test_grouped_counts_gpu"), 1)
