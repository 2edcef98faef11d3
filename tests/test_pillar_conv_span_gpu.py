"""pd3_pillar_conv_span_x3 (the sparse first backbone layer as one launch from the inverse map to NCHW,
csrc/pillar_conv_span.hip) against the three-step form it replaces where its tile fits (ops.conv.scatter_conv3x3_sparse:
rulebook -> bf16x3 gather-GEMM -> rows to NCHW): the same bytes on every occupancy that takes another path through the
kernel, the fp64 statement of the layer within the three-step form's own bound
(tests/test_conv_gpu.py::test_scatter_conv_as_sparse_convolution), the shapes it refuses, SecondBackbone's dispatch.  The
entry point's row in paddle3d_amd._lib.ENTRY_POINTS names this module: its scenario under guarded allocations
(tests/guarded.py: Protocol) and the completeness assertion over the rows that name this module are at the end of this
file.

Shapes: 2 frames, input 16 x 512 and 32 x 1024 = one and two 256-cell spans per output row, whose first and last rows and
columns see the padding; 64 input channels, 64 and 128 output channels (one and two workgroups per span)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import Protocol, launch_ledger  # noqa: E402

pytestmark = pytest.mark.gpu

CIN = 64
SHAPES = [(16, 512), (32, 1024)]
CASES = ["random11", "empty_frame", "full_span", "corner", "all_masks", "padding_rows", "nothing"]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _cells(g, b, ny, nx, occ):
    """random cells of frame b at occupancy occ (duplicates possible: the highest row wins in the inverse map)"""
    m = max(1, int(ny * nx * occ))
    return torch.stack([torch.full((m,), b), torch.zeros(m, dtype=torch.long), torch.randint(0, ny, (m,), generator=g),
                        torch.randint(0, nx, (m,), generator=g)], 1)


def _coords(case, ny, nx):
    g = torch.Generator().manual_seed(ny * 31 + nx + len(case))
    if case == "random11":        # the occupancy of a nuScenes canvas
        c = torch.cat([_cells(g, 0, ny, nx, 0.11), _cells(g, 1, ny, nx, 0.11)])
    elif case == "empty_frame":   # frame 0 holds nothing: its spans are fill alone, between spans that are not
        c = _cells(g, 1, ny, nx, 0.11)
    elif case == "full_span":     # five full input rows: output rows 0 .. 2 are full spans, eight blocks in every tap
        ys, xs = torch.meshgrid(torch.arange(5), torch.arange(nx), indexing="ij")
        full = torch.stack([torch.zeros(5 * nx, dtype=torch.long), torch.zeros(5 * nx, dtype=torch.long), ys.reshape(-1),
                            xs.reshape(-1)], 1)
        c = torch.cat([full, _cells(g, 1, ny, nx, 0.05)])
    elif case == "corner":        # one pillar alone in a corner of each frame: one cell, one tap
        c = torch.tensor([[0, 0, 0, 0], [1, 0, ny - 1, nx - 1]])
    elif case == "all_masks":     # half the cells: every span has far more than 32 active cells, all 512 masks possible
        c = torch.cat([_cells(g, 0, ny, nx, 0.7), _cells(g, 1, ny, nx, 0.7)])
    elif case == "padding_rows":  # a third of the pillar rows are padding (batch index -1)
        c = torch.cat([_cells(g, 0, ny, nx, 0.2), _cells(g, 1, ny, nx, 0.2)])
        c[::3, 0] = -1
    elif case == "nothing":       # pillar rows, none of them on the canvas
        c = _cells(g, 0, ny, nx, 0.01)
        c[:, 0] = -1
    else:
        raise KeyError(case)
    return c[torch.randperm(c.shape[0], generator=g)].int()


_INPUTS = {}


def _inputs(case, ny, nx, cout):
    """(SparseCanvas, weight, bias, the three-step form's result), computed once per case and left unchanged"""
    from paddle3d_amd.ops import conv
    from paddle3d_amd.ops import pointpillars_scatter as ps

    key = (case, ny, nx, cout)
    if key not in _INPUTS:
        coords = _coords(case, ny, nx)
        g = torch.Generator().manual_seed(coords.shape[0] + cout)
        m = coords.shape[0]
        feats = (torch.randn(m, CIN, generator=g) * torch.exp(torch.randn(m, CIN, generator=g))).cuda()
        w = (torch.randn(cout, CIN, 3, 3, generator=g) * 0.05).cuda()
        b = torch.randn(cout, generator=g).cuda()
        sc = ps.SparseCanvas(feats, coords.cuda(), 2, ny, nx)
        assert conv.scatter_conv_sparse_supported(CIN, cout, ny, nx, 2)
        want, _ = conv.scatter_conv3x3_sparse(sc, w, b)
        _INPUTS[key] = (sc, w, b, want)
    return _INPUTS[key]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("cout", [64, 128])
@pytest.mark.parametrize("ny,nx", SHAPES)
def test_span_form_equals_three_step_form(ny, nx, cout, case):
    from paddle3d_amd.ops import conv

    sc, w, b, want = _inputs(case, ny, nx, cout)
    assert conv.scatter_conv_span_supported(CIN, cout, ny, nx, 2)
    got, packed = conv.scatter_conv3x3_span(sc, w, b)
    again, _ = conv.scatter_conv3x3_span(sc, w, b, packed)
    torch.cuda.synchronize()
    assert got.shape == want.shape == (2, cout, ny // 2, nx // 2)
    diff = int((_bits(got) != _bits(want)).sum())
    print(f"{case} {ny}x{nx} cout {cout}: {diff} of {got.numel()} elements differ from the three-step form")
    assert torch.equal(got, want)
    assert torch.equal(_bits(got), _bits(want))      # (-0.0 == +0.0 for torch.equal: the bits as well)
    assert torch.equal(_bits(again), _bits(got))     # run-to-run identical, the cached weight pieces and fill included
    if case != "nothing":                            # not fill alone
        assert not torch.equal(got, torch.relu(b).view(1, -1, 1, 1).expand_as(got))


@pytest.mark.parametrize("ny,nx,cout,case", [(16, 512, 64, c) for c in CASES] + [(16, 512, 128, "random11"),
                                                                              (32, 1024, 64, "random11")])
def test_span_form_against_fp64_convolution(ny, nx, cout, case):
    """The bound of tests/test_conv_gpu.py::test_scatter_conv_as_sparse_convolution, unchanged: within 2x the dense fp32
    kernel's own error against fp64 (or 2e-6 of the magnitude) and inside 1e-3; cells without an occupied tap hold
    relu(bias) exactly."""
    import torch.nn.functional as F

    from paddle3d_amd.ops import conv

    sc, w, b, _ = _inputs(case, ny, nx, cout)
    got, _ = conv.scatter_conv3x3_span(sc, w, b)
    canvas = sc.dense()
    ref64 = F.relu(F.conv2d(canvas.double().cpu(), w.double().cpu(), b.double().cpu(), stride=2, padding=1))
    dense32 = conv.conv3x3_bias_relu(canvas, conv.pack_conv3x3_weight(w), b, cout, relu=True, stride=2)[..., : nx // 2]
    mag = max(1.0, float(ref64.abs().max()))
    err = float((got.double().cpu() - ref64).abs().max())
    err_dense = float((dense32.double().cpu() - ref64).abs().max())
    print(f"{case} {ny}x{nx} cout {cout}: err {err:.3e}, dense fp32 kernel {err_dense:.3e}, magnitude {mag:.3e}")
    assert err <= max(2.0 * err_dense, 2e-6 * mag) and err < 1e-3, (err, err_dense, mag)
    occd = (canvas.abs().sum(1, keepdim=True) > 0).float()
    active = F.max_pool2d(F.pad(occd, (1, 1, 1, 1)), 3, 2)[..., : ny // 2, : nx // 2] > 0
    fill = torch.relu(b).view(1, -1, 1, 1).expand_as(got)
    assert torch.equal(got[(~active).expand_as(got)], fill[(~active).expand_as(got)])


def test_span_form_without_relu_and_without_bias():
    """the epilogue's other forms: no ReLU (fill = bias), no bias at all (fill = 0) -- against the three-step form"""
    from paddle3d_amd._lib import lib
    from paddle3d_amd.ops import conv
    from paddle3d_amd.ops._common import check, ptr, stream_ptr

    sc, w, b, _ = _inputs("random11", 16, 512, 64)
    want, _ = conv.scatter_conv3x3_sparse(sc, w, b, relu=False)
    got, packed = conv.scatter_conv3x3_span(sc, w, b, relu=False)
    assert torch.equal(_bits(got), _bits(want)) and bool((got < 0).any())
    zero = torch.zeros_like(b)
    want0, _ = conv.scatter_conv3x3_sparse(sc, w, zero)
    out = torch.full_like(want0, -12345.0)
    check(lib().pd3_pillar_conv_span_x3(ptr(sc.features), sc.features.shape[0], ptr(sc.inv), 2, 16, 512, 2, CIN, 64,
                                        ptr(packed[0]), None, ptr(zero), 1, ptr(out), stream_ptr(out.device)), "span")
    assert torch.equal(out, want0)


def test_refused_shapes_return_unsupported():
    """status -3 from the C entry point, nothing written; the predicate says the same"""
    from paddle3d_amd._lib import lib
    from paddle3d_amd.ops import conv
    from paddle3d_amd.ops._common import ptr, stream_ptr

    f = torch.zeros(8, 128, device="cuda")
    inv = torch.full((2, 64 * 1024), -1, dtype=torch.int32, device="cuda")
    wpk = torch.zeros(3 * 9 * 128 * 128, dtype=torch.bfloat16, device="cuda")
    bias = torch.zeros(128, device="cuda")
    out = torch.full((2 * 128 * 32 * 512,), -12345.0, device="cuda")
    #            ny   nx  stride cin cout
    refused = [(16, 24, 2, 64, 64),      # the lattice test's canvas: 12 output columns
               (16, 510, 2, 64, 64),     # 255 output columns
               (16, 640, 2, 64, 64),     # 320: a whole span and a quarter
               (16, 512, 1, 64, 64),     # stride 1
               (16, 512, 2, 32, 64),     # other input widths
               (16, 512, 2, 128, 64),
               (16, 512, 2, 64, 32),     # other output widths
               (16, 512, 2, 64, 256)]
    for ny, nx, stride, cin, cout in refused:
        assert not conv.scatter_conv_span_supported(cin, cout, ny, nx, stride), (ny, nx, stride, cin, cout)
        st = lib().pd3_pillar_conv_span_x3(ptr(f), 8, ptr(inv), 2, ny, nx, stride, cin, cout, ptr(wpk), ptr(bias), ptr(bias),
                                           1, ptr(out), stream_ptr(out.device))
        assert st == -3, (ny, nx, stride, cin, cout, st)
    assert conv.scatter_conv_span_supported(64, 128, 15, 511, 2)  # (odd canvases: ho = 8, wo = 256)
    torch.cuda.synchronize()
    assert bool((out == -12345.0).all())


def _backbone(cin, widths, seed):
    from paddle3d_amd import centerpoint as cpm

    torch.manual_seed(seed)
    bb = cpm.SecondBackbone(cin, widths, (1, 1), (2, 2)).eval()
    with torch.no_grad():
        for m in bb.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.2)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
    return bb.cuda()


def test_second_backbone_takes_the_span_form_where_it_fits():
    """at 16 x 512 the span form runs (and neither the rulebook nor the row writer); at 16 x 24 and with span_first off the
    three-step form does; the outputs are equal where both can run"""
    from paddle3d_amd import _lib
    from paddle3d_amd.ops import pointpillars_scatter as ps

    names = ("pd3_pillar_conv_span_x3", "pd3_pillar_conv_rulebook", "pd3_rows_to_dense_fill")
    bb = _backbone(CIN, (64, 64), 5)
    outs = {}
    for ny, nx, span_first, want in [(16, 512, True, (1, 0, 0)), (16, 512, False, (0, 1, 1)), (16, 24, True, (0, 1, 1))]:
        g = torch.Generator().manual_seed(ny + nx)
        coords = torch.cat([_cells(g, 0, ny, nx, 0.3), _cells(g, 1, ny, nx, 0.3)]).int().cuda()
        feats = torch.randn(coords.shape[0], CIN, generator=g).cuda()
        bb.span_first = span_first
        with launch_ledger(_lib.lib(), names) as calls:
            outs[(ny, nx, span_first)] = bb(ps.SparseCanvas(feats, coords, 2, ny, nx))
        assert tuple(calls[n] for n in names) == want, (ny, nx, span_first, calls)
    for a, b in zip(outs[(16, 512, True)], outs[(16, 512, False)]):
        assert torch.equal(_bits(a), _bits(b))
    bb.span_first = True


P = Protocol("test_pillar_conv_span_gpu", "pillar-conv-span", "cuda")


@P.scenario
def span_form():
    """Seeded inputs (computed once per case, see _inputs) and calls whose outputs -- and the cached weight pieces -- are
    allocated under the guard (torch.empty: stale bytes there): both channel widths, two spans per row."""
    from paddle3d_amd.ops import conv

    sc64, w64, b64, _ = _inputs("random11", 32, 1024, 64)
    sc128, w128, b128, _ = _inputs("full_span", 16, 512, 128)
    inputs = dict(f64=sc64.features, inv64=sc64.inv, w64=w64, b64=b64, f128=sc128.features, inv128=sc128.inv, w128=w128,
                  b128=b128)

    def call():
        o64, p64 = conv.scatter_conv3x3_span(sc64, w64, b64)
        o128, p128 = conv.scatter_conv3x3_span(sc128, w128, b128)
        return dict(o64=o64, o128=o128, pieces64=p64[0].view(torch.int16), pieces128=p128[0].view(torch.int16))

    return inputs, call


def test_span_form_under_guarded_allocations():
    P.check_scenario("span_form")


def test_every_entry_point_of_symbols_span_is_exercised():
    """Runs last; runs the scenario itself when it was not selected."""
    from paddle3d_amd import _lib

    P.check_complete(_lib.symbols("test_pillar_conv_span_gpu"), 1)
