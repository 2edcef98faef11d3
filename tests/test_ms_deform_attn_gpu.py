"""ms_deform_attn on the device (paddle3d_amd/ops/ms_deform_attn.py, csrc/ms_deform_attn.hip): the forward equals the
NumPy restatement tests/golden/ms_deform_attn_numpy.py bit for bit in fp32 and fp64 at BEVFormer-tiny's three call
sites and a four-level shape; the gradients match the fp64 restatement; edge locations, bad level tables, im2col_step,
empty inputs and the absence of host synchronisation."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import ms_deform_attn_numpy as md  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# BEVFormer-tiny (embed 256, 8 heads => C = 32; BEV 50 x 50; one FPN level 15 x 25), bs = 1
CALL_SITES = {
    "tsa": dict(B=2, Q=2500, M=8, C=32, shapes=[[50, 50]], P=4),
    "sca": dict(B=6, Q=2500, M=8, C=32, shapes=[[15, 25]], P=8),
    "decoder": dict(B=1, Q=900, M=8, C=32, shapes=[[50, 50]], P=4),
    "four_level": dict(B=2, Q=10000, M=8, C=32, shapes=[[100, 176], [50, 88], [25, 44], [13, 22]], P=4),
}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _op():
    from paddle3d_amd.ops import ms_deform_attn

    return ms_deform_attn


def _run(value, loc, attn, shapes, starts, step=64):
    return _op().ms_deform_attn(_t(value), _t(loc), _t(attn), _t(shapes), _t(starts), step)


def _bits(x, dtype):
    return x.cpu().numpy().view(np.uint32 if dtype == np.float32 else np.uint64)


def _case(seed, B, Q, M, C, shapes, P, dtype, lo=-0.1, hi=1.1):
    return md.random_case(np.random.default_rng(seed), B, Q, M, C, shapes, P, dtype, lo, hi)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("site", list(CALL_SITES))
def test_forward_bit_exact_call_sites(site, dtype):
    c = CALL_SITES[site]
    value, loc, attn, shapes, starts = _case(11, c["B"], c["Q"], c["M"], c["C"], c["shapes"], c["P"], dtype)
    out = _run(value, loc, attn, shapes, starts)
    assert tuple(out.shape) == (c["B"], c["Q"], c["M"] * c["C"]) and out.dtype == _t(value).dtype
    want = md.forward(value, loc, attn, shapes, starts)
    np.testing.assert_array_equal(_bits(out, dtype), want.view(_bits(out, dtype).dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("C", [32, 64, 16, 3])
@pytest.mark.parametrize("M", [1, 8])
@pytest.mark.parametrize("shapes,P", [([[7, 9]], 1), ([[12, 10], [6, 5], [3, 3], [2, 1]], 8), ([[5, 11], [3, 6]], 3)])
def test_forward_bit_exact_channels(C, M, shapes, P, dtype):
    value, loc, attn, sh, st = _case(C * 100 + M * 10 + P, 2, 37, M, C, shapes, P, dtype, -0.3, 1.3)
    want = md.forward(value, loc, attn, sh, st)
    out = _run(value, loc, attn, sh, st)
    np.testing.assert_array_equal(_bits(out, dtype), want.view(_bits(out, dtype).dtype))


def test_forward_unaligned_value_takes_the_generic_path():
    value, loc, attn, sh, st = _case(5, 2, 300, 8, 32, [[20, 30], [10, 15]], 4, np.float32)
    buf = torch.empty(value.size + 1, dtype=torch.float32, device=DEV)
    v = buf[1:].view(value.shape)  # contiguous, 4-B but not 16-B aligned
    v.copy_(_t(value))
    out = _op().ms_deform_attn(v, _t(loc), _t(attn), _t(sh), _t(st), 64)
    np.testing.assert_array_equal(_bits(out, np.float32), md.forward(value, loc, attn, sh, st).view(np.uint32))


def _edge_locations(H, W, dtype):
    """x, y pairs on and around the map's edges: 0, 1, h in (-1, 0) and (H-1, H), exactly -1 and H, far, NaN, Inf."""
    def xs(n):
        return [0.0, 1.0, 0.25 / n, 1.0 - 0.25 / n, -0.5 / n, (n + 0.5) / n, 0.2 / n, (n + 0.3) / n, 0.5, -3.0, 5.0,
                1e30, -1e30, np.nan, np.inf, -np.inf]
    pts = [(x, y) for x in xs(W) for y in xs(H)]
    return np.asarray(pts, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_edges_and_non_finite_locations(dtype):
    H, W, M, C = 6, 9, 2, 32
    shapes, starts, S = md.level_layout([[H, W]])
    pts = _edge_locations(H, W, dtype)  # [N, 2]
    N = pts.shape[0]
    rng = np.random.default_rng(3)
    value = rng.standard_normal((1, S, M, C)).astype(dtype)
    loc = np.broadcast_to(pts[None, :, None, None, None, :], (1, N, M, 1, 1, 2)).astype(dtype).copy()
    attn = rng.uniform(0.1, 1.0, (1, N, M, 1, 1)).astype(dtype)
    want = md.forward(value, loc, attn, shapes, starts)
    out = _run(value, loc, attn, shapes, starts)
    bt = np.uint32 if dtype == np.float32 else np.uint64
    np.testing.assert_array_equal(_bits(out, dtype), want.view(bt))
    bad = ~np.isfinite(pts).all(1)
    assert bad.sum() > 0 and np.all(out.cpu().numpy()[0, bad] == 0)
    go = rng.standard_normal((1, N, M * C)).astype(dtype)
    gv, gl, ga = _op().ms_deform_attn_backward(_t(go), _t(value), _t(loc), _t(attn), _t(shapes), _t(starts), 64)
    assert bool(torch.isfinite(gv).all())
    gl, ga = gl.cpu().numpy(), ga.cpu().numpy()
    assert np.all(gl[0, bad] == 0) and np.all(ga[0, bad] == 0)
    # the restatement in the same dtype takes the same range and floor decisions at these exact edges
    rv, rl, ra = md.backward(go, value, loc, attn, shapes, starts)
    tol = 1e-4 if dtype == np.float32 else 1e-10
    assert np.abs(gl - rl).max() <= tol * max(np.abs(rl).max(), 1.0)
    assert np.abs(ga - ra).max() <= tol * max(np.abs(ra).max(), 1.0)
    assert np.abs(gv.cpu().numpy() - rv).max() <= tol * max(np.abs(rv).max(), 1.0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_level_start_past_s_reads_nothing_outside(dtype):
    value, loc, attn, shapes, starts = _case(9, 2, 200, 4, 32, [[10, 12], [5, 6], [3, 3]], 4, dtype, -0.2, 1.2)
    S = value.shape[1]
    for bad in (starts + np.array([0, 0, S - 4], np.int64), starts + np.array([0, S, 10 * S], np.int64),
                starts - np.array([0, 200, 0], np.int64)):
        want = md.forward(value, loc, attn, shapes, bad)
        out = _run(value, loc, attn, shapes, bad)
        assert bool(torch.isfinite(out).all())
        bt = np.uint32 if dtype == np.float32 else np.uint64
        np.testing.assert_array_equal(_bits(out, dtype), want.view(bt))
        go = np.ones(out.shape, dtype)
        gv, gl, ga = _op().ms_deform_attn_backward(_t(go), _t(value), _t(loc), _t(attn), _t(shapes), _t(bad), 64)
        assert bool(torch.isfinite(gv).all() and torch.isfinite(gl).all() and torch.isfinite(ga).all())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_absurd_level_tables_contribute_nothing(dtype):
    value, loc, attn, shapes, starts = _case(10, 1, 100, 2, 32, [[6, 7], [3, 4], [2, 2], [1, 3]], 4, dtype,
                                             -0.2, 1.2)
    i64 = np.iinfo(np.int64)
    shapes = shapes.copy()
    starts = starts.copy()
    shapes[1] = [2 ** 40, 5]             # H beyond int32
    shapes[2] = [0, -3]                  # empty / negative
    starts[3] = i64.max - 2              # s0 + y*W + x would overflow
    want = md.forward(value, loc, attn, shapes, starts)
    keep = md.forward(value, loc[:, :, :, :1], attn[:, :, :, :1], shapes[:1], starts[:1])
    np.testing.assert_array_equal(want, keep)  # only level 0 counts
    out = _run(value, loc, attn, shapes, starts)
    bt = np.uint32 if dtype == np.float32 else np.uint64
    np.testing.assert_array_equal(_bits(out, dtype), want.view(bt))
    go = np.ones(out.shape, dtype)
    gv, gl, ga = _op().ms_deform_attn_backward(_t(go), _t(value), _t(loc), _t(attn), _t(shapes), _t(starts), 64)
    assert bool((gl[:, :, :, 1:] == 0).all() and (ga[:, :, :, 1:] == 0).all() and torch.isfinite(gv).all())


def _golden():
    g = np.load(os.path.join(HERE, "golden", "python_ms_deform_attn.npz"))
    return {k: {n: g[f"{k}_{n}"] for n in ("value", "sampling_locations", "attention_weights", "spatial_shapes",
                                           "level_start_index", "im2col_step", "out")}
            for k in ("tsa", "sca", "decoder")}


@pytest.mark.parametrize("case", ["tsa", "sca", "decoder"])
def test_reference_callers_golden_through_the_op(case):
    c = _golden()[case]
    out = _op().ms_deform_attn(_t(c["value"]), _t(c["sampling_locations"]), _t(c["attention_weights"]),
                               _t(c["spatial_shapes"]), _t(c["level_start_index"]), int(c["im2col_step"]))
    B, Q = c["sampling_locations"].shape[:2]
    want = c["out"].reshape(B, Q, -1)
    err = float(np.abs(out.cpu().numpy() - want).max())
    print(f"{case}: max |op - reference caller's golden| = {err:.2e}")
    assert err <= 1e-5


@pytest.mark.parametrize("site", ["sca", "small4"])
def test_backward_against_fp64_restatement(site):
    if site == "sca":
        c = dict(B=6, Q=600, M=8, C=32, shapes=[[15, 25]], P=8)
    else:
        c = dict(B=2, Q=300, M=8, C=32, shapes=[[20, 36], [10, 18], [5, 9], [3, 5]], P=4)
    value, loc, attn, shapes, starts = _case(21, c["B"], c["Q"], c["M"], c["C"], c["shapes"], c["P"], np.float32)
    loc = _away_from_grid(loc, shapes, 1e-3).astype(np.float32)
    go = np.random.default_rng(22).standard_normal((c["B"], c["Q"], c["M"] * c["C"])).astype(np.float32)
    gv, gl, ga = _op().ms_deform_attn_backward(_t(go), _t(value), _t(loc), _t(attn), _t(shapes), _t(starts), 64)
    rv, rl, ra = md.backward(go.astype(np.float64), value.astype(np.float64), loc.astype(np.float64),
                             attn.astype(np.float64), shapes, starts)
    ev = np.abs(gv.cpu().numpy() - rv).max() / np.abs(rv).max()
    el = np.abs(gl.cpu().numpy() - rl).max() / np.abs(rl).max()
    ea = np.abs(ga.cpu().numpy() - ra).max() / np.abs(ra).max()
    print(f"{site}: grad_value {ev:.2e}, grad_sampling_locations {el:.2e}, grad_attention_weights {ea:.2e} "
          f"(max abs error / max |ref|)")
    assert ev <= 1e-5 and el <= 1e-4 and ea <= 1e-4
    gv2, gl2, ga2 = _op().ms_deform_attn_backward(_t(go), _t(value), _t(loc), _t(attn), _t(shapes), _t(starts), 64)
    assert np.array_equal(_bits(gl, np.float32), _bits(gl2, np.float32))
    assert np.array_equal(_bits(ga, np.float32), _bits(ga2, np.float32))
    assert float((gv - gv2).abs().max()) <= 1e-6 * float(gv.abs().max())


def test_backward_fp64_matches_restatement():
    value, loc, attn, shapes, starts = _case(31, 2, 80, 3, 5, [[6, 8], [3, 4]], 3, np.float64)
    go = np.random.default_rng(32).standard_normal((2, 80, 15))
    gv, gl, ga = _op().ms_deform_attn_backward(_t(go), _t(value), _t(loc), _t(attn), _t(shapes), _t(starts), 64)
    rv, rl, ra = md.backward(go, value, loc, attn, shapes, starts)
    np.testing.assert_allclose(gv.cpu().numpy(), rv, rtol=0, atol=1e-12)
    np.testing.assert_allclose(gl.cpu().numpy(), rl, rtol=0, atol=1e-11)
    np.testing.assert_allclose(ga.cpu().numpy(), ra, rtol=0, atol=1e-12)


def _away_from_grid(loc, sh, margin):
    """Moves every h / w at least `margin` of a cell away from integer coordinates (cell edges, -1 and H: the op is
    only piecewise smooth there, and fp32 and fp64 may round to different sides)."""
    loc = loc.astype(np.float64)
    for l in range(sh.shape[0]):
        for k, n in ((0, sh[l, 1]), (1, sh[l, 0])):
            x = loc[:, :, :, l, :, k] * n - 0.5
            f = np.clip(x - np.floor(x), margin, 1 - margin)
            loc[:, :, :, l, :, k] = (np.floor(x) + f + 0.5) / n
    return loc


def _off_grid_case(seed, B, Q, M, C, shapes, P):
    """fp64 locations inside the map, 0.1 of a cell away from integer coordinates."""
    value, loc, attn, sh, st = _case(seed, B, Q, M, C, shapes, P, np.float64, 0.05, 0.95)
    return value, _away_from_grid(loc, sh, 0.1), attn, sh, st


def test_gradcheck_fp64():
    value, loc, attn, sh, st = _off_grid_case(41, 1, 3, 2, 3, [[4, 5], [2, 3]], 2)
    op = _op().ms_deform_attn
    ins = [_t(value).requires_grad_(), _t(loc).requires_grad_(), _t(attn).requires_grad_()]
    shd, std = _t(sh), _t(st)
    assert torch.autograd.gradcheck(lambda v, l, a: op(v, l, a, shd, std, 64), ins, eps=1e-6, atol=1e-7)


def test_autograd_wrapper_equals_backward_op():
    value, loc, attn, sh, st = _case(51, 2, 400, 8, 32, [[15, 25], [8, 13]], 4, np.float32)
    v, l, a = (_t(x).requires_grad_() for x in (value, loc, attn))
    out = _op().ms_deform_attn(v, l, a, _t(sh), _t(st), 64)
    go = torch.randn_like(out)
    out.backward(go)
    gv, gl, ga = _op().ms_deform_attn_backward(go, v.detach(), l.detach(), a.detach(), _t(sh), _t(st), 64)
    assert torch.equal(l.grad, gl) and torch.equal(a.grad, ga)
    assert float((v.grad - gv).abs().max()) <= 1e-6 * float(gv.abs().max())
    # value and locations need grad, the weights do not: the backward returns None for them
    v2, l2, a2 = _t(value).requires_grad_(), _t(loc).requires_grad_(), _t(attn)
    seen = {}
    hook = _op().MSDeformAttnFunction.backward

    def spy(ctx, g):
        seen["grads"] = hook(ctx, g)
        return seen["grads"]

    _op().MSDeformAttnFunction.backward = staticmethod(spy)
    try:
        _op().ms_deform_attn(v2, l2, a2, _t(sh), _t(st), 64).backward(go)
    finally:
        _op().MSDeformAttnFunction.backward = staticmethod(hook)
    gv3, gl3, ga3 = seen["grads"][:3]
    assert ga3 is None and a2.grad is None
    assert torch.equal(gl3, gl) and torch.equal(l2.grad, gl) and v2.grad is not None


def test_im2col_step_does_not_change_bits_and_is_checked():
    value, loc, attn, sh, st = _case(61, 4, 500, 8, 32, [[15, 25]], 8, np.float32)
    outs = [_run(value, loc, attn, sh, st, step) for step in (1, 2, 64)]
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int32), outs[0].view(torch.int32))
    with pytest.raises(RuntimeError, match=r"batch\(4\) must divide im2col_step\(3\)"):
        _run(value, loc, attn, sh, st, 3)
    with pytest.raises(RuntimeError, match=r"must divide im2col_step"):
        _op().ms_deform_attn_backward(_t(np.zeros((4, 500, 256), np.float32)), _t(value), _t(loc), _t(attn), _t(sh),
                                      _t(st), 3)


def test_no_host_synchronisation():
    value, loc, attn, sh, st = _case(71, 2, 500, 8, 32, [[15, 25], [8, 13]], 4, np.float32)
    v, l, a = (_t(x).requires_grad_() for x in (value, loc, attn))
    shd, std = _t(sh), _t(st)
    go = torch.randn(2, 500, 256, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = _op().ms_deform_attn(v, l, a, shd, std, 64)
        out.backward(go)
        grads = _op().ms_deform_attn_backward(go, v.detach(), l.detach(), a.detach(), shd, std, 1)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.equal(l.grad, grads[1]) and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("B,Q", [(0, 10), (2, 0), (0, 0)])
def test_empty_batch_or_queries(B, Q):
    value, loc, attn, sh, st = _case(81, max(B, 1), max(Q, 1), 2, 8, [[3, 4]], 2, np.float32)
    value, loc, attn = value[:B], loc[:B, :Q], attn[:B, :Q]
    out = _run(value, loc, attn, sh, st)
    assert tuple(out.shape) == (B, Q, 16)
    gv, gl, ga = _op().ms_deform_attn_backward(_t(np.zeros((B, Q, 16), np.float32)), _t(value), _t(loc), _t(attn),
                                               _t(sh), _t(st), 64)
    assert tuple(gv.shape) == value.shape and tuple(gl.shape) == loc.shape and tuple(ga.shape) == attn.shape
    assert bool((gv == 0).all())


def test_refusals():
    value, loc, attn, sh, st = _case(91, 2, 10, 2, 8, [[3, 4]], 2, np.float32)
    op = _op().ms_deform_attn
    v, l, a, s, i = _t(value), _t(loc), _t(attn), _t(sh), _t(st)
    with pytest.raises(RuntimeError, match="Unsupported device type for ms_deform_attn operator"):
        op(v, l.cpu(), a, s, i, 64)
    with pytest.raises(RuntimeError, match="float32 or float64"):
        op(v.half(), l.half(), a.half(), s, i, 64)
    with pytest.raises(RuntimeError, match="sampling_locations must have value's dtype"):
        op(v, l.double(), a, s, i, 64)
    with pytest.raises(RuntimeError, match="attention_weights must have value's dtype"):
        op(v.double(), l.double(), a, s, i, 64)
    with pytest.raises(RuntimeError, match="spatial_shapes must be int64"):
        op(v, l, a, s.int(), i, 64)
    with pytest.raises(RuntimeError, match="level_start_index must be int64"):
        op(v, l, a, s, i.int(), 64)
    with pytest.raises(RuntimeError, match="ms_deform_attn"):
        op(v, l[:, :, :1], a, s, i, 64)  # heads disagree
