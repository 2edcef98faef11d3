"""assign_score_withk on the device (csrc/assign_score_withk.hip) against the NumPy restatement
(tests/golden/assign_score_withk_numpy.py): forward and the three gradients bit for bit at PAConv's per-frame shapes
and at edge shapes, tolerance against a torch float64 composition at B = 32, reproducibility, the autograd wrapper,
refusals, host synchronisation, and the PAConv mirror against the reference's recorded preds and a torch-composition
twin in one training step."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import assign_score_withk_numpy as an  # noqa: E402
import make_assign_score_withk_golden as mk  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
DEV = "cuda"


def _op():
    from paddle3d_amd.ops import assign_score_withk

    return assign_score_withk


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    """Bit patterns, every NaN as one (the host's default NaN is negative, the device's positive)."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    b = np.ascontiguousarray(a, F32).view(np.uint32).copy()
    b[np.isnan(np.asarray(a, F32))] = 0x7FC00000
    return b


def _inputs(seed, B, N, K, M, O, knn=True):
    rng = np.random.default_rng(seed)
    s = (rng.random((B, N, K, M), dtype=F32) + F32(0.5)).astype(F32)
    p = rng.standard_normal((B, N, M, O)).astype(F32)
    c = rng.standard_normal((B, N, M, O)).astype(F32)
    if knn and N >= K:  # a real kNN of a random cloud: neighbour lists of uneven popularity
        x = rng.standard_normal((B, N, 3)).astype(F32)
        d = ((x[:, :, None] - x[:, None]) ** 2).sum(-1)
        idx = np.argsort(d, -1, kind="stable")[..., :K].astype(np.int64)
    else:
        idx = rng.integers(0, max(N, 1), (B, N, K)).astype(np.int64)
    g = rng.standard_normal((B, O, N)).astype(F32)
    return s, p, c, idx, g


def _check_bits(s, p, c, idx, g):
    op = _op()
    args = [_d(a) for a in (s, p, c, idx)]
    out = op.assign_score_withk(*args)
    assert np.array_equal(_bits(out), _bits(an.forward(s, p, c, idx)))
    got = op.assign_score_withk_backward(_d(g), *args)
    for name, x, want in zip(("scores", "points", "centers"), got, an.backward(g, s, p, c, idx)):
        assert np.array_equal(_bits(x), _bits(want)), name


@pytest.mark.parametrize("O", [64, 128, 256])
def test_bit_equal_paconv_shapes(O):
    _check_bits(*_inputs(O, 4, 1024, 20, 8, O))


@pytest.mark.parametrize("shape", [(2, 50, 20, 8, 1), (2, 50, 20, 8, 3), (2, 33, 5, 3, 17), (3, 70, 9, 11, 100),
                                   (2, 1, 1, 8, 64), (2, 1, 3, 2, 5), (2, 9, 0, 4, 6), (1, 300, 300, 1, 65)])
def test_bit_equal_edge_shapes(shape):
    _check_bits(*_inputs(sum(shape), *shape, knn=False))


def test_bit_equal_bad_indices_and_nonfinite_scores():
    s, p, c, idx, g = _inputs(9, 3, 40, 20, 8, 70, knn=False)
    idx[0, 0] = 7  # a whole row of one neighbour
    idx[0, 1, :3] = -1
    idx[1, 2, 4:9] = 40
    idx[2, 3, 0], idx[2, 5, 19] = 2 ** 31 + 5, -(2 ** 40)
    s[1, 1, 1, 1], s[2, 2, 2, 2], s[0, 0, 3, 0] = np.inf, np.nan, -np.inf
    s[0, 1, 1, 0] = np.inf  # an infinite score on an out-of-range neighbour: 0 * inf
    _check_bits(s, p, c, idx, g)


def _torch_composition(s, p, c, idx, sign=-1):
    """Gather into [B, N, K, M, O] and contract (autograd-able); sign=+1 with absolute inputs gives the terms'
    magnitude sum."""
    B, N, M, O = p.shape
    ok = (idx >= 0) & (idx < N)
    rows = p[torch.arange(B, device=p.device)[:, None, None], idx.clamp(0, max(N - 1, 0))]
    rows = rows * ok[..., None, None]
    return torch.einsum("bnkmo,bnkm->bon", rows + sign * c[:, :, None], s)


def test_b32_within_tolerance_of_torch_f64():
    s, p, c, idx, g = _inputs(32, 32, 1024, 20, 8, 64)
    args = [_d(a) for a in (s, p, c, idx)]
    out = _op().assign_score_withk(*args)
    a64 = [t.double().requires_grad_() for t in args[:3]]
    want = _torch_composition(*a64, args[3])
    mag = _torch_composition(*(t.detach().abs() for t in a64), args[3], sign=1)
    assert bool(((out.double() - want).abs() <= 1e-5 * mag + 1e-6).all())
    gs, gp, gc = _op().assign_score_withk_backward(_d(g), *args)
    want = torch.autograd.grad(want, a64, _d(g).double())
    for got, w in zip((gs, gp, gc), want):
        assert torch.allclose(got.double(), w, rtol=1e-4, atol=1e-4)


def test_backward_reproducible():
    s, p, c, idx, g = _inputs(5, 4, 1024, 20, 8, 128)
    args = [_d(a) for a in (g, s, p, c, idx)]
    op = _op()
    first = op.assign_score_withk_backward(*args)
    second = op.assign_score_withk_backward(*args)
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_autograd_matches_explicit_backward_and_skips():
    s, p, c, idx, g = _inputs(6, 2, 200, 20, 8, 64)
    op = _op()
    st, pt, ct = (_d(a).requires_grad_() for a in (s, p, c))
    out = op.assign_score_withk(st, pt, ct, _d(idx))
    out.backward(_d(g))
    want = op.assign_score_withk_backward(_d(g), st.detach(), pt.detach(), ct.detach(), _d(idx))
    for t, w in zip((st, pt, ct), want):
        assert torch.equal(t.grad, w)
    # only points needs a gradient: the others are neither computed nor returned
    pt2 = _d(p).requires_grad_()
    op.assign_score_withk(_d(s), pt2, _d(c), _d(idx)).backward(_d(g))
    assert torch.equal(pt2.grad, want[1])
    gs, gp, gc = op.assign_score_withk_backward(_d(g), _d(s), _d(p), _d(c), _d(idx), need=(False, True, False))
    assert gs is None and gc is None and torch.equal(gp, want[1])


def test_inputs_unchanged_and_noncontiguous():
    s, p, c, idx, g = _inputs(7, 2, 100, 20, 8, 64)
    args = [_d(a) for a in (s, p, c, idx)]
    before = [a.clone() for a in args]
    op = _op()
    out = op.assign_score_withk(*args)
    op.assign_score_withk_backward(_d(g), *args)
    for a, b in zip(args, before):
        assert torch.equal(a, b)
    pn = _d(np.ascontiguousarray(p.transpose(0, 1, 3, 2))).transpose(2, 3)  # non-contiguous view of p
    assert not pn.is_contiguous()
    assert torch.equal(op.assign_score_withk(args[0], pn, args[2], args[3]), out)


def test_empty_batch_and_empty_dims():
    op = _op()
    s, p, c, idx, g = _inputs(8, 0, 16, 4, 2, 8, knn=False)
    out = op.assign_score_withk(*(_d(a) for a in (s, p, c, idx)))
    assert out.shape == (0, 8, 16)
    gs, gp, gc = op.assign_score_withk_backward(_d(g), *(_d(a) for a in (s, p, c, idx)))
    assert gs.shape == s.shape and gp.shape == p.shape
    for K, M in ((0, 3), (3, 0)):
        s, p, c, idx, g = _inputs(9, 2, 6, K, M, 5, knn=False)
        out = op.assign_score_withk(*(_d(a) for a in (s, p, c, idx)))
        assert out.shape == (2, 5, 6) and not out.any()


def test_refusals():
    op = _op()
    s, p, c, idx, g = _inputs(10, 2, 16, 4, 2, 8, knn=False)
    args = [_d(a) for a in (s, p, c, idx)]
    with pytest.raises(RuntimeError, match="float32"):
        op.assign_score_withk(args[0].double(), *args[1:])
    with pytest.raises(RuntimeError, match="int64"):
        op.assign_score_withk(*args[:3], args[3].int())
    with pytest.raises(RuntimeError, match="centers"):
        op.assign_score_withk(args[0], args[1], args[2][:, :8], args[3])
    with pytest.raises(RuntimeError, match="knn_idx"):
        op.assign_score_withk(*args[:3], args[3][:, :, :3])
    with pytest.raises(RuntimeError, match="grad_out"):
        op.assign_score_withk_backward(_d(g)[:, :4], *args)
    with pytest.raises(RuntimeError, match="Unsupported device"):
        op.assign_score_withk(*(torch.from_numpy(a) for a in (s, p, c, idx)))
    with pytest.raises(RuntimeError):
        op.assign_score_withk(args[0], torch.from_numpy(p), *args[2:])


def test_no_host_sync():
    s, p, c, idx, g = _inputs(11, 2, 256, 20, 8, 64)
    args = [_d(a).requires_grad_() for a in (s, p, c)] + [_d(idx)]
    gd = _d(g)
    op = _op()
    op.assign_score_withk(*args).backward(gd)  # warm up: allocator, code objects
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = op.assign_score_withk(*args)
        out.backward(gd)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


def _mirror(g):
    from paddle3d_amd.checkpoint import load_paddle_state_dict
    from paddle3d_amd.paconv import PAConv

    torch.manual_seed(0)
    model = PAConv(k_neighbors=20, calc_scores="softmax", num_matrices=(8, 8, 8, 8), dropout=0.0)
    load_paddle_state_dict(model, mk.rebuild_state(g))
    return model.to(DEV)


def test_mirror_reproduces_golden_preds():
    g = mk.load()
    model = _mirror(g).eval()
    with torch.no_grad():
        preds = model({"data": _d(g["cloud"])})["preds"].cpu().numpy()
    assert np.allclose(preds, g["preds"], rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(g["preds"]).max())))


def test_train_step_matches_torch_composition():
    """One train-mode step (batch-statistics BN, dropout 0) of the mirror at its own initialisation: parameter
    gradients on the device op against the same model on the torch composition (per parameter, relative L2)."""
    from paddle3d_amd.paconv import PAConv

    torch.manual_seed(0)
    model = PAConv(k_neighbors=20, calc_scores="softmax", num_matrices=(8, 8, 8, 8), dropout=0.0).to(DEV).train()
    twin = copy.deepcopy(model)
    twin.assign_score_withk = lambda scores, points, centers, knn_idx: _torch_composition(scores, points, centers,
                                                                                          knn_idx)
    rng = np.random.default_rng(12)
    data = _d(rng.standard_normal((4, 256, 3)).astype(F32))
    labels = _d(rng.integers(0, 40, 4).astype(np.int64))
    for m in (model, twin):
        m.zero_grad()
        m({"data": data, "labels": labels})["loss"].backward()
    for (name, a), (_, b) in zip(model.named_parameters(), twin.named_parameters()):
        assert (a.grad is None) == (b.grad is None), name
        if b.grad is None:  # ScoreNet's last BN is built but unused with last_bn=False, as in the reference
            continue
        assert float((a.grad - b.grad).norm()) <= 1e-2 * float(b.grad.norm()) + 1e-9, name
