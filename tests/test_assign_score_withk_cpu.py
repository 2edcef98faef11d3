"""The NumPy restatement of assign_score_withk (tests/golden/assign_score_withk_numpy.py) against a literal
transcription of the reference's CPU kernels, the float64 formulation, the CUDA kernel's p*s - c*s form and the
reference's recorded PAConv calls (tests/golden/python_assign_score_withk.npz); paddle3d_amd.paconv.PAConv on the CPU
with the op replaced by the restatement; the backward workspace query without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import assign_score_withk_numpy as an  # noqa: E402
import make_assign_score_withk_golden as mk  # noqa: E402

F32 = np.float32


@pytest.fixture(scope="module")
def golden():
    return mk.load()


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- literal transcription of assign_score_withk_cuda.cc:32-123, one element at a time ----------------------------
def ref_forward(scores, points, centers, knn):
    B, N, M, O = points.shape
    K = scores.shape[2]
    out = np.zeros((B, O, N), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            for n in range(N):
                for o in range(O):
                    for k in range(K):
                        for m in range(M):
                            kn = int(knn[b, n, k])
                            p = points[b, kn, m, o] if 0 <= kn < N else F32(0)  # departure: no OOB read
                            s = scores[b, n, k, m]
                            out[b, o, n] = F32(out[b, o, n] + F32(p * s))
                            out[b, o, n] = F32(out[b, o, n] - F32(centers[b, n, m, o] * s))
    return out


def ref_backward(grad_out, scores, points, centers, knn):
    B, N, M, O = points.shape
    K = scores.shape[2]
    gs, gp, gc = np.zeros_like(scores), np.zeros_like(points), np.zeros_like(centers)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):  # backward_points_cpu_kernel: one writer per (b, m, o), (n, k) ascending
            for m in range(M):
                for o in range(O):
                    for n in range(N):
                        for k in range(K):
                            kn = int(knn[b, n, k])
                            t = F32(scores[b, n, k, m] * grad_out[b, o, n])
                            if 0 <= kn < N:
                                gp[b, kn, m, o] = F32(gp[b, kn, m, o] + t)
                            gc[b, n, m, o] = F32(gc[b, n, m, o] - t)
        for b in range(B):  # backward_scores_cpu_kernel
            for n in range(N):
                for k in range(K):
                    for m in range(M):
                        kn = int(knn[b, n, k])
                        for o in range(O):
                            p = points[b, kn, m, o] if 0 <= kn < N else F32(0)
                            d = F32(p - centers[b, n, m, o])
                            gs[b, n, k, m] = F32(gs[b, n, k, m] + F32(d * grad_out[b, o, n]))
    return gs, gp, gc


def _case(seed, B, N, K, M, O, oob=True, nonfinite=False):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((B, N, K, M)).astype(F32)
    p = rng.standard_normal((B, N, M, O)).astype(F32)
    c = rng.standard_normal((B, N, M, O)).astype(F32)
    idx = rng.integers(0, N, (B, N, K)).astype(np.int64)
    if K > 1:
        idx[0, 0, :2] = idx[0, 0, 0]  # repeated within a row
    if oob and K:
        idx[0, -1, -1], idx[-1, 0, 0] = -1, N
        if B * N * K > 2:
            idx.reshape(-1)[1] = 2 ** 31 + 3
    if nonfinite and K and M:
        s[0, 0, 0, 0], s[-1, -1, -1, -1] = np.inf, np.nan
    g = rng.standard_normal((B, O, N)).astype(F32)
    return s, p, c, idx, g


CASES = [(1, 2, 5, 3, 2, 3, True, False), (2, 1, 6, 1, 3, 5, True, False), (3, 2, 4, 3, 1, 7, True, True),
         (4, 1, 7, 4, 3, 65, False, False), (5, 2, 3, 2, 2, 2, True, True), (6, 1, 1, 2, 2, 3, False, False)]


@pytest.mark.parametrize("case", CASES)
def test_restatement_bit_equals_reference_loops(case):
    s, p, c, idx, g = _case(*case)
    assert np.array_equal(_bits(an.forward(s, p, c, idx)), _bits(ref_forward(s, p, c, idx)))
    for got, want in zip(an.backward(g, s, p, c, idx), ref_backward(g, s, p, c, idx)):
        assert np.array_equal(_bits(got), _bits(want))


def test_empty_dims():
    for K, M in ((0, 3), (3, 0)):
        s, p, c, idx, g = _case(7, 2, 4, K, M, 5, oob=False)
        assert np.array_equal(_bits(an.forward(s, p, c, idx)), _bits(np.zeros((2, 5, 4), F32)))
        gs, gp, gc = an.backward(g, s, p, c, idx)
        assert gs.shape == s.shape and not gp.any() and not gc.any()


def _cuda_form(scores, points, centers, knn):
    """The CUDA kernel's term: p*s - c*s formed first, then added (in fp64 here, its order otherwise)."""
    s, p, c = (np.asarray(a, np.float64) for a in (scores, points, centers))
    kn, ok = an._valid(knn, p.shape[1])
    P = np.where(ok[..., None, None], p[np.arange(p.shape[0])[:, None, None], kn], 0.0)
    return np.einsum("bnkmo,bnkm->bon", P, s) - np.einsum("bnmo,bnkm->bon", c, s)


def test_restatement_within_tolerance_of_f64_and_cuda_form():
    s, p, c, idx, g = _case(8, 2, 40, 20, 8, 70)
    got = an.forward(s, p, c, idx).astype(np.float64)
    mag = an.forward_magnitude(s, p, c, idx)
    for want in (an.forward_f64(s, p, c, idx), _cuda_form(s, p, c, idx)):
        assert np.all(np.abs(got - want) <= 1e-5 * mag)
    gs, gp, gc = an.backward(g, s, p, c, idx)
    ws, wp, wc = an.backward_f64(g, s, p, c, idx)
    for got, want in ((gs, ws), (gp, wp), (gc, wc)):
        assert np.allclose(got, want, rtol=1e-4, atol=1e-4)


def _call_args(g, i):
    """What PAConv's call i handed the op: points / centers rebuilt with feat_trans_dgcnn from the recorded feed."""
    state = mk.rebuild_state(g)
    w = state[f"matrice{i + 1}"]
    xt = g[f"call{i}_x"].transpose(0, 2, 1)
    s = g[f"call{i}_scores"]
    B, N, K, M = s.shape
    pts = (np.concatenate([xt, xt], -1) @ w).reshape(B, N, M, -1).astype(F32)
    ctr = (xt @ w[:xt.shape[-1]]).reshape(B, N, M, -1).astype(F32)
    return s, pts, ctr, g["knn_idx"]


@pytest.mark.parametrize("i", range(4))
def test_restatement_reproduces_golden_calls(golden, i):
    s, p, c, idx = _call_args(golden, i)
    assert np.allclose(p[..., :4], golden[f"call{i}_points4"], rtol=1e-5, atol=1e-5)
    assert np.allclose(c[..., :4], golden[f"call{i}_centers4"], rtol=1e-5, atol=1e-5)
    out = an.forward(s, p, c, idx)
    mag = an.forward_magnitude(s, p, c, idx)
    assert np.all(np.abs(out.astype(np.float64) - golden[f"call{i}_out"]) <= 1e-5 * mag + 1e-6)
    gs, gp, gc = an.backward(mk.grad_out(i, p.shape[-1]), s, p, c, idx)
    assert np.allclose(gs[:, :4], golden[f"call{i}_gs4"], rtol=1e-4, atol=1e-4)
    assert np.allclose(gp[..., :4], golden[f"call{i}_gp4"], rtol=1e-4, atol=1e-4)
    assert np.allclose(gc[..., :4], golden[f"call{i}_gc4"], rtol=1e-4, atol=1e-4)


def test_restatement_reproduces_golden_tiny_call(golden):
    args = [golden[f"tiny_{k}"] for k in ("scores", "points", "centers", "idx")]
    assert (args[3] < 0).any() and (args[3] >= args[3].shape[1]).any() and (args[3] >= 2 ** 31).any()
    assert np.allclose(an.forward(*args), golden["tiny_out"], rtol=1e-5, atol=1e-6)
    for got, want in zip(an.backward(golden["tiny_grad_out"], *args), (golden["tiny_gs"], golden["tiny_gp"],
                                                                        golden["tiny_gc"])):
        assert np.allclose(got, want, rtol=1e-5, atol=1e-6)


def restatement_op(scores, points, centers, knn_idx):
    """The restatement as a torch op on the CPU (forward only)."""
    out = an.forward(*(t.detach().cpu().numpy() for t in (scores, points, centers, knn_idx)))
    return torch.from_numpy(out)


def build_mirror(g):
    from paddle3d_amd.checkpoint import load_paddle_state_dict
    from paddle3d_amd.paconv import PAConv

    torch.manual_seed(0)
    model = PAConv(k_neighbors=20, calc_scores="softmax", num_matrices=(8, 8, 8, 8), dropout=0.5)
    load_paddle_state_dict(model, mk.rebuild_state(g))
    return model.eval()


def test_paconv_mirror_on_cpu_reproduces_golden(golden):
    model = build_mirror(golden)
    model.assign_score_withk = restatement_op
    outs = []

    def hook(i):
        return lambda mod, a, r: outs.append((i, r.detach().numpy()))

    for i in range(4):
        getattr(model, f"bn{i + 1}").register_forward_hook(hook(i))
    x = torch.from_numpy(golden["cloud"])
    with torch.no_grad():
        idx, _ = model.knn(x.transpose(1, 2), 20)
        assert np.array_equal(idx.numpy(), golden["knn_idx"])
        preds = model({"data": x})["preds"].numpy()
        loss = model.get_loss(torch.from_numpy(preds), torch.from_numpy(golden["labels"]))["loss"].item()
    assert np.allclose(preds, golden["preds"], rtol=1e-4, atol=1e-4)
    assert abs(loss - float(golden["loss"])) < 1e-4
    feeds = [golden[f"call{i}_x"] for i in range(1, 4)] + [golden["layer4"]]
    for i, bn_out in outs:  # activations grow to ~1e3 under the seeded weights: 1e-4 of the layer's scale
        scale = max(1.0, float(np.abs(feeds[i]).max()))
        assert np.abs(np.maximum(bn_out, 0) - feeds[i]).max() <= 1e-4 * scale, i


def test_backward_workspace_query_needs_no_gpu():
    from paddle3d_amd import _lib, build

    build.build()
    L = _lib.lib()
    ws = L.pd3_assign_score_withk_backward_workspace(32, 1024, 20, 256)
    assert ws >= 32 * 1024 * 256 * 4 + 4 * 32 * 1024 * 20 * 4
    assert L.pd3_assign_score_withk_backward_workspace(0, 0, 0, 0) >= 0
    assert L.pd3_assign_score_withk_backward_workspace(-1, 4, 4, 4) == 0
