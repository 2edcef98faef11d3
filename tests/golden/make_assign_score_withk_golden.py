"""Golden vectors for assign_score_withk from the reference's own PAConv (models/classification/paconv/paconv.py:29-272)
and ScoreNet (score_net.py:20-85), executed through tests/golden/paddle_shim.py:

    python tests/golden/make_assign_score_withk_golden.py     # needs /root/reference; writes python_assign_score_withk.npz

The op is bound to an independent float64 einsum over gathered rows (assign_score_withk_numpy.forward_f64, whose
result the model receives in float32).  What the shim lacks (Tensor.topk, Conv1D, Dropout, the adaptive pools, one_hot,
log_softmax, create_parameter / add_parameter, the initialisers) is supplied here.  After the model is built, every
parameter and BN statistic is overwritten, in name order, by paddle_shim.fill_state(seed): the file stores the seed and
the key -> shape list, not the weights.

Recorded, at B = 1, N = 24 and the model's K = 20, M = 8 and widths 64 / 64 / 128 / 256:
    cloud, knn_idx, preds, the loss of get_loss for `labels`;
    call{i}_x       what feeds call i's feat_trans_dgcnn (the cloud [1, 3, N], then the BN / ReLU output of call i-1);
                    call i's points / centers are feat_trans_dgcnn(call{i}_x, matrice{i+1}), so the file keeps only
                    their first 4 channels (call{i}_points4, call{i}_centers4) to pin that rebuild;
    call{i}_scores, call{i}_out     what call i hands the op and gets back; layer4 = relu(bn4(call3_out));
    one backward per call: grad_out = default_rng(GRAD_SEED + i).standard_normal([1, O, N]) and the float64
                    gradients, grad_scores of the first 4 rows of n, grad_points / grad_centers of the first 4
                    channels (call{i}_gs4, call{i}_gp4, call{i}_gc4);
    tiny_*          a standalone call at B = 2, N = 5, K = 3, M = 2, O = 3 with repeated and out-of-range indices
                    (-1, N, 2^31 + 1), its float64 result and gradients for a seeded grad_out.
The cloud's 20th and 21st neighbour distances differ by at least MARGIN at every point (asserted), so a device kNN
cannot disagree with the recorded one through rounding.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import assign_score_withk_numpy as an  # noqa: E402
import paddle_shim as ps  # noqa: E402

REF = "/root/reference"
PACONV = os.path.join(REF, "paddle3d/models/classification/paconv/paconv.py")
SCORE_NET = os.path.join(REF, "paddle3d/models/classification/paconv/score_net.py")

N, K = 24, 20
WEIGHT_SEED = 31
GRAD_SEED = 400
MARGIN = 1e-2  # relative gap between the 20th and 21st squared neighbour distance


def _t(x):
    return x.as_subclass(torch.Tensor) if isinstance(x, torch.Tensor) else torch.as_tensor(x)


def cloud_with_margin():
    """The first seeded unit-sphere cloud of N points whose 20th / 21st neighbour distances are well apart."""
    for seed in range(1000):
        x = np.random.default_rng(seed).standard_normal((N, 3)).astype(np.float32)
        x /= np.float32(np.abs(x).max())
        d = ((x[:, None, :].astype(np.float64) - x[None]) ** 2).sum(-1)
        srt = np.sort(d, 1)
        if np.all(srt[:, K] - srt[:, K - 1] > MARGIN * srt[:, K]):
            return seed, x
    raise AssertionError("no cloud with the margin")


def weight_shapes(g):
    return json.loads(str(g["state_shapes"]))


def rebuild_state(g):
    """The Paddle state dict the maker wrote into the reference model (paddle_shim.fill_state order)."""
    rng = np.random.default_rng(int(g["weight_seed"]))
    shapes = weight_shapes(g)
    return {k: ps.synth_param(k, tuple(shapes[k]), rng) for k in sorted(shapes)}


def grad_out(i, O):
    return np.random.default_rng(GRAD_SEED + i).standard_normal((1, O, N)).astype(np.float32)


def tiny_inputs():
    rng = np.random.default_rng(5)
    B, n, k, m, o = 2, 5, 3, 2, 3
    scores = rng.standard_normal((B, n, k, m)).astype(np.float32)
    points = rng.standard_normal((B, n, m, o)).astype(np.float32)
    centers = rng.standard_normal((B, n, m, o)).astype(np.float32)
    idx = rng.integers(0, n, (B, n, k)).astype(np.int64)
    idx[0, 1] = (2, 2, 2)  # repeated within a row
    idx[0, 3, 1], idx[1, 0, 0], idx[1, 2, 2] = -1, n, 2 ** 31 + 1  # out of range
    go = rng.standard_normal((B, o, n)).astype(np.float32)
    return scores, points, centers, idx, go


def main():
    p = ps.install(REF)
    calls = []

    def op(scores, points, centers, knn_idx):
        args = [_t(a).numpy().copy() for a in (scores, points, centers, knn_idx)]
        r = an.forward_f64(*args).astype(np.float32)
        calls.append((args, r))
        return ps._wrap(torch.from_numpy(r))

    class Conv1D(p.nn.Layer):
        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias_attr=None, **_):
            super().__init__()
            self.weight = torch.nn.Parameter(torch.zeros((out_channels, in_channels, kernel_size)))
            self.bias = None if bias_attr is False else torch.nn.Parameter(torch.zeros(out_channels))

        def forward(self, x):
            return torch.nn.functional.conv1d(_t(x), self.weight, self.bias)

    class Dropout(p.nn.Layer):
        def __init__(self, p=0.5):
            super().__init__()

        def forward(self, x):
            return x  # eval mode

    p.nn.Conv1D, p.nn.Dropout = Conv1D, Dropout
    p.nn.Layer.add_parameter = lambda self, name, param: self.register_parameter(name, param)
    p.create_parameter = lambda shape, dtype="float32", default_initializer=None, **_: torch.nn.Parameter(
        torch.zeros(tuple(int(s) for s in shape)))
    ps.Tensor.topk = lambda self, k, axis=-1: tuple(ps._wrap(t) for t in torch.topk(self, k, dim=axis))
    F = p.nn.functional
    F.adaptive_max_pool1d = lambda x, s: ps._wrap(torch.nn.functional.adaptive_max_pool1d(_t(x), s))
    F.adaptive_avg_pool1d = lambda x, s: ps._wrap(torch.nn.functional.adaptive_avg_pool1d(_t(x), s))
    F.one_hot = lambda x, n: ps._wrap(torch.nn.functional.one_hot(_t(x).long(), n).float())
    F.log_softmax = lambda x, axis=-1: ps._wrap(torch.nn.functional.log_softmax(_t(x), dim=axis))
    noop = lambda *a, **k: None  # noqa: E731  (weights are seeded by ps.fill_state below)
    base = dict(paddle=p, nn=p.nn, F=F, os=os, manager=ps._Anything("manager"), constant_init=noop,
                kaiming_normal_init=noop, logger=ps._Anything("logger"),
                assign_score_withk=types.SimpleNamespace(assign_score_withk=op))
    sn = ps.exec_lines(SCORE_NET, [(20, 85)], dict(base))
    mod = ps.exec_lines(PACONV, [(29, 272)], dict(base, ScoreNet=sn["ScoreNet"]))

    seed, cloud = cloud_with_margin()
    out = {"cloud_seed": np.int64(seed), "cloud": cloud[None], "weight_seed": np.int64(WEIGHT_SEED),
           "labels": np.array([7], np.int64)}
    with torch.no_grad():
        model = mod["PAConv"](k_neighbors=K, calc_scores="softmax", num_matrices=(8, 8, 8, 8), dropout=0.5)
        model.eval()
        shapes = ps.fill_state(model, WEIGHT_SEED)
        out["state_shapes"] = np.asarray(json.dumps(shapes, sort_keys=True))
        preds = model({"data": ps.tensor(cloud[None])})["preds"]
        out["preds"] = _t(preds).numpy()
        out["loss"] = np.float32(_t(model.get_loss(preds, ps.tensor(out["labels"]))["loss"]).item())
        x = ps.tensor(cloud[None]).transpose([0, 2, 1])
        idx, _ = model.knn(x, K)
        out["knn_idx"] = _t(idx).numpy()
        state = model.state_dict()
        feeds = [cloud[None].transpose(0, 2, 1)]
        for i in range(4):
            h = torch.from_numpy(calls[i][1])
            bn = getattr(model, f"bn{i + 1}")
            feeds.append(_t(torch.relu(bn(ps._wrap(h)))).numpy())
        out["layer4"] = feeds[4]
        assert len(calls) == 4
        for i, (args, res) in enumerate(calls):
            scores, points, centers, knn = args
            assert np.array_equal(knn, out["knn_idx"])
            w = state[f"matrice{i + 1}"].numpy()
            xt = feeds[i].transpose(0, 2, 1)
            # feat_trans_dgcnn rebuilt from the stored feed and weight reproduces what the call received
            pts = (np.concatenate([xt, xt], -1) @ w).reshape(points.shape)
            assert np.allclose(pts, points, rtol=1e-5, atol=1e-5) and np.allclose(
                (xt @ w[:xt.shape[-1]]).reshape(centers.shape), centers, rtol=1e-5, atol=1e-5)
            O = points.shape[-1]
            out[f"call{i}_x"] = feeds[i]
            out[f"call{i}_points4"], out[f"call{i}_centers4"] = points[..., :4], centers[..., :4]
            out[f"call{i}_scores"], out[f"call{i}_out"] = scores, res
            gs, gp, gc = an.backward_f64(grad_out(i, O), scores, points, centers, knn)
            out[f"call{i}_gs4"], out[f"call{i}_gp4"], out[f"call{i}_gc4"] = gs[:, :4], gp[..., :4], gc[..., :4]
            # the float32 restatement agrees with the float64 formulation
            err = np.abs(an.forward(scores, points, centers, knn).astype(np.float64) - an.forward_f64(*args))
            assert np.all(err <= 1e-5 * an.forward_magnitude(*args)), err.max()

    s, pt, c, idx, go = tiny_inputs()
    out.update(tiny_scores=s, tiny_points=pt, tiny_centers=c, tiny_idx=idx, tiny_grad_out=go,
               tiny_out=an.forward_f64(s, pt, c, idx))
    out["tiny_gs"], out["tiny_gp"], out["tiny_gc"] = an.backward_f64(go, s, pt, c, idx)
    path = os.path.join(HERE, "python_assign_score_withk.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


def load(path=os.path.join(HERE, "python_assign_score_withk.npz")):
    z = np.load(path)
    return {k: z[k] for k in z.files}


if __name__ == "__main__":
    main()
