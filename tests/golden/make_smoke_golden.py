"""Golden vectors for SMOKE's head and post-processing from the reference's own Python, executed by line range through
tests/golden/paddle_shim.py (the technique of make_anchor3d_golden.py):

    SMOKEPredictor, get_channel_spec        models/detection/smoke/smoke_predictor.py:28-123
    PostProcessor, numel_t                  models/detection/smoke/processor.py:29-201
    SMOKECoder and its decoders             models/detection/smoke/smoke_coder.py:25-390
    sigmoid_hm, nms_hm, select_topk, _gather_feat, gather, select_point_of_interest
                                            models/layers/layer_libs.py:31-43, :46-138, :163-207
    group_norm                              models/layers/layer_norm.py:20-33

    python tests/golden/make_smoke_golden.py   # needs the reference checkout; writes python_smoke.npz

What the shim lacks is added here (paddle_shim.py stays as it is): nn.GroupNorm, Sequential.sublayers, F.normalize, F.max_pool2d by keyword, paddle.topk / shape / atan
/ nonzero, Tensor.gather_nd, a Tensor.clip that takes a 0-d tensor as a bound, and paddle.zeros / ones in the dtype of
the run (the reference fills float32 buffers created that way; in the float64 run they have to hold float64).  Every
case (smoke_numpy.CASES: both norm types, forward and export_forward, B = 1 and 3 with a different K / trans_mat per
frame, maps of 12 x 40 and 5 x 7, head widths 32, 48 and 256) runs twice from the same float32 inputs: in float32 and
in float64.  Stored per case: the float32 and float64 result, and for each of the 14 columns `*_ref_err` (the largest
difference between the two runs) and `*_bound` (4 x that, one float32 ulp of the largest magnitude as floor:
make_bevformer_golden.bound), both taken over the columns of one quantity (COLUMN_GROUPS: the two angles, the four
image coordinates of the 2D box, the three dimensions, the three location coordinates, the score).  One bound over the
whole row would let the image coordinates (hundreds of pixels) decide for the angles; one per single column is a
maximum over as few as six rows, which for a column the reference happens to round well falls below two ulps -- less
than two equally valid fp32 operation orders differ by.  Inputs are rebuilt from the seed and not stored.

So that none of the reference's open choices decides a comparison, main() asserts (check_case) and says "change the
seed" otherwise: the selected scores of a frame are distinct, and distinct from the first one left out; no score lies
within 1e-5 of det_threshold; every forward case has a frame with fewer than K rows above the threshold and one case
has a frame with none; roty is not within 1e-4 of the wrap; o1 of a selected row is not within 1e-6 of 0; the two runs
agree on classes, pixels, counts and row order.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import smoke_numpy as sn  # noqa: E402
from make_bevformer_golden import bound  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "python_smoke.npz")
SMOKE_DIR = os.path.join(REF, "paddle3d/models/detection/smoke")
LAYERS = os.path.join(REF, "paddle3d/models/layers")
TAGS = sn.TAGS
_RUN = dict(dtype=torch.float32)
# columns of one quantity share one bound: (class), the two angles, the 2D box, the dimensions, the location, the score
COLUMN_GROUPS = ([0], [1, 12], [2, 3, 4, 5], [6, 7, 8], [9, 10, 11], [13])


def load():
    return dict(np.load(OUT))


def _extend_shim(ps, p):
    W = ps._wrap
    T = torch.Tensor
    nn, F = p.nn, p.nn.functional

    class GroupNorm(nn.Layer):
        def __init__(self, num_groups, num_channels, epsilon=1e-5, weight_attr=None, bias_attr=None, data_format="NCHW"):
            super().__init__()
            self._g, self._eps = num_groups, epsilon
            self.weight = torch.nn.Parameter(torch.ones(num_channels))
            self.bias = torch.nn.Parameter(torch.zeros(num_channels))

        def forward(self, x):
            return torch.nn.functional.group_norm(x, self._g, self.weight, self.bias, self._eps)

    nn.GroupNorm = GroupNorm
    nn.Sequential.sublayers = lambda self, include_self=False: list(self.modules())[0 if include_self else 1:]
    F.normalize = lambda x, p=2, axis=1, epsilon=1e-12: W(torch.nn.functional.normalize(x, p=p, dim=axis, eps=epsilon))

    F.max_pool2d = lambda x, kernel_size, stride=None, padding=0: W(torch.nn.functional.max_pool2d(
        x, kernel_size, stride, padding))

    def topk(x, k, axis=-1, largest=True, sorted=True):
        v, i = torch.topk(x.as_subclass(T), int(k), dim=axis, largest=largest, sorted=sorted)
        return W(v), W(i)

    p.topk = topk
    p.shape = lambda x: [int(s) for s in x.shape]
    p.atan = lambda x: W(torch.atan(x))
    p.nonzero = lambda x: W(torch.nonzero(x.as_subclass(T)))
    p.zeros = lambda shape, dtype=None: W(torch.zeros(tuple(int(s) for s in shape), dtype=ps._dt(dtype) or _RUN["dtype"]))
    p.ones = lambda shape, dtype=None: W(torch.ones(tuple(int(s) for s in shape), dtype=ps._dt(dtype) or _RUN["dtype"]))
    ps.Tensor.gather_nd = lambda self, index: W(self.as_subclass(T)[tuple(index.long().as_subclass(T).unbind(-1))])

    def clip(self, min=None, max=None):
        lo, hi = (float(v) if isinstance(v, torch.Tensor) else v for v in (min, max))
        return W(torch.clamp(self.as_subclass(T), min=lo, max=hi))

    ps.Tensor.clip = clip


def _namespace():
    import paddle_shim as ps

    p = ps.install(REF)
    _extend_shim(ps, p)
    import paddle.nn as nn
    import paddle.nn.functional as F

    noop = types.SimpleNamespace(constant_init=lambda *a, **k: None)
    ns = dict(paddle=p, nn=nn, F=F, np=np, param_init=noop)
    ps.exec_lines(os.path.join(LAYERS, "layer_norm.py"), [(20, 33)], ns)
    ps.exec_lines(os.path.join(LAYERS, "layer_libs.py"), [(31, 43), (46, 138), (163, 207)], ns)
    ps.exec_lines(os.path.join(SMOKE_DIR, "smoke_coder.py"), [(25, 390)], ns)
    ps.exec_lines(os.path.join(SMOKE_DIR, "smoke_predictor.py"), [(28, 123)], ns)
    ps.exec_lines(os.path.join(SMOKE_DIR, "processor.py"), [(29, 201)], ns)
    return ps, ns


def _reference(ps, ns, tag, dtype):
    """(heat, regression, result) of one run; the result is [n, 15] (forward) or [B * K, 14] (export)."""
    c, cam = sn.CASES[tag], sn.golden_camera(tag)
    _RUN["dtype"] = dtype
    head = ns["SMOKEPredictor"](num_classes=c["nc"], reg_channels=(1, 2, 3, 2, 2), num_channels=c["C"],
                                norm_type=c["norm"], in_channels=c["Cin"])
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sn.golden_state(tag).items()}, strict=True)
    head = head.to(dtype).eval()
    post = ns["PostProcessor"](depth_ref=[28.01, 16.32], dim_ref=sn.DIM_REF[:c["nc"]], reg_head=10,
                               det_threshold=c["thr"], max_detection=c["K"], pred_2d=True)
    T = lambda a: ps._wrap(torch.from_numpy(np.ascontiguousarray(a)).to(dtype))  # noqa: E731
    with torch.no_grad():
        heat, reg = head(T(sn.golden_inputs(tag)))
        if c["mode"] == "forward":
            res = post([heat.clone(), reg.clone()], dict(K=T(cam["K"]), trans_mat=T(cam["trans_mat"]),
                                                         image_size=T(cam["image_size"])))
        else:
            res = post.export_forward([heat.clone(), reg.clone()], [T(cam["K"]), T(cam["down_ratios"])])
    return heat.numpy(), reg.numpy(), res.numpy().reshape(-1, 15 if c["mode"] == "forward" else 14)


def frames_of(tag, res):
    """The result's rows per frame (forward: by the batch-id column; export: K rows each)."""
    c = sn.CASES[tag]
    if c["mode"] == "forward":
        return [res[res[:, 14] == b][:, :14] if res.size else np.zeros((0, 14), res.dtype) for b in range(c["B"])]
    return list(res.reshape(c["B"], c["K"], 14))


def check_case(tag, heat32, reg32, res32, heat64, res64):
    """The maker's conditions (see the module docstring); returns what it saw."""
    c = sn.CASES[tag]
    K, thr, HW = c["K"], np.float32(c["thr"]), c["H"] * c["W"]
    seen = dict(counts=[], min_gap=np.inf)
    f32, f64 = frames_of(tag, res32), frames_of(tag, res64)
    for b in range(c["B"]):
        s = np.sort(sn.peak_scores(heat32[b]).reshape(-1))[::-1][:K + 1].astype(np.float64)
        assert (np.diff(s) < 0).all(), f"{tag}: equal scores among the top K + 1 of frame {b}: change the seed"
        seen["min_gap"] = min(seen["min_gap"], float(-np.diff(s).max()))
        assert np.abs(s - thr).min() > 1e-5, f"{tag}: a score at det_threshold: change the seed"
        idx, sc = sn.select(heat32[b], K)
        idx64, _ = sn.select(heat64[b].astype(np.float32), K)
        assert np.array_equal(idx, idx64), f"{tag}: the two runs select different pixels: change the seed"
        n = int((sc > thr).sum()) if c["mode"] == "forward" else K
        seen["counts"].append(n)
        r32, r64 = f32[b], f64[b]
        assert len(r32) == len(r64) == n, f"{tag}: frame {b} has {len(r32)} / {len(r64)} rows, the restatement {n}"
        assert np.array_equal(r32[:, 0], r64[:, 0]) and np.array_equal(r32[:, 0], (idx // HW)[:n]), f"{tag}: classes differ"
        assert np.array_equal(r32[:, 13], sc[:n]), f"{tag}: the reference's scores are not the heat map's in this order"
        assert (np.abs(np.abs(r32[:, 12].astype(np.float64)) - 3.14159) > 1e-4).all(), f"{tag}: roty at the wrap: change the seed"
        o1 = reg32[b].reshape(10, -1)[7, (idx % HW)[:n]]
        assert (np.abs(o1) > 1e-6).all(), f"{tag}: o1 at 0: change the seed"
    if c["mode"] == "forward":
        assert min(seen["counts"]) < K, f"{tag}: every frame fills its K rows: change the seed or the threshold"
        assert max(seen["counts"]) > 0, f"{tag}: nothing passes: change the seed or the threshold"
    return seen


def main():
    ps, ns = _namespace()
    out, empty_frames = {}, 0
    for tag in TAGS:
        heat32, reg32, res32 = _reference(ps, ns, tag, torch.float32)
        heat64, _, res64 = _reference(ps, ns, tag, torch.float64)
        assert res32.dtype == np.float32 and res64.dtype == np.float64, (res32.dtype, res64.dtype)
        seen = check_case(tag, heat32, reg32, res32, heat64, res64)
        if sn.CASES[tag]["mode"] == "forward":
            empty_frames += sum(n == 0 for n in seen["counts"])
        assert res32.shape == res64.shape and np.array_equal(res32[:, 0], res64[:, 0])
        out[f"{tag}_rows"], out[f"{tag}_rows64"] = res32, res64
        bd, err = np.zeros(14), np.zeros(14)
        for cols in COLUMN_GROUPS:
            bd[cols], err[cols] = bound(res32[:, cols], res64[:, cols]) if len(res32) else (0.0, 0.0)
        out[f"{tag}_bound"], out[f"{tag}_ref_err"] = bd, err
        print(tag, seen, "ref_err", np.array2string(out[f"{tag}_ref_err"], precision=2))
    assert empty_frames >= 1, "no forward case has a frame without a detection: change the seed"
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
