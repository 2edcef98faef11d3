"""Golden vectors for DD3D's FCOS heads and post-processing from the reference's own Python, executed by line range
through tests/golden/paddle_shim.py (the technique of make_smoke_golden.py):

    FCOS2DHead, FCOS2DInference             models/heads/fcos_heads/fcos2d_head.py:30-186, :315-503
    allocentric_to_egocentric, predictions_to_boxes3d, FCOS3DHead, FCOS3DInference
                                            models/heads/fcos_heads/fcos3d_head.py:29-108, :112-296, :483-639
    Scale, Offset, LayerListDial            models/layers/normalization.py:19-67
    FrozenBatchNorm2d                       models/layers/layer_norm.py:36-92
    quaternion_to_matrix .. matrix_to_quaternion   utils/transform.py:167-246
    homogenize_points, unproject_points2d   models/losses/disentangled_box3d_loss.py:27-61
    DD3D's eval branch, compute_locations   models/detection/dd3d/dd3d.py:144-176, :183-212

    python tests/golden/make_dd3d_golden.py   # needs the reference checkout; writes python_dd3d.npz

What the shim lacks is added here (paddle_shim.py stays as it is): Tensor.shape as a list (the reference adds lists to
it), indexing with a one-element index tensor that drops the axis (the reference's `unsqueeze(0)` branches undo it), Tensor.clip / topk / tanh / rsqrt / nonzero / stop_gradient, paddle.create_parameter with initializer.Assign,
paddle.unbind / cross / bmm / allclose / kthvalue / take_along_axis / nonzero, nn.Pad1D, F.batch_norm,
paddle.regularizer.L2Decay, Sequential / LayerList.sublayers, a Conv2D that takes the `bias=True` FCOS2DHead's v1 towers pass
(Paddle's Conv2D has no such argument: v1 cannot be constructed there; here it means "with a bias"), paddle.zeros / ones
in the dtype of the run, and a logger whose warning raises (the renormalisation branch of allocentric_to_egocentric must
not be taken).  paddle.vision.ops.nms is WRITTEN HERE FROM ITS DOCUMENTED BEHAVIOUR (Paddle core's source is not in the
reference tree): with scores and categories, greedy NMS per category in descending score, IoU = inter / (a + b - inter)
without +1, a pair suppresses iff IoU > iou_threshold, the kept indices of all categories in descending score.  With
only_box2d the reference's nms_and_top_k fails on the keys scores_3d / pred_boxes3d it reads unconditionally; this file
adds them as zeros, which is what the device writes.  nms_and_top_k does not filter `fpn_levels` and `locations`, so
those three columns are not part of the stored rows.

Every case (dd3d_numpy.CASES) runs twice from the same float32 inputs: in float32 and in float64.  Stored per case: the
float32 and float64 rows [n, 18] (pred_boxes 4, scores, scores_3d, pred_classes, pred_boxes3d 10, image id), and per
column group `*_ref_err` (the largest difference between the two runs) and `*_bound` (4 x that, one float32 ulp of the
largest magnitude as floor: make_bevformer_golden.bound); groups: the 2D box, the two scores, the quaternion, proj_ctr,
depth, size.  Inputs are rebuilt from the seed and not stored.

check_case asserts what the module docstring of tests/test_dd3d_cpu.py relies on and says "change the seed" otherwise.
"""
import functools
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import dd3d_numpy as dn  # noqa: E402
from make_bevformer_golden import bound  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "python_dd3d.npz")
P3D = os.path.join(REF, "paddle3d")
TAGS = dn.TAGS
_RUN = dict(dtype=torch.float32)
# stored columns: pred_boxes 0:4, scores 4, scores_3d 5, pred_classes 6, pred_boxes3d 7:17 (quat 7:11, proj_ctr 11:13,
# depth 13, size 14:17), image id 17; GROUPS: the columns that share one bound
GROUPS = ([0, 1, 2, 3], [4, 5], [7, 8, 9, 10], [11, 12], [13], [14, 15, 16])
ROW_COLS = [0, 1, 2, 3, 4, 5, 6] + list(range(10, 20))  # the same columns in the kernels' 20-float row


def load():
    return dict(np.load(OUT))


def reference_nms(boxes, iou_threshold, scores=None, category_idxs=None, categories=None, top_k=None):
    """paddle.vision.ops.nms from its documented behaviour (see the module docstring)."""
    T = torch.Tensor
    b, s, c = boxes.as_subclass(T), scores.as_subclass(T), category_idxs.as_subclass(T)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    kept = []
    for cat in categories:
        idx = torch.nonzero(c == cat).reshape(-1)
        idx = idx[torch.argsort(s[idx], descending=True, stable=True)]
        alive = torch.ones(len(idx), dtype=torch.bool)
        for i in range(len(idx)):
            if not alive[i]:
                continue
            kept.append(int(idx[i]))
            a, rest = b[idx[i]], b[idx[i + 1:]]
            w = (torch.minimum(a[2], rest[:, 2]) - torch.maximum(a[0], rest[:, 0])).clamp(min=0)
            h = (torch.minimum(a[3], rest[:, 3]) - torch.maximum(a[1], rest[:, 1])).clamp(min=0)
            inter = w * h
            iou = inter / (area[idx[i]] + area[idx[i + 1:]] - inter)
            alive[i + 1:] &= ~(iou > iou_threshold)
    kept = torch.as_tensor(kept, dtype=torch.long)
    return kept[torch.argsort(s[kept], descending=True, stable=True)]


def _extend_shim(ps, p):
    W = ps._wrap
    T = torch.Tensor
    nn, F = p.nn, p.nn.functional

    class Shape(list):  # a list (the reference adds lists to it) that still compares equal to a torch.Size
        def __eq__(self, other):
            return list(self) == list(other)

        def __ne__(self, other):
            return not self == other

    ps.Tensor.shape = property(lambda self: Shape(T.shape.__get__(self)))
    ps.Tensor.stop_gradient = True

    def getitem(self, idx):  # Paddle's indexing of that time: a one-element index tensor drops the axis it indexes
        out = T.__getitem__(self, idx)
        if (isinstance(idx, torch.Tensor) and not idx.dtype.is_floating_point and idx.dtype != torch.bool and
                idx.dim() == 1 and idx.numel() == 1 and self.dim() > 1):
            out = out.squeeze(0)
        return out

    ps.Tensor.__getitem__ = getitem
    ps.Tensor.tanh = lambda self: W(torch.tanh(self.as_subclass(T)))
    ps.Tensor.rsqrt = lambda self: W(torch.rsqrt(self.as_subclass(T)))

    def clip(self, min=None, max=None):
        lo, hi = (float(v) if isinstance(v, torch.Tensor) else v for v in (min, max))
        return W(torch.clamp(self.as_subclass(T), min=lo, max=hi))

    ps.Tensor.clip = clip

    def topk(self, k, axis=-1, largest=True, sorted=True):
        v, i = torch.topk(self.as_subclass(T), int(k), dim=axis, largest=largest, sorted=sorted)
        return W(v), W(i)

    ps.Tensor.topk = topk
    ps.Tensor.nonzero = lambda self, as_tuple=False: W(torch.nonzero(self.as_subclass(T)))
    nn.Sequential.sublayers = lambda self, include_self=False: list(self.modules())[0 if include_self else 1:]
    nn.LayerList.sublayers = nn.Sequential.sublayers
    nn.initializer.Assign = lambda value: value
    p.create_parameter = lambda shape, dtype="float32", default_initializer=None: torch.nn.Parameter(
        default_initializer.as_subclass(T).clone().to(ps._dt(dtype)).reshape(tuple(shape)))
    p.unbind = lambda x, axis=0: [W(t) for t in torch.unbind(x, axis)]
    p.cross = lambda x, y, axis=None: W(torch.cross(x, y, dim=axis))
    p.bmm = lambda x, y: W(torch.bmm(x, y))
    p.allclose = lambda x, y, rtol=1e-5, atol=1e-8: torch.allclose(x.as_subclass(T), y.as_subclass(T), rtol=rtol, atol=atol)
    p.nonzero = lambda x, as_tuple=False: W(torch.nonzero(x.as_subclass(T)))
    p.take_along_axis = lambda arr, indices, axis: W(torch.take_along_dim(arr.as_subclass(T), indices.as_subclass(T).long(),
                                                                          dim=axis))

    def kthvalue(x, k, axis=-1, keepdim=False):
        v, i = torch.kthvalue(x.as_subclass(T), int(k), dim=axis, keepdim=keepdim)
        return W(v), W(i)

    p.kthvalue = kthvalue
    p.zeros = lambda shape, dtype=None: W(torch.zeros(tuple(int(s) for s in shape), dtype=ps._dt(dtype) or _RUN["dtype"]))
    p.ones = lambda shape, dtype=None: W(torch.ones(tuple(int(s) for s in shape), dtype=ps._dt(dtype) or _RUN["dtype"]))
    to_tensor = p.to_tensor

    def to_tensor_run(data, dtype=None, place=None, stop_gradient=True):  # float data in the dtype of the run
        t = to_tensor(data, dtype)
        return W(t.to(_RUN["dtype"])) if dtype is None and t.dtype == torch.float32 else t

    p.to_tensor = to_tensor_run
    p.vision = types.SimpleNamespace(ops=types.SimpleNamespace(nms=reference_nms))

    class Pad1D(nn.Layer):
        def __init__(self, padding, mode="constant", value=0.0, data_format="NCL"):
            super().__init__()
            self._p, self._m, self._v = list(padding), mode, value

        def forward(self, x):
            return torch.nn.functional.pad(x, self._p, mode=self._m, value=self._v)

    nn.Pad1D = Pad1D
    F.batch_norm = lambda x, mean, var, weight, bias, training=False, epsilon=1e-5: W(torch.nn.functional.batch_norm(
        x, mean, var, weight, bias, False, 0.0, epsilon))
    base = nn.Conv2D

    class Conv2D(base):
        def __init__(self, *a, bias=None, **k):  # `bias=True` (fcos2d_head.py:75): with a bias, which is the default
            assert bias in (None, True)
            super().__init__(*a, **k)

    nn.Conv2D = Conv2D
    reg = types.ModuleType("paddle.regularizer")
    reg.L2Decay = lambda *a, **k: None
    sys.modules["paddle.regularizer"] = reg
    p.regularizer = reg


class _Logger:
    @staticmethod
    def warning(msg):
        raise AssertionError("allocentric_to_egocentric renormalises (" + str(msg) + "): change the seed")


def _namespace():
    import paddle_shim as ps

    p = ps.install(REF)
    _extend_shim(ps, p)
    import paddle.nn as nn
    import paddle.nn.functional as F

    noop = types.SimpleNamespace(kaiming_normal_init=lambda *a, **k: None, kaiming_uniform_init=lambda *a, **k: None,
                                 constant_init=lambda *a, **k: None)
    ns = dict(paddle=p, nn=nn, F=F, np=np, param_init=noop, ParamAttr=p.ParamAttr, L2Decay=lambda *a, **k: None,
              logger=_Logger, manager=ps._Anything("manager"))
    ps.exec_lines(os.path.join(P3D, "models/layers/normalization.py"), [(19, 67)], ns)
    ps.exec_lines(os.path.join(P3D, "models/layers/layer_norm.py"), [(36, 92)], ns)
    ps.exec_lines(os.path.join(P3D, "utils/transform.py"), [(167, 246)], ns)
    ps.exec_lines(os.path.join(P3D, "models/losses/disentangled_box3d_loss.py"), [(27, 61)], ns)
    heads = os.path.join(P3D, "models/heads/fcos_heads")
    ps.exec_lines(os.path.join(heads, "fcos2d_head.py"), [(30, 186), (315, 503)], ns)
    ps.exec_lines(os.path.join(heads, "fcos3d_head.py"), [(29, 108), (112, 296), (483, 639)], ns)
    dd3d = os.path.join(P3D, "models/detection/dd3d/dd3d.py")
    ps.exec_lines(dd3d, [(183, 212)], ns)
    lines = open(dd3d).read().split("\n")
    import textwrap

    ns["_eval_branch"] = compile(textwrap.dedent("\n".join(lines[143:176])), dd3d + ":144-176", "exec")
    return ps, ns


def build_heads(ns, tag, dtype):
    c = dn.CASES[tag]
    s2, s3 = dn.golden_state(tag)
    L = len(c["shapes"])
    head2 = ns["FCOS2DHead"](in_strides=list(c["strides"]), in_channels=[c["C"]] * L, num_classes=c["nc"],
                            version=c["version"], num_cls_convs=dn.NUM_CONVS, num_box_convs=dn.NUM_CONVS, norm=c["norm"])
    head2.load_state_dict({k: torch.from_numpy(v) for k, v in s2.items()}, strict=True)
    head3 = None
    if s3 is not None:
        head3 = ns["FCOS3DHead"](in_strides=list(c["strides"]), in_channels=[c["C"]] * L, num_classes=c["nc"],
                                num_convs=dn.NUM_CONVS, norm=c["norm"], use_per_level_predictors=bool(c.get("per_level")),
                                per_level_predictors=bool(c.get("per_level")),
                                class_agnostic_box3d=bool(c.get("class_agnostic")))
        head3.load_state_dict({k: torch.from_numpy(v) for k, v in s3.items()}, strict=True)
        head3 = head3.to(dtype).eval()
    return head2.to(dtype).eval(), head3


def _reference(ps, ns, tag, dtype):
    """The reference's per-image instance dicts (after nms_and_top_k) and before it, as numpy."""
    c, cfg = dn.CASES[tag], dn.cfg_of(tag)
    _RUN["dtype"] = dtype
    head2, head3 = build_heads(ns, tag, dtype)
    inf2 = ns["FCOS2DInference"](thresh_with_ctr=cfg["thresh_with_ctr"], pre_nms_thresh=cfg["pre_nms_thresh"],
                                pre_nms_topk=cfg["pre_nms_topk"], post_nms_topk=cfg["post_nms_topk"],
                                nms_thresh=cfg["nms_thresh"], num_classes=c["nc"])
    inf3 = None
    if head3 is not None:
        inf3 = ns["FCOS3DInference"](canon_box_sizes=dn.CANON, min_depth=cfg["min_depth"], max_depth=cfg["max_depth"],
                                    predict_distance=cfg["predict_distance"], num_classes=c["nc"],
                                    class_agnostic=bool(c.get("class_agnostic")))
    me = types.SimpleNamespace(input_strides=list(c["strides"]), feature_locations_offset=c["offset"],
                               fcos2d_inference=inf2, fcos3d_inference=inf3, only_box2d=head3 is None, do_nms=False)
    me.compute_features_locations = functools.partial(ns["compute_features_locations"], me)
    T = lambda a: ps._wrap(torch.from_numpy(np.ascontiguousarray(a)).to(dtype))  # noqa: E731
    with torch.no_grad():
        features = [T(f) for f in dn.golden_inputs(tag)]
        scope = dict(ns)
        scope.update(self=me, locations=ns["compute_locations"](me, features))
        scope["logits"], scope["box2d_reg"], scope["centerness"], _ = head2(features)
        if head3 is not None:
            (scope["box3d_quat"], scope["box3d_ctr"], scope["box3d_depth"], scope["box3d_size"], scope["box3d_conf"],
             _) = head3(features)
            scope["inv_intrinsics"] = T(dn.golden_camera(tag)).inverse()
        exec(ns["_eval_branch"], scope)  # do_nms False: the concatenation only
        cat = scope["pred_instances_cat"]
        if head3 is None:  # (see the module docstring)
            for inst in cat:
                n = inst["scores"].shape[0]
                inst["scores_3d"], inst["pred_boxes3d"] = ps._wrap(torch.zeros(n, dtype=dtype)), ps._wrap(torch.zeros((n, 10), dtype=dtype))
        keys = ("pred_boxes", "scores", "scores_3d", "pred_classes", "pred_boxes3d")
        before = [{k: inst[k].numpy().copy() for k in keys + ("fpn_levels", "locations")} for inst in cat]
        after = inf2.nms_and_top_k([dict(inst) for inst in cat], scope["score_key"])
        after = [{k: inst[k].numpy().copy() for k in keys} for inst in after]
        names = ("logits", "centerness", "box2d_reg") + (() if head3 is None else tuple(
            "box3d_" + k for k in ("quat", "ctr", "depth", "size", "conf")))
        maps = {k: [t.numpy() for t in scope[k]] for k in names}
    return before, after, maps


def stored_rows(after, dtype):
    out = []
    for b, inst in enumerate(after):
        n = len(inst["scores"])
        out.append(np.concatenate([inst["pred_boxes"].reshape(n, 4), inst["scores"].reshape(n, 1),
                                   inst["scores_3d"].reshape(n, 1), inst["pred_classes"].reshape(n, 1).astype(dtype),
                                   inst["pred_boxes3d"].reshape(n, 10), np.full((n, 1), b, dtype)], 1).astype(dtype))
    return np.concatenate(out)


def check_case(tag, before32, after32, before64, after64, maps32):
    """The maker's conditions; returns what it saw."""
    c, cfg = dn.CASES[tag], dn.cfg_of(tag)
    thr, K, P, nthr = np.float32(cfg["pre_nms_thresh"]), cfg["pre_nms_topk"], cfg["post_nms_topk"], cfg["nms_thresh"]
    seen = dict(over_k=0, empty_levels=0, empty_images=0, suppressed=0, cross_class=0, cut_images=0, class5=0,
                clip_lo=0, clip_hi=0)
    for b in range(c["B"]):
        for l in range(len(c["shapes"])):
            s, cand = dn.scores_of(maps32["logits"][l][b], maps32["centerness"][l][b], cfg)
            sl = dn.sigmoid(maps32["logits"][l][b].reshape(c["nc"], -1).T).reshape(-1)
            tested = s if cfg["thresh_with_ctr"] else sl
            assert np.abs(tested.astype(np.float64) - thr).min() > 1e-5, f"{tag}: a score at pre_nms_thresh: change the seed"
            top = np.sort(s[cand])[::-1][:K + 1].astype(np.float64)
            assert (np.diff(top) < 0).all(), f"{tag}: equal scores among the selected of ({l}, {b}): change the seed"
            seen["over_k"] += cand.sum() > K
            seen["empty_levels"] += cand.sum() == 0
            if c["nc"] > 5:
                seen["class5"] += int((np.nonzero(cand)[0] % c["nc"] >= 5).sum())
        b32, b64, a32, a64 = before32[b], before64[b], after32[b], after64[b]
        assert np.array_equal(b32["pred_classes"], b64["pred_classes"]) and np.array_equal(b32["locations"], b64["locations"]), \
            f"{tag}: the two runs select different entries: change the seed"
        assert np.array_equal(a32["pred_classes"], a64["pred_classes"]) and len(a32["scores"]) == len(a64["scores"]), \
            f"{tag}: the two runs keep different rows: change the seed"
        seen["empty_images"] += len(a32["scores"]) == 0
        # NMS: every same-class pair's IoU away from the threshold; a suppressed pair; a surviving cross-class pair
        ok = b32["pred_classes"] < 5
        boxes, cls = b32["pred_boxes"][ok].astype(np.float32), b32["pred_classes"][ok]
        key = b32["scores" if c.get("only_box2d") else "scores_3d"][ok]
        if len(key):
            top = np.sort(key.astype(np.float64))[::-1]
            assert (np.diff(top) < 0).all(), f"{tag}: equal NMS scores in image {b}: change the seed"
        for i in range(len(boxes)):
            iou = dn.iou_xyxy(boxes[i], boxes).astype(np.float64)
            same = cls == cls[i]
            same[i] = False
            assert (np.abs(iou[same] - nthr) > 1e-5).all(), f"{tag}: an IoU at nms_thresh: change the seed"
            seen["suppressed"] += int((iou[same] > nthr).sum())
        kept_boxes, kept_cls = a32["pred_boxes"].astype(np.float32), a32["pred_classes"]
        for i in range(len(kept_boxes)):
            iou = dn.iou_xyxy(kept_boxes[i], kept_boxes)
            seen["cross_class"] += int(((iou > nthr) & (kept_cls != kept_cls[i])).sum())
        # the post-NMS cut: more survivors than post_nms_topk somewhere, no tie at the cut
        nms_only = reference_nms(torch.from_numpy(boxes), nthr, torch.from_numpy(key), torch.from_numpy(cls), range(5)) \
            if len(boxes) else []
        if len(nms_only) > P:
            seen["cut_images"] += 1
            s2 = np.sort(b32["scores"][ok][nms_only.numpy()].astype(np.float64))[::-1]
            assert s2[P - 1] > s2[P], f"{tag}: a tie at the post-NMS cut: change the seed"
            assert len(a32["scores"]) == P
        if not c.get("only_box2d") and len(b32["scores"]):
            d = b32["pred_boxes3d"][:, 6]
            seen["clip_lo"] += int((d == np.float32(cfg["min_depth"])).sum())
            seen["clip_hi"] += int((d == np.float32(cfg["max_depth"])).sum())
    return seen


def check_margins(tag, after32):
    """_sqrt_positive_part arguments and _copysign differences of the stored rows, from their egocentric quaternions:
    o0 .. z are 0.5 sqrt(t) with t = 4 q^2, and the differences are 4 o0 q_k."""
    q = np.concatenate([a["pred_boxes3d"][:, :4] for a in after32]).astype(np.float64)
    if not len(q):
        return np.inf, np.inf
    worst_sqrt, worst_sign = float((4 * q * q).min()), float(np.abs(4 * q[:, :1] * q[:, 1:]).min())
    assert worst_sqrt > 1e-4, f"{tag}: a _sqrt_positive_part argument of {worst_sqrt}: change the seed"
    assert worst_sign > 1e-6, f"{tag}: a _copysign difference of {worst_sign}: change the seed"
    return worst_sqrt, worst_sign


def main(tags=TAGS, save=True):
    ps, ns = _namespace()
    out, total = {}, {}
    for tag in tags:
        before32, after32, maps32 = _reference(ps, ns, tag, torch.float32)
        before64, after64, _ = _reference(ps, ns, tag, torch.float64)
        seen = check_case(tag, before32, after32, before64, after64, maps32)
        r32, r64 = stored_rows(after32, np.float32), stored_rows(after64, np.float64)
        assert r32.shape == r64.shape and np.array_equal(r32[:, 6], r64[:, 6]) and np.array_equal(r32[:, 17], r64[:, 17])
        out[f"{tag}_rows"], out[f"{tag}_rows64"] = r32, r64
        out[f"{tag}_counts"] = np.array([len(a["scores"]) for a in after32], np.int32)
        bd, err = np.zeros(17), np.zeros(17)
        for cols in GROUPS:
            bd[cols], err[cols] = bound(r32[:, cols], r64[:, cols]) if len(r32) else (0.0, 0.0)
        out[f"{tag}_bound"], out[f"{tag}_ref_err"] = bd, err
        # the restatement on the reference's float32 maps: the same entries per (level, image), and its margins
        dense = [dict(logits=maps32["logits"][l], centerness=maps32["centerness"][l], box2d_reg=maps32["box2d_reg"][l],
                      **{k: maps32["box3d_" + k][l] for k in ("quat", "ctr", "depth", "size", "conf") if "box3d_quat" in maps32})
                 for l in range(len(dn.CASES[tag]["shapes"]))]
        details = {}
        dn.post_process(dense, dn.CASES[tag]["strides"], dn.golden_camera(tag), dn.CANON, dn.cfg_of(tag), details)
        for b, per_level in enumerate(details["levels"]):
            mine = np.concatenate([cand[:, [6, 8, 9]] for _, _, cand in per_level])
            ref = np.concatenate([before32[b]["pred_classes"][:, None], before32[b]["locations"]], 1)
            assert sorted(map(tuple, mine.tolist())) == sorted(map(tuple, ref.astype(np.float32).tolist())), \
                f"{tag}: the restatement selects other entries than the reference in image {b}"
        if "box3d_quat" in maps32:
            seen["margins"] = check_margins(tag, after32)
        for k, v in seen.items():
            if k != "margins":
                total[k] = total.get(k, 0) + int(v)
        print(tag, seen, "counts", out[f"{tag}_counts"], "ref_err", np.array2string(err, precision=2))
    need = dict(over_k="no (level, image) has more candidates than pre_nms_topk", empty_levels="no (level, image) is empty",
                empty_images="no image is without a detection", suppressed="no same-class pair is suppressed",
                cross_class="no cross-class pair above nms_thresh survives", cut_images="the post-NMS cut never bites",
                class5="the nc = 6 case has no class-5 candidate", clip_lo="the depth clip never bites below",
                clip_hi="the depth clip never bites above")
    if not save:
        return total
    for k, msg in need.items():
        assert total[k] >= 1, msg + ": change the seed"
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes", total)


if __name__ == "__main__":
    main()
