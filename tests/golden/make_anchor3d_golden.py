"""Golden vectors for BEVFusion's Anchor3DHead from the reference's own Python, executed by line range through
tests/golden/paddle_shim.py (the technique of make_bevdet_head_golden.py):

    Anchor3DHead.get_bboxes / get_bboxes_single   models/heads/dense_heads/anchor3d_head.py:378-520
    limit_period                                  models/detection/bevfusion/utils.py:92-103
    box3d_multiclass_nms                          models/detection/bevfusion/utils.py:189-276
    DeltaXYZWLHRBBoxCoder.decode                  utils/box_coder.py:270-306
    Anchor3DRangeGenerator /                      models/heads/dense_heads/target_assigner/anchor3d_generator.py:24-198,
    AlignedAnchor3DRangeGenerator                 :202-304

    python tests/golden/make_anchor3d_golden.py   # needs the reference checkout; writes python_anchor3d.npz

`self` is a SimpleNamespace; the three maps are torch's 1x1 convolutions of the seeded feature map and state dict
(anchor3d_numpy.golden_inputs / golden_state); nms_gpu is the reference's IoU + sweep compiled under oracle/_ref.  What
the shim lacks (paddle.nonzero, paddle.sort) is added here; np.floor inside limit_period is torch's floor.  Every case
runs twice from the same float32 inputs: in float32 and in float64.  Stored per case and frame: the float32 and float64
results, `*_ref_err` (the largest difference between the two runs) and `*_bound` (4 x that, one float32 ulp of the
largest magnitude as floor: make_bevformer_golden.bound), and the reference's anchor table.  Inputs are rebuilt from the
seed and not stored.

So that none of the reference's open choices decides a comparison, main() asserts (check_case) and says "change the
seed" otherwise: the maximum scores are distinct among the top K + 1 anchors of every frame; scores are distinct within
every class's candidate set and around the max_num cut; no candidate score lies within 1e-5 of score_thr; no pair of
same-class candidates has an IoU within 1e-3 of nms_thr (the oracle's IoU on the CPU); every case has a class without a
candidate and a frame where more than max_num boxes survive; both runs give the same labels, counts and row order.
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
import anchor3d_numpy as an  # noqa: E402
from make_bevformer_golden import bound  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "python_anchor3d.npz")
HEAD = os.path.join(REF, "paddle3d/models/heads/dense_heads/anchor3d_head.py")
UTILS = os.path.join(REF, "paddle3d/models/detection/bevfusion/utils.py")
CODER = os.path.join(REF, "paddle3d/utils/box_coder.py")
GENERATOR = os.path.join(REF, "paddle3d/models/heads/dense_heads/target_assigner/anchor3d_generator.py")
TAGS = an.TAGS


def load():
    return dict(np.load(OUT))


def _extend_shim(ps, p):
    """What get_bboxes calls and the shim lacks (added here, paddle_shim.py stays as it is)."""
    W = ps._wrap
    p.nonzero = lambda x: W(torch.nonzero(x.as_subclass(torch.Tensor)))
    p.sort = lambda x, axis=-1, descending=False: W(torch.sort(x.as_subclass(torch.Tensor), dim=axis,
                                                               descending=descending, stable=True).values)


def _namespace():
    import paddle_shim as ps

    p = ps.install(REF)
    _extend_shim(ps, p)
    from oracle import pyoracle as O

    O.build(ref=True)
    assert O.have_ref(), "oracle/_ref must be built"
    T = ps.tensor

    def nms_gpu(boxes, thresh):
        keep = O.nms(boxes.numpy().astype(np.float32), float(thresh), kind="ref")
        full = np.zeros(boxes.shape[0], np.int32)
        full[: len(keep)] = keep
        return T(full), T(np.array([len(keep)], np.int64))

    import paddle.nn.functional as F

    ns = dict(paddle=p, F=F, np=np, iou3d_nms=types.SimpleNamespace(nms_gpu=nms_gpu))
    ps.exec_lines(GENERATOR, [(24, 198), (202, 304)], ns)
    ps.exec_lines(CODER, [(270, 306)], ns)            # decode
    # limit_period applies np.floor to a tensor: torch's floor, the same fp32 operation
    util_ns = dict(ns, np=types.SimpleNamespace(floor=lambda x: torch.floor(x), pi=np.pi))
    ps.exec_lines(UTILS, [(92, 103), (189, 276)], util_ns)
    ns.update(limit_period=util_ns["limit_period"], box3d_multiclass_nms=util_ns["box3d_multiclass_nms"])
    ps.exec_lines(HEAD, [(378, 520)], ns)             # get_bboxes, get_bboxes_single (methods)
    return ps, ns


def torch_maps(tag, dtype):
    """The head's three maps by torch's convolution, from the float32 inputs, in `dtype`."""
    st, x = an.golden_state(tag), torch.from_numpy(an.golden_inputs(tag)).to(dtype)
    return [torch.nn.functional.conv2d(x, torch.from_numpy(st[k + ".weight"]).to(dtype),
                                       torch.from_numpy(st[k + ".bias"]).to(dtype))
            for k in ("conv_cls", "conv_reg", "conv_dir_cls")]


def _reference(ps, ns, tag, dtype):
    c = an.CASES[tag]
    gen = ns["AlignedAnchor3DRangeGenerator"](ranges=c["ranges"], sizes=c["sizes"], scales=[1], rotations=c["rotations"],
                                              custom_values=c["custom_values"], reshape_out=True, size_per_range=True)
    self = types.SimpleNamespace(num_classes=c["num_classes"], box_code_size=c["code_size"], use_sigmoid_cls=True,
                                 anchor_generator=gen, bbox_coder=types.SimpleNamespace(decode=ns["decode"]),
                                 dir_offset=c["dir_offset"], dir_limit_offset=c["dir_limit_offset"],
                                 test_cfg=dict(c["test_cfg"]))
    self.get_bboxes_single = types.MethodType(ns["get_bboxes_single"], self)
    maps = [[ps._wrap(m)] for m in torch_maps(tag, dtype)]
    with torch.no_grad():
        res = ns["get_bboxes"](self, *maps, input_metas=[{}] * c["B"])
        anchors = gen.grid_anchors([(c["H"], c["W"])])[0]
    return [(b.numpy(), s.numpy(), l.numpy().astype(np.int32)) for b, s, l in res], anchors.numpy()


def check_case(tag):
    """The maker's conditions on the seeded inputs (see the module docstring); returns what it saw."""
    from oracle import pyoracle as O

    c, cfg = an.CASES[tag], an.cfg_of(tag)
    kind = "ref" if O.have_ref() else "port"
    maps = [m.numpy() for m in torch_maps(tag, torch.float32)]
    anchors = anchors_of(tag)
    seen = dict(empty_classes=None, over_max=0, candidates=[])
    empty = set(range(c["num_classes"]))
    for b in range(c["B"]):
        scores_all = 1 / (1 + np.exp(-maps[0][b].transpose(1, 2, 0).reshape(-1, c["num_classes"]).astype(np.float64)))
        mx = np.sort(scores_all.max(1))[::-1][: cfg["nms_pre"] + 1]
        assert (np.diff(mx) < 0).all(), f"{tag}: equal maximum scores among the top K + 1: change the seed"
        trace = {}
        an.frame_bboxes(maps[0][b], maps[1][b], maps[2][b], anchors, cfg, kind, trace)
        s = trace["scores"]
        assert np.abs(s - np.float32(cfg["score_thr"])).min() > 1e-5, f"{tag}: a score at score_thr: change the seed"
        nb = trace["boxes"][:, :7].copy()
        nb[:, 6] = -nb[:, 6]
        kept_scores = []
        for cl, cand, keep in trace["sets"]:
            empty.discard(cl)
            sc = s[cand, cl]
            assert len(np.unique(sc)) == len(sc), f"{tag}: equal scores in class {cl}: change the seed"
            iou = O.boxes_iou_bev(nb[cand], nb[cand], kind=kind)[np.triu_indices(len(cand), 1)]
            assert iou.size == 0 or np.abs(iou - cfg["nms_thr"]).min() > 1e-3, f"{tag}: an IoU at nms_thr: change the seed"
            kept_scores += list(sc[keep])
            seen["candidates"].append(len(cand))
        ks = np.sort(np.array(kept_scores))[::-1]
        assert (np.diff(ks) < 0).all(), f"{tag}: equal scores around the max_num cut: change the seed"
        seen["over_max"] += int(trace["total"] > cfg["max_num"])
    assert empty, f"{tag}: every class has a candidate: change the seed"
    assert seen["over_max"] >= 1, f"{tag}: no frame keeps more than max_num: change the seed"
    seen["empty_classes"] = sorted(empty)
    return seen


def anchors_of(tag):
    """The case's anchor table by the product's restatement of the generator (the golden file holds the reference's)."""
    from paddle3d_amd.ops.anchor3d_head import aligned_anchor3d_grid

    c = an.CASES[tag]
    return aligned_anchor3d_grid(c["ranges"], c["sizes"], c["rotations"], c["custom_values"], (c["H"], c["W"])).numpy()


def main():
    ps, ns = _namespace()
    out = {}
    for tag in TAGS:
        c = an.CASES[tag]
        print(tag, check_case(tag))
        (r32, anchors), (r64, _) = _reference(ps, ns, tag, torch.float32), _reference(ps, ns, tag, torch.float64)
        out[f"{tag}_anchors"] = anchors.astype(np.float32)
        for b in range(c["B"]):
            (b32, s32, l32), (b64, s64, l64) = r32[b], r64[b]
            assert b32.dtype == np.float32 and b64.dtype == np.float64
            assert np.array_equal(l32, l64) and b32.shape == b64.shape, f"{tag}: the two runs select differently: change the seed"
            out[f"{tag}_labels_{b}"] = l32
            for name, v32, v64 in (("bboxes", b32, b64), ("scores", s32, s64)):
                out[f"{tag}_{name}_{b}"], out[f"{tag}_{name}64_{b}"] = v32, v64
                bd, err = bound(v32, v64) if v32.size else (np.float64(0), np.float64(0))
                out[f"{tag}_{name}_{b}_bound"], out[f"{tag}_{name}_{b}_ref_err"] = bd, err
            print(f"  frame {b}: {len(s32)} boxes, labels {np.bincount(l32, minlength=c['num_classes'])}, "
                  f"ref_err boxes {out[f'{tag}_bboxes_{b}_ref_err']:.3g} scores {out[f'{tag}_scores_{b}_ref_err']:.3g}")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
