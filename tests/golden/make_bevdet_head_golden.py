"""Golden vectors for BEVDet4D's CenterHead post-processing from the reference's own Python:
CenterHeadMatch.get_bboxes -> CenterPointBBoxCoder.decode / _topk -> get_task_detections / _circle_nms -> nms_bev ->
rotate_nms_pcdet (paddle3d/models/heads/dense_heads/bevdet_centerhead.py:669-968, :1049-1214;
paddle3d/models/layers/layer_libs.py:210-249; circle_nms, paddle3d/geometries/bbox.py:449-474), executed through
tests/golden/paddle_shim.py.

    python tests/golden/make_bevdet_head_golden.py     # needs /root/reference; writes python_bevdet_head.npz

The functions are executed from their line ranges (the module's imports drag in the whole framework); get_bboxes runs
on a SimpleNamespace carrying num_classes, test_cfg, bbox_coder, norm_bbox and task_heads, so no convolution is
built.  numba.jit is the identity (circle_nms runs as plain Python), nms_gpu is the reference's IoU + sweep compiled
under oracle/_ref.  The inputs are rebuilt from a seed (bevdet_head_numpy.golden_inputs) and not stored; the seed's
maps have no equal scores among the selected cells, so the reference's open tie order does not matter.
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
import bevdet_head_numpy as bh  # noqa: E402
import paddle_shim as ps  # noqa: E402

REF = "/root/reference"
HEAD = os.path.join(REF, "paddle3d/models/heads/dense_heads/bevdet_centerhead.py")
LAYER_LIBS = os.path.join(REF, "paddle3d/models/layers/layer_libs.py")
BBOX = os.path.join(REF, "paddle3d/geometries/bbox.py")


def _extend_shim(p):
    """What the post-processing calls and the shim lacks (added here, paddle_shim.py stays as it is)."""
    W = ps._wrap

    def topk(x, k, axis=-1, largest=True, sorted=True):
        v, i = torch.topk(x.as_subclass(torch.Tensor), int(k), dim=axis, largest=largest, sorted=sorted)
        return W(v), W(i)

    p.topk = topk
    p.empty = lambda shape, dtype="float32": W(torch.empty(tuple(int(s) for s in shape), dtype=ps._dt(dtype)))
    p.empty_like = lambda x, dtype=None: W(torch.empty_like(x, dtype=ps._dt(dtype)))

    def take_along_axis(self, indices, axis):
        return W(torch.gather(self.as_subclass(torch.Tensor), axis, indices.as_subclass(torch.Tensor).long()))

    def index_select(self, index, axis=0):
        if not isinstance(index, torch.Tensor):
            index = torch.as_tensor(np.asarray(index, np.int64).reshape(-1))
        return W(torch.index_select(self.as_subclass(torch.Tensor), axis, index.as_subclass(torch.Tensor).long()))

    def masked_select(self, mask):
        return W(torch.masked_select(self.as_subclass(torch.Tensor), mask.as_subclass(torch.Tensor)))

    ps.Tensor.take_along_axis = take_along_axis
    ps.Tensor.index_select = index_select
    ps.Tensor.masked_select = masked_select


def main():
    p = ps.install(REF)
    _extend_shim(p)
    from oracle import pyoracle as O

    O.build(ref=True)
    assert O.have_ref(), "oracle/_ref must be built"
    T = ps.tensor

    def nms_gpu(boxes, thresh):
        keep = O.nms(boxes.numpy(), float(thresh), kind="ref")
        full = np.zeros(boxes.shape[0], np.int32)
        full[: len(keep)] = keep
        return T(full), T(np.array([len(keep)], np.int64))

    import paddle.nn.functional as F

    ns = dict(paddle=p, F=F, np=np, iou3d_nms=types.SimpleNamespace(nms_gpu=nms_gpu),
              numba=types.SimpleNamespace(jit=lambda *a, **k: (lambda f: f)))
    ps.exec_lines(BBOX, [(449, 474)], ns)                      # circle_nms (numba.jit as identity)
    ps.exec_lines(LAYER_LIBS, [(210, 249)], ns)                # rotate_nms_pcdet
    ps.exec_lines(HEAD, [(669, 906)], ns)                      # get_bboxes, get_task_detections (methods)
    ps.exec_lines(HEAD, [(909, 921), (939, 968), (1049, 1214)], ns)  # _circle_nms, nms_bev, CenterPointBBoxCoder

    cfg = bh.GOLDEN_TEST_CFG
    coder = ns["CenterPointBBoxCoder"](**bh.GOLDEN_CODER)
    self = types.SimpleNamespace(num_classes=list(bh.GOLDEN_TASKS), test_cfg=dict(cfg), bbox_coder=coder,
                                 norm_bbox=True, task_heads=[None] * len(bh.GOLDEN_TASKS))
    self.get_task_detections = types.MethodType(ns["get_task_detections"], self)
    heads = bh.golden_inputs()
    # the selected cells have distinct scores (the reference's tie order is left open)
    for hd in heads:
        s = torch.sigmoid(torch.from_numpy(hd["heatmap"])).reshape(bh.GOLDEN_BATCH, -1)
        top = torch.sort(s, dim=1, descending=True).values[:, : bh.GOLDEN_CODER["max_num"] + 1]
        assert bool((top[:, 1:] != top[:, :-1]).all()), "equal scores among the selected cells: change the seed"
    preds = [{k: T(v) for k, v in hd.items()} for hd in heads]
    with torch.no_grad():
        res = ns["get_bboxes"](self, preds, img_metas=None)
    out = {}
    for i, (b, s, l) in enumerate(res):
        out[f"bboxes_{i}"] = b.numpy().astype(np.float32)
        out[f"scores_{i}"] = s.numpy().astype(np.float32)
        out[f"labels_{i}"] = l.numpy().astype(np.int32)  # (concatenated onto an empty float32 tensor in the shim)
        print(f"frame {i}: {len(s)} boxes, labels {np.bincount(out[f'labels_{i}'])}")
    np.savez_compressed(os.path.join(HERE, "python_bevdet_head.npz"), **out)


if __name__ == "__main__":
    main()
