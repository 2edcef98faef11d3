"""BEVFusion's Anchor3DHead at inference (reference: paddle3d/models/heads/dense_heads/anchor3d_head.py, with
target_assigner/anchor3d_generator.py:202-304, utils/box_coder.py:217-310 and models/detection/bevfusion/utils.py:92-103,
:189-276).  Constructor arguments and state-dict keys (conv_cls / conv_reg / conv_dir_cls, .weight / .bias) are the
reference's; training targets and losses are not here.

    forward(feats)                         the three maps per level, as the reference returns them
    get_bboxes(cls_scores, bbox_preds, dir_cls_preds, input_metas, cfg=None)
                                           from existing maps (ops.anchor3d_head.anchor3d_get_bboxes)
    forward_get_bboxes(feats, input_metas, cfg=None, fused=True)
                                           the LAZY head (ops.anchor3d_head.anchor3d_head_forward): only conv_cls runs
                                           densely; the regression, direction and class rows are evaluated at the
                                           <= nms_pre selected anchors; none of the three maps is formed
Both return, per frame, (bboxes [n, code_size], scores [n], labels int64 [n]) as views of the fixed-size device results;
the counts are read on the host once, to cut those views.  return_padded=True returns (boxes [B, max_num, code_size],
scores [B, max_num], labels int32 [B, max_num], counts int32 [B]) untouched and reads nothing back.

A shape the kernels refuse (ops.anchor3d_head.anchor3d_supported), a multi-level input, a CPU tensor or fused=False takes
`get_bboxes_torch`, a plain-torch transcription of the reference that runs ops.iou3d_nms.nms_gpu per class.

Default of forward_get_bboxes(fused=True): LAZY_BY_DEFAULT below, set from the measurement in DESIGN.md (the lazy path
is the default only where it measured faster than the dense convolutions + the from-maps op); fused="force" always takes
the lazy path when the shape is supported.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .derived import InferenceCache, derived
from .ops import anchor3d_head as _ops
from .ops import conv as _conv
from .ops import iou3d_nms as _nms

__all__ = ["AlignedAnchor3DRangeGenerator", "DeltaXYZWLHRBBoxCoder", "Anchor3DHead", "limit_period",
           "box3d_multiclass_nms", "LAZY_BY_DEFAULT"]

# forward_get_bboxes(fused=True) takes the lazy kernel sequence (see DESIGN.md's Anchor3DHead section for the numbers)
LAZY_BY_DEFAULT = True


class AlignedAnchor3DRangeGenerator:
    """anchor3d_generator.py:24-84, :202-304 with align_corner=False and size_per_range=True (the configs' form)."""

    def __init__(self, ranges, sizes=((1.6, 3.9, 1.56),), scales=(1,), rotations=(0, 1.5707963), custom_values=(),
                 reshape_out=True, size_per_range=True, align_corner=False):
        if not size_per_range or align_corner or not reshape_out:
            raise NotImplementedError("AlignedAnchor3DRangeGenerator: size_per_range=True, align_corner=False and "
                                      "reshape_out=True only")
        self.sizes = [list(s) for s in torch.tensor(sizes, dtype=torch.float64).reshape(-1, 3).tolist()]
        self.ranges = [list(r) for r in ranges]
        if len(self.ranges) != len(self.sizes):
            assert len(self.ranges) == 1
            self.ranges = self.ranges * len(self.sizes)
        self.scales = list(scales)
        self.rotations = list(rotations)
        self.custom_values = tuple(custom_values)

    @property
    def num_base_anchors(self):
        return len(self.rotations) * len(self.sizes)

    @property
    def num_levels(self):
        return len(self.scales)

    def grid_anchors(self, featmap_sizes, device="cpu"):
        assert self.num_levels == len(featmap_sizes)
        return [_ops.aligned_anchor3d_grid(self.ranges, self.sizes, self.rotations, self.custom_values, tuple(fs),
                                           scale).to(device) for fs, scale in zip(featmap_sizes, self.scales)]


class DeltaXYZWLHRBBoxCoder:
    """box_coder.py:217-310 (decode only)."""

    def __init__(self, code_size=7):
        self.code_size = code_size

    @staticmethod
    def decode(anchors, deltas):
        xa, ya, za, wa, la, ha, ra = (anchors[..., k:k + 1] for k in range(7))
        xt, yt, zt, wt, lt, ht, rt = (deltas[..., k:k + 1] for k in range(7))
        za = za + ha / 2
        diagonal = torch.sqrt(la ** 2 + wa ** 2)
        xg = xt * diagonal + xa
        yg = yt * diagonal + ya
        zg = zt * ha + za
        lg = torch.exp(lt) * la
        wg = torch.exp(wt) * wa
        hg = torch.exp(ht) * ha
        rg = rt + ra
        zg = zg - hg / 2
        return torch.cat([xg, yg, zg, wg, lg, hg, rg, deltas[..., 7:] + anchors[..., 7:]], dim=-1)


def limit_period(val, offset=0.5, period=math.pi):
    """utils.py:92-103."""
    return val - torch.floor(val / period + offset) * period


def box3d_multiclass_nms(mlvl_bboxes, mlvl_bboxes_for_nms, mlvl_scores, score_thr, max_num, cfg, mlvl_dir_scores):
    """utils.py:189-276 in torch; nms_gpu is ops.iou3d_nms.nms_gpu (keep indices on the host, as in the reference)."""
    num_classes = mlvl_scores.shape[1] - 1
    bboxes, scores, labels, dir_scores = [], [], [], []
    for i in range(num_classes):
        cls_inds = torch.nonzero(mlvl_scores[:, i] > score_thr).reshape(-1)
        if cls_inds.numel() == 0:
            continue
        _scores = mlvl_scores[cls_inds, i]
        order = torch.argsort(_scores, descending=True, stable=True)
        keep, num_out = _nms.nms_gpu(mlvl_bboxes_for_nms[cls_inds][order].contiguous(), cfg["nms_thr"])
        selected = order[keep[:int(num_out)].to(order.device).long()]
        bboxes.append(mlvl_bboxes[cls_inds][selected])
        scores.append(_scores[selected])
        labels.append(torch.full((len(selected),), i, dtype=torch.int64, device=_scores.device))
        dir_scores.append(mlvl_dir_scores[cls_inds][selected])
    if not bboxes:
        z = mlvl_bboxes.new_zeros
        return z((0, mlvl_bboxes.shape[-1])), z((0,)), z((0,), dtype=torch.int64), z((0,), dtype=torch.int64)
    bboxes, scores, labels, dir_scores = (torch.cat(t, dim=0) for t in (bboxes, scores, labels, dir_scores))
    if bboxes.shape[0] > max_num:
        inds = torch.argsort(scores, descending=True, stable=True)[:max_num]
        bboxes, scores, labels, dir_scores = bboxes[inds], scores[inds], labels[inds], dir_scores[inds]
    return bboxes, scores, labels, dir_scores


class Anchor3DHead(InferenceCache, nn.Module):
    def __init__(self, num_classes, in_channels, feat_channels=256, use_direction_classifier=True, anchor_generator=None,
                 assigner_per_size=False, assign_per_class=False, diff_rad_by_sin=True, dir_offset=0, dir_limit_offset=1,
                 bbox_coder=None, loss_cls=None, loss_bbox=None, loss_dir=None, use_sigmoid_cls=True, bbox_assigner=None,
                 train_cfg=None, test_cfg=None):
        super().__init__()
        self.in_channels = in_channels
        self.num_classes = num_classes
        self.feat_channels = feat_channels
        self.diff_rad_by_sin = diff_rad_by_sin
        self.use_direction_classifier = use_direction_classifier
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg
        self.assigner_per_size = assigner_per_size
        self.assign_per_class = assign_per_class
        self.dir_offset = dir_offset
        self.dir_limit_offset = dir_limit_offset
        if isinstance(anchor_generator, dict):
            anchor_generator = AlignedAnchor3DRangeGenerator(**anchor_generator)
        self.anchor_generator = anchor_generator
        self.num_anchors = self.anchor_generator.num_base_anchors
        if isinstance(bbox_coder, dict):
            bbox_coder = DeltaXYZWLHRBBoxCoder(**bbox_coder)
        self.bbox_coder = bbox_coder if bbox_coder is not None else DeltaXYZWLHRBBoxCoder()
        self.box_code_size = self.bbox_coder.code_size
        self.use_sigmoid_cls = use_sigmoid_cls
        if not self.use_sigmoid_cls:
            self.num_classes += 1
        # anchor3d_head.py:120-128
        self.cls_out_channels = self.num_anchors * self.num_classes
        self.conv_cls = nn.Conv2d(self.feat_channels, self.cls_out_channels, 1)
        self.conv_reg = nn.Conv2d(self.feat_channels, self.num_anchors * self.box_code_size, 1)
        if self.use_direction_classifier:
            self.conv_dir_cls = nn.Conv2d(self.feat_channels, self.num_anchors * 2, 1)
        self._anchors = {}

    # ---- derived tensors ---------------------------------------------------------------------------------------------
    def _plan(self):
        def build():
            convs = [self.conv_cls, self.conv_reg] + ([self.conv_dir_cls] if self.use_direction_classifier else [])
            return dict(
                cls_packed=_ops.pack_cls_weight(self.conv_cls.weight.detach(), self.num_classes),
                patch=[_conv.pack_patch_weight(c.weight.detach(), 1, False) for c in convs])
        return derived(self, "plan", build)

    def anchors_for(self, featmap_size, device):
        """The level-0 anchor table [H * W * A, code_size] of a map size, built once per (size, device)."""
        key = (int(featmap_size[0]), int(featmap_size[1]), str(device))
        if key not in self._anchors:
            a = self.anchor_generator.grid_anchors([key[:2]] + [key[:2]] * (self.anchor_generator.num_levels - 1))[0]
            self._anchors[key] = a.reshape(-1, self.box_code_size).to(device)
        return self._anchors[key]

    # ---- the reference's forward -------------------------------------------------------------------------------------
    def forward_single(self, x):
        convs = [self.conv_cls, self.conv_reg] + ([self.conv_dir_cls] if self.use_direction_classifier else [])
        h, w = int(x.shape[2]), int(x.shape[3])
        if x.is_cuda and not self.training and x.dtype == torch.float32 and all(
                _conv.patch_supported(1, c.in_channels, c.out_channels, h, w) for c in convs):
            packed = self._plan()["patch"]
            outs = []
            for c, wp in zip(convs, packed):
                out = torch.empty((x.shape[0], c.out_channels, h, w), dtype=torch.float32, device=x.device)
                outs.append(_conv.patch_conv_bias_relu(x, wp, c.bias.detach(), 1, c.out_channels, out, 0, relu=False))
        else:
            outs = [c(x) for c in convs]
        return outs[0], outs[1], (outs[2] if self.use_direction_classifier else None)

    def forward(self, feats):
        res = [self.forward_single(x) for x in feats]
        return tuple([r[k] for r in res] for k in range(3))

    # ---- get_bboxes --------------------------------------------------------------------------------------------------
    def _cfg(self, cfg):
        cfg = self.test_cfg if cfg is None else cfg
        return dict(nms_pre=int(cfg.get("nms_pre", -1)), max_num=int(cfg["max_num"]),
                    score_thr=float(cfg.get("score_thr", 0)), nms_thr=float(cfg["nms_thr"]))

    def _supported(self, channels, h, w, cfg):
        return _ops.anchor3d_supported(channels, self.num_classes, self.num_anchors, self.box_code_size, cfg["nms_pre"],
                                       cfg["max_num"], h * w * self.num_anchors, self.use_sigmoid_cls,
                                       self.use_direction_classifier)

    @staticmethod
    def _as_lists(padded):
        boxes, scores, labels, counts = padded
        labels = labels.long()
        return [(boxes[b, :n], scores[b, :n], labels[b, :n]) for b, n in enumerate(counts.tolist())]

    @staticmethod
    def _as_padded(results, max_num, code_size, device):
        b = len(results)
        boxes = torch.zeros((b, max_num, code_size), dtype=torch.float32, device=device)
        scores = torch.zeros((b, max_num), dtype=torch.float32, device=device)
        labels = torch.zeros((b, max_num), dtype=torch.int32, device=device)
        counts = torch.tensor([len(r[1]) for r in results], dtype=torch.int32, device=device)
        for i, (bx, sc, lb) in enumerate(results):
            boxes[i, :len(sc)], scores[i, :len(sc)], labels[i, :len(sc)] = bx, sc, lb.to(torch.int32)
        return boxes, scores, labels, counts

    def get_bboxes_single_torch(self, cls_scores, bbox_preds, dir_cls_preds, mlvl_anchors, cfg):
        """anchor3d_head.py:427-520 for one frame: lists of per-level maps [channels, H, W]."""
        mlvl_bboxes, mlvl_scores, mlvl_dir_scores = [], [], []
        for cls_score, bbox_pred, dir_cls_pred, anchors in zip(cls_scores, bbox_preds, dir_cls_preds, mlvl_anchors):
            dir_cls_score = torch.argmax(dir_cls_pred.permute(1, 2, 0).reshape(-1, 2), dim=-1)
            cls_score = cls_score.permute(1, 2, 0).reshape(-1, self.num_classes)
            scores = torch.sigmoid(cls_score) if self.use_sigmoid_cls else F.softmax(cls_score, dim=-1)
            bbox_pred = bbox_pred.permute(1, 2, 0).reshape(-1, self.box_code_size)
            nms_pre = cfg["nms_pre"]
            if nms_pre > 0 and scores.shape[0] > nms_pre:
                max_scores = scores.max(dim=1).values if self.use_sigmoid_cls else scores[:, :-1].max(dim=1).values
                topk_inds = torch.sort(max_scores.topk(nms_pre).indices).values
                anchors, bbox_pred, scores = anchors[topk_inds], bbox_pred[topk_inds], scores[topk_inds]
                dir_cls_score = dir_cls_score[topk_inds]
            mlvl_bboxes.append(self.bbox_coder.decode(anchors, bbox_pred))
            mlvl_scores.append(scores)
            mlvl_dir_scores.append(dir_cls_score)
        mlvl_bboxes = torch.cat(mlvl_bboxes)
        mlvl_bboxes_for_nms = mlvl_bboxes[:, :7].clone()
        mlvl_bboxes_for_nms[:, -1] = -mlvl_bboxes_for_nms[:, -1]
        mlvl_scores = torch.cat(mlvl_scores)
        mlvl_dir_scores = torch.cat(mlvl_dir_scores)
        if self.use_sigmoid_cls:
            mlvl_scores = torch.cat([mlvl_scores, mlvl_scores.new_zeros((mlvl_scores.shape[0], 1))], dim=1)
        bboxes, scores, labels, dir_scores = box3d_multiclass_nms(mlvl_bboxes, mlvl_bboxes_for_nms, mlvl_scores,
                                                                  cfg["score_thr"], cfg["max_num"], cfg, mlvl_dir_scores)
        if bboxes.shape[0] > 0:
            dir_rot = limit_period(bboxes[..., 6] - self.dir_offset, self.dir_limit_offset, math.pi)
            bboxes[..., 6] = dir_rot + self.dir_offset + math.pi * dir_scores.to(bboxes.dtype)
        return bboxes, scores, labels

    def get_bboxes_torch(self, cls_scores, bbox_preds, dir_cls_preds, input_metas, cfg=None):
        """anchor3d_head.py:378-425, any number of levels: the unfused path."""
        cfg = self._cfg(cfg)
        dev = cls_scores[0].device
        sizes = [tuple(int(s) for s in c.shape[-2:]) for c in cls_scores]
        anchors = [a.reshape(-1, self.box_code_size) for a in self.anchor_generator.grid_anchors(sizes, device=dev)]
        out = []
        for i in range(len(input_metas)):
            out.append(self.get_bboxes_single_torch([c[i].detach() for c in cls_scores], [c[i].detach() for c in bbox_preds],
                                                    [c[i].detach() for c in dir_cls_preds], anchors, cfg))
        return out

    def get_bboxes(self, cls_scores, bbox_preds, dir_cls_preds, input_metas, cfg=None, rescale=False, fused=True,
                   return_padded=False):
        c = self._cfg(cfg)
        padded = None
        if fused and len(cls_scores) == 1 and cls_scores[0].is_cuda and self.use_direction_classifier:
            h, w = (int(s) for s in cls_scores[0].shape[-2:])
            if self._supported(None, h, w, c):
                n = len(input_metas)
                padded = _ops.anchor3d_get_bboxes(cls_scores[0][:n].detach(), bbox_preds[0][:n].detach(),
                                                  dir_cls_preds[0][:n].detach(), self.anchors_for((h, w), cls_scores[0].device),
                                                  self.num_classes, c["nms_pre"], c["max_num"], c["score_thr"],
                                                  c["nms_thr"], self.dir_offset, self.dir_limit_offset)
        if padded is None:
            res = self.get_bboxes_torch(cls_scores, bbox_preds, dir_cls_preds, input_metas, cfg)
            return self._as_padded(res, c["max_num"], self.box_code_size, cls_scores[0].device) if return_padded else res
        return padded if return_padded else self._as_lists(padded)

    def forward_get_bboxes(self, feats, input_metas, cfg=None, fused=True, return_padded=False):
        c = self._cfg(cfg)
        lazy = fused == "force" or (fused is True and LAZY_BY_DEFAULT)
        if lazy and len(feats) == 1 and feats[0].is_cuda and not self.training and feats[0].dtype == torch.float32:
            x = feats[0][:len(input_metas)].detach()
            ch, h, w = (int(s) for s in x.shape[1:])
            if self._supported(ch, h, w, c):
                padded = _ops.anchor3d_head_forward(
                    x, self._plan()["cls_packed"], self.conv_cls.bias.detach(), self.conv_reg.weight.detach(),
                    self.conv_reg.bias.detach(), self.conv_dir_cls.weight.detach(), self.conv_dir_cls.bias.detach(),
                    self.anchors_for((h, w), x.device), self.num_classes, c["nms_pre"], c["max_num"], c["score_thr"],
                    c["nms_thr"], self.dir_offset, self.dir_limit_offset)
                if padded is not None:
                    return padded if return_padded else self._as_lists(padded)
        with torch.no_grad():
            maps = self.forward(feats)
        return self.get_bboxes(*maps, input_metas, cfg, fused=bool(fused), return_padded=return_padded)
