"""DD3D, the reference's FCOS-based monocular 3D detector, at inference: heads and post-processing on the device.

Reference: paddle3d/models/detection/dd3d/dd3d.py:32-212 (DD3D), models/heads/fcos_heads/fcos2d_head.py:29-186, :314-503
(FCOS2DHead, FCOS2DInference), fcos3d_head.py:33-296, :482-639 (predictions_to_boxes3d, FCOS3DHead, FCOS3DInference),
models/layers/normalization.py:19-67 (Scale, Offset, LayerListDial), layers/layer_norm.py:36-92 (FrozenBatchNorm2d),
utils/transform.py:167-246, losses/disentangled_box3d_loss.py:36-60; configs/dd3d/*.yml.  Constructor arguments and
state-dict keys are the reference's (cls_tower.{3i}.weight, cls_tower.{3i + 1}.{level}.*, scales_box2d_reg.{level}.scale,
box3d_quat.{i}.weight, offsets_depth.{level}.bias, ...; BatchNorm's _mean / _variance as checkpoint.py maps them).  The
backbone and the FPN are torch.nn.Modules handed in.  Inference only: targets, the losses and BatchNorm's training mode
are not here, and neither is convert_3d_box_to_kitti (it needs pyquaternion).

    FCOS2DHead(...)(features) / FCOS3DHead(...)(features)   the reference's dense outputs (torch layers)
    FCOS2DHead.towers / FCOS3DHead.tower                    the towers' outputs per level: what the lazy form reads
    FCOS2DInference / FCOS3DInference                       the plain-torch transcription of the reference's tail
    DD3D.towers(features)                                   the three towers' outputs per level (dense in every form)
    DD3D.tail_padded(cls_out, box_out, box3d_out, K, fused) the same as head_padded from the towers' outputs
    DD3D.head_padded(features, intrinsics, fused)           (rows [B, R, 20], counts int32 [B]) on the device without a
                                                            host synchronisation: fused "lazy" (towers, cls_logits and
                                                            centerness densely, then ops.dd3d.dd3d_head_forward: the
                                                            4 + 11 predictor channels at the selected entries only),
                                                            "dense" (torch heads + ops.dd3d.dd3d_post_process), True
                                                            (LAZY_BY_DEFAULT decides) or False (the transcription)
    DD3D.forward(samples)                                   {"preds": per-image dicts} (rows_to_instances: the one host
                                                            synchronisation)

The transcription also runs for CPU tensors, shapes the kernels refuse (ops.dd3d.dd3d_supported), do_nms=False and
nms_thresh <= 0.  The towers' 3x3 convolutions are torch's; conv_kernel="winograd43" asks for the F(4x4, 3x3) Winograd
kernel where ops.conv.winograd43_supported holds.  FrozenBatchNorm2d is folded: scale = weight * rsqrt(var + eps) and
shift = bias - mean * scale, each rounded to fp32 once, y = x * scale + shift.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .derived import derived
from .ops import conv as conv_ops
from .ops import dd3d as dd3d_ops

__all__ = ["Scale", "Offset", "LayerListDial", "FrozenBatchNorm2d", "FCOS2DHead", "FCOS3DHead", "FCOS2DInference",
           "FCOS3DInference", "DD3D", "rows_to_instances", "predictions_to_boxes3d", "LAZY_BY_DEFAULT", "CANON_BOX_SIZES"]

# fused=True takes the lazy kernel sequence (see DESIGN.md's DD3D section for the numbers); fused="dense" the other
LAZY_BY_DEFAULT = True
EPS = 1e-7
CANON_BOX_SIZES = [[1.61876949, 3.89154523, 1.52969237], [0.62806586, 0.82038497, 1.76784787],
                   [0.56898187, 1.77149234, 1.7237099], [1.9134491, 5.15499603, 2.18998422],
                   [2.61168401, 9.22692319, 3.36492722], [0.5390196, 1.08098042, 1.28392158],
                   [2.36044838, 15.56991038, 3.5289238], [1.24489164, 2.51495357, 1.61402478]]  # (width, length, height)


class Scale(nn.Module):
    def __init__(self, init_value=1.0):
        super().__init__()
        self.scale = nn.Parameter(torch.tensor([float(init_value)], dtype=torch.float32))

    def forward(self, x):
        return x * self.scale


class Offset(nn.Module):
    def __init__(self, init_value=0.0):
        super().__init__()
        self.bias = nn.Parameter(torch.tensor([float(init_value)], dtype=torch.float32))

    def forward(self, x):
        return x + self.bias


class LayerListDial(nn.ModuleList):
    """normalization.py:53-67: call k goes to layer k modulo the length (one norm layer per FPN level)."""

    def __init__(self, layers=None):
        super().__init__(layers)
        self.cur_position = 0

    def forward(self, x):
        result = self[self.cur_position](x)
        self.cur_position = (self.cur_position + 1) % len(self)
        return result


class FrozenBatchNorm2d(nn.Module):
    """layer_norm.py:36-92, folded to one scale and one shift per channel (fp32)."""

    def __init__(self, num_features, eps=1e-5):
        super().__init__()
        self.num_features, self.eps = num_features, eps
        self.register_buffer("weight", torch.ones(num_features))
        self.register_buffer("bias", torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features) - eps)

    def forward(self, x):
        scale = self.weight * (self.running_var + self.eps).rsqrt()
        shift = self.bias - self.running_mean * scale
        return x * scale.reshape(1, -1, 1, 1).to(x.dtype) + shift.reshape(1, -1, 1, 1).to(x.dtype)


class _TowerConv(nn.Conv2d):
    """A tower's 3x3 convolution: torch's, or the F(4x4, 3x3) Winograd kernel on request (conv_kernel="winograd43")."""

    conv_kernel = "torch"

    def forward(self, x):
        b, cin, h, w = x.shape
        if (self.conv_kernel == "winograd43" and x.is_cuda and x.dtype == torch.float32 and
                conv_ops.winograd43_supported(cin, self.out_channels, h, w)):
            def build():
                bias = self.bias if self.bias is not None else torch.zeros(self.out_channels, device=x.device)
                return conv_ops.pack_winograd43_weight(self.weight.float()), bias.float().contiguous()
            packed = derived(self, "winograd43", build)
            pitch = conv_ops.pitch4(w)
            xp = x.contiguous() if pitch == w else F.pad(x, (0, pitch - w))
            out = conv_ops.conv3x3_winograd43_bias_relu(xp, packed[0], packed[1], self.out_channels,
                                                        relu=False, w_valid=w)
            return out[:, :, :, :w]
        return super().forward(x)


def _norm(norm, channels, levels):
    if norm == "BN":
        return LayerListDial([nn.BatchNorm2d(channels) for _ in range(levels)])
    if norm == "FrozenBN":
        return LayerListDial([FrozenBatchNorm2d(channels) for _ in range(levels)])
    raise NotImplementedError(norm)


def _tower(channels, num_convs, levels, norm, bias, conv_kernel):
    layers = []
    for _ in range(num_convs):
        conv = _TowerConv(channels, channels, 3, stride=1, padding=1, bias=bias)
        conv.conv_kernel = conv_kernel
        layers += [conv, _norm(norm, channels, levels), nn.ReLU()]
    return nn.Sequential(*layers)


def _init_predictors(layers):
    for m in layers:
        nn.init.kaiming_uniform_(m.weight, a=1)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0.0)


def _init_tower(tower):
    for m in tower.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            if m.bias is not None:
                nn.init.constant_(m.bias, 0.0)


class FCOS2DHead(nn.Module):
    """fcos2d_head.py:29-186."""

    def __init__(self, in_strides, in_channels, num_classes=5, use_scale=True, box2d_scale_init_factor=1.0, version="v2",
                 num_cls_convs=4, num_box_convs=4, use_deformable=False, norm="BN", conv_kernel="torch"):
        super().__init__()
        self.in_strides, self.num_levels, self.num_classes = list(in_strides), len(in_strides), num_classes
        self.use_scale, self.box2d_scale_init_factor, self.version = use_scale, box2d_scale_init_factor, version
        assert len(set(in_channels)) == 1, "Each level must have the same channel!"
        c = self.channels = in_channels[0]
        if use_deformable:
            raise ValueError("Not supported yet.")
        if version == "v1":
            if norm != "BN":
                raise NotImplementedError()
        elif version != "v2":
            raise ValueError(f"Invalid FCOS2D version: {version}")
        self.cls_tower = _tower(c, num_cls_convs, self.num_levels, norm, version == "v1", conv_kernel)
        self.box2d_tower = _tower(c, num_box_convs, self.num_levels, norm, version == "v1", conv_kernel)
        self.cls_logits = nn.Conv2d(c, num_classes, 3, stride=1, padding=1)
        self.box2d_reg = nn.Conv2d(c, 4, 3, stride=1, padding=1)
        self.centerness = nn.Conv2d(c, 1, 3, stride=1, padding=1)
        if use_scale:
            scales = nn.ModuleList([Scale(init_value=s * box2d_scale_init_factor) for s in self.in_strides])
            if version == "v1":
                self.scales_reg = scales
            else:
                self.scales_box2d_reg = scales
        _init_tower(self.cls_tower), _init_tower(self.box2d_tower)
        _init_predictors([self.cls_logits, self.box2d_reg, self.centerness])

    @property
    def scales(self):
        if not self.use_scale:
            return None
        return self.scales_reg if self.version == "v1" else self.scales_box2d_reg

    def towers(self, x):
        """(cls_tower outputs, box2d_tower outputs) per level, in level order (the norm layers dial through the levels)."""
        return [self.cls_tower(f) for f in x], [self.box2d_tower(f) for f in x]

    def predict(self, cls_out, box_out):
        """The dense predictors from the towers' outputs: (logits, box2d_reg, centerness) per level."""
        logits = [self.cls_logits(t) for t in cls_out]
        centerness = [self.centerness(t) for t in box_out]
        box2d_reg = []
        for l, t in enumerate(box_out):
            reg = self.box2d_reg(t)
            if self.use_scale:
                reg = self.scales[l](reg)
            box2d_reg.append(F.relu(reg))
        return logits, box2d_reg, centerness

    def forward(self, x):
        cls_out, box_out = self.towers(x)
        return (*self.predict(cls_out, box_out), {"cls_tower_out": cls_out})


class FCOS3DHead(nn.Module):
    """fcos3d_head.py:111-296."""

    def __init__(self, in_strides, in_channels, num_classes=5, use_scale=True, depth_scale_init_factor=0.3,
                 proj_ctr_scale_init_factor=1.0, use_per_level_predictors=False,
                 mean_depth_per_level=(32.594, 15.178, 8.424, 5.004, 4.662),
                 std_depth_per_level=(14.682, 7.139, 4.345, 2.399, 2.587), num_convs=4, use_deformable=False,
                 norm="FrozenBN", class_agnostic_box3d=False, per_level_predictors=False, conv_kernel="torch"):
        super().__init__()
        self.in_strides, self.num_levels, self.num_classes = list(in_strides), len(in_strides), num_classes
        self.use_scale, self.use_per_level_predictors = use_scale, use_per_level_predictors
        self.class_agnostic_box3d = class_agnostic_box3d
        self.register_buffer("mean_depth_per_level", torch.tensor(mean_depth_per_level, dtype=torch.float32))
        self.register_buffer("std_depth_per_level", torch.tensor(std_depth_per_level, dtype=torch.float32))
        assert len(set(in_channels)) == 1, "Each level must have the same channel!"
        c = self.channels = in_channels[0]
        if use_deformable:
            raise ValueError("Not supported yet.")
        self.box3d_tower = _tower(c, num_convs, self.num_levels, norm, False, conv_kernel)
        ncp = self.box3d_classes = 1 if class_agnostic_box3d else num_classes
        n = self.num_levels if per_level_predictors else 1

        def predictors(k, bias=True):
            return nn.ModuleList([nn.Conv2d(c, k * ncp, 3, stride=1, padding=1, bias=bias) for _ in range(n)])

        self.box3d_quat, self.box3d_ctr = predictors(4), predictors(2)
        self.box3d_depth = predictors(1, bias=not use_scale)
        self.box3d_size, self.box3d_conf = predictors(3), predictors(1)
        if use_scale:
            self.scales_proj_ctr = nn.ModuleList([Scale(s * proj_ctr_scale_init_factor) for s in self.in_strides])
            self.scales_size = nn.ModuleList([Scale(1.0) for _ in range(self.num_levels)])
            self.scales_conf = nn.ModuleList([Scale(1.0) for _ in range(self.num_levels)])
            self.scales_depth = nn.ModuleList([Scale(float(s) * depth_scale_init_factor) for s in std_depth_per_level])
            self.offsets_depth = nn.ModuleList([Offset(float(b)) for b in mean_depth_per_level])
        _init_tower(self.box3d_tower)
        for group in (self.box3d_quat, self.box3d_ctr, self.box3d_depth, self.box3d_size, self.box3d_conf):
            _init_predictors(group)

    def tower(self, x):
        return [self.box3d_tower(f) for f in x]

    def predict(self, tower_out):
        """The dense predictors from the tower's outputs: (quat, ctr, depth, size, conf) per level."""
        quat, ctr, depth, size, conf = [], [], [], [], []
        for l, t in enumerate(tower_out):
            i = l if self.use_per_level_predictors else 0
            q, c, d = self.box3d_quat[i](t), self.box3d_ctr[i](t), self.box3d_depth[i](t)
            s, k = self.box3d_size[i](t), self.box3d_conf[i](t)
            if self.use_scale:
                c, s, k = self.scales_proj_ctr[l](c), self.scales_size[l](s), self.scales_conf[l](k)
                d = self.offsets_depth[l](self.scales_depth[l](d))
            quat.append(q), ctr.append(c), depth.append(d), size.append(s), conf.append(k)
        return quat, ctr, depth, size, conf

    def forward(self, x):
        return (*self.predict(self.tower(x)), None)


# ---- the torch transcription of the reference's tail ----------------------------------------------------------------
def quaternion_to_matrix(q):
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def _copysign(a, b):
    return torch.where((a < 0) != (b < 0), -a, a)


def _sqrt_positive_part(x):
    return torch.sqrt(torch.where(x > 0, x, torch.zeros_like(x)))


def matrix_to_quaternion(m):
    m00, m11, m22 = m[..., 0, 0], m[..., 1, 1], m[..., 2, 2]
    o0 = 0.5 * _sqrt_positive_part(1 + m00 + m11 + m22)
    x = 0.5 * _sqrt_positive_part(1 + m00 - m11 - m22)
    y = 0.5 * _sqrt_positive_part(1 - m00 + m11 - m22)
    z = 0.5 * _sqrt_positive_part(1 - m00 - m11 + m22)
    return torch.stack((o0, _copysign(x, m[..., 2, 1] - m[..., 1, 2]), _copysign(y, m[..., 0, 2] - m[..., 2, 0]),
                        _copysign(z, m[..., 1, 0] - m[..., 0, 1])), -1)


def unproject_points2d(points2d, inv_K, scale=1.0):
    p = F.pad(points2d, (0, 1), value=1.0)
    return torch.matmul(inv_K, p.reshape(-1, 3).unsqueeze(-1)).reshape(p.shape) * scale


def allocentric_to_egocentric(quat, proj_ctr, inv_intrinsics):
    R_obj_to_local = quaternion_to_matrix(quat)
    ray = unproject_points2d(proj_ctr, inv_intrinsics)
    z = ray / torch.linalg.norm(ray, dim=1, keepdim=True)
    y = torch.tensor([[0.0, 1.0, 0.0]], dtype=z.dtype, device=z.device) - z[:, 1:2] * z
    y = y / torch.linalg.norm(y, dim=1, keepdim=True)
    x = torch.cross(y, z, dim=1)
    R_obj_to_global = torch.bmm(torch.stack([x, y, z], -1), R_obj_to_local)
    # (fcos3d_head.py:60-65 renormalises when a norm is off by more than 1e-3: a product of two rotations is not)
    return matrix_to_quaternion(R_obj_to_global)


def predictions_to_boxes3d(quat, proj_ctr, depth, size, locations, inv_intrinsics, canon_box_sizes, min_depth, max_depth,
                           scale_depth_by_focal_lengths_factor, scale_depth_by_focal_lengths=True,
                           quat_is_allocentric=True, depth_is_distance=False):
    quat = quat / torch.linalg.norm(quat, dim=1, keepdim=True).clamp(min=EPS)
    quat = quat / torch.linalg.norm(quat, dim=1, keepdim=True)
    if scale_depth_by_focal_lengths:
        pixel_size = torch.linalg.norm(torch.stack([inv_intrinsics[:, 0, 0], inv_intrinsics[:, 1, 1]], -1), dim=-1)
        depth = depth / (pixel_size * scale_depth_by_focal_lengths_factor)
    if depth_is_distance:
        depth = depth / torch.linalg.norm(unproject_points2d(locations, inv_intrinsics), dim=1).clamp(min=EPS)
    depth = depth.reshape(-1, 1).clamp(min_depth, max_depth)
    proj_ctr = proj_ctr + locations
    if quat_is_allocentric:
        quat = allocentric_to_egocentric(quat, proj_ctr, inv_intrinsics)
    size = (size.tanh() + 1.0) * canon_box_sizes
    return torch.cat([quat, proj_ctr, depth, size], -1)


def nms_by_category(boxes, iou_threshold, scores, category_idxs, categories):
    """paddle.vision.ops.nms with scores and categories, from its documented behaviour: greedy NMS per category in
    descending score, IoU = inter / (a + b - inter); the kept indices of all categories in descending score."""
    order = torch.argsort(scores, descending=True, stable=True)
    b, c = boxes[order], category_idxs[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt, rb = torch.maximum(b[:, None, :2], b[None, :, :2]), torch.minimum(b[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    iou = inter / (area[:, None] + area[None] - inter)
    hit = ((iou > iou_threshold) & (c[:, None] == c[None])).cpu()
    allowed = torch.isin(c.cpu(), torch.as_tensor(list(categories)))
    dead = torch.zeros(len(b), dtype=torch.bool)
    keep = []
    for i in range(len(b)):
        if dead[i] or not allowed[i]:
            continue
        keep.append(i)
        dead |= hit[i]
    return order[torch.as_tensor(keep, dtype=torch.long, device=order.device)]


class FCOS2DInference:
    """fcos2d_head.py:314-503."""

    def __init__(self, thresh_with_ctr=True, pre_nms_thresh=0.05, pre_nms_topk=1000, post_nms_topk=100, nms_thresh=0.75,
                 num_classes=5, nms_categories=5):
        self.thresh_with_ctr, self.pre_nms_thresh, self.pre_nms_topk = thresh_with_ctr, pre_nms_thresh, pre_nms_topk
        self.post_nms_topk, self.nms_thresh, self.num_classes = post_nms_topk, nms_thresh, num_classes
        self.nms_categories = nms_categories  # the reference passes categories=[0, 1, 2, 3, 4] whatever num_classes is

    def __call__(self, logits, box2d_reg, centerness, locations):
        pred_instances, extra_info = [], []
        for lvl, args in enumerate(zip(logits, box2d_reg, centerness, locations)):
            per_lvl, info = self.forward_for_single_feature_map(*args)
            for inst in per_lvl:
                inst["fpn_levels"] = torch.full((inst["pred_boxes"].shape[0],), float(lvl), dtype=torch.float64,
                                                device=inst["pred_boxes"].device)
            pred_instances.append(per_lvl)
            extra_info.append(info)
        return pred_instances, extra_info

    def forward_for_single_feature_map(self, logits, box2d_reg, centerness, locations):
        N, C = logits.shape[:2]
        scores = torch.sigmoid(logits.permute(0, 2, 3, 1).reshape(N, -1, C))
        box2d_reg = box2d_reg.permute(0, 2, 3, 1).reshape(N, -1, 4)
        centerness = torch.sigmoid(centerness.permute(0, 2, 3, 1).reshape(N, -1))
        if self.thresh_with_ctr:
            scores = scores * centerness[:, :, None]
        candidate_mask = scores > self.pre_nms_thresh
        if not self.thresh_with_ctr:
            scores = scores * centerness[:, :, None]
        results, all_fg, all_topk, all_cls = [], [], [], []
        for i in range(N):
            mask = candidate_mask[i]
            scores_per_im = scores[i][mask]
            inds = mask.nonzero()
            fg, cls = inds[:, 0], inds[:, 1]
            all_fg.append(fg), all_cls.append(cls)
            reg, loc = box2d_reg[i][fg], locations[fg]
            topk_indices = None
            if scores_per_im.shape[0] > self.pre_nms_topk:
                scores_per_im, topk_indices = scores_per_im.topk(self.pre_nms_topk, sorted=False)
                cls, reg, loc = cls[topk_indices], reg[topk_indices], loc[topk_indices]
            all_topk.append(topk_indices)
            boxes = torch.stack([loc[:, 0] - reg[:, 0], loc[:, 1] - reg[:, 1], loc[:, 0] + reg[:, 2],
                                 loc[:, 1] + reg[:, 3]], 1)
            results.append({"pred_boxes": boxes, "scores": torch.sqrt(scores_per_im), "pred_classes": cls,
                            "locations": loc})
        return results, {"fg_inds_per_im": all_fg, "class_inds_per_im": all_cls, "topk_indices": all_topk}

    def nms_and_top_k(self, instances_per_im, score_key_for_nms="scores"):
        results = []
        for inst in instances_per_im:
            if self.nms_thresh > 0 and inst["pred_boxes"].shape[0] > 0:
                keep = nms_by_category(inst["pred_boxes"], self.nms_thresh, inst[score_key_for_nms],
                                       inst["pred_classes"], range(self.nms_categories))
                inst = {k: v[keep] for k, v in inst.items()}
            n = inst["pred_boxes"].shape[0]
            if n > self.post_nms_topk > 0:
                scores = inst["scores"]
                thresh = torch.kthvalue(scores, n - self.post_nms_topk + 1).values
                keep = (scores >= thresh).nonzero().squeeze(1)
                inst = {k: v[keep] for k, v in inst.items()}
            results.append(inst)
        return results


class FCOS3DInference(nn.Module):
    """fcos3d_head.py:482-639."""

    def __init__(self, canon_box_sizes=CANON_BOX_SIZES, min_depth=0.1, max_depth=80.0, predict_allocentric_rot=True,
                 scale_depth_by_focal_lengths=True, scale_depth_by_focal_lengths_factor=500.0, predict_distance=False,
                 num_classes=5, class_agnostic=False):
        super().__init__()
        self.num_classes, self.class_agnostic, self.predict_distance = num_classes, class_agnostic, predict_distance
        self.canon_box_sizes, self.min_depth, self.max_depth = canon_box_sizes, min_depth, max_depth
        self.predict_allocentric_rot = predict_allocentric_rot
        self.scale_depth_by_focal_lengths_factor = scale_depth_by_focal_lengths_factor
        self.scale_depth_by_focal_lengths = scale_depth_by_focal_lengths

    def forward(self, box3d_quat, box3d_ctr, box3d_depth, box3d_size, box3d_conf, inv_intrinsics, pred_instances,
                fcos2d_info):
        for lvl, maps in enumerate(zip(box3d_quat, box3d_ctr, box3d_depth, box3d_size, box3d_conf)):
            self.forward_for_single_feature_map(*maps, inv_intrinsics, pred_instances[lvl], fcos2d_info[lvl])

    def forward_for_single_feature_map(self, quat, ctr, depth, size, conf, inv_intrinsics, pred_instances, info):
        N = quat.shape[0]
        ncp = 1 if self.class_agnostic else self.num_classes
        flat = lambda t, k: t.permute(0, 2, 3, 1).reshape(N, -1, k, ncp)  # noqa: E731
        quat, ctr, depth, size = flat(quat, 4), flat(ctr, 2), flat(depth, 1), flat(size, 3)
        conf = torch.sigmoid(flat(conf, 1))
        for i in range(N):
            fg, cls, topk = info["fg_inds_per_im"][i], info["class_inds_per_im"][i], info["topk_indices"][i]
            inst = pred_instances[i]
            cc = torch.zeros_like(cls) if self.class_agnostic else cls
            picked = [t[i][fg, :, cc] for t in (quat, ctr, depth, size, conf)]
            if topk is not None:
                picked = [t[topk] for t in picked]
            q, c, d, s, k = picked
            canon = torch.as_tensor(self.canon_box_sizes, dtype=q.dtype, device=q.device)[inst["pred_classes"]]
            inv_K = inv_intrinsics[i][None].expand(len(q), 3, 3)
            inst["pred_boxes3d"] = predictions_to_boxes3d(
                q, c, d[:, 0], s, inst["locations"], inv_K, canon, self.min_depth, self.max_depth,
                self.scale_depth_by_focal_lengths_factor, self.scale_depth_by_focal_lengths,
                self.predict_allocentric_rot, self.predict_distance)
            inst["scores_3d"] = inst["scores"] * k[:, 0]


def rows_to_instances(rows, counts):
    """The reference's per-image dicts from padded rows; reading the counts is the one host synchronisation."""
    out = []
    for r, n in zip(rows, counts.cpu().tolist()):
        r = r[:min(int(n), r.shape[0])]
        out.append({"pred_boxes": r[:, 0:4], "scores": r[:, 4], "scores_3d": r[:, 5], "pred_classes": r[:, 6].long(),
                    "fpn_levels": r[:, 7], "locations": r[:, 8:10], "pred_boxes3d": r[:, 10:20]})
    return out


class DD3D(nn.Module):
    """dd3d.py:32-212 at inference."""

    def __init__(self, backbone, feature_locations_offset, fpn, fcos2d_head, fcos2d_inference, fcos3d_head=None,
                 fcos3d_inference=None, do_nms=True, num_classes=5, pixel_mean=(103.53, 116.28, 123.675),
                 pixel_std=(57.375, 57.12, 58.395), input_strides=(8, 16, 32, 64, 128), size_divisibility=128,
                 fcos2d_loss=None, fcos3d_loss=None, prepare_targets=None, nusc_sample_aggregate=False,
                 pretrained=None, fused=True):
        super().__init__()
        self.backbone, self.fpn, self.feature_locations_offset = backbone, fpn, feature_locations_offset
        self.fcos2d_head, self.fcos2d_inference = fcos2d_head, fcos2d_inference
        self.fcos3d_head, self.fcos3d_inference = fcos3d_head, fcos3d_inference
        self.only_box2d = fcos3d_head is None
        self.do_nms, self.num_classes, self.fused = do_nms, num_classes, fused
        self.register_buffer("pixel_mean", torch.tensor(pixel_mean, dtype=torch.float32).reshape(1, -1, 1, 1))
        self.register_buffer("pixel_std", torch.tensor(pixel_std, dtype=torch.float32).reshape(1, -1, 1, 1))
        self.input_strides, self.size_divisibility = list(input_strides), size_divisibility

    def preprocess_image(self, x, size_divisibility=None):
        d = self.size_divisibility if size_divisibility is None else size_divisibility
        x = (x.float() - self.pixel_mean) / self.pixel_std
        h, w = x.shape[-2:]
        return F.pad(x, [0, (w + d - 1) // d * d - w, 0, (h + d - 1) // d * d - h], value=0.0)

    def compute_features_locations(self, h, w, stride, dtype=torch.float32, offset="none", device=None):
        shifts_x = torch.arange(0, w * stride, step=stride, dtype=dtype, device=device)
        shifts_y = torch.arange(0, h * stride, step=stride, dtype=dtype, device=device)
        shift_y, shift_x = torch.meshgrid(shifts_y, shifts_x, indexing="ij")
        locations = torch.stack((shift_x.reshape(-1), shift_y.reshape(-1)), 1)
        if offset == "half":
            locations = locations + stride // 2
        else:
            assert offset == "none"
        return locations

    def compute_locations(self, features):
        return [self.compute_features_locations(f.shape[-2], f.shape[-1], self.input_strides[l], f.dtype,
                                                self.feature_locations_offset, f.device)
                for l, f in enumerate(features)]

    # ---- the torch transcription ----------------------------------------------------------------------------------------
    def towers(self, features):
        """(cls_tower, box2d_tower, box3d_tower) outputs per level; the last None without a 3D head."""
        cls_out, box_out = self.fcos2d_head.towers(features)
        return cls_out, box_out, None if self.only_box2d else self.fcos3d_head.tower(features)

    def instances_torch(self, cls_out, box_out, box3d_out, intrinsics):
        """dd3d.py:115-176 from the towers' outputs: per-image instance dicts from the dense predictors."""
        locations = self.compute_locations(cls_out)
        logits, box2d_reg, centerness = self.fcos2d_head.predict(cls_out, box_out)
        pred_instances, info = self.fcos2d_inference(logits, box2d_reg, centerness, locations)
        score_key = "scores"
        if not self.only_box2d:
            maps = self.fcos3d_head.predict(box3d_out)
            self.fcos3d_inference(*maps, torch.linalg.inv(intrinsics.to(cls_out[0].dtype)), pred_instances, info)
            score_key = "scores_3d"
        cat = [{k: torch.cat([inst[k] for inst in per_im], 0) for k in per_im[0]} for per_im in zip(*pred_instances)]
        if self.only_box2d:  # (the reference's nms_and_top_k reads both keys; without a 3D head they are zero here)
            for inst in cat:
                inst["scores_3d"] = torch.zeros_like(inst["scores"])
                inst["pred_boxes3d"] = inst["pred_boxes"].new_zeros((len(inst["scores"]), 10))
        if self.do_nms:
            cat = self.fcos2d_inference.nms_and_top_k(cat, score_key)
        return cat

    def row_capacity(self):
        inf = self.fcos2d_inference
        cap = len(self.input_strides) * inf.pre_nms_topk
        return inf.post_nms_topk if (self.do_nms and inf.post_nms_topk > 0) else cap

    def padded_torch(self, cls_out, box_out, box3d_out, intrinsics):
        """(rows [B, R, 20], counts) in the kernels' form from the transcription."""
        cat = self.instances_torch(cls_out, box_out, box3d_out, intrinsics)
        R, dev, dt = self.row_capacity(), cls_out[0].device, cls_out[0].dtype
        rows = torch.zeros((len(cat), R, 20), dtype=dt, device=dev)
        counts = torch.zeros((len(cat),), dtype=torch.int32, device=dev)
        for b, inst in enumerate(cat):
            n = inst["scores"].shape[0]
            r = torch.cat([inst["pred_boxes"], inst["scores"][:, None], inst["scores_3d"][:, None],
                           inst["pred_classes"][:, None].to(dt), inst["fpn_levels"][:, None].to(dt), inst["locations"],
                           inst["pred_boxes3d"]], 1)
            rows[b, :min(n, R)] = r[:R]
            counts[b] = n
        return rows, counts

    # ---- the device path ------------------------------------------------------------------------------------------------
    def op_config(self):
        i2, i3 = self.fcos2d_inference, self.fcos3d_inference
        cfg = dict(thresh_with_ctr=i2.thresh_with_ctr, pre_nms_thresh=i2.pre_nms_thresh, pre_nms_topk=i2.pre_nms_topk,
                   post_nms_topk=i2.post_nms_topk, nms_thresh=i2.nms_thresh, nms_categories=i2.nms_categories,
                   offset=self.feature_locations_offset)
        if i3 is not None:
            cfg.update(min_depth=i3.min_depth, max_depth=i3.max_depth, predict_allocentric_rot=i3.predict_allocentric_rot,
                       scale_depth_by_focal_lengths=i3.scale_depth_by_focal_lengths,
                       scale_depth_by_focal_lengths_factor=i3.scale_depth_by_focal_lengths_factor,
                       predict_distance=i3.predict_distance)
        return cfg

    def device_supported(self, features):
        i2 = self.fcos2d_inference
        ok = (self.do_nms and all(f.is_cuda and f.dtype == torch.float32 for f in features) and
              len(features) == len(self.input_strides) and
              dd3d_ops.dd3d_supported([tuple(f.shape[-2:]) for f in features], self.fcos2d_head.num_classes,
                                      i2.pre_nms_topk, i2.nms_thresh, self.fcos2d_head.channels))
        if ok and not self.only_box2d:
            ok = len(self.fcos3d_inference.canon_box_sizes) >= self.fcos2d_head.num_classes
        return ok

    def packed(self, device):
        """The lazy entry point's predictor arrays: box2d weight / bias, the stacked 3D predictors, the per-level scales."""
        h2, h3 = self.fcos2d_head, self.fcos3d_head
        L = len(self.input_strides)
        # what build() reads and nothing more: a signature over `self` would walk the whole backbone on every forward
        sources = [h2.box2d_reg, h2.scales if h2.use_scale else None]
        if h3 is not None:
            groups = (h3.box3d_quat, h3.box3d_ctr, h3.box3d_depth, h3.box3d_size, h3.box3d_conf)
            sources += groups
            if h3.use_scale:
                sources += [h3.scales_proj_ctr, h3.scales_size, h3.scales_conf, h3.scales_depth, h3.offsets_depth]

        def build():
            scales = torch.ones((L, 6), dtype=torch.float32, device=device)
            scales[:, 5] = 0
            if h2.use_scale:
                scales[:, 0] = torch.cat([s.scale for s in h2.scales]).float()
            p = dict(w2d=h2.box2d_reg.weight.float().contiguous(), b2d=h2.box2d_reg.bias.float().contiguous(),
                     w3d=None, b3d=None, canon=None)
            if h3 is not None:
                use = range(len(h3.box3d_quat)) if h3.use_per_level_predictors else (0,)
                p["w3d"] = torch.stack([torch.cat([g[i].weight for g in groups]) for i in use]).float().contiguous()
                p["b3d"] = torch.stack([torch.cat([g[i].bias if g[i].bias is not None else
                                                   g[i].weight.new_zeros(g[i].weight.shape[0]) for g in groups])
                                        for i in use]).float().contiguous()
                if h3.use_scale:
                    for col, group in enumerate((h3.scales_proj_ctr, h3.scales_size, h3.scales_conf, h3.scales_depth), 1):
                        scales[:, col] = torch.cat([s.scale for s in group]).float()[:L]
                    scales[:, 5] = torch.cat([o.bias for o in h3.offsets_depth]).float()[:L]
                p["canon"] = torch.tensor(self.fcos3d_inference.canon_box_sizes, dtype=torch.float32, device=device)
            p["scales"] = scales
            return p
        return derived(self, "packed", build, sources=sources, key=device)

    def tail_padded(self, cls_out, box_out, box3d_out, intrinsics=None, fused=None):
        """(rows [B, R, 20], counts int32 [B]) from the towers' outputs, no host synchronisation on the device paths.
        fused: True (LAZY_BY_DEFAULT decides between the two device paths), "lazy", "dense" or False (torch)."""
        fused = self.fused if fused is None else fused
        if fused and self.device_supported(cls_out):
            lazy = fused == "lazy" or (fused is True and LAZY_BY_DEFAULT)
            h2, h3, cfg = self.fcos2d_head, self.fcos3d_head, self.op_config()
            K = None if self.only_box2d else intrinsics.float()
            p = self.packed(cls_out[0].device)
            if lazy:
                out = dd3d_ops.dd3d_head_forward([h2.cls_logits(t) for t in cls_out], [h2.centerness(t) for t in box_out],
                                                 box_out, box3d_out, self.input_strides, p["w2d"], p["b2d"], p["w3d"],
                                                 p["b3d"], p["scales"], K, p["canon"], **cfg)
            else:
                logits, box2d_reg, centerness = h2.predict(cls_out, box_out)
                out = dd3d_ops.dd3d_post_process(logits, centerness, box2d_reg, None if h3 is None else h3.predict(box3d_out),
                                                 self.input_strides, K, p["canon"], **cfg)
            if out is not None:
                return out
        return self.padded_torch(cls_out, box_out, box3d_out, intrinsics)

    def head_padded(self, features, intrinsics=None, fused=None):
        """tail_padded from the FPN's features (the three towers run densely in every form)."""
        return self.tail_padded(*self.towers(list(features)), intrinsics, fused)

    def features(self, images):
        x = self.fpn(self.backbone(images))
        return [x[k] for k in x.keys()] if isinstance(x, dict) else list(x)

    def forward(self, samples, fused=None):
        with torch.no_grad():
            images = self.preprocess_image(samples["data"], self.size_divisibility)
            rows, counts = self.head_padded(self.features(images), samples["meta"]["camera_intrinsic"], fused)
            return {"preds": rows_to_instances(rows, counts)}
