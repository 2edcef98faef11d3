"""Voxel R-CNN and PV-RCNN from points to boxes: the reference's two KITTI two-stage detectors assembled from the
library's stages, inference only.

VoxelRCNN(num_class, voxelizer, voxel_encoder, middle_encoder, backbone, neck, dense_head, roi_head, post_process_cfg)
                                               models/detection/voxel_rcnn/voxel_rcnn.py:33-108, 145-220
PVRCNN(num_class, voxelizer, voxel_encoder, middle_encoder, point_encoder, backbone, neck, dense_head, point_head,
       roi_head, post_process_cfg)             models/detection/pv_rcnn/pv_rcnn.py:33-113, 151-220
    with the reference's constructor arguments and attribute names, so checkpoint.load_paddle_state_dict(model, path,
    strict=True) places every key of a reference checkpoint.  forward(points): a list of [N_i, 4] device tensors, one
    per frame (the reference's batch_dict['data']) -> per frame {box3d_lidar [K, 7], scores [K], label_preds [K]}, the
    reference's pred_dicts.  forward builds batch_dict as the reference does (data, batch_size, voxel_coords, points
    with the batch index in front) and runs the stages in its order: voxelizer -> voxel encoder -> SparseNet3D ->
    SecondBackbone -> SecondFPN -> AnchorHeadSingle -> (PV-RCNN: VoxelSetAbstraction -> PointHeadSimple ->) RoI head ->
    roi_heads.post_processing.  The models add no arithmetic of their own: the same stages run by hand give the same
    bits (up to the RoI heads' fully connected stacks, torch GEMMs whose last bits depend on the batch's row count and,
    for PV-RCNN's Conv1d form, on the run: DESIGN 4.5zd).  The voxelizer's padded [B, V, ...] output and its batch
    column (-1 on padding rows) go to VoxelMean and SparseNet3D as they are, as CenterPoint feeds SparseResNet3D: no
    row is cut on the host.

    Host synchronisations of one forward: 2.  SparseNet3D plans its index sets at their exact sizes (one read), and
    post_processing reads the per-frame counts to cut the padded result (one read; forward(points, padded=True) returns
    post_processing's padded tensors instead and leaves only the plan's).  The assembly itself adds none: the frames'
    point counts reach the device as fills, not as a copy of a host list.

to_kitti_detections(pred_dicts)                _parse_results_to_sample + _convert_origin_for_eval (voxel_rcnn.py:222-249):
                                               (w, l) swapped, the angle convention turned, the box origin moved from the
                                               centre to the bottom face, labels 0-based: what
                                               kitti_bridge.detections_to_kitti_annos takes.
voxel_rcnn_005voxel_kitti_car(fused=None, point_cloud_range=None)
                                               configs/voxel_rcnn/voxel_rcnn_005voxel_kitti_car.yml
pv_rcnn_005voxel_kitti(fused=None, point_cloud_range=None)
                                               configs/pv_rcnn/pv_rcnn_005voxel_kitti.yml
    random init.  fused: AnchorHeadSingle's (None = its measured default, True, False, "force"); where it is not None
    the second stage's fused pools follow it as well (VoxelRCNNHead(fused_pool=), pv_rcnn's fused=).  point_cloud_range
    replaces the KITTI range [0, -40, -3, 70.4, 40, 1] (the tests shrink x / y; z stays [-3, 1]: SparseNet3D's depth
    chain 41 -> 21 -> 11 -> 5 -> 2 is what makes the 256-channel BEV map).

Not built: training (targets, losses), export mode, multi-class NMS (the reference raises there too).  A frame
without a point runs through VoxelRCNN; PV-RCNN's keypoint sampling divides by the frame's point count, in the
reference as here, so PVRCNN wants at least one point per frame (they may all lie outside the range).  A batch in
which NO frame has a voxel is refused by VoxelRCNNHead's pool layers (a Conv1d over zero rows); one such frame next to
others is served.
"""
from __future__ import annotations

import copy

import numpy as np
import torch
from torch import nn

from . import roi_heads as _rh
from .anchor_head import AnchorHeadSingle
from .centerpoint import HardVoxelizer, SecondBackbone, SecondFPN, VoxelMean, invalidate_derived
from .pv_rcnn import PointHeadSimple, PVRCNNSecondStage, VoxelSetAbstraction
from .sparse import SparseNet3D

__all__ = ["VoxelRCNN", "PVRCNN", "to_kitti_detections", "voxel_rcnn_005voxel_kitti_car", "pv_rcnn_005voxel_kitti",
           "KITTI_RANGE", "KITTI_VOXEL", "ANCHOR_HEAD_MODEL_CFG", "CAR_ANCHOR_CFG", "KITTI_ANCHOR_CFG"]

KITTI_RANGE = [0, -40, -3, 70.4, 40, 1]
KITTI_VOXEL = [0.05, 0.05, 0.1]
ANCHOR_HEAD_MODEL_CFG = {"use_direction_classifier": True, "dir_offset": 0.78539, "dir_limit_offset": 0.0}
ANCHOR_TARGET_CFG = {"pos_fraction": -1.0, "sample_size": 512, "norm_by_num_examples": False, "match_height": False}
ANCHOR_LOSS_WEIGHTS = {"cls_weight": 1.0, "loc_weight": 2.0, "dir_weight": 0.2, "code_weights": [1.0] * 7}


def _anchors(name, size, height, matched, unmatched):
    return {"class_name": name, "anchor_sizes": [size], "anchor_rotations": [0, 1.57],
            "anchor_bottom_heights": [height], "align_center": False, "feature_map_stride": 8,
            "matched_threshold": matched, "unmatched_threshold": unmatched}


CAR_ANCHOR_CFG = [_anchors("Car", [3.9, 1.6, 1.56], -1.78, 0.6, 0.45)]
KITTI_ANCHOR_CFG = [CAR_ANCHOR_CFG[0], _anchors("Pedestrian", [0.8, 0.6, 1.73], -0.6, 0.5, 0.35),
                    _anchors("Cyclist", [1.76, 0.6, 1.73], -0.6, 0.5, 0.35)]


class _TwoStage(nn.Module):
    """What the two models share: the first stage up to the dense head, and the end."""

    def _first_stage(self, points):
        if self.training:
            raise NotImplementedError(f"{type(self).__name__}: inference only (targets and losses are not built)")
        points = list(points)
        batch_dict = {"data": points, "batch_size": len(points)}
        dev, dim = points[0].device, int(points[0].shape[1])
        counts = [int(p.shape[0]) for p in points]
        # the reference's voxelizer walks the frames; the library's takes them at once, padded to the longest, with
        # the frames' point counts (device fills: a tensor made from the host list would be a synchronising copy)
        padded = torch.zeros((len(points), max(max(counts), 1), dim), dtype=torch.float32, device=dev)
        for b, p in enumerate(points):
            padded[b, :counts[b]] = p
        lens = torch.cat([torch.full((1,), n, dtype=torch.int32, device=dev) for n in counts])
        voxels, coors, npv, _ = self.voxelizer(padded, lens)
        b, v, p, d = (int(s) for s in voxels.shape)
        batch_dict["voxel_coords"] = coors.view(b * v, 4)
        batch_dict["points"] = torch.cat([nn.functional.pad(pt, (1, 0), value=float(i)) for i, pt in enumerate(points)])
        voxel_features = self.voxel_encoder(voxels.view(b * v, p, d), npv.view(b * v))
        middle_out = self.middle_encoder(voxel_features, batch_dict["voxel_coords"], batch_dict["batch_size"])
        batch_dict.update(middle_out)
        backbone_out = self.backbone(middle_out["spatial_features"])
        batch_dict["spatial_features_2d"] = self.neck(backbone_out)
        return self.dense_head(batch_dict)

    def _second_stage(self, batch_dict):
        raise NotImplementedError

    def post_processing(self, batch_dict, padded=False):
        return _rh.post_processing(batch_dict, self.post_process_cfg, self.num_class, padded=padded)

    @torch.no_grad()
    def forward(self, points, padded=False):
        return self.post_processing(self._second_stage(self._first_stage(points)), padded=padded)

    def invalidate(self):
        """Rebuild every folded / packed weight on the next forward (after a write through `param.data`)."""
        invalidate_derived(self)
        return self


class VoxelRCNN(_TwoStage):
    def __init__(self, num_class, voxelizer, voxel_encoder, middle_encoder, backbone, neck, dense_head, roi_head,
                 post_process_cfg):
        super().__init__()
        self.num_class = num_class
        self.voxelizer = voxelizer
        self.voxel_encoder = voxel_encoder
        self.middle_encoder = middle_encoder
        self.backbone = backbone
        self.neck = neck
        self.dense_head = dense_head
        self.roi_head = roi_head
        self.post_process_cfg = post_process_cfg

    def _second_stage(self, batch_dict):
        return self.roi_head(batch_dict)


class PVRCNN(_TwoStage):
    def __init__(self, num_class, voxelizer, voxel_encoder, middle_encoder, point_encoder, backbone, neck, dense_head,
                 point_head, roi_head, post_process_cfg):
        super().__init__()
        self.num_class = num_class
        self.voxelizer = voxelizer
        self.voxel_encoder = voxel_encoder
        self.middle_encoder = middle_encoder
        self.point_encoder = point_encoder
        self.backbone = backbone
        self.neck = neck
        self.dense_head = dense_head
        self.point_head = point_head
        self.roi_head = roi_head
        self.post_process_cfg = post_process_cfg
        # the chain of the three modules above, kept off the module tree: its parameters are already named once, under
        # the reference's attribute names
        object.__setattr__(self, "second_stage", PVRCNNSecondStage(point_encoder, point_head, roi_head))

    def _second_stage(self, batch_dict):
        return self.second_stage(batch_dict)


def to_kitti_detections(pred_dicts):
    """pred_dicts as the models return them -> per frame dict(box3d_lidar [K, 7] (x, y, z bottom, w, l, h, r), scores,
    label_preds 0-based) in NumPy; a frame's box_empty row keeps its score -1, which the bridge drops."""
    out = []
    for det in pred_dicts:
        box = det["box3d_lidar"].detach().cpu().numpy().astype(np.float32).reshape(-1, 7).copy()
        box[..., 3:5] = box[..., [4, 3]]
        box[..., -1] = -(box[..., -1] + np.pi / 2.)
        box[:, :3] += box[:, 3:6] * (np.array([.5, .5, 0]) - np.array([.5, .5, .5]))  # origin (.5, .5, .5) -> (.5, .5, 0)
        out.append({"box3d_lidar": box, "scores": det["scores"].detach().cpu().numpy(),
                    "label_preds": det["label_preds"].detach().cpu().numpy() - 1})
    return out


def _second_fused(fused):
    return None if fused is None else bool(fused)


def _dense_head(channels, class_names, anchor_cfg, pcr, fused):
    return AnchorHeadSingle(model_cfg=dict(ANCHOR_HEAD_MODEL_CFG), input_channels=channels, class_names=class_names,
                            voxel_size=KITTI_VOXEL, point_cloud_range=pcr, anchor_target_cfg=dict(ANCHOR_TARGET_CFG),
                            predict_boxes_when_training=True, anchor_generator_cfg=copy.deepcopy(anchor_cfg),
                            num_dir_bins=2, loss_weights=copy.deepcopy(ANCHOR_LOSS_WEIGHTS), fused=fused)


def voxel_rcnn_005voxel_kitti_car(fused=None, point_cloud_range=None) -> VoxelRCNN:
    pcr = list(KITTI_RANGE) if point_cloud_range is None else [float(v) for v in point_cloud_range]
    vs = KITTI_VOXEL
    return VoxelRCNN(
        num_class=1,
        voxelizer=HardVoxelizer(vs, pcr, 5, [16000, 40000]),
        voxel_encoder=VoxelMean(4),
        middle_encoder=SparseNet3D(4, vs, pcr),
        backbone=SecondBackbone(256, (64, 128), (5, 5), (1, 2)),
        neck=SecondFPN((64, 128), (128, 128), (1, 2), use_conv_for_no_stride=False),
        dense_head=_dense_head(256, ["Car"], CAR_ANCHOR_CFG, pcr, fused),
        roi_head=_rh.VoxelRCNNHead(input_channels={"x_conv1": 16, "x_conv2": 32, "x_conv3": 64, "x_conv4": 64},
                                   model_cfg=_rh.KITTI_CAR_MODEL_CFG, point_cloud_range=pcr, voxel_size=vs,
                                   num_class=1, fused_pool=_second_fused(fused)),
        post_process_cfg=copy.deepcopy(_rh.KITTI_CAR_POST_PROCESS_CFG))


def pv_rcnn_005voxel_kitti(fused=None, point_cloud_range=None) -> PVRCNN:
    pcr = list(KITTI_RANGE) if point_cloud_range is None else [float(v) for v in point_cloud_range]
    vs = KITTI_VOXEL
    sa_fused = _rh.FUSED_SA_DEFAULT if fused is None else bool(fused)
    encoder = VoxelSetAbstraction(_rh.PV_RCNN_KITTI_POINT_ENCODER_CFG, vs, pcr, num_bev_features=256,
                                  num_rawpoint_features=4, fused=sa_fused)
    return PVRCNN(
        num_class=3,
        voxelizer=HardVoxelizer(vs, pcr, 5, [16000, 40000]),
        voxel_encoder=VoxelMean(4),
        middle_encoder=SparseNet3D(4, vs, pcr),
        point_encoder=encoder,
        backbone=SecondBackbone(256, (128, 256), (5, 5), (1, 2)),
        neck=SecondFPN((128, 256), (256, 256), (1, 2), use_conv_for_no_stride=False),
        dense_head=_dense_head(512, ["Car", "Pedestrian", "Cyclist"], KITTI_ANCHOR_CFG, pcr, fused),
        point_head=PointHeadSimple(num_class=3, input_channels=encoder.num_point_features_before_fusion,
                                   model_cfg=_rh.PV_RCNN_KITTI_POINT_HEAD_CFG),
        roi_head=_rh.PVRCNNHead(input_channels=encoder.num_point_features, model_cfg=_rh.PV_RCNN_KITTI_ROI_HEAD_CFG,
                                num_class=1, fused=sa_fused),
        post_process_cfg=copy.deepcopy(_rh.PV_RCNN_KITTI_POST_PROCESS_CFG))
