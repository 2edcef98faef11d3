"""PV-RCNN's keypoint branch at inference on the device ops (configs/pv_rcnn/pv_rcnn_005voxel_kitti.yml).

VoxelSetAbstraction(model_cfg, voxel_size, point_cloud_range, num_bev_features, num_rawpoint_features, fused=False)
                                               models/point_encoders/voxel_set_abstraction.py:112-424 with the
                                               reference's constructor arguments and sublayer names (sa_layers,
                                               sa_rawpoints, vsa_point_feature_fusion).  forward(batch_dict): batch_size,
                                               points [N, 1 + 3 + C] as (b, x, y, z, ...) with the frames' rows
                                               contiguous, the per-frame point counts as host values (points_batch_cnt,
                                               a list of ints, or data, the per-frame arrays whose shapes are read),
                                               spatial_features [B, C, H, W], spatial_features_stride,
                                               multi_scale_3d_features (SparseConvTensor per source) ->
                                               point_features_before_fusion, point_features, point_coords,
                                               sparse_rows_frame_contiguous (see below).
PointHeadSimple(num_class, input_channels, model_cfg)
                                               models/heads/dense_heads/point_head.py:32-128 (cls_layers):
                                               point_cls_preds, point_cls_scores = max over sigmoid.
PVRCNNSecondStage(point_encoder, point_head, roi_head)
                                               the three modules under PVRCNN's attribute names
                                               (detection/pv_rcnn/pv_rcnn.py:37-80); forward chains them.

Inference only: training (targets, losses) raises, as do filter_neighbor_with_roi, point_source != 'raw_points' and
sample_method != 'FPS' (the config uses none of them).  Nothing in the forwards synchronises with the host: the batch
counts are a device index_add_ over the batch column, the per-frame point counts that slice `points` for the farthest
point sampling are host values.

Rows of a sparse tensor: sparse.py's producers emit them in raster order (b, z, y, x), so the rows of a frame are
contiguous and the rows past n_dev (a plan made at a remembered capacity) are at the end, where the counts leave them
out.  The ball queries depend on that order: with rows of one frame scattered among another's, the per-frame counts
address the wrong rows and the pooled features are WRONG WITHOUT AN ERROR.  forward checks it on the device and
leaves the answer in batch_dict["sparse_rows_frame_contiguous"] (a 0-dim bool tensor: reading it is the caller's
host sync, at a time of the caller's choosing; forward itself cannot raise on it without one).  For a producer that
does not keep the order, sort_rows=True orders the rows by a stable device sort on the batch column first (uncounted
rows last); the flag is then True by construction.
"""
from __future__ import annotations

import copy

import numpy as np
import torch
from torch import nn

from .ops import pointnet2_ops, pvrcnn
from .pointnet2_stack import build_local_aggregation_module

__all__ = ["VoxelSetAbstraction", "PointHeadSimple", "PVRCNNSecondStage", "batch_counts", "voxel_centers"]


def batch_counts(batch_col, batch_size, valid=None):
    """[batch_size] int32 on the device: rows per frame of a batch column (float or int), without a host sync; rows
    with valid == False or a frame outside [0, batch_size) are left out."""
    b = batch_col.long()
    ok = (b >= 0) & (b < batch_size)
    if valid is not None:
        ok = ok & valid
    slot = torch.where(ok, b, torch.full_like(b, batch_size))
    cnt = torch.zeros(batch_size + 1, dtype=torch.int32, device=b.device)
    cnt.index_add_(0, slot, torch.ones_like(slot, dtype=torch.int32))
    return cnt[:batch_size]


def voxel_centers(indices, voxel_size, point_cloud_range, stride):
    """get_voxel_centers (models/common/box_utils.py:76-99) for indices [N, 4] as (b, z, y, x): (xyz + 0.5) *
    (voxel_size * stride) + range_min in fp32, column by column with host scalars (a list copied to the device would
    synchronise)."""
    cols = []
    for a, col in enumerate((3, 2, 1)):  # x, y, z
        size = float(np.float32(voxel_size[a]) * np.float32(stride))
        lo = float(np.float32(point_cloud_range[a]))
        cols.append((indices[:, col].to(torch.float32) + 0.5) * size + lo)
    return torch.stack(cols, dim=1)


def _host_counts(batch_dict):
    if batch_dict.get("points_batch_cnt", None) is not None:
        cnt = batch_dict["points_batch_cnt"]
        if isinstance(cnt, torch.Tensor):
            raise TypeError("points_batch_cnt must be host integers (a device tensor would synchronise)")
        return [int(c) for c in cnt]
    if batch_dict.get("data", None) is not None:
        return [int(d.shape[0]) for d in batch_dict["data"]]
    raise KeyError("VoxelSetAbstraction: the per-frame point counts (points_batch_cnt or data) are missing")


class VoxelSetAbstraction(nn.Module):
    def __init__(self, model_cfg, voxel_size, point_cloud_range, num_bev_features=None, num_rawpoint_features=None,
                 fused=False, sort_rows=False, **kwargs):
        super().__init__()
        model_cfg = copy.deepcopy(model_cfg)  # the reference prepends the input channels to cfg["mlps"] in place
        self.model_cfg = model_cfg
        self.voxel_size = [float(v) for v in voxel_size]
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.sort_rows = bool(sort_rows)
        if model_cfg["point_source"] != "raw_points":
            raise NotImplementedError(f"point_source {model_cfg['point_source']!r}")
        if model_cfg["sample_method"] != "FPS":
            raise NotImplementedError(f"sample_method {model_cfg['sample_method']!r}")
        sa_cfg = model_cfg["sa_layer"]
        for name, cfg in sa_cfg.items():
            if cfg.get("filter_neighbor_with_roi", False):
                raise NotImplementedError(f"sa_layer.{name}.filter_neighbor_with_roi")

        self.sa_layers = nn.ModuleList()
        self.sa_layer_names = []
        self.downsample_stride_map = {}
        c_in = 0
        for src_name in model_cfg["features_source"]:
            if src_name in ("bev", "raw_points"):
                continue
            self.downsample_stride_map[src_name] = sa_cfg[src_name]["downsample_stride"]
            if sa_cfg[src_name].get("in_channels", None) is None:
                first = sa_cfg[src_name]["mlps"][0]
                input_channels = first[0] if isinstance(first, list) else first
            else:
                input_channels = sa_cfg[src_name]["in_channels"]
            layer, c_out = build_local_aggregation_module(input_channels=input_channels, config=sa_cfg[src_name],
                                                          fused=fused)
            self.sa_layers.append(layer)
            self.sa_layer_names.append(src_name)
            c_in += c_out
        if "bev" in model_cfg["features_source"]:
            c_in += num_bev_features
        self.num_rawpoint_features = num_rawpoint_features
        if "raw_points" in model_cfg["features_source"]:
            self.sa_rawpoints, c_out = build_local_aggregation_module(input_channels=num_rawpoint_features - 3,
                                                                      config=sa_cfg["raw_points"], fused=fused)
            c_in += c_out
        out = model_cfg["out_channels"]
        self.vsa_point_feature_fusion = nn.Sequential(nn.Linear(c_in, out, bias=False), nn.BatchNorm1d(out), nn.ReLU())
        self.num_point_features = out
        self.num_point_features_before_fusion = c_in

    def interpolate_from_bev_features(self, keypoints, bev_features, batch_size, bev_stride):
        """keypoints [M, 4], bev_features [B, C, H, W] -> [M, C], every frame in one launch."""
        assert int(bev_features.shape[0]) == int(batch_size)
        return pvrcnn.bev_interpolate(keypoints, bev_features.float(), self.point_cloud_range, self.voxel_size,
                                      bev_stride)

    def get_sampled_points(self, batch_dict):
        """keypoints [B * num_keypoints, 4] as (b, x, y, z): farthest point sampling per frame; a frame with fewer
        points than num_keypoints repeats its samples (the reference's tile)."""
        batch_size = int(batch_dict["batch_size"])
        K = int(self.model_cfg["num_keypoints"])
        points = batch_dict["points"]
        counts = _host_counts(batch_dict)
        if len(counts) != batch_size or sum(counts) != int(points.shape[0]):
            raise RuntimeError(f"VoxelSetAbstraction: point counts {counts} for {int(points.shape[0])} rows of "
                               f"{batch_size} frames")
        out, start = [], 0
        for b, n in enumerate(counts):
            src = points[start:start + n, 1:4].contiguous()
            start += n
            idx = pointnet2_ops.farthest_point_sample(src.unsqueeze(0), K)[0].long()
            if n < K:
                times = int(K / n) + 1
                idx = idx[:n].repeat(times)[:K]
            out.append(torch.cat([torch.full((K, 1), float(b), dtype=torch.float32, device=src.device), src[idx]],
                                 dim=1))
        return torch.cat(out, dim=0)

    def _sparse_source(self, sp, batch_size, stride):
        """(xyz [N, 3], features [N, C], xyz_batch_cnt [B], contiguous) of a SparseConvTensor.  Rows past n_dev or of no
        frame count nowhere.  contiguous: a 0-dim bool on the device, whether the rows as they are used are ordered by
        frame with the uncounted rows last -- what the counts need to mean the rows they are meant for."""
        ind, feats = sp.indices, sp.features.float()
        N = int(ind.shape[0])
        rows = torch.arange(N, dtype=torch.int32, device=ind.device)
        b = ind[:, 0].long()
        ok = (b >= 0) & (b < batch_size)
        if sp.n_dev is not None:
            ok = ok & (rows < sp.n_dev.reshape(-1)[:1].to(torch.int32))
        key = torch.where(ok, b, torch.full_like(b, batch_size))  # uncounted rows sort behind every frame
        if self.sort_rows:
            key, order = torch.sort(key, stable=True)
            ind, feats, ok = ind[order], feats[order], ok[order]
        contiguous = (key[1:] >= key[:-1]).all()
        cnt = batch_counts(ind[:, 0], batch_size, ok)
        return voxel_centers(ind, self.voxel_size, self.point_cloud_range, stride), feats, cnt, contiguous

    def forward(self, batch_dict):
        if self.training:
            raise NotImplementedError("VoxelSetAbstraction: inference only")
        batch_size = int(batch_dict["batch_size"])
        keypoints = self.get_sampled_points(batch_dict)
        sources = self.model_cfg["features_source"]
        feats = []
        if "bev" in sources:
            feats.append(self.interpolate_from_bev_features(keypoints, batch_dict["spatial_features"], batch_size,
                                                            bev_stride=batch_dict["spatial_features_stride"]))
        new_xyz = keypoints[:, 1:4].contiguous()
        new_cnt = torch.full((batch_size,), int(self.model_cfg["num_keypoints"]), dtype=torch.int32,
                             device=keypoints.device)
        if "raw_points" in sources:
            raw = batch_dict["points"]
            _, pooled = self.sa_rawpoints(
                xyz=raw[:, 1:4].contiguous(), xyz_batch_cnt=batch_counts(raw[:, 0], batch_size), new_xyz=new_xyz,
                new_xyz_batch_cnt=new_cnt,
                features=raw[:, 4:].contiguous() if self.num_rawpoint_features > 3 else None)
            feats.append(pooled)
        ordered = []
        for k, src_name in enumerate(self.sa_layer_names):
            xyz, f, cnt, contiguous = self._sparse_source(batch_dict["multi_scale_3d_features"][src_name], batch_size,
                                              self.downsample_stride_map[src_name])
            _, pooled = self.sa_layers[k](xyz=xyz, xyz_batch_cnt=cnt, new_xyz=new_xyz, new_xyz_batch_cnt=new_cnt,
                                          features=f)
            feats.append(pooled)
            ordered.append(contiguous)
        if ordered:
            batch_dict["sparse_rows_frame_contiguous"] = torch.stack(ordered).all()
        point_features = torch.cat(feats, dim=-1)
        batch_dict["point_features_before_fusion"] = point_features
        batch_dict["point_features"] = self.vsa_point_feature_fusion(point_features)
        batch_dict["point_coords"] = keypoints
        return batch_dict


class PointHeadSimple(nn.Module):
    def __init__(self, num_class, input_channels, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class if not model_cfg["class_agnostic"] else 1
        layers, c_in = [], input_channels
        for w in model_cfg["cls_fc"]:
            layers += [nn.Linear(c_in, w, bias=False), nn.BatchNorm1d(w), nn.ReLU()]
            c_in = w
        layers.append(nn.Linear(c_in, self.num_class, bias=True))
        self.cls_layers = nn.Sequential(*layers)

    def forward(self, batch_dict):
        if self.training:
            raise NotImplementedError("PointHeadSimple: inference only (targets and losses are not built)")
        key = ("point_features_before_fusion" if self.model_cfg.get("use_point_features_before_fusion", False)
               else "point_features")
        preds = self.cls_layers(batch_dict[key])
        self.forward_ret_dict = {"point_cls_preds": preds}
        batch_dict["point_cls_scores"] = torch.sigmoid(preds).max(dim=-1).values
        return batch_dict


class PVRCNNSecondStage(nn.Module):
    def __init__(self, point_encoder, point_head, roi_head):
        super().__init__()
        self.point_encoder, self.point_head, self.roi_head = point_encoder, point_head, roi_head

    def forward(self, batch_dict):
        return self.roi_head(self.point_head(self.point_encoder(batch_dict)))
