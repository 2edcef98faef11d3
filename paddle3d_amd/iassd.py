"""IA-SSD's grouping and sampling on the device ops (paddle3d_amd/ops/pointnet2_ops.py).

QueryAndGroup(radius, nsample, use_xyz)   mirrors iassd_modules.py:29-60: ball query, group xyz relative to the
                                          centre, group features, concat [xyz, features] along channels.
sample_points(xyz, npoint, sample_type, cls_features=None)
                                          the sampling branch of SAModuleMSG_WithSampling.forward
                                          (iassd_modules.py:174-200): no downsample when N <= npoint, D-FPS, or
                                          ctr_aware (sigmoid of the class maximum, then torch.topk); returns
                                          (sample_idx [B, npoint] int32, new_xyz [B, npoint, 3]).
No host synchronisation on either path.
"""
from __future__ import annotations

import torch

from .ops import pointnet2_ops

__all__ = ["QueryAndGroup", "sample_points"]


class QueryAndGroup(torch.nn.Module):
    def __init__(self, radius: float, nsample: int, use_xyz: bool = True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz, new_xyz, features=None):
        """xyz [B, N, 3], new_xyz [B, npoint, 3], features [B, C, N] or None -> [B, 3 + C, npoint, nsample]
        ([B, C, ...] without use_xyz)."""
        idx = pointnet2_ops.ball_query_batch(new_xyz, xyz, self.radius, self.nsample)
        grouped_xyz = pointnet2_ops.grouping_operation_batch(xyz.transpose(1, 2), idx)
        grouped_xyz = grouped_xyz - new_xyz.transpose(1, 2).unsqueeze(-1)
        if features is not None:
            grouped_features = pointnet2_ops.grouping_operation_batch(features, idx)
            if self.use_xyz:
                return torch.cat([grouped_xyz, grouped_features], dim=1)
            return grouped_features
        if not self.use_xyz:
            raise ValueError("Cannot have not features and not use xyz as a feature!")
        return grouped_xyz


def sample_points(xyz, npoint, sample_type, cls_features=None):
    """(sample_idx [B, npoint] int32, new_xyz [B, npoint, 3]) as iassd_modules.py:174-200 samples them."""
    B, N = int(xyz.shape[0]), int(xyz.shape[1])
    if N <= npoint:
        sample_idx = torch.arange(N, dtype=torch.int32, device=xyz.device).expand(B, N).contiguous()
    elif "ctr" in sample_type:
        if cls_features is None:
            raise ValueError("ctr_aware sampling needs cls_features [B, N, num_class]")
        score = torch.sigmoid(cls_features.max(dim=-1).values)
        sample_idx = torch.topk(score, npoint, dim=-1).indices.int()
    elif "D-FPS" in sample_type:
        sample_idx = pointnet2_ops.farthest_point_sample(xyz, npoint)
    else:
        raise NotImplementedError(f"sample_type {sample_type!r}")
    new_xyz = pointnet2_ops.gather_operation(xyz.transpose(1, 2).contiguous(), sample_idx).transpose(1, 2)
    return sample_idx, new_xyz
