"""`paddle3d.models.common.pointnet2_stack` on the device stack ops (paddle3d_amd/ops/pointnet2_ops.py): the set
abstraction layers of PV-RCNN (StackSAModuleMSG) and Voxel R-CNN (NeighborVoxelSAModuleMSG).

QueryAndGroup(radius, nsample, use_xyz)        pointnet2_utils.py:27-89: ball query, xyz relative to the centre,
                                               features, concat [xyz, features]; empty balls give zero idx, xyz and
                                               features.  -> (new_features [M, 3 + C, nsample], idx)
StackSAModuleMSG(radii, nsamples, mlps, use_xyz, pool_method, fused=False)
build_local_aggregation_module(input_channels, config, fused=False)
                                               pointnet2_modules.py:31-157: per radius a QueryAndGroup, a 1x1
                                               Conv2d / BN / ReLU stack and a max or avg pool over nsample.
                                               fused=True: in eval mode without gradients, a max-pooled scale with
                                               use_xyz whose mlp is Conv / BN / ReLU twice and whose (C1, C2, nsample)
                                               the op takes runs from the ball query to the pool as
                                               ops.pvrcnn.stack_sa_pool (no [M, *, nsample] tensor); every other case
                                               runs the unfused forward.
voxel_query(max_range, radius, nsample, xyz, new_xyz, new_coords, point_indices)
VoxelQueryAndGrouping(max_range, radius, nsample)
                                               voxel_query_utils.py:28-106: the voxel query, its global indices made
                                               frame-local on the device, grouping of xyz and features.
NeighborVoxelSAModuleMSG(query_ranges, radii, nsamples, mlps, use_xyz, pool_method, fused=False)
                                               voxel_pool_modules.py:29-163.  fused=True: in eval mode without
                                               gradients, a scale whose (C1, nsample) the op takes runs from the voxel
                                               query to the pool as ops.roi_head.voxel_pool (no [M, *, nsample] tensor);
                                               every other case runs the unfused forward.
generate_voxel2pinds(sparse_tensor_shape, sparse_tensor_indices, n_dev=None)
                                               box_utils.py:102-110: [B, Z, Y, X] int32 row index per cell, -1 where
                                               a cell is empty.

Submodule names (groupers, mlps, mlps_in, mlps_pos, mlps_out) are the reference's, so checkpoint.py maps Paddle
weights onto them.  Nothing here synchronises with the host: the reference's asserts on the batch counts read device
tensors, so they run only with check_counts=True.
"""
from __future__ import annotations

from typing import List

import torch
import torch.nn.functional as F
from torch import nn

from .ops import pointnet2_ops, pvrcnn, roi_head

__all__ = ["QueryAndGroup", "StackSAModuleMSG", "build_local_aggregation_module", "voxel_query",
           "VoxelQueryAndGrouping", "NeighborVoxelSAModuleMSG", "generate_voxel2pinds"]


def _check_counts(rows, batch_cnt, what):
    total = int(batch_cnt.sum())  # a host sync: only with check_counts=True
    if int(rows.shape[0]) != total:
        raise AssertionError(f"{what}: {tuple(rows.shape)}, batch_cnt: {batch_cnt.tolist()}")


def _pool(x, pool_method):
    """[1, C, M, nsample] -> [1, C, M] (the reference's F.max_pool2d / F.avg_pool2d with kernel [1, nsample])."""
    if pool_method == "max_pool":
        return F.max_pool2d(x, kernel_size=(1, int(x.shape[3]))).squeeze(-1)
    if pool_method == "avg_pool":
        return F.avg_pool2d(x, kernel_size=(1, int(x.shape[3]))).squeeze(-1)
    raise NotImplementedError(pool_method)


def _init_weights(module):
    for m in module.modules():
        if isinstance(m, (nn.Conv1d, nn.Conv2d)):
            nn.init.kaiming_normal_(m.weight, a=0, mode="fan_in", nonlinearity="leaky_relu")
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)):
            nn.init.ones_(m.weight)
            nn.init.zeros_(m.bias)


class QueryAndGroup(nn.Module):
    def __init__(self, radius: float, nsample: int, use_xyz: bool = True, check_counts: bool = False):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz
        self.check_counts = check_counts

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features=None):
        """xyz [N, 3], new_xyz [M, 3], features [N, C] or None, counts [B] int32 ->
        (new_features [M, 3 + C, nsample] ([M, C, ...] without use_xyz), idx [M, nsample] with empty rows 0)."""
        if self.check_counts:
            _check_counts(xyz, xyz_batch_cnt, "xyz")
            _check_counts(new_xyz, new_xyz_batch_cnt, "new_xyz")
        idx = pointnet2_ops.ball_query_stack(new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, self.radius,
                                             self.nsample)
        empty = idx[:, 0] == -1
        idx = idx.masked_fill(empty[:, None], 0)
        grouped_xyz = pointnet2_ops.grouping_operation_stack(xyz, xyz_batch_cnt, idx, new_xyz_batch_cnt)
        grouped_xyz = (grouped_xyz - new_xyz.unsqueeze(-1)).masked_fill(empty[:, None, None], 0.0)
        if features is not None:
            grouped_features = pointnet2_ops.grouping_operation_stack(features, xyz_batch_cnt, idx, new_xyz_batch_cnt)
            grouped_features = grouped_features.masked_fill(empty[:, None, None], 0.0)
            if self.use_xyz:
                return torch.cat([grouped_xyz, grouped_features], dim=1), idx
            return grouped_features, idx
        if not self.use_xyz:
            raise ValueError("Cannot have not features and not use xyz as a feature!")
        return grouped_xyz, idx


class StackSAModuleMSG(nn.Module):
    def __init__(self, *, radii: List[float], nsamples: List[int], mlps: List[List[int]], use_xyz: bool = True,
                 pool_method: str = "max_pool", fused: bool = False):
        super().__init__()
        assert len(radii) == len(nsamples) == len(mlps)
        self.fused = fused
        self.use_xyz = use_xyz
        self.groupers = nn.ModuleList()
        self.mlps = nn.ModuleList()
        for radius, nsample, mlp_spec in zip(radii, nsamples, mlps):
            self.groupers.append(QueryAndGroup(radius, nsample, use_xyz=use_xyz))
            if use_xyz:
                mlp_spec[0] += 3  # in place, as the reference does: the caller's config sees it
            layers = []
            for k in range(len(mlp_spec) - 1):
                layers += [nn.Conv2d(mlp_spec[k], mlp_spec[k + 1], kernel_size=1, bias=False),
                           nn.BatchNorm2d(mlp_spec[k + 1]), nn.ReLU()]
            self.mlps.append(nn.Sequential(*layers))
        self.pool_method = pool_method
        _init_weights(self)

    def _takes_fused(self, k):
        mlp, g = self.mlps[k], self.groupers[k]
        return (self.fused and not self.training and not torch.is_grad_enabled() and self.use_xyz
                and self.pool_method == "max_pool" and len(mlp) == 6
                and pvrcnn.stack_sa_pool_supported(mlp[0].out_channels, mlp[3].out_channels, g.nsample))

    def _fused_pool(self, k, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features):
        """[M, C2]: scale k from the ball query to the pool in one kernel.  The first convolution is linear in
        [d; f]: its feature columns run once over the N source rows, its xyz columns go to the kernel; each
        BatchNorm in eval form, scale = gamma / sqrt(var + eps), shift = beta - mean * scale, formed in fp32."""
        mlp, g = self.mlps[k], self.groupers[k]
        c1, c2 = mlp[0].out_channels, mlp[3].out_channels
        w1 = mlp[0].weight.reshape(c1, -1)
        features_in = None if features is None else features @ w1[:, 3:].t()
        scale1 = mlp[1].weight / torch.sqrt(mlp[1].running_var + mlp[1].eps)
        shift1 = mlp[1].bias - mlp[1].running_mean * scale1
        scale2 = mlp[4].weight / torch.sqrt(mlp[4].running_var + mlp[4].eps)
        shift2 = mlp[4].bias - mlp[4].running_mean * scale2
        return pvrcnn.stack_sa_pool(new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, features_in, w1[:, :3], scale1,
                                    shift1, mlp[3].weight.reshape(c2, c1), scale2, shift2, g.radius, g.nsample)

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features=None, empty_voxel_set_zeros=True):
        """-> (new_xyz [M, 3], new_features [M, sum of mlps[k][-1]])."""
        out = []
        for k, (grouper, mlp) in enumerate(zip(self.groupers, self.mlps)):
            if self._takes_fused(k):
                out.append(self._fused_pool(k, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features))
                continue
            new_features, _ = grouper(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features)  # [M, C, nsample]
            new_features = mlp(new_features.permute(1, 0, 2).unsqueeze(0))  # [1, C', M, nsample]
            out.append(_pool(new_features, self.pool_method).squeeze(0).transpose(0, 1))  # [M, C']
        return new_xyz, torch.cat(out, dim=1)


def build_local_aggregation_module(input_channels, config, fused=False):
    """(StackSAModuleMSG, its output channels) from a config with mlps / pool_radius / nsample; config["mlps"] gets
    input_channels prepended in place, as the reference's does.  fused: StackSAModuleMSG's."""
    name = config.get("name", "StackSAModuleMSG")
    if name != "StackSAModuleMSG":
        raise NotImplementedError(name)
    mlps = config["mlps"]
    for k in range(len(mlps)):
        mlps[k] = [input_channels] + mlps[k]
    layer = StackSAModuleMSG(radii=config["pool_radius"], nsamples=config["nsample"], mlps=mlps, use_xyz=True,
                             pool_method="max_pool", fused=fused)
    return layer, sum(x[-1] for x in mlps)


def voxel_query(max_range, radius, nsample, xyz, new_xyz, new_coords, point_indices):
    """(idx [M, nsample] int32 rows of xyz with empty rows 0, empty_ball_mask [M])."""
    z_range, y_range, x_range = max_range
    idx = pointnet2_ops.voxel_query_wrapper(new_xyz, xyz, new_coords, point_indices, radius, nsample, z_range,
                                            y_range, x_range)
    empty = idx[:, 0] == -1
    return idx.masked_fill(empty[:, None], 0), empty


class VoxelQueryAndGrouping(nn.Module):
    def __init__(self, max_range, radius: float, nsample: int, check_counts: bool = False):
        super().__init__()
        self.max_range, self.radius, self.nsample = max_range, radius, nsample
        self.check_counts = check_counts

    def forward(self, new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features, voxel2point_indices):
        """-> (grouped_features [M, C, nsample], grouped_xyz [M, 3, nsample], empty_ball_mask [M])."""
        if self.check_counts:
            _check_counts(xyz, xyz_batch_cnt, "xyz")
            _check_counts(new_coords, new_xyz_batch_cnt, "new_coords")
        B = int(xyz_batch_cnt.shape[0])
        M = int(new_coords.shape[0])
        if B == 0 or M % B:
            raise RuntimeError(f"VoxelQueryAndGrouping: {M} rows do not split into {B} equal frames")
        idx, empty = voxel_query(self.max_range, self.radius, self.nsample, xyz, new_xyz, new_coords,
                                 voxel2point_indices)
        # the reference's reshape([B, -1, nsample]) and per-group subtraction of the running xyz count, in int32
        cnt = xyz_batch_cnt.to(torch.int32)
        start = torch.cumsum(cnt, 0, dtype=torch.int32) - cnt
        idx = (idx.view(B, -1, self.nsample) - start.view(B, 1, 1)).view(-1, self.nsample)
        idx = idx.masked_fill(empty[:, None], 0)
        grouped_xyz = pointnet2_ops.grouping_operation_stack(xyz, xyz_batch_cnt, idx, new_xyz_batch_cnt)
        grouped_features = pointnet2_ops.grouping_operation_stack(features, xyz_batch_cnt, idx, new_xyz_batch_cnt)
        return grouped_features, grouped_xyz, empty


class NeighborVoxelSAModuleMSG(nn.Module):
    def __init__(self, *, query_ranges, radii: List[float], nsamples: List[int], mlps: List[List[int]],
                 use_xyz: bool = True, pool_method: str = "max_pool", fused: bool = False):
        super().__init__()
        assert len(query_ranges) == len(nsamples) == len(mlps)
        self.fused = fused
        self.groupers = nn.ModuleList()
        self.mlps_in = nn.ModuleList()
        self.mlps_pos = nn.ModuleList()
        self.mlps_out = nn.ModuleList()
        for max_range, radius, nsample, spec in zip(query_ranges, radii, nsamples, mlps):
            self.groupers.append(VoxelQueryAndGrouping(max_range, radius, nsample))
            self.mlps_in.append(nn.Sequential(nn.Conv1d(spec[0], spec[1], kernel_size=1, bias=False),
                                              nn.BatchNorm1d(spec[1])))
            self.mlps_pos.append(nn.Sequential(nn.Conv2d(3, spec[1], kernel_size=1, bias=False),
                                               nn.BatchNorm2d(spec[1])))
            self.mlps_out.append(nn.Sequential(nn.Conv1d(spec[1], spec[2], kernel_size=1, bias=False),
                                               nn.BatchNorm1d(spec[2]), nn.ReLU()))
        self.relu = nn.ReLU()
        self.pool_method = pool_method
        _init_weights(self)

    def _takes_fused(self, k):
        g = self.groupers[k]
        return (self.fused and not self.training and not torch.is_grad_enabled()
                and self.pool_method in roi_head.POOLS
                and roi_head.voxel_pool_supported(self.mlps_pos[k][0].out_channels, g.nsample))

    def _fused_pool(self, k, new_xyz, new_coords, xyz, features_in, voxel2point_indices):
        """[M, C1]: scale k from the voxel query to the pool in one kernel; mlps_pos as its conv weight and its
        BatchNorm in eval form, scale = gamma / sqrt(var + eps), shift = beta - mean * scale, formed in fp32."""
        conv, bn = self.mlps_pos[k][0], self.mlps_pos[k][1]
        scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        shift = bn.bias - bn.running_mean * scale
        g = self.groupers[k]
        return roi_head.voxel_pool(new_xyz, new_coords, xyz, voxel2point_indices, features_in,
                                   conv.weight.reshape(conv.out_channels, 3), scale, shift, g.max_range, g.radius,
                                   g.nsample, self.pool_method)

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, features, voxel2point_indices):
        """xyz [N, 3] voxel centres, features [N, C], new_xyz [M, 3], new_coords [M, 4] as (b, x, y, z),
        voxel2point_indices [B, Z, Y, X] -> new_features [M, sum of mlps[k][2]]."""
        # (b, x, y, z) -> (b, z, y, x); no index list, whose copy to the device would synchronise
        new_coords = torch.cat([new_coords[:, :1], new_coords[:, 1:].flip(1)], dim=1)
        out = []
        for k, grouper in enumerate(self.groupers):
            features_in = self.mlps_in[k](features.transpose(0, 1).unsqueeze(0))  # [1, C1, N]
            features_in = features_in.transpose(1, 2).reshape(-1, int(features_in.shape[1]))  # [N, C1]
            if self._takes_fused(k):
                pooled = self._fused_pool(k, new_xyz, new_coords, xyz, features_in, voxel2point_indices)
                new_features = self.mlps_out[k](pooled.transpose(0, 1).unsqueeze(0))  # [1, C2, M]
                out.append(new_features.squeeze(0).transpose(0, 1))
                continue
            grouped_features, grouped_xyz, empty = grouper(new_coords, xyz, xyz_batch_cnt, new_xyz,
                                                           new_xyz_batch_cnt, features_in, voxel2point_indices)
            grouped_features = grouped_features.masked_fill(empty[:, None, None], 0.0)
            grouped_features = grouped_features.permute(1, 0, 2).unsqueeze(0)  # [1, C1, M, nsample]
            grouped_xyz = (grouped_xyz - new_xyz.unsqueeze(-1)).masked_fill(empty[:, None, None], 0.0)
            position_features = self.mlps_pos[k](grouped_xyz.permute(1, 0, 2).unsqueeze(0))
            new_features = self.relu(grouped_features + position_features)
            new_features = self.mlps_out[k](_pool(new_features, self.pool_method))  # [1, C2, M]
            out.append(new_features.squeeze(0).transpose(0, 1))
        return torch.cat(out, dim=1)


def generate_voxel2pinds(sparse_tensor_shape, sparse_tensor_indices, n_dev=None):
    """[B, Z, Y, X] int32: for each cell the row of sparse_tensor_indices ([N, 4] as (b, z, y, x)) that lands there,
    -1 for an empty cell; sparse_tensor_shape is [B, Z, Y, X, C] (box_utils.py:102-110).  As the reference's
    scatter_nd, rows landing in one cell add up.  n_dev ([1] int32 on the device, SparseConvTensor.n_dev): rows at
    or past it are ignored, without a host sync."""
    B = int(sparse_tensor_shape[0])
    Z, Y, X = (int(s) for s in sparse_tensor_shape[1:-1])
    ind = sparse_tensor_indices.long()
    N = int(ind.shape[0])
    total = B * Z * Y * X
    flat = ((ind[:, 0] * Z + ind[:, 1]) * Y + ind[:, 2]) * X + ind[:, 3]
    rows = torch.arange(N, dtype=torch.int32, device=ind.device)
    if n_dev is not None:
        flat = torch.where(rows < n_dev.reshape(-1)[:1].to(torch.int32), flat, torch.full_like(flat, total))
    out = torch.zeros(total + 1, dtype=torch.int32, device=ind.device)  # the last slot takes the ignored rows
    out.index_add_(0, flat, rows + 1)
    return (out[:total] - 1).view(B, Z, Y, X)
