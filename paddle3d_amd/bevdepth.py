"""BEVDepth's depth network and view transformer (reference paddle3d/models/transformers/bevdet_transformer.py:322-475,
:582-744), the `img_view_transformer` of configs/bevdet/bevdet4d_r50_depth_nuscenes.yml, at inference: the reference's
constructor arguments and state-dict keys (`depth_net.reduce_conv.0.weight`, `depth_net.depth_conv.3.aspp2.atrous_conv
.weight`, `depth_net.depth_conv.3.global_avg_pool.1.weight`, ...), so a checkpoint's `img_view_transformer.*` keys load
strictly through paddle3d_amd.checkpoint.

_ASPPModule, ASPP(inplanes, mid_channels=256, fused=True)
    the atrous pyramid at dilations 1, 6, 12, 18.  Fused, the four convolution branches, the pooled branch (a per-image
    bias behind conv1) and the projection run as pd3_aspp_forward: no concatenation, no broadcast pooled map, and only the
    taps inside the image are multiplied.
Mlp, SELayer, BasicBlock
    as the reference (BasicBlock is paddle.vision's: conv3x3-bn-relu-conv3x3-bn, add, relu, no downsample here); the SE
    gate and the MLPs act on [B N, C] vectors and stay torch, as do the plain 3 x 3 and 1 x 1 convolutions.
DepthNet(in_channels, mid_channels, context_channels, depth_channels, use_dcn=False, use_aspp=True, fused=True)
    forward(x, mlp_input) -> [B N, depth_channels + context_channels, H, W].
LSSViewTransformerBEVDepth(grid_config, input_size, downsample=16, in_channels=512, out_channels=64, accelerate=False,
                           depthnet_cfg=None, loss_depth_weight=3.0, fused=True)
    get_mlp_input(rot, tran, intrin, post_rot, post_tran, bda) and forward(input) -> (bev_feat, depth); the geometry and
    the pooling are paddle3d_amd.bevdet.LSSViewTransformer's.  Fused, the softmax over the depth channels and the
    channels-last copy of the context channels that bev_pool_v2 reads are one launch (pd3_depth_softmax_split).
bevdet4d_r50_depth_view_transformer(fused=True)
    the config's values: 512 -> 80 channels, 118 depth bins, 256 x 704 input at stride 16, accelerate off.

fused=False is the plain torch composition on any device and in any dtype; fused=True takes a kernel where its predicate
accepts and ops.depthnet.fused_by_default says it was measured faster than the composition; fused="force" wherever the
predicate accepts.  Inference only: a forward in training mode is refused where a BatchNorm would be folded.  The loss
methods of the reference are not here.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from .bevdet import BEVDET4D_GRID, LSSViewTransformer
from .derived import derived
from .ops import bev_pool_v2 as _bp
from .ops import depthnet as ops
from .ops.squeezeseg import fold_batch_norm

__all__ = ["ASPP", "Mlp", "SELayer", "BasicBlock", "DepthNet", "LSSViewTransformerBEVDepth",
           "bevdet4d_r50_depth_view_transformer"]

ASPP_DILATIONS = (1, 6, 12, 18)


def _check_fused(fused):
    if fused not in (True, False, "force"):
        raise ValueError(f"fused must be True, False or 'force', got {fused!r}")
    return fused


def _fold(bn):
    return fold_batch_norm(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)


class _ASPPModule(nn.Module):
    def __init__(self, inplanes, planes, kernel_size, padding, dilation, BatchNorm=nn.BatchNorm2d):
        super().__init__()
        self.atrous_conv = nn.Conv2d(inplanes, planes, kernel_size, stride=1, padding=padding, dilation=dilation,
                                     bias=False)
        self.bn = BatchNorm(planes)
        self.relu = nn.ReLU()
        nn.init.kaiming_normal_(self.atrous_conv.weight)

    def forward(self, x):
        return self.relu(self.bn(self.atrous_conv(x)))


class ASPP(nn.Module):
    def __init__(self, inplanes, mid_channels=256, BatchNorm=nn.BatchNorm2d, fused=True):
        super().__init__()
        d = ASPP_DILATIONS
        self.fused = _check_fused(fused)
        self.aspp1 = _ASPPModule(inplanes, mid_channels, 1, padding=0, dilation=d[0], BatchNorm=BatchNorm)
        self.aspp2 = _ASPPModule(inplanes, mid_channels, 3, padding=d[1], dilation=d[1], BatchNorm=BatchNorm)
        self.aspp3 = _ASPPModule(inplanes, mid_channels, 3, padding=d[2], dilation=d[2], BatchNorm=BatchNorm)
        self.aspp4 = _ASPPModule(inplanes, mid_channels, 3, padding=d[3], dilation=d[3], BatchNorm=BatchNorm)
        self.global_avg_pool = nn.Sequential(nn.AdaptiveAvgPool2d((1, 1)),
                                             nn.Conv2d(inplanes, mid_channels, 1, stride=1, bias=False),
                                             BatchNorm(mid_channels), nn.ReLU())
        self.conv1 = nn.Conv2d(int(mid_channels * 5), mid_channels, 1, bias=False)
        self.bn1 = BatchNorm(mid_channels)
        self.relu = nn.ReLU()
        self.dropout = nn.Dropout(0.5)
        nn.init.kaiming_normal_(self.global_avg_pool[1].weight)
        nn.init.kaiming_normal_(self.conv1.weight)

    def takes_kernel(self, x):
        """Whether this forward runs pd3_aspp_forward."""
        if not self.fused or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
            return False
        if any(type(m) is not nn.BatchNorm2d for m in (self.aspp1.bn, self.global_avg_pool[2], self.bn1)):
            return False
        N, ci, H, W = (int(v) for v in x.shape)
        cm = int(self.conv1.weight.shape[0])
        if N < 1 or not ops.aspp_supported(ci, cm, H, W, N, ASPP_DILATIONS[1:]):
            return False
        return self.fused == "force" or ops.fused_by_default("aspp", N, ci, cm, H, W)

    def _packed(self):
        branches = (self.aspp1, self.aspp2, self.aspp3, self.aspp4)
        return derived(self, "packed", lambda: ops.pack_aspp(
            [b.atrous_conv.weight for b in branches], [_fold(b.bn) for b in branches], self.global_avg_pool[1].weight,
            _fold(self.global_avg_pool[2]), self.conv1.weight, _fold(self.bn1)))

    def forward(self, x):
        if self.takes_kernel(x):
            if self.training:
                raise RuntimeError("ASPP: paddle3d_amd implements the inference path only (BatchNorm folded into the "
                                   "HIP kernels); call .eval() first")
            y = ops.aspp_forward(x, self._packed(), ASPP_DILATIONS[1:])
            if y is not None:
                return y
        x1, x2, x3, x4 = self.aspp1(x), self.aspp2(x), self.aspp3(x), self.aspp4(x)
        x5 = self.global_avg_pool(x)
        x5 = F.interpolate(x5, size=x4.shape[2:], mode="bilinear", align_corners=True)
        x = torch.cat((x1, x2, x3, x4, x5), dim=1)
        return self.dropout(self.relu(self.bn1(self.conv1(x))))


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.ReLU, drop=0.0):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(27, hidden_features)  # the reference's literal 27
        self.act = act_layer()
        self.drop1 = nn.Dropout(drop)
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop2 = nn.Dropout(drop)

    def forward(self, x):
        return self.drop2(self.fc2(self.drop1(self.act(self.fc1(x)))))


class SELayer(nn.Module):
    def __init__(self, channels, act_layer=nn.ReLU, gate_layer=nn.Sigmoid):
        super().__init__()
        self.conv_reduce = nn.Conv2d(channels, channels, 1, bias=True)
        self.act1 = act_layer()
        self.conv_expand = nn.Conv2d(channels, channels, 1, bias=True)
        self.gate = gate_layer()

    def forward(self, x, x_se):
        return x * self.gate(self.conv_expand(self.act1(self.conv_reduce(x_se))))


class BasicBlock(nn.Module):
    """paddle.vision.models.resnet.BasicBlock without a downsample: relu(bn2(conv2(relu(bn1(conv1(x))))) + x)."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        if downsample is not None or stride != 1:
            raise NotImplementedError("BasicBlock: DepthNet uses it without a downsample at stride 1")
        self.conv1 = nn.Conv2d(inplanes, planes, 3, padding=1, stride=stride, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU()
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + x)


class DepthNet(nn.Module):
    def __init__(self, in_channels, mid_channels, context_channels, depth_channels, use_dcn=False, use_aspp=True,
                 fused=True):
        super().__init__()
        if use_dcn:
            raise NotImplementedError("DepthNet: dcn not supported yet")  # as the reference
        self.fused = _check_fused(fused)
        self.reduce_conv = nn.Sequential(nn.Conv2d(in_channels, mid_channels, 3, stride=1, padding=1),
                                         nn.BatchNorm2d(mid_channels), nn.ReLU())
        self.context_conv = nn.Conv2d(mid_channels, context_channels, 1, stride=1, padding=0)
        self.bn = nn.BatchNorm1d(27)
        self.depth_mlp = Mlp(27, mid_channels, mid_channels)
        self.depth_se = SELayer(mid_channels)
        self.context_mlp = Mlp(27, mid_channels, mid_channels)
        self.context_se = SELayer(mid_channels)
        layers = [BasicBlock(mid_channels, mid_channels) for _ in range(3)]
        if use_aspp:
            layers.append(ASPP(mid_channels, mid_channels, fused=fused))
        layers.append(nn.Conv2d(mid_channels, depth_channels, 1, stride=1, padding=0))
        self.depth_conv = nn.Sequential(*layers)

    def forward(self, x, mlp_input):
        mlp_input = self.bn(mlp_input.reshape(-1, mlp_input.shape[-1]))
        x = self.reduce_conv(x)
        context_se = self.context_mlp(mlp_input)[..., None, None]
        context = self.context_conv(self.context_se(x, context_se))
        depth_se = self.depth_mlp(mlp_input)[..., None, None]
        depth = self.depth_conv(self.depth_se(x, depth_se))
        return torch.cat([depth, context], dim=1)


class LSSViewTransformerBEVDepth(nn.Module):
    def __init__(self, grid_config=None, input_size=(256, 704), downsample=16, in_channels=512, out_channels=64,
                 accelerate=False, depthnet_cfg=None, loss_depth_weight=3.0, fused=True):
        super().__init__()
        self.fused = _check_fused(fused)
        self.geometry = LSSViewTransformer(grid_config, input_size, downsample, accelerate)  # not a module: no keys
        self.grid_config, self.downsample, self.accelerate = self.geometry.grid_config, downsample, accelerate
        self.D, self.in_channels, self.out_channels = self.geometry.D, in_channels, out_channels
        self.loss_depth_weight = loss_depth_weight
        self.depth_net = DepthNet(in_channels, in_channels, out_channels, self.D, fused=fused, **dict(depthnet_cfg or {}))

    def get_mlp_input(self, rot, tran, intrin, post_rot, post_tran, bda):
        B, N = int(rot.shape[0]), int(rot.shape[1])
        bda = bda.reshape(B, 1, 3, 3).repeat(1, N, 1, 1)
        intrin = intrin.float()
        mlp_input = torch.stack([
            intrin[:, :, 0, 0], intrin[:, :, 1, 1], intrin[:, :, 0, 2], intrin[:, :, 1, 2],
            post_rot[:, :, 0, 0], post_rot[:, :, 0, 1], post_tran[:, :, 0],
            post_rot[:, :, 1, 0], post_rot[:, :, 1, 1], post_tran[:, :, 1],
            bda[:, :, 0, 0], bda[:, :, 0, 1], bda[:, :, 1, 0], bda[:, :, 1, 1], bda[:, :, 2, 2]], dim=-1)
        sensor2ego = torch.cat([rot, tran.reshape(B, N, 3, 1)], dim=-1).reshape(B, N, -1)
        return torch.cat([mlp_input, sensor2ego], dim=-1)

    def takes_tail_kernel(self, x):
        """Whether the softmax and the channels-last copy of `x` [B N, D + C, H, W] run pd3_depth_softmax_split."""
        if not self.fused or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
            return False
        n, dc, h, w = (int(v) for v in x.shape)
        if dc != self.D + self.out_channels or not ops.tail_supported(n, self.D, self.out_channels, h, w):
            return False
        return self.fused == "force" or ops.fused_by_default("tail", n, self.D, self.out_channels, h, w)

    def _tail(self, x):
        """(depth [B N, D, H, W], tran_feat channels last [B N, H, W, C])."""
        if self.takes_tail_kernel(x):
            out = ops.depth_softmax_split(x.contiguous(), self.D)
            if out is not None:
                return out
        depth = F.softmax(x[:, :self.D], dim=1)
        return depth, x[:, self.D:self.D + self.out_channels].permute(0, 2, 3, 1).contiguous()

    def forward(self, input):
        x, rots, trans, intrins, post_rots, post_trans, bda, mlp_input = input[:8]
        B, N, C, H, W = x.shape
        x = self.depth_net(x.reshape(B * N, C, H, W), mlp_input)
        depth, feat = self._tail(x)
        g = self.geometry
        if g.accelerate and g._prepared is not None:
            prep = g._prepared  # the index sets of the first call (a fixed calibration)
        else:
            prep = g.voxel_pooling_prepare_v2(g.get_lidar_coor(rots, trans, intrins, post_rots, post_trans, bda))
            if g.accelerate:
                g._prepared = prep
        gx, gy = int(g.grid_size[0]), int(g.grid_size[1])
        if prep[0] is None:
            return torch.zeros((B, feat.shape[-1], gx, gy), dtype=feat.dtype, device=feat.device), depth
        ranks_bev, ranks_depth, ranks_feat, starts, lengths = prep
        out = _bp.bev_pool_v2(depth.contiguous(), feat, ranks_depth, ranks_feat, ranks_bev, lengths, starts,
                              (B, gy, gx, feat.shape[-1]))
        return out.permute(0, 3, 1, 2), depth


def bevdet4d_r50_depth_view_transformer(fused=True):
    """The img_view_transformer of configs/bevdet/bevdet4d_r50_depth_nuscenes.yml."""
    return LSSViewTransformerBEVDepth(grid_config=BEVDET4D_GRID, input_size=(256, 704), downsample=16, in_channels=512,
                                      out_channels=80, accelerate=False, depthnet_cfg=dict(use_dcn=False), fused=fused)
