"""MMResNet with modulated deformable convolutions (reference paddle3d/models/backbones/mm_resnet.py), the image
backbone of the two CAPE ResNet-50 configs, at inference: the reference's constructor arguments and state-dict keys
(`bn1`, `layer3.0.conv2.conv_offset.weight`, `layer3.0.conv2.conv_dcn.weight`, ...), so a `.pdparams` loads strictly
through paddle3d_amd.checkpoint.

deform_conv2d_composition(x, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1)
    paddle.vision.ops.deform_conv2d as torch operators (gathers of the four corners and one matmul; no grid_sample), on
    any device and in the inputs' dtype: what fused=False runs and what a shape the kernel refuses falls back to.
DeformableConvV2(in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, deformable_groups=1, groups=1,
                 weight_attr=None, bias_attr=None, fused=True)
    conv_offset (27 channels: 18 offsets, 9 mask logits) and conv_dcn.  fused=True runs pd3_deform_conv2d_forward (the
    sigmoid, the bias or a following BatchNorm and relu in its epilogue; the two parts of conv_offset's output passed as
    views) where ops.deform_conv.fused_by_default says it was measured faster than the composition, fused="force"
    wherever deform_conv2d_supported accepts, fused=False never.
Bottleneck, ResLayer, MMResNet(depth, ..., fused=True)
    both styles; with `dcn` the block hands norm2 (folded) and the relu to the kernel.  Depths 50 and 101; what the
    configs under configs/cape/ and configs/rtebev/ leave at a default (conv_cfg, BasicBlock depths, plugins, a norm
    layer other than BatchNorm2D) raises NotImplementedError.
mm_resnet50_caffe_dcn(out_indices=(2, 3), fused=True)
    the backbone of cape_r50_1408x512 and capet_r50_704x256.

Inference only: a forward in training mode with norm_eval=False is refused where a BatchNorm would have to be folded.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from .derived import derived
from .ops import deform_conv as ops
from .ops.squeezeseg import fold_batch_norm

__all__ = ["deform_conv2d_composition", "DeformConv2D", "DeformableConvV2", "Bottleneck", "ResLayer", "MMResNet",
           "mm_resnet50_caffe_dcn"]


def _check_fused(fused):
    if fused not in (True, False, "force"):
        raise ValueError(f"fused must be True, False or 'force', got {fused!r}")
    return fused


def deform_conv2d_composition(x, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1):
    N, C, H, W = x.shape
    Co, _, kh, kw = weight.shape
    s, p, d = int(stride), int(padding), int(dilation)
    Ho = (H + 2 * p - d * (kh - 1) - 1) // s + 1
    Wo = (W + 2 * p - d * (kw - 1) - 1) // s + 1
    K = kh * kw
    dev, dt = x.device, x.dtype
    ky = torch.arange(kh, device=dev).repeat_interleave(kw)
    kx = torch.arange(kw, device=dev).repeat(kh)
    base_h = (torch.arange(Ho, device=dev) * s - p)[None, :, None] + (ky * d)[:, None, None]  # [K, Ho, 1]
    base_w = (torch.arange(Wo, device=dev) * s - p)[None, None, :] + (kx * d)[:, None, None]  # [K, 1, Wo]
    off = offset.reshape(N, K, 2, Ho, Wo)
    h = base_h.to(dt)[None] + off[:, :, 0]  # [N, K, Ho, Wo]
    w = base_w.to(dt)[None] + off[:, :, 1]
    inside = (h > -1) & (w > -1) & (h < H) & (w < W)
    h = torch.where(inside, h, torch.zeros_like(h))
    w = torch.where(inside, w, torch.zeros_like(w))
    hl, wl = torch.floor(h), torch.floor(w)
    lh, lw = h - hl, w - wl
    hh, hw = 1 - lh, 1 - lw
    ih, iw = hl.long(), wl.long()
    flat = x.reshape(N, C, H * W)

    def corner(yy, xx, coef):
        ok = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1) & inside
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).reshape(N, 1, K * Ho * Wo).expand(N, C, K * Ho * Wo)
        v = torch.gather(flat, 2, idx).reshape(N, C, K, Ho, Wo)
        return torch.where(ok[:, None], v, torch.zeros_like(v)) * coef[:, None]

    val = corner(ih, iw, hh * hw) + corner(ih, iw + 1, hh * lw) + corner(ih + 1, iw, lh * hw) + \
        corner(ih + 1, iw + 1, lh * lw)
    if mask is not None:
        val = val * mask[:, None]
    cols = val.reshape(N, C * K, Ho * Wo)
    y = torch.matmul(weight.reshape(Co, C * K), cols).reshape(N, Co, Ho, Wo)
    return y if bias is None else y + bias[None, :, None, None]


class DeformConv2D(nn.Module):
    """paddle.vision.ops.DeformConv2D's parameters: weight [Cout, Cin / groups, k, k] and bias [Cout] (absent with
    bias_attr=False)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, deformable_groups=1,
                 groups=1, weight_attr=None, bias_attr=None):
        super().__init__()
        k = int(kernel_size)
        self.stride, self.padding, self.dilation = int(stride), int(padding), int(dilation)
        self.deformable_groups, self.groups, self.kernel_size = int(deformable_groups), int(groups), k
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // self.groups, k, k))
        nn.init.normal_(self.weight, 0.0, (2.0 / (out_channels * k * k)) ** 0.5)
        self.bias = None if bias_attr is False else nn.Parameter(torch.zeros(out_channels))

    def forward(self, x, offset, mask=None):
        if self.groups != 1 or self.deformable_groups != 1:
            raise NotImplementedError("DeformConv2D: groups and deformable_groups other than 1")
        return deform_conv2d_composition(x, offset, mask, self.weight, self.bias, self.stride, self.padding,
                                         self.dilation)


class DeformableConvV2(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, deformable_groups=1,
                 groups=1, weight_attr=None, bias_attr=None, fused=True):
        super().__init__()
        k = int(kernel_size)
        self.offset_channel, self.mask_channel = 2 * k * k, k * k
        self.fused = _check_fused(fused)
        self.conv_offset = nn.Conv2d(in_channels, 3 * k * k, k, stride=stride, padding=(k - 1) // 2)
        nn.init.zeros_(self.conv_offset.weight)
        nn.init.zeros_(self.conv_offset.bias)
        self.conv_dcn = DeformConv2D(in_channels, out_channels, k, stride=stride, padding=(k - 1) // 2 * dilation,
                                     dilation=dilation, deformable_groups=deformable_groups, groups=groups,
                                     weight_attr=weight_attr, bias_attr=bias_attr)

    def takes_kernel(self, x):
        """Whether this forward runs pd3_deform_conv2d_forward."""
        c = self.conv_dcn
        if not self.fused or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
            return False
        N, ci, H, W = (int(v) for v in x.shape)
        co = int(c.weight.shape[0])
        if not ops.deform_conv2d_supported(ci, co, H, W, N, c.stride, c.padding, c.dilation, c.kernel_size, c.groups,
                                           c.deformable_groups):
            return False
        if self.fused == "force":
            return True
        pixels = N * ops.output_size(H, c.stride, c.padding, c.dilation) * ops.output_size(W, c.stride, c.padding, c.dilation)
        return ops.fused_by_default(ci, co, pixels)

    def _packed(self):
        w = self.conv_dcn.weight
        return derived(self, "packed", lambda: ops.pack_deform_conv_weight(w), sources=w)

    def forward(self, x, norm=None, relu=False):
        """conv_dcn(x, offset, sigmoid(mask)); with `norm` (an eval-mode BatchNorm2d) and `relu` what the block applies
        behind it as well -- in the kernel's epilogue when fused."""
        c = self.conv_dcn
        offset_mask = self.conv_offset(x)
        offset, mask = offset_mask[:, :self.offset_channel], offset_mask[:, self.offset_channel:]
        if self.takes_kernel(x):
            scale, shift = None, c.bias
            if norm is not None:
                scale, shift = derived(self, "folded", sources=(norm, c.bias),
                                       build=lambda: fold_batch_norm(norm.weight, norm.bias, norm.running_mean,
                                                                     norm.running_var, norm.eps, c.bias))
            y = ops.deform_conv2d_packed(x, offset, mask, self._packed(), scale, shift, relu, True, c.stride, c.padding,
                                         c.dilation)
            if y is not None:
                return y
        y = c(x, offset, torch.sigmoid(mask))
        if norm is not None:
            y = norm(y)
        return F.relu(y) if relu else y


def _norm(cfg, num_features, init_val=1.0):
    if not isinstance(cfg, dict) or cfg.get("type_name") != "BatchNorm2D":
        raise NotImplementedError(f"norm_cfg {cfg!r}: only BatchNorm2D")
    bn = nn.BatchNorm2d(num_features, eps=1e-5)
    nn.init.constant_(bn.weight, init_val)
    return bn


def _conv(cfg, inplanes, planes, k, fused=True, **kw):
    """build_conv_layer: Conv2D without a config, DeformableConvV2 for `DeformConv2D`."""
    bias = kw.pop("bias_attr", True)
    if cfg is None:
        return nn.Conv2d(inplanes, planes, k, bias=bool(bias), **kw)
    cfg = dict(cfg)
    if cfg.pop("type_name", None) != "DeformConv2D":
        raise NotImplementedError("conv_cfg: only None and DeformConv2D")
    return DeformableConvV2(inplanes, planes, k, bias_attr=bias, fused=fused, **kw, **cfg)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, style="pytorch", conv_cfg=None,
                 norm_cfg=dict(type_name="BatchNorm2D"), dcn=None, zero_init_residual=True, fused=True):
        super().__init__()
        if style not in ("pytorch", "caffe"):
            raise ValueError(f"style must be 'pytorch' or 'caffe', got {style!r}")
        if conv_cfg is not None:
            raise NotImplementedError("Bottleneck: conv_cfg")
        if dcn is not None and not isinstance(dcn, dict):
            raise TypeError("dcn must be a dict")
        self.inplanes, self.planes, self.stride, self.dilation, self.style = inplanes, planes, stride, dilation, style
        self.with_dcn = dcn is not None
        self.conv1_stride, self.conv2_stride = (1, stride) if style == "pytorch" else (stride, 1)
        self.conv1 = _conv(None, inplanes, planes, 1, stride=self.conv1_stride, bias_attr=False)
        self.bn1 = _norm(norm_cfg, planes)
        self.conv2 = _conv(dcn, planes, planes, 3, fused, stride=self.conv2_stride, padding=dilation, dilation=dilation,
                           bias_attr=False)
        self.bn2 = _norm(norm_cfg, planes)
        self.conv3 = _conv(None, planes, planes * self.expansion, 1, bias_attr=False)
        self.bn3 = _norm(norm_cfg, planes * self.expansion, 0.0 if zero_init_residual else 1.0)
        self.relu = nn.ReLU()
        self.downsample = downsample

    norm1 = property(lambda self: self.bn1)
    norm2 = property(lambda self: self.bn2)
    norm3 = property(lambda self: self.bn3)

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        if self.with_dcn and not self.bn2.training:
            out = self.conv2(out, self.bn2, True)
        else:
            out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class ResLayer(nn.Sequential):
    def __init__(self, block, inplanes, planes, num_blocks, stride=1, conv_cfg=None,
                 norm_cfg=dict(type_name="BatchNorm2D"), downsample_first=True, **kwargs):
        if not downsample_first:
            raise NotImplementedError("ResLayer: downsample_first=False")
        self.block = block
        downsample = None
        if stride != 1 or inplanes != planes * block.expansion:
            downsample = nn.Sequential(_conv(conv_cfg, inplanes, planes * block.expansion, 1, stride=stride,
                                             bias_attr=False), _norm(norm_cfg, planes * block.expansion))
        layers = [block(inplanes=inplanes, planes=planes, stride=stride, downsample=downsample, conv_cfg=conv_cfg,
                        norm_cfg=norm_cfg, **kwargs)]
        inplanes = planes * block.expansion
        for _ in range(1, num_blocks):
            layers.append(block(inplanes=inplanes, planes=planes, stride=1, conv_cfg=conv_cfg, norm_cfg=norm_cfg, **kwargs))
        super().__init__(*layers)


class MMResNet(nn.Module):
    arch_settings = {50: (Bottleneck, (3, 4, 6, 3)), 101: (Bottleneck, (3, 4, 23, 3))}

    def __init__(self, depth, in_channels=3, stem_channels=None, base_channels=64, num_stages=4, strides=(1, 2, 2, 2),
                 dilations=(1, 1, 1, 1), out_indices=(0, 1, 2, 3), style="pytorch", frozen_stages=-1, conv_cfg=None,
                 norm_cfg=dict(type_name="BatchNorm2D", requires_grad=True), norm_eval=True, dcn=None,
                 stage_with_dcn=(False, False, False, False), zero_init_residual=True, pretrained=None, lr_factor=1,
                 fused=True):
        super().__init__()
        if depth not in self.arch_settings:
            if depth in (18, 34, 152):
                raise NotImplementedError(f"MMResNet: depth {depth} (the configs use 50 and 101)")
            raise KeyError(f"invalid depth {depth} for resnet")
        if conv_cfg is not None or pretrained is not None:
            raise NotImplementedError("MMResNet: conv_cfg and pretrained (load a checkpoint through paddle3d_amd.checkpoint)")
        if not 1 <= num_stages <= 4 or len(strides) != num_stages or len(dilations) != num_stages:
            raise ValueError("num_stages must be 1 .. 4 with as many strides and dilations")
        if max(out_indices) >= num_stages or (dcn is not None and len(stage_with_dcn) != num_stages):
            raise ValueError("out_indices and stage_with_dcn must fit num_stages")
        self.depth, self.out_indices, self.style, self.norm_eval = depth, tuple(out_indices), style, norm_eval
        self.frozen_stages, self.fused = frozen_stages, _check_fused(fused)
        stem = base_channels if stem_channels is None else stem_channels
        block, stage_blocks = self.arch_settings[depth]
        norm_cfg = {k: v for k, v in norm_cfg.items() if k != "requires_grad"}
        self.conv1 = nn.Conv2d(in_channels, stem, 7, stride=2, padding=3, bias=False)
        self.bn1 = _norm(norm_cfg, stem)
        self.relu = nn.ReLU()
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.res_layers = []
        inplanes = stem
        for i, num_blocks in enumerate(stage_blocks[:num_stages]):
            planes = base_channels * 2 ** i
            layer = ResLayer(block, inplanes, planes, num_blocks, stride=strides[i], dilation=dilations[i], style=style,
                             norm_cfg=norm_cfg, dcn=dcn if (dcn is not None and stage_with_dcn[i]) else None,
                             zero_init_residual=zero_init_residual, fused=fused)
            inplanes = planes * block.expansion
            self.add_module(f"layer{i + 1}", layer)
            self.res_layers.append(f"layer{i + 1}")
        self.feat_dim = block.expansion * base_channels * 2 ** (num_stages - 1)
        self.train(False)

    norm1 = property(lambda self: self.bn1)

    def train(self, mode: bool = True):
        """The reference's train(): with norm_eval every BatchNorm stays in eval mode."""
        super().train(mode)
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, nn.BatchNorm2d):
                    m.eval()
        return self

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        outs = []
        for i, name in enumerate(self.res_layers):
            x = getattr(self, name)(x)
            if i in self.out_indices:
                outs.append(x)
        return tuple(outs)


def mm_resnet50_caffe_dcn(out_indices=(2, 3), fused=True):
    """The img_backbone of configs/cape/cape_r50_1408x512_* and capet_r50_704x256_*: depth 50, caffe style, DCNv2 as
    conv2 of every bottleneck of stages 3 and 4, frozen BatchNorm statistics."""
    return MMResNet(depth=50, num_stages=4, out_indices=out_indices, frozen_stages=-1,
                    norm_cfg=dict(type_name="BatchNorm2D", requires_grad=False), norm_eval=True, style="caffe",
                    dcn=dict(type_name="DeformConv2D", deformable_groups=1), stage_with_dcn=(False, False, True, True),
                    fused=fused)
