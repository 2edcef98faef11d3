"""SqueezeSegV3 for inference (reference paddle3d/models/backbones/sac.py, models/segmentation/squeezesegv3/
squeezesegv3.py): the SACRangeNet21 / SACRangeNet53 backbones and the model class, with the reference's constructor
arguments, attribute names and Sequential indices, so a Paddle checkpoint loads through checkpoint.load_paddle_state_dict
without a name table (`backbone.encoder.encoder_stages.2.layers.0.attention_layer._conv.weight`, `..._batch_norm._mean`,
`heads.4.weight`).

Inference only: Dropout2D is the identity, BatchNorm uses its running statistics, there is no loss.

SACISKBlock(num_channels, fused=True, conv3x3="auto")
    fused=True runs sigmoid(BN(conv7x7(xyz))) * unfold(feature) -> conv1x1 -> BN -> relu as ops.squeezeseg.sac_isk_forward
    (one launch, none of the three [N, 9C, H, W] tensors in memory) where `sac_isk_supported` holds and C <=
    SAC_FUSED_MAX_CHANNELS (128: at C = 256 the kernel is slower than torch on one frame; fused="force" takes it there
    too); otherwise, and with fused=False, `sac_isk_composition`: the same formula as torch operators.  Both use the BatchNorms folded once after
    loading (scale = gamma / sqrt(var + eps), shift = (bias - mean) * scale + beta).
conv3x3_bn_act(layer, x, act, kernel)
    the helper every remaining 3x3 stride-1 ConvBNLayer goes through (the block's second MLP convolution, the decoder's):
    `kernel` names a kernel of ops/conv.py ("direct", "winograd", "winograd43") taken when its *_supported predicate
    accepts the layer, else torch; "auto" is DEFAULT_CONV3X3's choice for the shape.
The stride-(1, 2) downsample, the (1, 4) transposed convolution, the 1x1 layers and the bilinear resize of xyz
(align_corners=True) are torch operators.

SqueezeSegV3.forward(image, proj_y, proj_x, offsets) takes ops.squeezeseg.range_project's outputs for the batch and
returns one label per point (0 for a point without a pixel); export_forward(image) returns the [N, H, W] prediction,
as the reference's does.  Neither synchronises with the host.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .derived import derived
from .ops import conv as conv_ops
from .ops import squeezeseg as ops

__all__ = ["ConvBNLayer", "DeconvBNLayer", "SACISKBlock", "DownsampleBlock", "EncoderStage", "Encoder",
           "InvertedResidual", "DecoderStage", "Decoder", "SACRangeNet", "SACRangeNet21", "SACRangeNet53", "SqueezeSegV3",
           "sac_isk_composition", "conv3x3_bn_act", "DEFAULT_CONV3X3", "SAC_FUSED_MAX_CHANNELS"]

# What "auto" picks for a 3x3 stride-1 layer, by (cin, cout); a shape that is not listed runs on torch.  The F(2x2, 3x3)
# Winograd kernel is the fastest of the candidates at each of the four SAC stages (1.6 to 2.7 x torch) and keeps the
# network inside the reference's bounds; the decoder's layers with cin != cout were not measured and stay on torch.  See
# DESIGN.md 4.5za for the table.
DEFAULT_CONV3X3 = {(32, 32): "winograd", (64, 64): "winograd", (128, 128): "winograd", (256, 256): "winograd"}
# The largest channel count at which SACISKBlock(fused=True) takes the kernel; a block built with fused="force" takes
# it wherever it is supported.  At one 64 x 1024 frame the kernel is 2.4, 2.1 and 1.5 x faster than the torch composition
# at C = 32, 64 and 128 and 0.88 x at C = 256 (the 64 x 128 stage), so C = 256 is opt-in.  See DESIGN.md 4.5za.
SAC_FUSED_MAX_CHANNELS = 128


def sac_isk_composition(xyz, feature, w, s_a, t_a, v, s_m, t_m):
    """relu(BN(conv1x1(unfold3x3(feature) * sigmoid(BN(conv7x7(xyz)))))) with the BatchNorms folded: w [9C, 3, 7, 7],
    s_a, t_a [9C], v [C, 9C], s_m, t_m [C]."""
    N, C, H, W = feature.shape
    u = F.unfold(feature, 3, padding=1).reshape(N, 9 * C, H, W)
    a = F.conv2d(xyz, w, None, padding=3) * s_a[None, :, None, None] + t_a[None, :, None, None]
    p = u * torch.sigmoid(a)
    y = F.conv2d(p, v.reshape(C, 9 * C, 1, 1)) * s_m[None, :, None, None] + t_m[None, :, None, None]
    return F.relu(y)


def _act(y, act):
    if act == "relu":
        return F.relu(y)
    if act == "leaky":
        return F.leaky_relu(y, 0.1)
    return y


_CONV3X3_KERNELS = {
    "direct": (lambda ci, co, h, w: conv_ops.supported(ci, co, h, w, 1), conv_ops.pack_conv3x3_weight,
               conv_ops.conv3x3_bias_relu),
    "winograd": (conv_ops.winograd_supported, conv_ops.pack_winograd_weight, conv_ops.conv3x3_winograd_bias_relu),
    "winograd43": (conv_ops.winograd43_supported, conv_ops.pack_winograd43_weight,
                   conv_ops.conv3x3_winograd43_bias_relu),
}


def conv3x3_kernel_for(kernel, cin, cout, h, w, device):
    """The name of the ops/conv.py kernel a 3x3 stride-1 layer runs on, or "torch"."""
    if kernel == "auto":
        kernel = DEFAULT_CONV3X3.get((cin, cout), "torch")
    if kernel == "torch" or device.type != "cuda" or w % 4 != 0:  # the kernels' rows are multiples of 4 wide
        return "torch"
    if kernel not in _CONV3X3_KERNELS:
        raise ValueError(f"conv3x3: unknown kernel {kernel!r}")
    return kernel if _CONV3X3_KERNELS[kernel][0](cin, cout, h, w) else "torch"


def conv3x3_bn_act(layer, x, act="relu", kernel="auto"):
    """act(BN(conv3x3(x))) for a stride-1, padding-1 ConvBNLayer with its BatchNorm folded into (scale, shift).  On a
    kernel of ops/conv.py the scale goes into the weights (packed once, kept on the layer in a slot named by the
    kernel), the shift is the kernel's bias, relu is the kernel's and a leaky relu follows it as a torch operator."""
    weight, (scale, shift) = layer._conv.weight, layer.folded()
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    name = conv3x3_kernel_for(kernel, cin, cout, int(x.shape[2]), int(x.shape[3]), x.device)
    if name == "torch":
        return _act(F.conv2d(x, weight, None, padding=1) * scale[None, :, None, None] + shift[None, :, None, None], act)
    _, pack, run = _CONV3X3_KERNELS[name]
    packed = derived(layer, name, sources=(weight, layer._batch_norm),
                     build=lambda: pack((weight.double() * scale.double()[:, None, None, None]).float().contiguous()))
    y = run(x.contiguous(), packed, shift, cout, relu=(act == "relu"))
    return y if act == "relu" else _act(y, act)


class ConvBNLayer(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=None, bn_momentum=.9):
        super().__init__()
        # Paddle's bias_attr=None creates a bias; only False omits it
        self._conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=_pair(stride), padding=_pair(padding),
                               bias=bias is not False)
        self._batch_norm = nn.BatchNorm2d(out_channels)

    def folded(self):
        """(scale, shift) float32 of the BatchNorm with the convolution's bias folded in, kept until either changes."""
        bn = self._batch_norm
        return derived(self, "folded", sources=(bn, self._conv.bias),
                       build=lambda: ops.fold_batch_norm(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps,
                                                         self._conv.bias))

    def forward(self, x):
        bn = self._batch_norm
        return F.batch_norm(self._conv(x), bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)


class DeconvBNLayer(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=None, bn_momentum=.9):
        super().__init__()
        self._deconv = nn.ConvTranspose2d(in_channels, out_channels, _pair(kernel_size), stride=_pair(stride),
                                          padding=_pair(padding), bias=bias is not False)
        self._batch_norm = nn.BatchNorm2d(out_channels)

    def forward(self, x):
        bn = self._batch_norm
        return F.batch_norm(self._deconv(x), bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)


def _pair(v):
    return tuple(v) if isinstance(v, (list, tuple)) else (v, v)


class SACISKBlock(nn.Module):
    """SAC-ISK.  forward(xyz, feature) -> (xyz, fused_feature)."""

    def __init__(self, num_channels, fused=True, conv3x3="auto"):
        super().__init__()
        self.num_channels = num_channels
        self.fused = fused
        self.conv3x3 = conv3x3
        self.attention_layer = ConvBNLayer(3, 9 * num_channels, 7, padding=3, bn_momentum=.9)
        self.position_mlp = nn.Sequential(
            ConvBNLayer(9 * num_channels, num_channels, 1, bn_momentum=.9), nn.ReLU(),
            ConvBNLayer(num_channels, num_channels, 3, padding=1, bn_momentum=.9), nn.ReLU())

    def _params(self):
        att, mlp = self.attention_layer, self.position_mlp[0]

        def build():
            C = self.num_channels
            s_a, t_a = att.folded()
            s_m, t_m = mlp.folded()
            f = dict(w=att._conv.weight.detach(), s_a=s_a, t_a=t_a, v=mlp._conv.weight.detach().reshape(C, 9 * C),
                     s_m=s_m, t_m=t_m)
            if ops.sac_isk_supported(C):
                f["w1p"] = ops.pack_sac_attention_weight(f["w"])
                f["w2p"] = ops.pack_sac_mlp_weight(f["v"])
            return f
        return derived(self, "params", build, sources=(att, mlp))

    def takes_kernel(self, feature):
        N, C, H, W = feature.shape
        if not self.fused or not feature.is_cuda or feature.dtype != torch.float32:
            return False
        if self.fused != "force" and C > SAC_FUSED_MAX_CHANNELS:
            return False
        return ops.sac_isk_supported(C, H, W, N)

    def first_layer(self, xyz, feature):
        """The block up to its 1x1 layer's relu."""
        f = self._params()
        if self.takes_kernel(feature):
            y = ops.sac_isk_forward(xyz, feature, f["w1p"], f["s_a"], f["t_a"], f["w2p"], f["s_m"], f["t_m"])
            if y is not None:
                return y
        return sac_isk_composition(xyz, feature, f["w"], f["s_a"], f["t_a"], f["v"], f["s_m"], f["t_m"])

    def forward(self, xyz, feature):
        y = self.first_layer(xyz, feature)
        z = conv3x3_bn_act(self.position_mlp[2], y, "relu", self.conv3x3)
        return xyz, z + feature


class DownsampleBlock(nn.Module):
    def __init__(self, in_channels, out_channels, bn_momentum=.9):
        super().__init__()
        self.ds_layer = nn.Sequential(
            ConvBNLayer(in_channels, out_channels, 3, stride=[1, 2], padding=1, bias=False, bn_momentum=bn_momentum),
            nn.LeakyReLU(.1))

    def forward(self, xyz, feature):
        feature = self.ds_layer(feature)
        xyz = F.interpolate(xyz, size=[xyz.shape[2], xyz.shape[3] // 2], mode="bilinear", align_corners=True)
        return xyz, feature


class EncoderStage(nn.Module):
    def __init__(self, num_blocks, in_channels, out_channels, dropout_prob, downsample=True, bn_momentum=.9, fused=True,
                 conv3x3="auto"):
        super().__init__()
        self.downsample = downsample
        self.layers = nn.ModuleList([SACISKBlock(in_channels, fused, conv3x3) for _ in range(num_blocks)])
        if downsample:
            self.layers.append(DownsampleBlock(in_channels, out_channels, bn_momentum=bn_momentum))
        self.dropout = nn.Identity()  # Dropout2D at inference

    def forward(self, xyz, feature):
        for layer in self.layers:
            xyz, feature = layer(xyz, feature)
        return xyz, self.dropout(feature)


class Encoder(nn.Module):
    def __init__(self, in_channels, num_stage_blocks=(1, 2, 8, 8, 4), dropout_prob=.01, bn_momentum=.9, fused=True,
                 conv3x3="auto"):
        super().__init__()
        down_channels = ((32, 64), (64, 128), (128, 256), (256, 256), (256, 256))
        self.conv3x3 = conv3x3
        self.conv_1 = nn.Sequential(
            ConvBNLayer(in_channels, 32, 3, stride=1, padding=1, bias=False, bn_momentum=bn_momentum), nn.LeakyReLU(.1))
        self.encoder_stages = nn.ModuleList([
            EncoderStage(n, in_ch, out_ch, dropout_prob, downsample=i < 3, bn_momentum=bn_momentum, fused=fused,
                         conv3x3=conv3x3)
            for i, (n, (in_ch, out_ch)) in enumerate(zip(num_stage_blocks, down_channels))])

    def forward(self, inputs):
        xyz = inputs[:, 1:4, :, :].contiguous()
        feature = self.conv_1(inputs)
        short_cuts = []
        for stage in self.encoder_stages:
            if stage.downsample:
                short_cuts.append(feature)
            xyz, feature = stage(xyz, feature)
        return feature, short_cuts


class InvertedResidual(nn.Module):
    def __init__(self, channels, bn_momentum=.9, conv3x3="auto"):
        super().__init__()
        self.conv3x3 = conv3x3
        self.conv = nn.Sequential(
            ConvBNLayer(channels[1], channels[0], 1, stride=1, padding=0, bias=False, bn_momentum=bn_momentum),
            nn.LeakyReLU(.1),
            ConvBNLayer(channels[0], channels[1], 3, stride=1, padding=1, bias=False, bn_momentum=bn_momentum),
            nn.LeakyReLU(.1))

    def forward(self, x):
        y = self.conv[1](self.conv[0](x))
        return conv3x3_bn_act(self.conv[2], y, "leaky", self.conv3x3) + x


class DecoderStage(nn.Module):
    def __init__(self, in_channels, out_channels, upsample=True, bn_momentum=.9, conv3x3="auto"):
        super().__init__()
        self.upsample = upsample
        self.conv3x3 = conv3x3
        self.layers = nn.ModuleList()
        if upsample:
            self.layers.append(DeconvBNLayer(in_channels, out_channels, [1, 4], stride=[1, 2], padding=[0, 1],
                                             bn_momentum=bn_momentum))
        else:
            self.layers.append(ConvBNLayer(in_channels, out_channels, 3, padding=1, bn_momentum=bn_momentum))
        self.layers.append(nn.LeakyReLU(.1))
        self.layers.append(InvertedResidual([in_channels, out_channels], bn_momentum=bn_momentum, conv3x3=conv3x3))

    def forward(self, feature):
        if self.upsample:
            feature = self.layers[1](self.layers[0](feature))
        else:
            feature = conv3x3_bn_act(self.layers[0], feature, "leaky", self.conv3x3)
        return self.layers[2](feature)


class Decoder(nn.Module):
    def __init__(self, dropout_prob=.01, bn_momentum=.9, conv3x3="auto"):
        super().__init__()
        up_channels = ((256, 256), (256, 256), (256, 128), (128, 64), (64, 32))
        self.decoder_stages = nn.ModuleList([
            DecoderStage(in_ch, out_ch, upsample=i > 1, bn_momentum=bn_momentum, conv3x3=conv3x3)
            for i, (in_ch, out_ch) in enumerate(up_channels)])
        self.dropout = nn.Identity()

    def forward(self, feature, short_cuts):
        short_cuts = list(short_cuts)
        feature_list = []
        for stage in self.decoder_stages:
            feature = stage(feature)
            if stage.upsample:
                feature = feature + short_cuts.pop()
            feature_list.append(feature)
        return feature_list


class SACRangeNet(nn.Module):
    """Backbone of SqueezeSegV3: RangeNet++ with spatially-adaptive convolution (SAC-ISK)."""

    def __init__(self, in_channels, num_layers=53, encoder_dropout_prob=.01, decoder_dropout_prob=.01, bn_momentum=.99,
                 pretrained=None, fused=True, conv3x3="auto"):
        if num_layers not in (21, 53):
            raise ValueError(f"Invalid number of layers ({num_layers}) for SACRangeNet backbone, supported values are "
                             "{21, 53}.")
        super().__init__()
        self.in_channels = in_channels
        self.pretrained = pretrained
        blocks = (1, 1, 2, 2, 1) if num_layers == 21 else (1, 2, 8, 8, 4)
        self.encoder = Encoder(in_channels, blocks, encoder_dropout_prob, bn_momentum=bn_momentum, fused=fused,
                               conv3x3=conv3x3)
        self.decoder = Decoder(decoder_dropout_prob, bn_momentum=bn_momentum, conv3x3=conv3x3)
        self.eval()
        if pretrained is not None:
            from .checkpoint import load_paddle_state_dict

            load_paddle_state_dict(self, pretrained)

    def forward(self, inputs):
        feature, short_cuts = self.encoder(inputs)
        return self.decoder(feature, short_cuts)


def SACRangeNet21(**kwargs):
    return SACRangeNet(num_layers=21, **kwargs)


def SACRangeNet53(**kwargs):
    return SACRangeNet(num_layers=53, **kwargs)


class SqueezeSegV3(nn.Module):
    def __init__(self, backbone, loss=None, num_classes=20, pretrained=None):
        super().__init__()
        self.backbone = backbone
        self.loss = None  # inference only
        self.heads = nn.ModuleList([nn.Conv2d(256, num_classes, 1), nn.Conv2d(256, num_classes, 1),
                                    nn.Conv2d(128, num_classes, 1), nn.Conv2d(64, num_classes, 1),
                                    nn.Conv2d(32, num_classes, 3, padding=1)])
        self.pretrained = pretrained
        self.eval()
        if pretrained is not None:
            from .checkpoint import load_paddle_state_dict

            load_paddle_state_dict(self, pretrained)

    def logits(self, range_images):
        return self.heads[-1](self.backbone(range_images)[-1])

    def export_forward(self, range_images):
        """[N, H, W] int64: the class of every pixel."""
        return torch.argmax(self.logits(range_images), dim=1)

    def forward(self, range_images, proj_y, proj_x, offsets):
        """range_images [N, in_channels, H, W], proj_y, proj_x int32 [P] and offsets int32 [N + 1] as
        ops.squeezeseg.range_project gives them -> labels int64 [P]: the prediction at the point's pixel, 0 for a point
        without one."""
        pred = self.export_forward(range_images)
        P = proj_y.shape[0]
        frame = torch.bucketize(torch.arange(P, device=pred.device, dtype=torch.int32), offsets[1:].contiguous(),
                                right=True).clamp_(max=pred.shape[0] - 1)
        y, x = proj_y.long(), proj_x.long()
        labels = pred[frame, y.clamp(min=0), x.clamp(min=0)]
        return torch.where((y < 0) | (x < 0), torch.zeros_like(labels), labels)
