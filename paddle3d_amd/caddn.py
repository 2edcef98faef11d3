"""CaDDN's frustum-to-voxel and map-to-BEV stage at inference on the device ops (configs/caddn/*.yml from ffe_cfg down;
paddle3d/models/detection/caddn).  The modules have the reference's constructor arguments, batch_dict keys and
state-dict keys, so checkpoint.load_paddle_state_dict places a `.pdparams` of the reference unchanged.

ConvBNReLU(in_channels, out_channels, kernel_size, padding='same', **kwargs)
                                    models/layers/layer_libs.py:316-339 (_conv, _batch_norm).
FrustumGridGenerator(voxel_size, pc_range, disc_cfg)
                                    f2v/frustum_grid_generator.py: forward(lidar_to_cam, cam_to_img, image_shape) ->
                                    [B, X, Y, Z, 3] (ops.caddn.frustum_grid).
Sampler(mode, padding_mode)         f2v/sampler.py: the 5-D grid_sample (torch's; the comparison path only).
FFE(ffe_cfg, disc_cfg)              ffe/ffe.py: channel_reduce and create_frustum_features, the UNFUSED comparison path
                                    (it forms the [B, C, D, h, w] frustum volume); the DDN loss is training only.
FrustumToVoxel(voxel_size, pc_range, sample_cfg, disc_cfg)
                                    f2v/frustum_to_voxel.py.  forward(batch_dict): with "frustum_features" it samples
                                    them through the grid as the reference does; with "image_features" and "depth_logits"
                                    instead it runs ops.caddn.frustum_to_voxel, which forms neither.  Either way
                                    batch_dict["voxel_features"] is [B, C, Z, Y, X].
FrustumToBEV(f2v_cfg, disc_cfg, map_to_bev_cfg, fused=True)
                                    caddn.py:110-122 from the reduced image features to spatial_features:
                                    forward(image_features, depth_logits, batch_dict) -> [B, C_out, Y, X], with the
                                    sublayers f2v and map_to_bev under CADDN's attribute names.  fused=True runs
                                    ops.caddn.frustum_to_bev (the voxel volume is never formed); fused=False, or a shape
                                    that kernel does not take, runs frustum_to_voxel and a torch 1x1 convolution.

Inference only; nothing in the forwards synchronises with the host.  The image backbone, the depth head, the 2-D BEV
backbone, the anchor head and the post-processing (roi_heads' class_agnostic_nms) are not part of this module.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .ops import caddn as _ops

__all__ = ["ConvBNReLU", "FrustumGridGenerator", "Sampler", "FFE", "FrustumToVoxel", "FrustumToBEV"]


class ConvBNReLU(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, padding="same", **kwargs):
        super().__init__()
        bias = kwargs.pop("bias_attr", None) is not False
        kwargs.pop("data_format", None)
        self._conv = nn.Conv2d(in_channels, out_channels, kernel_size, padding=padding, bias=bias, **kwargs)
        self._batch_norm = nn.BatchNorm2d(out_channels, eps=1e-5)
        self._relu = nn.ReLU()

    def forward(self, x):
        return self._relu(self._batch_norm(self._conv(x)))

    def folded(self):
        """(weight [C_out, C_in], scale, shift) of a 1x1 layer at inference: relu(scale * (weight @ x) + shift)."""
        bn, conv = self._batch_norm, self._conv
        if tuple(conv.kernel_size) != (1, 1) or tuple(conv.stride) != (1, 1) or conv.groups != 1:
            raise RuntimeError("ConvBNReLU.folded: a 1x1 stride-1 convolution only")
        scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        shift = bn.bias - bn.running_mean * scale
        if conv.bias is not None:
            shift = shift + conv.bias * scale
        return conv.weight.reshape(conv.out_channels, conv.in_channels), scale, shift


def _grid_size(voxel_size, pc_range):
    r = np.asarray(pc_range, dtype=np.float64)
    return tuple(int(v) for v in np.round((r[3:] - r[:3]) / np.asarray(voxel_size, dtype=np.float64)).astype(np.int64))


class FrustumGridGenerator(nn.Module):
    def __init__(self, voxel_size, pc_range, disc_cfg):
        super().__init__()
        self.grid_size = _grid_size(voxel_size, pc_range)  # (X, Y, Z)
        self.pc_min = [float(v) for v in pc_range[:3]]
        self.voxel_size = [float(v) for v in voxel_size]
        self.disc_cfg = dict(disc_cfg)
        self.out_of_bounds_val = -2

    def forward(self, lidar_to_cam, cam_to_img, image_shape):
        return _ops.frustum_grid(lidar_to_cam, cam_to_img, image_shape, self.grid_size, self.pc_min, self.voxel_size,
                                 self.disc_cfg)


class Sampler(nn.Module):
    def __init__(self, mode="bilinear", padding_mode="zeros"):
        super().__init__()
        self.mode, self.padding_mode = mode, padding_mode

    def forward(self, input_features, grid):
        # the reference passes 'bilinear' / 'zeros' whatever it was constructed with (sampler.py:46-51)
        return F.grid_sample(input_features, grid, mode="bilinear", padding_mode="zeros", align_corners=False)


class FFE(nn.Module):
    def __init__(self, ffe_cfg, disc_cfg):
        super().__init__()
        self.disc_cfg = dict(disc_cfg)
        self.downsample_factor = ffe_cfg["downsample_factor"]
        self.channel_reduce = ConvBNReLU(**ffe_cfg["channel_reduce_cfg"])

    @staticmethod
    def create_frustum_features(image_features, depth_logits):
        probs = F.softmax(depth_logits.unsqueeze(1), dim=2)[:, :, :-1]
        return probs * image_features.unsqueeze(2)

    def forward(self, image_features, depth_logits, batch_dict):
        if self.training:
            raise NotImplementedError("FFE: inference only")
        h, w = image_features.shape[2:]
        depth_logits = F.interpolate(depth_logits, size=[h, w], mode="bilinear", align_corners=False)
        batch_dict["image_features"] = self.channel_reduce(image_features)
        batch_dict["depth_logits"] = depth_logits
        return batch_dict


class FrustumToVoxel(nn.Module):
    def __init__(self, voxel_size, pc_range, sample_cfg, disc_cfg):
        super().__init__()
        self.pc_range = pc_range
        self.disc_cfg = dict(disc_cfg)
        self.grid_generator = FrustumGridGenerator(voxel_size=voxel_size, pc_range=pc_range, disc_cfg=disc_cfg)
        self.sampler = Sampler(**sample_cfg)

    def forward(self, batch_dict):
        g = self.grid_generator
        calib = (batch_dict["trans_lidar_to_cam"], batch_dict["trans_cam_to_img"], batch_dict["image_shape"])
        if "frustum_features" in batch_dict:
            voxel = self.sampler(batch_dict["frustum_features"], g(*calib)).permute(0, 1, 4, 3, 2)
        else:
            voxel = _ops.frustum_to_voxel(batch_dict["image_features"], batch_dict["depth_logits"], *calib, g.grid_size,
                                          g.pc_min, g.voxel_size, g.disc_cfg)
        batch_dict["voxel_features"] = voxel
        return batch_dict


class FrustumToBEV(nn.Module):
    def __init__(self, f2v_cfg, disc_cfg, map_to_bev_cfg, fused=True):
        super().__init__()
        self.f2v = FrustumToVoxel(**f2v_cfg, disc_cfg=disc_cfg)
        self.map_to_bev = ConvBNReLU(**map_to_bev_cfg)
        self.fused = bool(fused)

    def forward(self, image_features, depth_logits, batch_dict):
        if self.training:
            raise NotImplementedError("FrustumToBEV: inference only")
        g = self.f2v.grid_generator
        weight, scale, shift = self.map_to_bev.folded()
        C, Z = int(image_features.shape[1]), g.grid_size[2]
        if int(weight.shape[1]) != C * Z:
            raise RuntimeError(f"FrustumToBEV: map_to_bev takes {int(weight.shape[1])} channels, the voxels have {C} x {Z}")
        calib = (batch_dict["trans_lidar_to_cam"], batch_dict["trans_cam_to_img"], batch_dict["image_shape"])
        if self.fused and _ops.frustum_to_bev_supported(C, weight.shape[0], Z):
            bev = _ops.frustum_to_bev(image_features, depth_logits, *calib, g.grid_size, g.pc_min, g.voxel_size,
                                      g.disc_cfg, weight, scale, shift)
        else:
            voxel = _ops.frustum_to_voxel(image_features, depth_logits, *calib, g.grid_size, g.pc_min, g.voxel_size,
                                          g.disc_cfg)
            flat = voxel.flatten(1, 2)
            bev = torch.relu(F.conv2d(flat, weight[:, :, None, None]) * scale[None, :, None, None]
                             + shift[None, :, None, None])
        batch_dict["spatial_features"] = bev
        return bev
