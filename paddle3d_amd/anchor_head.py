"""The first-stage head of the reference's anchor-based two-stage detectors (Voxel R-CNN, PV-RCNN) at inference.

AnchorGenerator(anchor_range, anchor_generator_config)
                                               heads/dense_heads/target_assigner/anchor_generator.py:18-108.
                                               generate_anchors(feature_map_sizes) -> (anchors_list, each
                                               [nz, ny, nx, num_sizes, num_rotations, 7], num_anchors_per_location).
                                               The reference's order of operations is kept (the strides in float64 from
                                               the range and the map size, the shifts by a float32 arange of them), so
                                               the values are the reference's bit for bit.
AnchorHeadSingle(model_cfg, input_channels, class_names, voxel_size, point_cloud_range, anchor_generator_cfg,
                 num_dir_bins, anchor_target_cfg=None, predict_boxes_when_training=None, loss_weights=None, fused=None)
                                               heads/dense_heads/anchor_head.py:37-204 with the reference's constructor
                                               arguments (the training-only ones are accepted and ignored) and
                                               state-dict keys (conv_cls.*, conv_box.*, conv_dir_cls.*; `anchors` is a
                                               buffer that is not saved).  forward(batch_dict): spatial_features_2d
                                               [B, C, H, W] -> batch_cls_preds [B, A, num_class], batch_box_preds
                                               [B, A, 7], cls_preds_normalized = False; A = H * W * anchors per
                                               location, in the reference's order (y, x, class, rotation).

The three 1x1 convolutions read the same map.  fused=False is the transcription: three F.conv2d, the permutes, the
decode; it also serves CPU tensors.  fused=True stacks the three weight matrices into one
[nA * (num_class + 7 + num_dir_bins), C] GEMM and runs it as ONE launch of the library's 1x1 kernel
(ops.conv.patch_conv_bias_relu, mode 1, without the ReLU) into one NCHW map, so the input map is read once instead of
three times; the decode reads that map through strided views, without a [B, H, W, C] copy of it.  A shape the kernel
refuses (conv.patch_supported(1, C, rows, H, W): C % 16, H * W % 4) takes the transcription; fused="force" raises
there instead (and on CPU tensors).  fused=None: FUSED_HEAD_DEFAULT (DESIGN 4.5zd has the measurement behind it).  The
stacked, packed weight is kept with the signature of the parameters it was made from and rebuilt when that changes
(derived.py: a state-dict load, .to(), an in-place write, train()).

The decode (ResidualCoder.decode_paddle, utils/box_coder.py:66-100, and the direction fix of anchor_head.py:151-163) is
elementwise torch on the device, the same statements for both paths.  Nothing in forward synchronises with the host.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from ._lib import Paddle3DAmdError
from .derived import InferenceCache, derived
from .ops import conv as _conv
from .roi_heads import ResidualCoder

__all__ = ["AnchorGenerator", "AnchorHeadSingle", "FUSED_HEAD_DEFAULT"]

# Whether AnchorHeadSingle(fused=None) runs its three 1x1 convolutions as the one stacked GEMM.
FUSED_HEAD_DEFAULT = True


class AnchorGenerator:
    def __init__(self, anchor_range, anchor_generator_config):
        self.anchor_generator_cfg = anchor_generator_config
        # float64, as the head hands the range over (np.asarray of the config's list): the strides are float64 quotients
        self.anchor_range = np.asarray(anchor_range, dtype=np.float64)
        self.anchor_sizes = [cfg["anchor_sizes"] for cfg in anchor_generator_config]
        self.anchor_rotations = [cfg["anchor_rotations"] for cfg in anchor_generator_config]
        self.anchor_heights = [cfg["anchor_bottom_heights"] for cfg in anchor_generator_config]
        self.align_center = [cfg.get("align_center", False) for cfg in anchor_generator_config]
        assert len(self.anchor_sizes) == len(self.anchor_rotations) == len(self.anchor_heights)
        self.num_of_anchor_sets = len(self.anchor_sizes)

    def generate_anchors(self, grid_sizes):
        assert len(grid_sizes) == self.num_of_anchor_sets
        r = self.anchor_range
        all_anchors, num_anchors_per_location = [], []
        for grid_size, sizes, rotations, heights, align_center in zip(
                grid_sizes, self.anchor_sizes, self.anchor_rotations, self.anchor_heights, self.align_center):
            num_anchors_per_location.append(len(rotations) * len(sizes) * len(heights))
            gx, gy = np.int64(grid_size[0]), np.int64(grid_size[1])
            with np.errstate(divide="ignore"):  # a one-cell map: an infinite stride, as the reference's numpy quotient
                if align_center:
                    x_stride, y_stride = (r[3] - r[0]) / gx, (r[4] - r[1]) / gy
                    x_offset, y_offset = x_stride / 2, y_stride / 2
                else:
                    x_stride, y_stride = (r[3] - r[0]) / (gx - 1), (r[4] - r[1]) / (gy - 1)
                    x_offset, y_offset = 0, 0
            x_shifts = torch.arange(float(r[0] + x_offset), float(r[3] + 1e-5), float(x_stride), dtype=torch.float32)
            y_shifts = torch.arange(float(r[1] + y_offset), float(r[4] + 1e-5), float(y_stride), dtype=torch.float32)
            z_shifts = torch.tensor(heights, dtype=torch.float32)
            size = torch.tensor(sizes, dtype=torch.float32).reshape(-1, 3)
            rot = torch.tensor(rotations, dtype=torch.float32)
            nx, ny, nz, ns, nr = len(x_shifts), len(y_shifts), len(z_shifts), int(size.shape[0]), len(rot)
            anchors = torch.empty((nx, ny, nz, ns, nr, 7), dtype=torch.float32)
            anchors[..., 0] = x_shifts.view(nx, 1, 1, 1, 1)
            anchors[..., 1] = y_shifts.view(1, ny, 1, 1, 1)
            anchors[..., 2] = z_shifts.view(1, 1, nz, 1, 1)
            anchors[..., 3:6] = size.view(1, 1, 1, ns, 1, 3)
            anchors[..., 6] = rot.view(1, 1, 1, 1, nr)
            anchors = anchors.permute(2, 1, 0, 3, 4, 5).contiguous()  # [z, y, x, size, rotation, 7]
            anchors[..., 2] += anchors[..., 5] / 2  # bottom heights -> box centres
            all_anchors.append(anchors)
        return all_anchors, num_anchors_per_location


class AnchorHeadSingle(InferenceCache, nn.Module):
    def __init__(self, model_cfg, input_channels, class_names, voxel_size, point_cloud_range, anchor_generator_cfg,
                 num_dir_bins, anchor_target_cfg=None, predict_boxes_when_training=None, loss_weights=None, fused=None):
        super().__init__()
        if fused not in (None, True, False, "force"):
            raise ValueError(f"fused must be None, True, False or 'force', got {fused!r}")
        self.fused = FUSED_HEAD_DEFAULT if fused is None else fused
        self.model_cfg = model_cfg
        self.num_class = len(class_names)
        self.class_names = list(class_names)
        self.anchor_generator_cfg = anchor_generator_cfg
        self.num_dir_bins = int(num_dir_bins)
        self.box_coder = ResidualCoder()
        pcr = np.asarray(point_cloud_range)
        grid_size = np.round((pcr[3:] - pcr[:3]) / voxel_size).astype(np.int64)
        self.anchors_list, per_location = self.generate_anchors(grid_size, pcr, self.box_coder.code_size)
        self.register_buffer("anchors", torch.cat(self.anchors_list, dim=-3), persistent=False)
        self.num_anchors_per_location = sum(per_location)
        nA = self.num_anchors_per_location
        self.conv_cls = nn.Conv2d(input_channels, nA * self.num_class, kernel_size=1)
        self.conv_box = nn.Conv2d(input_channels, nA * self.box_coder.code_size, kernel_size=1)
        self.conv_dir_cls = nn.Conv2d(input_channels, nA * self.num_dir_bins, kernel_size=1)
        self.forward_ret_dict = {}
        self.init_weight()

    def init_weight(self):
        nn.init.constant_(self.conv_cls.bias, -float(np.log((1.0 - 0.01) / 0.01)))
        nn.init.normal_(self.conv_box.weight, mean=0.0, std=0.001)

    def generate_anchors(self, grid_size, point_cloud_range, anchor_ndim=7):
        assert anchor_ndim == 7
        generator = AnchorGenerator(anchor_range=point_cloud_range, anchor_generator_config=self.anchor_generator_cfg)
        feature_map_size = [grid_size[:2] // cfg["feature_map_stride"] for cfg in self.anchor_generator_cfg]
        return generator.generate_anchors(feature_map_size)

    @staticmethod
    def limit_period(val, offset=0.5, period=np.pi):
        return val - torch.floor(val / period + offset) * period

    def generate_predicted_boxes(self, batch_size, cls_preds, box_preds, dir_cls_preds=None):
        """cls_preds [B, H, W, nA * num_class], box_preds [B, H, W, nA * 7], dir_cls_preds [B, H, W, nA * bins] (views of
        any strides) -> (batch_cls_preds [B, A, num_class], batch_box_preds [B, A, 7])."""
        num_anchors = int(self.anchors.numel()) // 7
        h, w, nA = int(cls_preds.shape[1]), int(cls_preds.shape[2]), self.num_anchors_per_location
        if h * w * nA != num_anchors:
            raise RuntimeError(f"AnchorHeadSingle: a {h} x {w} map for {num_anchors} anchors ({nA} per location)")
        # one bottom height per class (every configuration of the reference): the anchors' order (y, x, size, rotation)
        # is the maps' (y, x, channel), and the decode stays on [B, H, W, nA] views of the maps.  Several heights: the
        # reference pairs its z-major anchors with the rows of the flat reshape, which is then restated as it is.
        lay = (batch_size, h, w, nA) if int(self.anchors.shape[0]) == 1 else (batch_size, num_anchors)
        anchors = self.anchors.reshape(1, *lay[1:], 7)
        batch_cls_preds = cls_preds.reshape(batch_size, num_anchors, -1)
        t = box_preds.reshape(batch_size, h, w, nA, 7)  # a view: the channel axis splits in place
        t = [t[..., c].reshape(lay) for c in range(7)]
        xa, ya, za, dxa, dya, dza, ra = (anchors[..., c] for c in range(7))
        diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
        cols = [t[0] * diagonal + xa, t[1] * diagonal + ya, t[2] * dza + za,
                torch.exp(t[3]) * dxa, torch.exp(t[4]) * dya, torch.exp(t[5]) * dza, t[6] + ra]
        if dir_cls_preds is not None:
            dir_offset, dir_limit_offset = self.model_cfg["dir_offset"], self.model_cfg["dir_limit_offset"]
            dir_labels = torch.argmax(dir_cls_preds.reshape(batch_size, h, w, nA, -1), dim=-1).reshape(lay)
            period = 2 * np.pi / self.num_dir_bins
            dir_rot = self.limit_period(cols[6] - dir_offset, dir_limit_offset, period)
            cols[6] = dir_rot + dir_offset + period * dir_labels.to(cols[6].dtype)
        return batch_cls_preds, torch.stack(cols, dim=-1).reshape(batch_size, num_anchors, 7)

    # ---- the three convolutions as one GEMM ---------------------------------------------------------------------
    def _rows(self):
        return self.num_anchors_per_location * (self.num_class + self.box_coder.code_size + self.num_dir_bins)

    def fused_supported(self, channels, h, w):
        """Whether the stacked GEMM serves a [*, channels, h, w] map."""
        return _conv.patch_supported(1, int(channels), self._rows(), int(h), int(w))

    def _stacked(self):
        """(packed [rows, C] weight in the 1x1 kernel's operand order, bias [rows]) of cls | box | dir."""
        def build():
            convs = (self.conv_cls, self.conv_box, self.conv_dir_cls)
            w = torch.cat([c.weight.detach().float() for c in convs], dim=0)
            b = torch.cat([c.bias.detach().float() for c in convs], dim=0).contiguous()
            return _conv.pack_patch_weight(w, 1, False), b
        return derived(self, "stacked", build)

    def _maps(self, x):
        """cls, box, dir predictions as [B, H, W, C'] views."""
        n, c, h, w = (int(s) for s in x.shape)
        take = self.fused in (True, "force") and x.is_cuda and x.dtype == torch.float32 and self.fused_supported(c, h, w)
        if self.fused == "force" and not take:
            raise Paddle3DAmdError(f"AnchorHeadSingle(fused='force'): unsupported configuration (a {tuple(x.shape)} "
                                   f"{x.dtype} map on {x.device}, {self._rows()} rows) (status -3)")
        if not take:
            return tuple(conv(x).permute(0, 2, 3, 1) for conv in (self.conv_cls, self.conv_box, self.conv_dir_cls))
        wp, bias = self._stacked()
        rows = self._rows()
        out = torch.empty((n, rows, h, w), dtype=torch.float32, device=x.device)
        _conv.patch_conv_bias_relu(x, wp, bias, 1, rows, out, 0, relu=False)
        k0 = self.num_anchors_per_location * self.num_class
        k1 = k0 + self.num_anchors_per_location * self.box_coder.code_size
        return tuple(out[:, a:b].permute(0, 2, 3, 1) for a, b in ((0, k0), (k0, k1), (k1, rows)))

    def forward(self, data_dict):
        if self.training:
            raise NotImplementedError("AnchorHeadSingle: inference only (targets and losses are not built)")
        x = data_dict["spatial_features_2d"]
        cls_preds, box_preds, dir_cls_preds = self._maps(x)
        self.forward_ret_dict = {"cls_preds": cls_preds, "box_preds": box_preds, "dir_cls_preds": dir_cls_preds}
        batch_size = int(data_dict["batch_size"]) if "batch_size" in data_dict else int(x.shape[0])
        with torch.no_grad():
            batch_cls_preds, batch_box_preds = self.generate_predicted_boxes(batch_size, cls_preds, box_preds,
                                                                             dir_cls_preds)
        data_dict["batch_cls_preds"] = batch_cls_preds
        data_dict["batch_box_preds"] = batch_box_preds
        data_dict["cls_preds_normalized"] = False
        return data_dict
