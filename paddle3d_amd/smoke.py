"""SMOKE, the reference's monocular 3D detector, at inference: head and post-processing on the device.

Reference: paddle3d/models/detection/smoke/smoke.py:36-105 (SMOKE), smoke_predictor.py:28-123 (SMOKEPredictor),
processor.py:29-194 (PostProcessor), smoke_coder.py:25-383 (SMOKECoder), models/layers/layer_libs.py:36-116, :181-207,
layers/layer_norm.py:20-33; configs/smoke/*.yml.  Constructor arguments and state-dict keys are the reference's
(heads.class_head.{0,1,3}.*, heads.regression_head.{0,1,3}.*; BatchNorm's _mean / _variance as checkpoint.py maps them).
The backbone (DLA34 / HRNet) is any torch.nn.Module handed in.

    SMOKEPredictor(fused=...)(features)                 the reference's two maps: conv3x3 below, then torch layers
    SMOKEPredictor.conv3x3(features)                    the two 3x3 convolutions as ONE stacked 64 -> 512 launch of the
                                                        F(4x4, 3x3) Winograd kernel (relu=False) where
                                                        ops.conv.winograd43_supported holds and the head is at least
                                                        WINOGRAD_MIN_WIDTH wide (conv_kernel="winograd43": wherever it
                                                        is supported; "torch": never), else torch's convolution
    PostProcessor.forward_padded(predictions, targets)  (rows [B, K, 14], counts int32 [B]) on the device, no
                                                        synchronisation (ops.smoke.smoke_post_process)
    PostProcessor.forward(predictions, targets)         the reference's [n, 15] tensor (batch id last, empty when nothing
                                                        passes): exactly one host synchronisation
    PostProcessor.export_forward(predictions, cam_info) [B * K, 14]
    SMOKE.head_padded(features, targets, mode)          the fused path: conv3x3 + the LAZY entry point
                                                        (ops.smoke.smoke_head_forward): three launches of csrc/smoke.hip
                                                        behind the stacked convolution
    SMOKE.test_forward(samples) / export_forward        mirror the reference down to per-frame results

fused=False, CPU tensors and shapes the kernels refuse (ops.smoke.smoke_supported) take the plain torch transcription of
the reference below (`*_torch`).  Default of fused=True: LAZY_BY_DEFAULT, set from the measurement in DESIGN.md's SMOKE
section; the dense path (torch layers + the from-maps op) stays reachable as fused="dense".
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .derived import derived
from .ops import conv as conv_ops
from .ops import smoke as smoke_ops

__all__ = ["SMOKEPredictor", "PostProcessor", "SMOKECoder", "SMOKE", "group_norm", "smoke_dla34_no_dcn_kitti",
           "smoke_hrnet18_no_dcn_kitti", "LAZY_BY_DEFAULT", "WINOGRAD_MIN_WIDTH"]

# fused=True takes the lazy kernel sequence (see DESIGN.md's SMOKE section for the numbers); fused="dense" the other
LAZY_BY_DEFAULT = True
# conv_kernel="auto" takes the stacked F(4x4, 3x3) Winograd launch from this head width on: at 256, the width of every
# reference config, the module stays within 4 x the reference's own fp32 error with it; at 32 and 48 the transform's
# rounding (about ten times a direct convolution's) does not (DESIGN.md's SMOKE section has the figures), so narrower
# heads take torch's convolution unless conv_kernel="winograd43" asks for the kernel
WINOGRAD_MIN_WIDTH = 256
PI = 3.14159  # smoke_coder.py:269


def group_norm(out_channels):
    """layer_norm.py:20-33: 32 groups when the channels divide by 32, else 16."""
    return nn.GroupNorm(32 if out_channels % 32 == 0 else 16, out_channels)


def sigmoid_hm(x):
    return torch.sigmoid(x).clamp(min=1e-4, max=1 - 1e-4)


def nms_hm(heat_map, kernel=3):
    hmax = F.max_pool2d(heat_map, kernel, stride=1, padding=(kernel - 1) // 2)
    return heat_map * (hmax == heat_map).to(heat_map.dtype)


def select_topk(heat_map, K=100):
    """layer_libs.py:65-116: the top K per class, then the top K of those nc * K."""
    batch, c, _, width = heat_map.shape
    scores_all, inds_all = torch.topk(heat_map.reshape(batch, c, -1), K)
    ys = torch.div(inds_all, width, rounding_mode="floor").to(heat_map.dtype).reshape(batch, -1)
    xs = (inds_all % width).to(heat_map.dtype).reshape(batch, -1)
    scores, inds = torch.topk(scores_all.reshape(batch, -1), K)
    clses = torch.div(inds, K, rounding_mode="floor").to(heat_map.dtype)
    return dict(topk_score=scores, topk_inds_all=inds_all.reshape(batch, -1).gather(1, inds), topk_clses=clses,
                topk_ys=ys.gather(1, inds), topk_xs=xs.gather(1, inds))


def select_point_of_interest(batch, index, feature_maps):
    c = feature_maps.shape[1]
    fm = feature_maps.permute(0, 2, 3, 1).reshape(batch, -1, c)
    return fm.gather(1, index.reshape(batch, -1, 1).expand(-1, -1, c))


class SMOKECoder(nn.Module):
    """smoke_coder.py:25-383, the decoders the post-processing uses (torch transcription)."""

    def __init__(self, depth_ref, dim_ref):
        super().__init__()
        self.register_buffer("depth_ref", torch.tensor(depth_ref, dtype=torch.float32), persistent=False)
        self.register_buffer("dim_ref", torch.tensor(dim_ref, dtype=torch.float32).reshape(-1, 3), persistent=False)

    def decode_depth(self, depths_offset):
        return depths_offset * self.depth_ref[1].to(depths_offset.dtype) + self.depth_ref[0].to(depths_offset.dtype)

    @staticmethod
    def _obj_id(n, n_batch, device):
        return torch.arange(n_batch, device=device).repeat_interleave(n // n_batch)

    def decode_location(self, points, points_offset, depths, Ks, trans_mats):
        n = points_offset.shape[0]
        obj = self._obj_id(n, Ks.shape[0], Ks.device)
        proj = points_offset + points.reshape(-1, 2).to(points_offset.dtype)
        ext = torch.cat((proj, torch.ones((n, 1), dtype=proj.dtype, device=proj.device)), 1).unsqueeze(-1)
        img = torch.matmul(torch.linalg.inv(trans_mats)[obj], ext) * depths.reshape(n, -1, 1)
        return torch.matmul(torch.linalg.inv(Ks)[obj], img).squeeze(2)

    def decode_location_without_transmat(self, points, points_offset, depths, Ks, down_ratios=None):
        down_ratio = ((1, 1),) if down_ratios is None else down_ratios
        down_ratio = down_ratio[0]
        n = points_offset.shape[0]
        obj = self._obj_id(n, Ks.shape[0], Ks.device)
        proj = points.reshape(-1, 2) + points_offset
        proj = torch.stack([down_ratio[0] * proj[:, 0], down_ratio[1] * proj[:, 1]], 1)
        ext = torch.cat((proj, torch.ones((n, 1), dtype=proj.dtype, device=proj.device)), 1).unsqueeze(-1)
        return torch.matmul(torch.linalg.inv(Ks)[obj], ext * depths.reshape(n, -1, 1)).squeeze(2)

    def decode_dimension(self, cls_id, dims_offset):
        return dims_offset.exp() * self.dim_ref.to(dims_offset.dtype)[cls_id.flatten().long()]

    def decode_orientation(self, vector_ori, locations):
        locations = locations.reshape(-1, 3)
        rays = torch.atan(locations[:, 0] / (locations[:, 2] + 1e-7))
        alphas = torch.atan(vector_ori[:, 0] / (vector_ori[:, 1] + 1e-7))
        cos_pos_diff = ((vector_ori[:, 1] >= 0).float() * 2 - 1) * PI / 2
        alphas = alphas - cos_pos_diff
        rotys = alphas + rays
        diff = (rotys > PI).float() * 2 * PI + (rotys < -PI).float() * (-2) * PI
        return rotys - diff, alphas

    @staticmethod
    def _box2d(points, bbox_size):
        points = points.reshape(-1, 2)
        return torch.stack([points[:, 0] - bbox_size[:, 0] / 2, points[:, 1] - bbox_size[:, 1] / 2,
                            points[:, 0] + bbox_size[:, 0] / 2, points[:, 1] + bbox_size[:, 1] / 2], 1)

    def decode_bbox_2d(self, points, bbox_size, trans_mats, img_size):
        img_size = img_size.flatten()
        n = bbox_size.shape[0]
        inv = torch.linalg.inv(trans_mats)[self._obj_id(n, trans_mats.shape[0], trans_mats.device)]
        box = self._box2d(points, bbox_size)
        one = torch.ones((n, 1), dtype=box.dtype, device=box.device)
        top = torch.matmul(inv, torch.cat((box[:, :2], one), 1).unsqueeze(-1)).squeeze(2)[:, :2]
        bot = torch.matmul(inv, torch.cat((box[:, 2:], one), 1).unsqueeze(-1)).squeeze(2)[:, :2]
        box = torch.cat((top, bot), 1)
        zero = torch.zeros((), dtype=box.dtype, device=box.device)
        xs = torch.minimum(torch.maximum(box[:, ::2], zero), img_size[0].to(box.dtype))
        ys = torch.minimum(torch.maximum(box[:, 1::2], zero), img_size[1].to(box.dtype))
        return torch.stack([xs[:, 0], ys[:, 0], xs[:, 1], ys[:, 1]], 1)

    def decode_bbox_2d_without_transmat(self, points, bbox_size, down_ratios=None):
        down_ratio = ((1, 1),) if down_ratios is None else down_ratios
        down_ratio = down_ratio[0]
        box = self._box2d(points, bbox_size)
        return torch.stack([down_ratio[0] * box[:, 0], down_ratio[1] * box[:, 1], down_ratio[0] * box[:, 2],
                            down_ratio[1] * box[:, 3]], 1)


class SMOKEPredictor(nn.Module):
    """smoke_predictor.py:28-123."""

    def __init__(self, num_classes=3, reg_channels=(1, 2, 3, 2, 2), num_channels=256, norm_type="gn", in_channels=64,
                 fused=True, conv_kernel="auto"):
        super().__init__()
        self.fused, self.conv_kernel = fused, conv_kernel
        self.num_classes, self.reg_channels = int(num_classes), tuple(int(c) for c in reg_channels)
        self.reg_heads = sum(self.reg_channels)
        self.norm_type, self.num_channels, self.in_channels = norm_type, int(num_channels), int(in_channels)
        norm_func = nn.BatchNorm2d if norm_type == "bn" else group_norm
        self.dim_channel = slice(sum(self.reg_channels[:2]), sum(self.reg_channels[:3]))
        self.ori_channel = slice(sum(self.reg_channels[:3]), sum(self.reg_channels[:4]))

        def branch(out):
            return nn.Sequential(nn.Conv2d(in_channels, num_channels, 3, padding=1), norm_func(num_channels), nn.ReLU(),
                                 nn.Conv2d(num_channels, out, 1))

        self.class_head = branch(self.num_classes)
        self.regression_head = branch(self.reg_heads)
        nn.init.constant_(self.class_head[-1].bias, -2.19)
        for m in self.regression_head:
            if isinstance(m, nn.Conv2d):
                nn.init.constant_(m.bias, 0.0)

    def forward(self, features, fused=None):
        if (self.fused if fused is None else fused) and features.is_cuda:
            cls_feat, reg_feat = self.conv3x3(features)  # one stacked launch where the kernel takes the layer
            head_class, reg = self.class_head[1:](cls_feat), self.regression_head[1:](reg_feat)
        else:
            head_class, reg = self.class_head(features), self.regression_head(features)
        head_class = sigmoid_hm(head_class)
        dims = torch.sigmoid(reg[:, self.dim_channel]) - 0.5
        ori = F.normalize(reg[:, self.ori_channel])
        head_regression = torch.cat([reg[:, :self.dim_channel.start], dims, ori, reg[:, self.ori_channel.stop:]], 1)
        return [head_class, head_regression]

    @property
    def groups(self):
        norm = self.class_head[1]
        return norm.num_groups if isinstance(norm, nn.GroupNorm) else self.num_channels

    def conv3x3(self, features):
        """The two branches' 3x3 convolution outputs (class, regression) [B, C, H, W], without norm or ReLU: views of
        one stacked map from one Winograd launch where the kernel takes the layer, else torch's convolutions."""
        b, cin, h, w = features.shape
        c = self.num_channels
        convs = (self.class_head[0], self.regression_head[0])
        winograd = self.conv_kernel == "winograd43" or (self.conv_kernel == "auto" and c >= WINOGRAD_MIN_WIDTH)
        if (winograd and features.is_cuda and features.dtype == torch.float32 and
                conv_ops.winograd43_supported(cin, 2 * c, h, w)):
            def build():
                weight = torch.cat([m.weight for m in convs]).float()
                return (conv_ops.pack_winograd43_weight(weight),
                        torch.cat([m.bias for m in convs]).float().contiguous())
            packed = derived(self, "winograd43", build, sources=convs)
            pitch = conv_ops.pitch4(w)
            x = features.contiguous() if pitch == w else F.pad(features, (0, pitch - w))
            out = conv_ops.conv3x3_winograd43_bias_relu(x, packed[0], packed[1], 2 * c, relu=False, w_valid=w)
            return out[:, :c, :, :w], out[:, c:, :, :w]
        return tuple(m(features) for m in convs)

    def norm_tables(self, batch):
        """None for GroupNorm (the kernels compute the statistics); BatchNorm's running statistics as tables."""
        if self.norm_type != "bn":
            return None, None
        return tuple(smoke_ops.batch_norm_tables(m[1].running_mean, m[1].running_var, batch, m[1].eps)
                     for m in (self.class_head, self.regression_head))


class PostProcessor(nn.Module):
    """processor.py:29-194."""

    def __init__(self, depth_ref, dim_ref, reg_head=10, det_threshold=0.25, max_detection=50, pred_2d=True):
        super().__init__()
        self.smoke_coder = SMOKECoder(depth_ref, dim_ref)
        self.reg_head, self.max_detection, self.det_threshold, self.pred_2d = reg_head, max_detection, det_threshold, pred_2d

    # ---- the torch transcription -------------------------------------------------------------------------------------
    def _rows_torch(self, predictions, Ks, trans, image_size, export):
        heat, reg = predictions[0], predictions[1]
        batch = heat.shape[0]
        top = select_topk(nms_hm(heat), K=self.max_detection)
        scores, clses, ys, xs = top["topk_score"], top["topk_clses"], top["topk_ys"], top["topk_xs"]
        pois = select_point_of_interest(batch, top["topk_inds_all"], reg).reshape(-1, self.reg_head)
        points = torch.cat([xs.reshape(-1, 1), ys.reshape(-1, 1)], 1)
        coder = self.smoke_coder
        depths = coder.decode_depth(pois[:, 0])
        if export:
            locations = coder.decode_location_without_transmat(points, pois[:, 1:3], depths, Ks, trans)
        else:
            locations = coder.decode_location(points, pois[:, 1:3], depths, Ks, trans)
        dims = coder.decode_dimension(clses, pois[:, 3:6])
        locations = torch.cat([locations[:, :1], locations[:, 1:2] + dims[:, 1:2] / 2, locations[:, 2:]], 1)
        rotys, alphas = coder.decode_orientation(pois[:, 6:8], locations)
        if export:
            box2d = coder.decode_bbox_2d_without_transmat(points, pois[:, 8:10], trans)
        elif self.pred_2d:
            box2d = coder.decode_bbox_2d(points, pois[:, 8:10], trans, image_size)
        else:
            raise RuntimeError("PostProcessor: pred_2d=False cannot run in the reference either (its concat fails)")
        return torch.cat([clses.reshape(-1, 1), alphas.reshape(-1, 1), box2d, dims[:, 1:2], dims[:, 2:3], dims[:, 0:1],
                          locations, rotys.reshape(-1, 1), scores.reshape(-1, 1)], 1)

    def forward_torch(self, predictions, targets):
        result = self._rows_torch(predictions, targets["K"], targets["trans_mat"], targets["image_size"], False)
        keep = result[:, -1] > self.det_threshold
        batch = targets["K"].shape[0]
        ids = torch.arange(batch, dtype=result.dtype, device=result.device).repeat_interleave(self.max_detection)
        result = torch.cat([result, ids.reshape(-1, 1)], 1)[keep]
        return result if result.shape[0] else result.new_zeros((0,))

    def export_forward_torch(self, predictions, cam_info):
        return self._rows_torch(predictions, cam_info[0], cam_info[1], None, True)

    def padded_torch(self, predictions, targets=None, cam_info=None):
        """(rows [B, K, 14], counts) in the kernels' form from the torch transcription."""
        export = cam_info is not None
        rows = (self.export_forward_torch(predictions, cam_info) if export else
                self._rows_torch(predictions, targets["K"], targets["trans_mat"], targets["image_size"], False))
        rows = rows.reshape(predictions[0].shape[0], self.max_detection, 14)
        if export:
            return rows, torch.full((rows.shape[0],), self.max_detection, dtype=torch.int32, device=rows.device)
        keep = rows[..., -1] > self.det_threshold
        return rows * keep[..., None].to(rows.dtype), keep.sum(1).to(torch.int32)

    # ---- the device path -----------------------------------------------------------------------------------------------
    def _device_ok(self, heat, fused):
        return bool(fused) and heat.is_cuda and heat.dtype == torch.float32 and self.reg_head == 10

    def forward_padded(self, predictions, targets=None, cam_info=None, fused=True):
        """(rows [B, K, 14], counts int32 [B]) on the predictions' device, no host synchronisation.  targets: the
        forward mode; cam_info = [K, down_ratios]: the export mode."""
        heat, reg = predictions[0], predictions[1]
        if self._device_ok(heat, fused):
            c = self.smoke_coder
            if cam_info is None:
                args = (targets["K"].float(), targets["trans_mat"].float(), targets["image_size"].float())
                mode = smoke_ops.FORWARD
            else:
                args = (cam_info[0].float(), torch.as_tensor(cam_info[1], dtype=torch.float32, device=heat.device), None)
                mode = smoke_ops.EXPORT
            out = smoke_ops.smoke_post_process(heat, reg, *args, c.depth_ref, c.dim_ref, self.max_detection,
                                               self.det_threshold, mode, pred_2d=self.pred_2d)
            if out is not None:
                return out
        return self.padded_torch(predictions, targets, cam_info)

    @staticmethod
    def rows_to_result(rows, counts):
        """The reference's [n, 15] tensor from padded rows: the batch id as the last column, an empty tensor when
        nothing passes.  The boolean index is the one host synchronisation."""
        b, k, _ = rows.shape
        keep = torch.arange(k, device=rows.device)[None] < counts[:, None]
        ids = torch.arange(b, dtype=rows.dtype, device=rows.device)[:, None, None].expand(b, k, 1)
        result = torch.cat([rows, ids], 2)[keep]
        return result if result.shape[0] else result.new_zeros((0,))

    def forward(self, predictions, targets, fused=True):
        if not self._device_ok(predictions[0], fused):
            return self.forward_torch(predictions, targets)
        return self.rows_to_result(*self.forward_padded(predictions, targets, fused=fused))

    def export_forward(self, predictions, cam_info, fused=True):
        if not self._device_ok(predictions[0], fused):
            return self.export_forward_torch(predictions, cam_info)
        return self.forward_padded(predictions, cam_info=cam_info, fused=fused)[0].reshape(-1, 14)


class SMOKE(nn.Module):
    """smoke.py:31-145 at inference."""

    def __init__(self, backbone, head, depth_ref, dim_ref, max_detection=50, pred_2d=True, box_with_velocity=False,
                 fused=True):
        super().__init__()
        self.backbone, self.heads, self.max_detection, self.fused = backbone, head, max_detection, fused
        self.post_process = PostProcessor(depth_ref=depth_ref, dim_ref=dim_ref, reg_head=head.reg_heads,
                                          max_detection=max_detection, pred_2d=pred_2d)

    def _features(self, images):
        features = self.backbone(images)
        return features[-1] if isinstance(features, (list, tuple)) else features

    def lazy_supported(self, features):
        h = self.heads
        return (features.is_cuda and features.dtype == torch.float32 and
                smoke_ops.smoke_supported(h.num_channels, h.groups, h.num_classes, features.shape[2], features.shape[3],
                                          self.max_detection, h.reg_channels, self.post_process.pred_2d))

    def head_padded(self, features, targets=None, cam_info=None, fused=None):
        """(rows [B, K, 14], counts int32 [B]) from the backbone's features, no host synchronisation.  fused: True
        (LAZY_BY_DEFAULT decides between the two device paths), "lazy", "dense" or False (torch)."""
        fused = self.fused if fused is None else fused
        lazy = fused == "lazy" or (fused is True and LAZY_BY_DEFAULT)
        h, pp = self.heads, self.post_process
        if lazy and self.lazy_supported(features):
            cls_feat, reg_feat = h.conv3x3(features)
            tabs = h.norm_tables(features.shape[0])
            if cam_info is None:
                cam = (targets["K"].float(), targets["trans_mat"].float(), targets["image_size"].float())
                mode = smoke_ops.FORWARD
            else:
                cam = (cam_info[0].float(), torch.as_tensor(cam_info[1], dtype=torch.float32, device=features.device),
                       None)
                mode = smoke_ops.EXPORT
            cn, rn, c1, r1 = h.class_head[1], h.regression_head[1], h.class_head[3], h.regression_head[3]
            out = smoke_ops.smoke_head_forward(cls_feat, reg_feat, (cn.weight, cn.bias), (rn.weight, rn.bias), c1.weight,
                                               c1.bias, r1.weight, r1.bias, *cam, pp.smoke_coder.depth_ref,
                                               pp.smoke_coder.dim_ref, h.groups, self.max_detection, pp.det_threshold,
                                               mode, tabs[0], tabs[1], h.reg_channels, pp.pred_2d)
            if out is not None:
                return out
        return pp.forward_padded(h(features, fused=bool(fused)), targets, cam_info, fused=bool(fused))

    def export_forward(self, samples, fused=None):
        features = self._features(samples["images"])
        return self.head_padded(features, cam_info=[samples["trans_cam_to_img"], samples["down_ratios"]],
                                fused=fused)[0].reshape(-1, 14)

    def test_forward(self, samples, fused=None):
        features = self._features(samples["data"])
        rows, counts = self.head_padded(features, targets=samples["target"], fused=fused)
        results = PostProcessor.rows_to_result(rows, counts)
        return {"preds": [self._parse_results_to_sample(results, samples, i) for i in range(rows.shape[0])]}

    def forward(self, samples, fused=None):
        with torch.no_grad():
            return self.test_forward(samples, fused)

    @staticmethod
    def _parse_results_to_sample(results, sample, index):
        """smoke.py:112-145 with plain dicts for Sample / BBoxes2D / BBoxes3D (KittiCamera coordinates, origin
        (0.5, 1, 0.5), rot_axis 1)."""
        ret = {"path": sample["path"][index] if "path" in sample else None,
               "modality": sample["modality"][index] if "modality" in sample else None,
               "meta": {k: v[index] for k, v in sample.get("meta", {}).items()}}
        if "calibs" in sample:
            ret["calibs"] = [c[index] for c in sample["calibs"]]
        if results.shape[0] != 0:
            r = results[results[:, 14] == index][:, :14].cpu().numpy()
            ret.update(labels=r[:, 0], bboxes_2d=r[:, 2:6], bboxes_3d=r[:, [9, 10, 11, 8, 6, 7, 12]],
                       confidences=r[:, 13])
        return ret


_KITTI = dict(depth_ref=(28.01, 16.32), dim_ref=((3.88, 1.63, 1.53), (1.78, 1.70, 0.58), (0.88, 1.73, 0.67)),
              max_detection=50, pred_2d=True)


def smoke_dla34_no_dcn_kitti(backbone, fused=True):
    """configs/smoke/smoke_dla34_no_dcn_kitti.yml."""
    head = SMOKEPredictor(num_classes=3, reg_channels=(1, 2, 3, 2, 2), num_channels=256, norm_type="gn", in_channels=64,
                          fused=bool(fused))
    return SMOKE(backbone, head, fused=fused, **_KITTI)


def smoke_hrnet18_no_dcn_kitti(backbone, fused=True):
    """configs/smoke/smoke_hrnet18_no_dcn_kitti.yml (in_channels 270: the 3x3 convolutions are torch's)."""
    head = SMOKEPredictor(num_classes=3, reg_channels=(1, 2, 3, 2, 2), num_channels=256, norm_type="gn", in_channels=270,
                          fused=bool(fused))
    return SMOKE(backbone, head, fused=fused, **_KITTI)
