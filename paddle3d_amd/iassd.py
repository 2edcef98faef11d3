"""IA-SSD's grouping and sampling on the device ops (paddle3d_amd/ops/pointnet2_ops.py).

QueryAndGroup(radius, nsample, use_xyz)   mirrors iassd_modules.py:29-60: ball query, group xyz relative to the
                                          centre, group features, concat [xyz, features] along channels.
sample_points(xyz, npoint, sample_type, cls_features=None)
                                          the sampling branch of SAModuleMSG_WithSampling.forward
                                          (iassd_modules.py:174-200): no downsample when N <= npoint, D-FPS, or
                                          ctr_aware (sigmoid of the class maximum, then torch.topk); returns
                                          (sample_idx [B, npoint] int32, new_xyz [B, npoint, 3]).
No host synchronisation on either path.

SAModuleMSG_WithSampling, Vote_layer, IASSD_Backbone, PointResidual_BinOri_Coder, IASSD_Head, IASSD
                                          the reference's modules at inference with its constructor arguments and
                                          state-dict keys (models/detection/iassd/); a set-abstraction scale runs as
                                          pd3_sa_msg_pool (fused=), the head's decode as pd3_iassd_decode, the NMS as
                                          ops.roi_head.class_agnostic_nms for the whole batch.
iassd_kitti(), iassd_waymo()              the two reference configs.
"""
from __future__ import annotations

import math

import torch

from .derived import derived
from .ops import pointnet2_ops

__all__ = ["QueryAndGroup", "sample_points", "SAModuleMSG_WithSampling", "Vote_layer", "IASSD_Backbone",
           "PointResidual_BinOri_Coder", "IASSD_Head", "IASSD", "iassd_kitti", "iassd_waymo", "MEASURED_FASTER"]


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


# ---- the model at inference ----------------------------------------------------------------------------------------
# (csrc/iassd.hip through ops/iassd.py: pd3_sa_msg_pool per fused scale, pd3_iassd_decode in the head.)

# Scales (c1, c2, c3, nsample) for which pd3_sa_msg_pool was measured faster than the composition over the pointnet2
# ops at B = 1 by more than the run-to-run spread, with the largest number of source points n at which that held
# (tools/prof/iassd.py, DESIGN.md section 4.5zc: all six at KITTI's shapes, 1.9 - 3.8 x, and five at Waymo's, 1.1 - 1.9 x;
# Waymo's first scale scans 65536 points for each of 16384 queries and is 0.77 x, so it stops at KITTI's n).  fused=True
# takes the kernel for these only; fused="force" takes it wherever it is supported.
MEASURED_FASTER = {(16, 16, 32, 16): 16384, (32, 32, 64, 32): 65536, (64, 64, 128, 16): 16384, (64, 96, 128, 32): 16384,
                   (128, 128, 256, 16): 4096, (128, 256, 256, 32): 4096}


def _fold_bn(bn):
    """(scale, shift) of an eval BatchNorm in fp32: scale = gamma / sqrt(var + eps), shift = beta - mean * scale."""
    scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.float() + bn.eps)
    return scale.contiguous(), (bn.bias.detach().float() - bn.running_mean.float() * scale).contiguous()


def _fold_stack(layers):
    """[(W [out, in], bias [out] or None, relu)] of a Sequential of 1x1 Conv / Linear (+ BatchNorm + ReLU) groups, each
    eval BatchNorm folded into the layer in front of it."""
    out, mods, i = [], list(layers), 0
    while i < len(mods):
        w = mods[i].weight.detach().float().reshape(mods[i].weight.shape[0], -1)
        b = None if mods[i].bias is None else mods[i].bias.detach().float()
        i += 1
        if i < len(mods) and isinstance(mods[i], torch.nn.modules.batchnorm._BatchNorm):
            scale, shift = _fold_bn(mods[i])
            w, b = w * scale[:, None], shift if b is None else b * scale + shift
            i += 1
        relu = i < len(mods) and isinstance(mods[i], torch.nn.ReLU)
        i += int(relu)
        out.append((w.contiguous(), b, relu))
    return out


def _run_rows(folded, rows):
    for w, b, relu in folded:
        rows = torch.nn.functional.linear(rows, w, b)
        if relu:
            rows = torch.relu(rows)
    return rows


class SAModuleMSG_WithSampling(torch.nn.Module):
    """iassd_modules.py:63-241 at inference.  fused=True: a scale runs as pd3_sa_msg_pool where the shape is supported
    and in MEASURED_FASTER up to its number of source points; "force": wherever it is supported; False: never.  Training mode, an avg_pool scale and CPU
    tensors take the unfused composition over QueryAndGroup."""

    def __init__(self, *, npoint, sample_range, sample_type, radii, nsamples, mlps, use_xyz=True, dilated_group=False,
                 pool_method="max_pool", aggregation_mlp, confidence_mlp, num_classes, fused=True):
        super().__init__()
        assert len(radii) == len(nsamples)
        if fused not in (True, False, "force"):
            raise ValueError(f"fused must be True, False or 'force', got {fused!r}")
        self.npoint, self.sample_type, self.sample_range = npoint, sample_type, sample_range
        self.dilated_group, self.pool_method, self.use_xyz, self.fused = dilated_group, pool_method, use_xyz, fused
        nn = torch.nn
        self.groupers, self.mlps = nn.ModuleList(), nn.ModuleList()
        out_channels = 0
        for i in range(len(radii)):
            if dilated_group:
                raise NotImplementedError
            self.groupers.append(QueryAndGroup(radii[i], nsamples[i], use_xyz=use_xyz))
            spec = list(mlps[i])
            if use_xyz:
                spec[0] += 3
            layers = []
            for k in range(len(spec) - 1):
                layers += [nn.Conv2d(spec[k], spec[k + 1], 1, bias=False), nn.BatchNorm2d(spec[k + 1]), nn.ReLU()]
            self.mlps.append(nn.Sequential(*layers))
            out_channels += spec[-1]
        self.aggregation_layer = self.confidence_layer = None
        if aggregation_mlp and len(self.mlps) > 0:
            layers = []
            for k in range(len(aggregation_mlp)):
                layers += [nn.Conv1d(out_channels, aggregation_mlp[k], 1, bias=False),
                           nn.BatchNorm1d(aggregation_mlp[k]), nn.ReLU()]
            out_channels = aggregation_mlp[k]  # the reference's: the last width (every layer reads the concat's)
            self.aggregation_layer = nn.Sequential(*layers)
        if confidence_mlp:
            layers = []
            for k in range(len(confidence_mlp)):
                layers += [nn.Conv1d(out_channels, confidence_mlp[k], 1, bias=False),
                           nn.BatchNorm1d(confidence_mlp[k]), nn.ReLU()]
                out_channels = confidence_mlp[k]
            layers.append(nn.Conv1d(out_channels, num_classes, 1, bias=True))
            self.confidence_layer = nn.Sequential(*layers)

    def scale_is_fused(self, i, n=None):
        """Whether scale i runs as pd3_sa_msg_pool (on GPU tensors in eval mode) with n source points per frame."""
        from .ops import iassd as ops

        m, g = self.mlps[i], self.groupers[i]
        if self.fused is False or self.pool_method != "max_pool" or not self.use_xyz or len(m) != 9:
            return False
        key = (m[0].out_channels, m[3].out_channels, m[6].out_channels, int(g.nsample))
        if not ops.sa_msg_pool_supported(*key):
            return False
        return self.fused == "force" or (key in MEASURED_FASTER and (n is None or n <= MEASURED_FASTER[key]))

    def _fold(self):
        def build():
            scales = []
            for m in self.mlps:
                if len(m) != 9:
                    scales.append(None)
                    continue
                w1 = m[0].weight.detach().float().reshape(m[0].out_channels, -1)
                p = [w1[:, :3].contiguous(), w1[:, 3:].contiguous(), *_fold_bn(m[1])]
                for k in (3, 6):
                    p += [m[k].weight.detach().float().reshape(m[k].out_channels, -1).contiguous(), *_fold_bn(m[k + 1])]
                scales.append(p)
            return dict(
                scales=scales,
                agg=None if self.aggregation_layer is None else _fold_stack(self.aggregation_layer),
                conf=None if self.confidence_layer is None else _fold_stack(self.confidence_layer))
        return derived(self, "folded", build, sources=(self.mlps, self.aggregation_layer, self.confidence_layer))

    def _unfused_scale(self, i, xyz, new_xyz, features):
        x = self.mlps[i](self.groupers[i](xyz, new_xyz, features))  # [B, C, npoint, nsample]
        if self.pool_method == "max_pool":
            return x.max(dim=-1).values
        if self.pool_method == "avg_pool":
            return x.mean(dim=-1)
        raise NotImplementedError

    def forward(self, xyz, features=None, cls_features=None, new_xyz=None, ctr_xyz=None):
        """xyz [B, N, 3], features [B, C, N] -> (new_xyz [B, npoint, 3], new_features [B, C', npoint], cls_features
        [B, npoint, num_class] or None)."""
        from .ops import iassd as ops

        sample_idx = None
        if ctr_xyz is None:
            sample_idx, new_xyz = sample_points(xyz, self.npoint, self.sample_type, cls_features)
        else:
            new_xyz = ctr_xyz
        device_path = xyz.is_cuda and not self.training
        if len(self.groupers) == 0:
            new_features = pointnet2_ops.gather_operation(features.contiguous(), sample_idx)
            rows = None
        elif not device_path:
            new_features = torch.cat([self._unfused_scale(i, xyz, new_xyz, features)
                                      for i in range(len(self.groupers))], dim=1)
            if self.aggregation_layer is not None:
                new_features = self.aggregation_layer(new_features)
            rows = None
        else:
            fd = self._fold()
            B, M = int(new_xyz.shape[0]), int(new_xyz.shape[1])
            widths = [m[-3].out_channels for m in self.mlps]
            rows = torch.empty((B, M, sum(widths)), dtype=torch.float32, device=xyz.device)
            q, p, col = new_xyz.contiguous(), xyz.contiguous(), 0
            pts = None if features is None else features.transpose(1, 2)  # [B, N, C]
            for i, g in enumerate(self.groupers):
                if self.scale_is_fused(i, int(p.shape[1])):
                    w_pos, w_feat, sc1, sh1, w2, sc2, sh2, w3, sc3, sh3 = fd["scales"][i]
                    f_in = None if pts is None else torch.matmul(pts, w_feat.t())
                    ops.sa_msg_pool(q, p, f_in, w_pos, sc1, sh1, w2, sc2, sh2, w3, sc3, sh3, g.radius, g.nsample,
                                    out=rows, col=col)
                else:
                    rows[:, :, col:col + widths[i]] = self._unfused_scale(i, xyz, new_xyz, features).transpose(1, 2)
                col += widths[i]
            if fd["agg"] is not None:
                rows = _run_rows(fd["agg"], rows.reshape(B * M, -1)).reshape(B, M, -1)
            new_features = rows.transpose(1, 2)
        if self.confidence_layer is None:
            cls_features = None
        elif device_path:
            r = new_features.transpose(1, 2) if rows is None else rows
            cls_features = _run_rows(self._fold()["conf"], r.reshape(-1, r.shape[-1])).reshape(r.shape[0], r.shape[1], -1)
        else:
            cls_features = self.confidence_layer(new_features).transpose(1, 2)
        return new_xyz, new_features, cls_features


class Vote_layer(torch.nn.Module):
    """iassd_modules.py:244-293."""

    def __init__(self, mlp_list, pre_channel, max_translate_range):
        super().__init__()
        nn = torch.nn
        self.mlps = None
        if len(mlp_list) > 0:
            layers = []
            for width in mlp_list:
                layers += [nn.Conv1d(pre_channel, width, 1, bias=False), nn.BatchNorm1d(width), nn.ReLU()]
                pre_channel = width
            self.mlps = nn.Sequential(*layers)
        self.ctr_reg = nn.Conv1d(pre_channel, 3, 1)
        self.register_buffer("max_offset_limit", None if max_translate_range is None else
                             torch.tensor(max_translate_range, dtype=torch.float32), persistent=False)

    def forward(self, xyz, features):
        """xyz [B, M, 3], features [B, C, M] -> (vote_xyz, the empty feature slice [B, M, 0], xyz, ctr_offsets)."""
        x = features if self.mlps is None else self.mlps(features)
        ctr_offsets = self.ctr_reg(x).transpose(1, 2)
        new_features, ctr_offsets = ctr_offsets[..., 3:], ctr_offsets[..., :3]
        if self.max_offset_limit is None:
            return xyz + ctr_offsets, new_features, xyz, ctr_offsets
        # the reference's two where()s: a NaN offset stays a NaN in both forms
        limit = self.max_offset_limit.to(ctr_offsets.dtype)
        limited = torch.maximum(torch.minimum(ctr_offsets, limit), -1 * limit)
        return xyz + limited, new_features, xyz, ctr_offsets


class IASSD_Backbone(torch.nn.Module):
    """iassd_backbone.py:29-275 at inference; forward(batch_dict) with the reference's keys in and out."""

    def __init__(self, npoint_list, sample_method_list, radius_list, nsample_list, mlps, layer_types, dilated_group,
                 aggregation_mlps, confidence_mlps, layer_input, ctr_index, max_translate_range, input_channel,
                 num_classes, fused=True):
        super().__init__()
        self.npoint_list, self.sample_method_list, self.radius_list = npoint_list, sample_method_list, radius_list
        self.nsample_list, self.mlps, self.layer_types, self.dilated_group = nsample_list, mlps, layer_types, dilated_group
        self.aggregation_mlps, self.confidence_mlps, self.layer_input = aggregation_mlps, confidence_mlps, layer_input
        self.ctr_idx_list, self.max_translate_range = ctr_index, max_translate_range
        channel_out_list = [input_channel - 3]
        self.SA_modules = torch.nn.ModuleList()
        channel_out = input_channel - 3
        for k in range(len(nsample_list)):
            channel_in = channel_out_list[layer_input[k]]
            if layer_types[k] == "SA_Layer":
                spec = [[channel_in] + list(m) for m in mlps[k]]
                channel_out = sum(s[-1] for s in spec)
                agg = list(aggregation_mlps[k]) if aggregation_mlps and aggregation_mlps[k] else None
                if agg:
                    channel_out = agg[-1]
                conf = list(confidence_mlps[k]) if confidence_mlps and confidence_mlps[k] else None
                self.SA_modules.append(SAModuleMSG_WithSampling(
                    npoint=npoint_list[k], sample_range=-1, sample_type=sample_method_list[k], radii=radius_list[k],
                    nsamples=nsample_list[k], mlps=spec, use_xyz=True, dilated_group=dilated_group[k],
                    aggregation_mlp=agg, confidence_mlp=conf, num_classes=num_classes, fused=fused))
            elif layer_types[k] == "Vote_Layer":
                self.SA_modules.append(Vote_layer(mlp_list=mlps[k], pre_channel=channel_in,
                                                  max_translate_range=max_translate_range))
            channel_out_list.append(channel_out)
        self.num_point_features = channel_out

    def forward(self, batch_dict):
        points, B = batch_dict["data"], batch_dict["batch_size"]
        batch_idx, xyz = points[:, 0].reshape(B, -1), points[:, 1:4].reshape(B, -1, 3)
        features = points[:, 4:].reshape(B, xyz.shape[1], -1).transpose(1, 2) if points.shape[-1] > 4 else None

        def coords(t):
            return torch.cat([batch_idx[:, :t.shape[1], None].float(), t.reshape(B, -1, t.shape[-1])], dim=-1)

        encoder_xyz, encoder_features, sa_ins_preds, encoder_coords = [xyz], [features], [], [coords(xyz)]
        li_cls_pred, var = None, {}
        for i, layer in enumerate(self.SA_modules):
            xyz_in, feat_in = encoder_xyz[self.layer_input[i]], encoder_features[self.layer_input[i]]
            if self.layer_types[i] == "SA_Layer":
                ctr_xyz = encoder_xyz[self.ctr_idx_list[i]] if self.ctr_idx_list[i] != -1 else None
                li_xyz, li_features, li_cls_pred = layer(xyz_in, feat_in, li_cls_pred, ctr_xyz=ctr_xyz)
            else:
                li_xyz, li_features, origin, offsets = layer(xyz_in, feat_in)
                var.update(ctr_offsets=offsets, centers=li_xyz, centers_origin=origin)
                encoder_coords.append(coords(origin))
            encoder_xyz.append(li_xyz)
            encoder_coords.append(coords(li_xyz))
            encoder_features.append(li_features)
            sa_ins_preds.append(coords(li_cls_pred) if li_cls_pred is not None else [])
        ctr_batch_idx = batch_idx[:, :encoder_xyz[-1].shape[1]].reshape(-1)
        for key in ("ctr_offsets", "centers", "centers_origin"):
            batch_dict[key] = torch.cat([ctr_batch_idx[:, None].float(), var[key].reshape(-1, 3)], dim=1)
        last = encoder_features[-1]
        batch_dict["centers_features"] = last.transpose(1, 2).reshape(-1, last.shape[1])
        batch_dict.update(ctr_batch_idx=ctr_batch_idx, encoder_xyz=encoder_xyz, encoder_coords=encoder_coords,
                          sa_ins_preds=sa_ins_preds, encoder_features=encoder_features)
        return batch_dict


class PointResidual_BinOri_Coder(torch.nn.Module):
    """iassd_coder.py:21-121, the decoding half.  decode() runs pd3_iassd_decode on GPU tensors and decode_paddle (the
    reference's operation order in torch) on CPU tensors."""

    def __init__(self, code_size=8, use_mean_size=True, **kwargs):
        super().__init__()
        self.bin_size = kwargs.get("bin_size", 12)
        self.code_size = 6 + 2 * self.bin_size
        self.bin_inter = 2 * math.pi / self.bin_size
        self.use_mean_size = use_mean_size
        self.register_buffer("mean_size", torch.tensor(kwargs["mean_size"], dtype=torch.float32) if use_mean_size
                             else None, persistent=False)
        if use_mean_size:
            assert float(self.mean_size.min()) > 0

    def decode(self, box_encodings, points, cls_preds):
        """box_encodings [N, 6 + 2 * bins], points [N, 3] (a column view is read in place), cls_preds [N, K] raw logits
        -> boxes [N, 7]."""
        if box_encodings.is_cuda:
            from .ops import iassd as ops

            return ops.iassd_decode(cls_preds, box_encodings, points, self.mean_size, self.bin_size)
        return self.decode_paddle(box_encodings, points, cls_preds.argmax(dim=-1) + 1)

    def decode_paddle(self, box_encodings, points, pred_classes=None):
        xt, yt, zt, dxt, dyt, dzt = torch.split(box_encodings[..., :6], 1, dim=-1)
        xa, ya, za = torch.split(points, 1, dim=-1)
        if self.use_mean_size:
            dxa, dya, dza = torch.split(self.mean_size[pred_classes - 1], 1, dim=-1)
            diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
            xg, yg, zg = xt * diagonal + xa, yt * diagonal + ya, zt * dza + za
            dxg, dyg, dzg = torch.exp(dxt) * dxa, torch.exp(dyt) * dya, torch.exp(dzt) * dza
        else:
            xg, yg, zg = xt + xa, yt + ya, zt + za
            dxg, dyg, dzg = torch.split(torch.exp(box_encodings[..., 3:6]), 1, dim=-1)
        bin_id = box_encodings[..., 6:6 + self.bin_size].argmax(dim=-1)
        bin_res = torch.gather(box_encodings[..., 6 + self.bin_size:], -1, bin_id.unsqueeze(-1)).squeeze(-1)
        rg = bin_id.to(torch.float32) * self.bin_inter - math.pi + self.bin_inter / 2
        rg = (rg + bin_res * (self.bin_inter / 2)).unsqueeze(-1)
        return torch.cat([xg, yg, zg, dxg, dyg, dzg, rg], dim=-1)


class IASSD_Head(torch.nn.Module):
    """iassd_head.py:33-78, 606-663 at inference (no loss, no target assignment)."""

    def __init__(self, input_channel, cls_fc, reg_fc, num_classes, target_config, loss_config=None):
        super().__init__()
        self.num_classes, self.target_config, self.loss_config = num_classes, target_config, loss_config
        self.box_coder = PointResidual_BinOri_Coder(**target_config.get("box_coder_config"))
        self.cls_center_layers = self.make_fc_layers(cls_fc, input_channel, num_classes)
        self.box_center_layers = self.make_fc_layers(reg_fc, input_channel, self.box_coder.code_size)
        self.forward_ret_dict = None

    @staticmethod
    def make_fc_layers(fc_cfg, input_channel, output_channel):
        nn, layers = torch.nn, []
        for width in fc_cfg:
            layers += [nn.Linear(input_channel, width, bias=False), nn.BatchNorm1d(width), nn.ReLU()]
            input_channel = width
        layers.append(nn.Linear(input_channel, output_channel, bias=True))
        return nn.Sequential(*layers)

    def generate_predicted_boxes(self, points, point_cls_preds, point_box_preds):
        return point_cls_preds, self.box_coder.decode(point_box_preds, points, point_cls_preds)

    def _fold(self):
        stacks = (self.cls_center_layers, self.box_center_layers)
        return derived(self, "folded", lambda: (_fold_stack(stacks[0]), _fold_stack(stacks[1])), sources=stacks)

    def forward(self, batch_dict):
        if self.training:
            raise NotImplementedError("IASSD_Head: inference only (no target assignment, no loss)")
        feats, centers = batch_dict["centers_features"], batch_dict["centers"]
        folded = self._fold()
        cls_preds, box_preds = _run_rows(folded[0], feats), _run_rows(folded[1], feats)
        ret = {"center_cls_preds": cls_preds, "center_box_preds": box_preds}
        for k in ("ctr_offsets", "centers", "centers_origin", "sa_ins_preds"):
            ret[k] = batch_dict[k]
        cls_preds, boxes = self.generate_predicted_boxes(centers[:, 1:4], cls_preds, box_preds)
        batch_dict.update(batch_cls_preds=cls_preds, batch_box_preds=boxes, batch_index=centers[:, 0],
                          cls_preds_normalized=False)
        ret["point_box_preds"] = boxes
        self.forward_ret_dict = ret
        return batch_dict


class IASSD(torch.nn.Module):
    """detection/iassd/iassd.py:37-212 at inference: backbone, head, class-agnostic NMS for the whole batch in one call."""

    def __init__(self, backbone, head, post_process_cfg):
        super().__init__()
        self.backbone, self.head, self.post_process_cfg = backbone, head, post_process_cfg

    def forward(self, batch_dict, as_list=False):
        if self.training:
            raise NotImplementedError("IASSD: inference only")
        with torch.no_grad():
            return self.post_process(self.head(self.backbone(batch_dict)), as_list=as_list)

    def post_process(self, batch_dict, as_list=False):
        """(boxes [B, post, 7], scores [B, post], labels [B, post] int64, count [B] int32), zero padded, without a host
        synchronisation; as_list=True: the reference's per-frame list of pred_boxes / pred_scores / pred_labels with
        its fake row (zero box, score 0, label -1) for a frame that keeps nothing (reads count on the host)."""
        from .ops import roi_head

        B = int(batch_dict["batch_size"])
        if batch_dict.get("cls_preds_normalized", False):
            raise NotImplementedError("post_process: raw class logits expected")
        boxes = batch_dict["batch_box_preds"].reshape(B, -1, 7)  # every frame has the last layer's npoint centres
        cls = batch_dict["batch_cls_preds"].reshape(B, boxes.shape[1], -1)
        out = roi_head.class_agnostic_nms(boxes, cls, self.post_process_cfg["nms_config"],
                                          score_thresh=self.post_process_cfg["score_thresh"], apply_sigmoid=True)
        if not as_list:
            return out
        bx, sc, lb, cnt = out
        cnt = cnt.tolist()
        preds = []
        for b in range(B):
            if cnt[b] == 0:
                preds.append({"pred_boxes": bx.new_zeros((1, 7)), "pred_scores": sc.new_zeros((1,)),
                              "pred_labels": sc.new_full((1,), -1.0)})
            else:
                preds.append({"pred_boxes": bx[b, :cnt[b]], "pred_scores": sc[b, :cnt[b]], "pred_labels": lb[b, :cnt[b]]})
        return preds


_SA = dict(sample_method_list=["D-FPS", "D-FPS", "ctr_aware", "ctr_aware", None, None],
           radius_list=[[0.2, 0.8], [0.8, 1.6], [1.6, 4.8], [], [], [4.8, 6.4]],
           nsample_list=[[16, 32], [16, 32], [16, 32], [], [], [16, 32]],
           mlps=[[[16, 16, 32], [32, 32, 64]], [[64, 64, 128], [64, 96, 128]], [[128, 128, 256], [128, 256, 256]], [],
                 [128], [[256, 256, 512], [256, 512, 1024]]],
           layer_types=["SA_Layer", "SA_Layer", "SA_Layer", "SA_Layer", "Vote_Layer", "SA_Layer"],
           dilated_group=[False] * 6, aggregation_mlps=[[64], [128], [256], [256], [], [512]],
           confidence_mlps=[[], [128], [256], [], [], []], layer_input=[0, 1, 2, 3, 4, 3],
           ctr_index=[-1, -1, -1, -1, -1, 5], max_translate_range=[3.0, 3.0, 2.0], num_classes=3)


def _iassd(npoint_list, input_channel, mean_size, nms_thresh, fused):
    backbone = IASSD_Backbone(npoint_list=npoint_list, input_channel=input_channel, fused=fused,
                              **{k: (list(v) if isinstance(v, list) else v) for k, v in _SA.items()})
    head = IASSD_Head(input_channel=512, cls_fc=[256, 256], reg_fc=[256, 256], num_classes=3, target_config={
        "gt_extra_width": [0.2, 0.2, 0.2], "extra_width": [1.0, 1.0, 1.0],
        "box_coder_config": {"angle_bin_num": 12, "use_mean_size": True, "mean_size": mean_size}})
    return IASSD(backbone, head, {"score_thresh": 0.1, "nms_config": {
        "nms_thresh": nms_thresh, "nms_pre_maxsize": 4096, "nms_post_maxsize": 500}})


def iassd_kitti(fused=True):
    """configs/iassd/iassd_kitti.yaml: 16384 points of (x, y, z, intensity) per frame."""
    return _iassd([4096, 1024, 512, 256, None, 256], 4, [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], 0.01,
                  fused)


def iassd_waymo(fused=True):
    """configs/iassd/iassd_waymo.yaml: 65536 points of (x, y, z, intensity, elongation) per frame."""
    return _iassd([16384, 4096, 2048, 1024, None, 1024], 5,
                  [[4.7, 2.1, 1.7], [0.91, 0.86, 1.73], [1.78, 0.84, 1.78]], 0.1, fused)
