"""BEVFormer's decoder, detection head and NMS-free decode at inference on the device ops (paddle3d/models/transformers:
decoders.py, decoder_layers.py, transformer.py:361-392, attentions/multihead_attention.py,
attentions/spatial_cross_attention.py:431-640; detection/bevformer/bevformer_head.py:284-332, :613-634;
utils/box_coder.py:103-214).  The modules have the reference's constructor arguments, forward signatures and state-dict
keys, so checkpoint.load_paddle_state_dict places the head's entries of a BEVFormer `.pdparams` unchanged.

MultiheadAttention(embed_dims, num_heads, attn_drop, proj_drop, dropout_layer, batch_first, fused=True)
                                    the wrapper of paddle.nn.MultiHeadAttention (attn.q_proj / k_proj / v_proj /
                                    out_proj).  fused=True without attn_mask / key_padding_mask: the three Linears, then
                                    ops.bevformer_decoder.multihead_attention (the [M, Nq, Nk] scores never reach memory),
                                    then out_proj.  Otherwise the same arithmetic in torch.  Inside a decoder layer
                                    the kernel is opt-in (`fused=True` in the attention's own cfg; the layer's `fused`
                                    reaches the cross-attention only): measured at the tiny config it is no faster than
                                    torch's four kernels.
CustomMSDeformableAttention(embed_dims, num_heads, num_levels, num_points, im2col_step, dropout, batch_first, norm_cfg,
                            fused=True)
                                    fused=True: ops.bevformer_decoder.decoder_cross_attention_sample on the raw Linear
                                    rows; otherwise (or reference points of 4, or a refused shape) softmax and sampling
                                    locations in torch and ops.ms_deform_attn.
DetrTransformerDecoderLayer(attn_cfgs, feedforward_channels, ffn_dropout, operation_order, ..., fused=True)
DetectionTransformerDecoder(transformerlayers, num_layers, return_intermediate, fused=True)
                                    with the box refinement of decoders.py:112-124, in torch.
PerceptionTransformer(..., encoder=None, decoder=None, embed_dims, ..., fused=True)
                                    decode(bev_embed, object_query_embed, bev_h, bev_w, reg_branches) is the decoder half
                                    of forward (transformer.py:361-392); get_bev_features (can-bus shift, rotation of
                                    prev_bev, camera / level embeddings) is not implemented.
NMSFreeCoder(point_cloud_range, voxel_size, post_center_range, max_num, score_threshold, num_classes, fused=True)
                                    decode(preds_dicts) -> (boxes [B, max_num, code - 1], scores, labels int32, count):
                                    one launch for the batch, no host synchronisation; to_list() gives the reference's
                                    list of dicts and is the only place that synchronises.
BEVFormerHead(num_classes, in_channels, transformer, bbox_coder, num_query, num_reg_fcs, with_box_refine, bev_h, bev_w,
              code_size, positional_encoding=None, ...)
                                    forward_from_bev(bev_embed) is bevformer_head.py:284-332 on a BEV map [bs, H*W, E];
                                    get_bboxes(preds_dicts) decodes with z moved to the box bottom.

Where this departs from the reference, on purpose:
  * CustomMSDeformableAttention does not assert sum(H_l * W_l) == num_value (a host read of a device tensor), and its
    key_padding_mask zeroes the value rows (the reference calls an undefined masked_fill there).
  * max_num is at most 1024 and at most num_query * num_classes (the reference's topk raises beyond the latter).
  * The coder's post_center_range is required (the reference raises NotImplementedError without it).

Linear, LayerNorm, the FFN, the sigmoid / inverse_sigmoid of the refinement and the head's branches are torch.  Inference
only; nothing in the forwards synchronises with the host.
"""
from __future__ import annotations

import copy

import torch
from torch import nn

from .bevformer import FFN, _bev_levels, _check_heads, _normalizer
from .ops import bevformer_decoder as _ops
from .ops.ms_deform_attn import ms_deform_attn

__all__ = ["MultiheadAttention", "CustomMSDeformableAttention", "DetrTransformerDecoderLayer",
           "DetectionTransformerDecoder", "PerceptionTransformer", "NMSFreeCoder", "BEVFormerHead", "inverse_sigmoid"]


def inverse_sigmoid(x, eps=1e-5):
    x = x.clamp(min=0, max=1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


class _PaddleMHA(nn.Module):
    """The parameters of paddle.nn.MultiHeadAttention (kdim = vdim = embed_dim)."""

    def __init__(self, embed_dim, num_heads):
        super().__init__()
        self.embed_dim, self.num_heads, self.head_dim = embed_dim, num_heads, embed_dim // num_heads
        self.q_proj = nn.Linear(embed_dim, embed_dim)
        self.k_proj = nn.Linear(embed_dim, embed_dim)
        self.v_proj = nn.Linear(embed_dim, embed_dim)
        self.out_proj = nn.Linear(embed_dim, embed_dim)


class MultiheadAttention(nn.Module):
    def __init__(self, embed_dims, num_heads, attn_drop=0.0, proj_drop=0.0, dropout_layer=dict(type_name="Dropout", p=0.0),
                 batch_first=False, fused=True, **kwargs):
        super().__init__()
        _check_heads(embed_dims, num_heads)
        dropout_layer = copy.deepcopy(dropout_layer)
        if "dropout" in kwargs:
            attn_drop = kwargs.pop("dropout")
            dropout_layer["p"] = attn_drop
        self.embed_dims = embed_dims
        self.num_heads = num_heads
        self.batch_first = batch_first
        self.attn = _PaddleMHA(embed_dims, num_heads)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj_drop = nn.Dropout(proj_drop)
        if dropout_layer:
            cfg = dict(dropout_layer)
            self.dropout_layer = getattr(nn, cfg.pop("type_name"))(**cfg)
        else:
            self.dropout_layer = nn.Identity()
        self.fused = bool(fused)

    def core(self, q, k, v, attn_mask=None):
        """The projected q [B, Nq, E], k, v [B, Nk, E] -> [B, Nq, E] in torch: paddle.nn.MultiHeadAttention's core."""
        b, nq, e = q.shape
        m, d = self.num_heads, e // self.num_heads
        q, k, v = (t.reshape(b, t.shape[1], m, d).permute(0, 2, 1, 3) for t in (q, k, v))
        product = torch.matmul(q * (d ** -0.5), k.transpose(-1, -2))
        if attn_mask is not None:
            if attn_mask.dtype == torch.bool:
                attn_mask = (attn_mask.to(product.dtype) - 1.0) * 1e9
            product = product + attn_mask
        weights = self.attn_drop(torch.softmax(product, -1))
        return torch.matmul(weights, v).permute(0, 2, 1, 3).reshape(b, nq, e)

    def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_pos=None, attn_mask=None,
                key_padding_mask=None, **kwargs):
        if self.training:
            raise NotImplementedError("MultiheadAttention: inference only")
        if key is None:
            key = query
        if value is None:
            value = key
        if identity is None:
            identity = query
        if key_pos is None and query_pos is not None and query_pos.shape == key.shape:
            key_pos = query_pos
        if query_pos is not None:
            query = query + query_pos
        if key_pos is not None:
            key = key + key_pos
        if not self.batch_first:
            query, key, value = query.permute(1, 0, 2), key.permute(1, 0, 2), value.permute(1, 0, 2)
        if key_padding_mask is not None:
            if attn_mask is not None:
                raise ValueError("key_padding_mask is not None")
            attn_mask = ~key_padding_mask
        elif attn_mask is not None:
            attn_mask = ~attn_mask
        a = self.attn
        q, k, v = a.q_proj(query).float(), a.k_proj(key).float(), a.v_proj(value).float()
        out = None
        if self.fused and attn_mask is None and _ops.mha_supported(a.head_dim, int(k.shape[1])):
            out = _ops.multihead_attention(q, k, v, self.num_heads)
        if out is None:
            out = self.core(q, k, v, attn_mask)
        out = a.out_proj(out)
        if not self.batch_first:
            out = out.permute(1, 0, 2)
        return identity + self.dropout_layer(self.proj_drop(out))


class CustomMSDeformableAttention(nn.Module):
    def __init__(self, embed_dims=256, num_heads=8, num_levels=4, num_points=4, im2col_step=64, dropout=0.1,
                 batch_first=False, norm_cfg=None, fused=True):
        super().__init__()
        _check_heads(embed_dims, num_heads)
        self.norm_cfg = norm_cfg
        self.dropout = nn.Dropout(dropout)
        self.batch_first = batch_first
        self.im2col_step = im2col_step
        self.embed_dims = embed_dims
        self.num_levels = num_levels
        self.num_heads = num_heads
        self.num_points = num_points
        self.sampling_offsets = nn.Linear(embed_dims, num_heads * num_levels * num_points * 2)
        self.attention_weights = nn.Linear(embed_dims, num_heads * num_levels * num_points)
        self.value_proj = nn.Linear(embed_dims, embed_dims)
        self.output_proj = nn.Linear(embed_dims, embed_dims)
        self.fused = bool(fused)

    def _unfused(self, value, off, logits, reference_points, spatial_shapes, level_start_index):
        b, q, m, l, p, _ = off.shape
        attn = torch.softmax(logits, -1).reshape(b, q, m, l, p)
        if reference_points.shape[-1] == 2:
            loc = reference_points[:, :, None, :, None, :] + off / _normalizer(spatial_shapes)[None, None, None, :, None, :]
        else:
            ref = reference_points[:, :, None, :, None, :2]
            loc = ref + off / self.num_points * ref * 0.5
        return ms_deform_attn(value, loc.float().contiguous(), attn, spatial_shapes, level_start_index, self.im2col_step)

    def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_padding_mask=None,
                reference_points=None, spatial_shapes=None, level_start_index=None, flag="decoder", **kwargs):
        if self.training:
            raise NotImplementedError("CustomMSDeformableAttention: inference only")
        if value is None:
            value = query
        if identity is None:
            identity = query
        if query_pos is not None:
            query = query + query_pos
        if not self.batch_first:
            query, value = query.permute(1, 0, 2), value.permute(1, 0, 2)
        bs, nq, _ = query.shape
        value = self.value_proj(value)
        if key_padding_mask is not None:
            value = value.masked_fill(key_padding_mask[..., None], 0.0)
        m, l, p = self.num_heads, self.num_levels, self.num_points
        value = value.reshape(bs, value.shape[1], m, -1).float()
        off = self.sampling_offsets(query).reshape(bs, nq, m, l, p, 2).float()
        logits = self.attention_weights(query).reshape(bs, nq, m, l * p).float()
        if reference_points.shape[-1] not in (2, 4):
            raise ValueError(f"Last dim of reference_points must be 2 or 4, but get {reference_points.shape[-1]} instead.")
        reference_points = reference_points.float()
        out = None
        if self.fused and reference_points.shape[-1] == 2 and _ops.dec_ca_supported(int(value.shape[-1]), l, p):
            out = _ops.decoder_cross_attention_sample(value, off, logits, reference_points, spatial_shapes,
                                                      level_start_index)
        if out is None:
            out = self._unfused(value, off, logits, reference_points, spatial_shapes, level_start_index)
        out = self.output_proj(out)
        if not self.batch_first:
            out = out.permute(1, 0, 2)
        return self.dropout(out) + identity


ATTENTIONS = {"MultiheadAttention": MultiheadAttention, "CustomMSDeformableAttention": CustomMSDeformableAttention}


class DetrTransformerDecoderLayer(nn.Module):
    def __init__(self, attn_cfgs, feedforward_channels, ffn_dropout=0.0, operation_order=None, ffn_cfgs=None,
                 act_cfg=dict(type_name="ReLU"), norm_cfg=dict(type_name="LayerNorm"), ffn_num_fcs=2, batch_first=False,
                 fused=True, **kwargs):
        super().__init__()
        self.batch_first = batch_first
        names = {"self_attn", "norm", "ffn", "cross_attn"}
        assert set(operation_order) == names and len(operation_order) == 6, operation_order
        num_attn = operation_order.count("self_attn") + operation_order.count("cross_attn")
        if isinstance(attn_cfgs, dict):
            attn_cfgs = [copy.deepcopy(attn_cfgs) for _ in range(num_attn)]
        else:
            assert num_attn == len(attn_cfgs)
            attn_cfgs = [copy.deepcopy(c) for c in attn_cfgs]
        self.num_attn = num_attn
        self.operation_order = tuple(operation_order)
        self.norm_cfg = norm_cfg
        self.pre_norm = operation_order[0] == "norm"
        self.attentions = nn.ModuleList()
        index = 0
        for name in operation_order:
            if name in ("self_attn", "cross_attn"):
                cfg = attn_cfgs[index]
                if "batch_first" in cfg:
                    assert self.batch_first == cfg["batch_first"]
                else:
                    cfg["batch_first"] = self.batch_first
                # the self-attention kernel is opt-in (`fused=True` in its own attn cfg): at the tiny config it is
                # no faster than the torch formulation
                cfg.setdefault("fused", fused and cfg["type_name"] != "MultiheadAttention")
                attention = ATTENTIONS[cfg.pop("type_name")](**cfg)
                attention.operation_name = name
                self.attentions.append(attention)
                index += 1
        self.embed_dims = self.attentions[0].embed_dims
        self.ffns = nn.ModuleList(FFN(embed_dims=self.embed_dims, feedforward_channels=feedforward_channels,
                                      num_fcs=ffn_num_fcs, ffn_drop=ffn_dropout, act_cfg=act_cfg)
                                  for _ in range(operation_order.count("ffn")))
        if dict(norm_cfg).get("type_name", "LayerNorm") != "LayerNorm":
            raise ValueError("DetrTransformerDecoderLayer: LayerNorm only")
        self.norms = nn.ModuleList(nn.LayerNorm(self.embed_dims, eps=1e-5) for _ in range(operation_order.count("norm")))

    def forward(self, query, key=None, value=None, query_pos=None, key_pos=None, attn_masks=None,
                query_key_padding_mask=None, key_padding_mask=None, **kwargs):
        norm_index = attn_index = ffn_index = 0
        identity = query
        if attn_masks is None:
            attn_masks = [None] * self.num_attn
        elif isinstance(attn_masks, torch.Tensor):
            attn_masks = [attn_masks] * self.num_attn
        else:
            assert len(attn_masks) == self.num_attn
        for layer in self.operation_order:
            if layer == "self_attn":
                query = self.attentions[attn_index](
                    query, query, query, identity if self.pre_norm else None, query_pos=query_pos, key_pos=query_pos,
                    attn_mask=attn_masks[attn_index], key_padding_mask=query_key_padding_mask, **kwargs)
                attn_index += 1
                identity = query
            elif layer == "norm":
                query = self.norms[norm_index](query)
                norm_index += 1
            elif layer == "cross_attn":
                query = self.attentions[attn_index](
                    query, key, value, identity if self.pre_norm else None, query_pos=query_pos, key_pos=key_pos,
                    attn_mask=attn_masks[attn_index], key_padding_mask=key_padding_mask, **kwargs)
                attn_index += 1
                identity = query
            elif layer == "ffn":
                query = self.ffns[ffn_index](query, identity if self.pre_norm else None)
                ffn_index += 1
        return query


LAYERS = {"DetrTransformerDecoderLayer": DetrTransformerDecoderLayer}


class DetectionTransformerDecoder(nn.Module):
    def __init__(self, transformerlayers=None, num_layers=None, return_intermediate=False, fused=True):
        super().__init__()
        if isinstance(transformerlayers, dict):
            transformerlayers = [copy.deepcopy(transformerlayers) for _ in range(num_layers)]
        else:
            assert isinstance(transformerlayers, list) and len(transformerlayers) == num_layers
            transformerlayers = [copy.deepcopy(c) for c in transformerlayers]
        self.num_layers = num_layers
        self.layers = nn.ModuleList()
        for cfg in transformerlayers:
            cfg.setdefault("fused", fused)
            self.layers.append(LAYERS[cfg.pop("type_name")](**cfg))
        self.embed_dims = self.layers[0].embed_dims
        self.pre_norm = self.layers[0].pre_norm
        self.return_intermediate = return_intermediate

    def forward(self, query, key, value, query_pos, reference_points, reg_branches=None, key_padding_mask=None, **kwargs):
        """query, query_pos [Q, bs, E]; value [S, bs, E]; reference_points [bs, Q, 3] -> (states [Q, bs, E],
        reference points [bs, Q, 3]), each stacked over the layers with return_intermediate."""
        if self.training:
            raise NotImplementedError("DetectionTransformerDecoder: inference only")
        kwargs.pop("cls_branches", None)
        output = query
        intermediate, intermediate_reference_points = [], []
        for lid, layer in enumerate(self.layers):
            reference_points_input = reference_points[..., :2].unsqueeze(2)  # [bs, Q, 1, 2]
            output = layer(output, key, value, query_pos, reference_points=reference_points_input,
                           key_padding_mask=key_padding_mask, **kwargs)
            if reg_branches is not None:
                tmp = reg_branches[lid](output.permute(1, 0, 2))
                assert reference_points.shape[-1] == 3
                new_reference_points = torch.zeros_like(reference_points)
                new_reference_points[..., :2] = tmp[..., :2] + inverse_sigmoid(reference_points[..., :2])
                new_reference_points[..., 2:3] = tmp[..., 4:5] + inverse_sigmoid(reference_points[..., 2:3])
                reference_points = torch.sigmoid(new_reference_points).detach()
            if self.return_intermediate:
                intermediate.append(output)
                intermediate_reference_points.append(reference_points)
        if self.return_intermediate:
            return torch.stack(intermediate), torch.stack(intermediate_reference_points)
        return output, reference_points


class PerceptionTransformer(nn.Module):
    def __init__(self, num_feature_levels=4, num_cams=6, encoder=None, decoder=None, embed_dims=256, rotate_prev_bev=True,
                 use_shift=True, use_can_bus=True, can_bus_norm=True, use_cams_embeds=True, rotate_center=[100, 100],
                 fused=True, **kwargs):
        super().__init__()
        if isinstance(decoder, dict):
            cfg = copy.deepcopy(decoder)
            cfg.pop("type_name", None)
            cfg.setdefault("fused", fused)
            decoder = DetectionTransformerDecoder(**cfg)
        if isinstance(encoder, dict):
            from .bevformer import BEVFormerEncoder

            cfg = copy.deepcopy(encoder)
            cfg.pop("type_name", None)
            cfg.setdefault("fused", fused)
            encoder = BEVFormerEncoder(**cfg)
        self.encoder = encoder
        self.decoder = decoder
        self.embed_dims = embed_dims
        self.num_feature_levels = num_feature_levels
        self.num_cams = num_cams
        self.rotate_prev_bev = rotate_prev_bev
        self.use_shift = use_shift
        self.use_can_bus = use_can_bus
        self.can_bus_norm = can_bus_norm
        self.use_cams_embeds = use_cams_embeds
        self.rotate_center = rotate_center
        self.level_embeds = nn.Parameter(torch.zeros(num_feature_levels, embed_dims))
        self.cams_embeds = nn.Parameter(torch.zeros(num_cams, embed_dims))
        self.reference_points = nn.Linear(embed_dims, 3)
        self.can_bus_mlp = nn.Sequential(nn.Linear(18, embed_dims // 2), nn.ReLU(), nn.Linear(embed_dims // 2, embed_dims),
                                         nn.ReLU())
        if can_bus_norm:
            self.can_bus_mlp.add_module("norm", nn.LayerNorm(embed_dims))

    def get_bev_features(self, *args, **kwargs):
        raise NotImplementedError("PerceptionTransformer.get_bev_features: the can-bus shift, the rotation of prev_bev "
                                  "and the camera / level embeddings are not implemented; run the encoder "
                                  "(paddle3d_amd.bevformer.BEVFormerEncoder) and pass its BEV map to decode()")

    def decode(self, bev_embed, object_query_embed, bev_h, bev_w, reg_branches=None, cls_branches=None, **kwargs):
        """bev_embed [bs, bev_h * bev_w, E], object_query_embed [Q, 2 E] -> (bev_embed [S, bs, E], inter_states,
        init_reference_out [bs, Q, 3], inter_references_out): transformer.py:361-392."""
        bs = bev_embed.shape[0]
        query_pos, query = torch.split(object_query_embed, [self.embed_dims, self.embed_dims], dim=1)
        query_pos = query_pos.unsqueeze(0).expand(bs, -1, -1)
        query = query.unsqueeze(0).expand(bs, -1, -1)
        reference_points = torch.sigmoid(self.reference_points(query_pos))
        init_reference_out = reference_points
        query = query.permute(1, 0, 2)
        query_pos = query_pos.permute(1, 0, 2)
        bev_embed = bev_embed.permute(1, 0, 2)
        spatial_shapes, level_start_index = _bev_levels(bev_h, bev_w, bev_embed.device)
        inter_states, inter_references = self.decoder(
            query=query, key=None, value=bev_embed, query_pos=query_pos, reference_points=reference_points,
            reg_branches=reg_branches, cls_branches=cls_branches, spatial_shapes=spatial_shapes,
            level_start_index=level_start_index, **kwargs)
        return bev_embed, inter_states, init_reference_out, inter_references

    def forward(self, *args, **kwargs):
        return self.get_bev_features(*args, **kwargs)


def threshold_steps(score_threshold):
    """The values `tmp_score` takes in the loop of box_coder.py:158-166 before it drops below 0.01 (Python doubles)."""
    steps, tmp = [], float(score_threshold)
    while True:
        tmp *= 0.9
        if tmp < 0.01:
            return steps
        steps.append(tmp)


class NMSFreeCoder:
    def __init__(self, point_cloud_range, voxel_size=None, post_center_range=None, max_num=100, score_threshold=None,
                 num_classes=10, fused=True):
        if post_center_range is None:
            raise NotImplementedError("NMSFreeCoder: post_center_range is required")
        self.point_cloud_range = point_cloud_range
        self.voxel_size = voxel_size
        self.post_center_range = [float(v) for v in post_center_range]
        self.max_num = max_num
        self.score_threshold = score_threshold
        self.num_classes = num_classes
        self.fused = bool(fused)

    def _decode_torch(self, cls_scores, bbox_preds, bottom_center):
        """decode_single over the batch in torch, without a host synchronisation (the loop's thresholds are computed on
        the host beforehand and picked on the device)."""
        b, q, k = cls_scores.shape
        s = torch.sigmoid(cls_scores.float()).reshape(b, q * k)
        s = torch.where(torch.isnan(s), s.new_full((), -1.0), s)
        scores, idx = torch.sort(s, dim=1, descending=True, stable=True)
        scores, idx = scores[:, :self.max_num], idx[:, :self.max_num]
        labels = (idx % k).to(torch.int32)
        p = torch.gather(bbox_preds.float(), 1, (idx // k)[..., None].expand(-1, -1, bbox_preds.shape[-1]))
        rot = torch.atan2(p[..., 6:7], p[..., 7:8])
        parts = [p[..., 0:1], p[..., 1:2], p[..., 4:5], p[..., 2:3].exp(), p[..., 3:4].exp(), p[..., 5:6].exp(), rot]
        if p.shape[-1] > 8:
            parts += [p[..., 8:9], p[..., 9:10]]
        boxes = torch.cat(parts, -1)
        rng = torch.tensor(self.post_center_range, dtype=torch.float32).pin_memory().to(boxes.device, non_blocking=True) \
            if boxes.is_cuda else torch.tensor(self.post_center_range, dtype=torch.float32)
        keep = (boxes[..., :3] >= rng[:3]).all(-1) & (boxes[..., :3] <= rng[3:]).all(-1) & (scores >= 0)
        if self.score_threshold:
            thr = float(self.score_threshold)
            top = scores[:, :1]
            mask = scores > thr
            steps = threshold_steps(thr)
            lowered = torch.ones_like(mask)
            for t in reversed(steps):  # the first step the top score reaches wins
                lowered = torch.where(top >= t, scores >= t, lowered)
            keep = keep & torch.where(top > thr, mask, lowered)
        if bottom_center:
            boxes = torch.cat([boxes[..., :2], boxes[..., 2:3] - boxes[..., 5:6] * 0.5, boxes[..., 3:]], -1)
        count = keep.sum(1).to(torch.int32)
        order = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices
        kept = torch.arange(self.max_num, device=boxes.device)[None] < count[:, None]
        boxes = torch.where(kept[..., None], torch.gather(boxes, 1, order[..., None].expand_as(boxes)), boxes.new_zeros(()))
        scores = torch.where(kept, torch.gather(scores, 1, order), scores.new_zeros(()))
        labels = torch.where(kept, torch.gather(labels, 1, order), labels.new_full((), -1))
        return boxes, scores, labels, count

    def decode(self, preds_dicts, bottom_center=False):
        """preds_dicts['all_cls_scores'] [layers, B, Q, K] and ['all_bbox_preds'] [layers, B, Q, code] -> (boxes
        [B, max_num, code - 1], scores [B, max_num], labels [B, max_num] int32, count [B] int32) of the last layer."""
        cls_scores = preds_dicts["all_cls_scores"][-1].float()
        bbox_preds = preds_dicts["all_bbox_preds"][-1].float()
        if int(cls_scores.shape[-1]) != self.num_classes:
            raise ValueError(f"NMSFreeCoder: {cls_scores.shape[-1]} class scores, num_classes {self.num_classes}")
        if self.fused and cls_scores.is_cuda:
            return _ops.nms_free_decode(cls_scores, bbox_preds, self.post_center_range, self.max_num,
                                        self.score_threshold, bottom_center)
        return self._decode_torch(cls_scores, bbox_preds, bottom_center)

    @staticmethod
    def to_list(boxes, scores, labels, count):
        """The reference's list of dicts, one per frame (this reads `count` back: a host synchronisation)."""
        out = []
        for b, n in enumerate(count.tolist()):
            out.append(dict(bboxes=boxes[b, :n], scores=scores[b, :n], labels=labels[b, :n].to(torch.int64)))
        return out


class BEVFormerHead(nn.Module):
    def __init__(self, num_classes, in_channels, transformer, positional_encoding=None, num_query=100, num_reg_fcs=2,
                 num_cls_fcs=2, sync_cls_avg_factor=False, with_box_refine=False, as_two_stage=False, bbox_coder=None,
                 code_weights=None, bev_h=30, bev_w=30, code_size=10, fused=True, **kwargs):
        super().__init__()
        if as_two_stage:
            raise NotImplementedError("BEVFormerHead: as_two_stage is not supported")
        self.bev_h, self.bev_w = bev_h, bev_w
        self.with_box_refine = with_box_refine
        self.as_two_stage = as_two_stage
        self.code_size = code_size
        self.code_weights = code_weights if code_weights is not None else [1.0] * 8 + [0.2, 0.2]
        if isinstance(bbox_coder, dict):
            cfg = copy.deepcopy(bbox_coder)
            cfg.pop("type_name", None)
            cfg.setdefault("fused", fused)
            bbox_coder = NMSFreeCoder(**cfg)
        self.bbox_coder = bbox_coder
        self.point_cloud_range = bbox_coder.point_cloud_range
        self.real_w = self.point_cloud_range[3] - self.point_cloud_range[0]
        self.real_h = self.point_cloud_range[4] - self.point_cloud_range[1]
        self.num_query = num_query
        self.num_classes = num_classes
        self.in_channels = in_channels
        self.num_reg_fcs = num_reg_fcs
        self.cls_out_channels = num_classes
        if isinstance(transformer, dict):
            cfg = copy.deepcopy(transformer)
            cfg.pop("type_name", None)
            cfg.setdefault("fused", fused)
            transformer = PerceptionTransformer(**cfg)
        self.transformer = transformer
        self.positional_encoding = positional_encoding
        self.embed_dims = transformer.embed_dims
        self._init_layers()

    def _init_layers(self):
        e = self.embed_dims
        cls_branch = []
        for _ in range(self.num_reg_fcs):
            cls_branch += [nn.Linear(e, e), nn.LayerNorm(e), nn.ReLU()]
        cls_branch.append(nn.Linear(e, self.cls_out_channels))
        fc_cls = nn.Sequential(*cls_branch)
        reg_branch = []
        for _ in range(self.num_reg_fcs):
            reg_branch += [nn.Linear(e, e), nn.ReLU()]
        reg_branch.append(nn.Linear(e, self.code_size))
        reg_branch = nn.Sequential(*reg_branch)
        num_pred = self.transformer.decoder.num_layers
        if self.with_box_refine:
            self.cls_branches = nn.ModuleList(copy.deepcopy(fc_cls) for _ in range(num_pred))
            self.reg_branches = nn.ModuleList(copy.deepcopy(reg_branch) for _ in range(num_pred))
        else:
            self.cls_branches = nn.ModuleList(fc_cls for _ in range(num_pred))
            self.reg_branches = nn.ModuleList(reg_branch for _ in range(num_pred))
        self.bev_embedding = nn.Embedding(self.bev_h * self.bev_w, e)
        self.query_embedding = nn.Embedding(self.num_query, e * 2)

    def forward_from_bev(self, bev_embed):
        """bev_embed [bs, bev_h * bev_w, E] (the encoder's output) -> the reference's `outs` dict."""
        if self.training:
            raise NotImplementedError("BEVFormerHead: inference only")
        object_query_embeds = self.query_embedding.weight.to(bev_embed.dtype)
        bev_embed, hs, init_reference, inter_references = self.transformer.decode(
            bev_embed, object_query_embeds, self.bev_h, self.bev_w,
            reg_branches=self.reg_branches if self.with_box_refine else None)
        hs = hs.permute(0, 2, 1, 3)
        pc = self.point_cloud_range
        outputs_classes, outputs_coords = [], []
        for lvl in range(hs.shape[0]):
            reference = inverse_sigmoid(init_reference if lvl == 0 else inter_references[lvl - 1])
            outputs_class = self.cls_branches[lvl](hs[lvl])
            tmp = self.reg_branches[lvl](hs[lvl]).clone()
            assert reference.shape[-1] == 3
            tmp[..., 0:2] = torch.sigmoid(tmp[..., 0:2] + reference[..., 0:2])
            tmp[..., 4:5] = torch.sigmoid(tmp[..., 4:5] + reference[..., 2:3])
            tmp[..., 0:1] = tmp[..., 0:1] * (pc[3] - pc[0]) + pc[0]
            tmp[..., 1:2] = tmp[..., 1:2] * (pc[4] - pc[1]) + pc[1]
            tmp[..., 4:5] = tmp[..., 4:5] * (pc[5] - pc[2]) + pc[2]
            outputs_classes.append(outputs_class)
            outputs_coords.append(tmp)
        return dict(bev_embed=bev_embed, all_cls_scores=torch.stack(outputs_classes),
                    all_bbox_preds=torch.stack(outputs_coords), enc_cls_scores=None, enc_bbox_preds=None)

    def forward(self, mlvl_feats, img_metas, prev_bev=None, only_bev=False):
        raise NotImplementedError("BEVFormerHead.forward needs PerceptionTransformer.get_bev_features, which is not "
                                  "implemented; run the encoder and call forward_from_bev(bev_embed)")

    def get_bboxes(self, preds_dicts, img_metas=None, rescale=False):
        """(boxes [B, max_num, code - 1] with z at the box bottom, scores, labels, count); NMSFreeCoder.to_list turns them
        into the reference's per-frame list."""
        preds = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in preds_dicts.items()}
        return self.bbox_coder.decode(preds, bottom_center=True)
