"""BEVFormer's encoder at inference on the device ops (paddle3d/models/transformers: encoders.py, encoder_layers.py,
attentions/spatial_cross_attention.py, attentions/temporal_self_attention.py).  The modules have the reference's
constructor arguments, forward signatures and state-dict keys, so checkpoint.load_paddle_state_dict places the
`encoder.*` entries of a BEVFormer `.pdparams` unchanged.

MSDeformableAttention3D(embed_dims, num_heads, num_levels, num_points, im2col_step, dropout, batch_first)
                                    the reference's forward around ops.ms_deform_attn (sampling_offsets,
                                    attention_weights, value_proj); query_rows() / project_value() are its two halves.
SpatialCrossAttention(embed_dims, num_cams, pc_range, dropout, batch_first, deformable_attention, fused=True)
                                    forward(query, key, value, ..., reference_points_cam, bev_mask, ...).  fused=True:
                                    the two query Linears once per BEV query (a rebatched row of the reference is the
                                    BEV query row itself), then ops.bevformer.spatial_cross_attention_sample: no
                                    nonzero(), no rebatch, no sampling_locations, no scatter.  fused=False, or a shape
                                    the kernel refuses: every camera samples all Q queries through ops.ms_deform_attn,
                                    the misses are masked and the cameras summed in index order.
TemporalSelfAttention(embed_dims, num_heads, num_levels, num_points, num_bev_queue, ..., fused=True)
                                    fused=True: ops.bevformer.temporal_self_attention_sample on the Linear's own
                                    layout; otherwise the reference's two transposes around ops.ms_deform_attn.
FFN, BEVFormerLayer(attn_cfgs, feedforward_channels, ffn_dropout, operation_order, ..., fused=True)
BEVFormerEncoder(transformerlayers, num_layers, point_cloud_range, num_points_in_pillar, ..., fused=True)
                                    get_reference_points (both dims), point_sampling (ops.bevformer.point_sampling, one
                                    launch per forward; all layers reuse it) and forward.

Where this departs from the reference, on purpose:
  * Each frame of a batch uses its own bev_mask.  The reference gathers every frame's queries with frame 0's mask
    (`mask_per_img[0]`, spatial_cross_attention.py:152) and counts with each frame's own, which cannot be seen at its
    batch size of 1; at batch 1 the two agree.
  * TemporalSelfAttention concatenates each frame's own history BEV (value row 2b) to its query; the reference takes
    `value[:bs]`, which is that row only at its batch size of 1.
  * point_sampling takes the pillar anchors of frame 0 for every frame (get_reference_points tiles one set over the
    batch) and, as the reference does, frame 0 / camera 0's img_shape for every image.
  * The `prev_bev` selection (encoders.py:258-264) is a torch.where on a device flag, never read back.
  * BEVFormerLayer builds its FFN with the layer's embed_dims (the reference hard-codes 256 and asserts it).
`ref_2d += shift` is reproduced as the reference keeps it: both queue entries get the shifted points.

Linear, LayerNorm and the FFN are torch.  Inference only; with device tensors in img_metas nothing in the forwards
synchronises with the host.  The decoder, the detection head and the NMS-free decode are in paddle3d_amd/bevformer_head.py;
PerceptionTransformer's can-bus handling is not implemented.
"""
from __future__ import annotations

import copy

import torch
from torch import nn

from .ops import bevformer as _ops
from .ops.ms_deform_attn import ms_deform_attn

__all__ = ["MSDeformableAttention3D", "SpatialCrossAttention", "TemporalSelfAttention", "FFN", "BEVFormerLayer",
           "BEVFormerEncoder"]


def _check_heads(embed_dims, num_heads):
    if embed_dims % num_heads != 0:
        raise ValueError(f"embed_dims must be divisible by num_heads, but got {embed_dims} and {num_heads}")


def _normalizer(spatial_shapes):
    return torch.stack([spatial_shapes[..., 1], spatial_shapes[..., 0]], -1)  # (W, H) per level


class MSDeformableAttention3D(nn.Module):
    def __init__(self, embed_dims=256, num_heads=8, num_levels=4, num_points=8, im2col_step=64, dropout=0.1,
                 batch_first=True):
        super().__init__()
        _check_heads(embed_dims, num_heads)
        self.batch_first = batch_first
        self.output_proj = None
        self.im2col_step = im2col_step
        self.embed_dims = embed_dims
        self.num_levels = num_levels
        self.num_heads = num_heads
        self.num_points = num_points
        self.sampling_offsets = nn.Linear(embed_dims, num_heads * num_levels * num_points * 2)
        self.attention_weights = nn.Linear(embed_dims, num_heads * num_levels * num_points)
        self.value_proj = nn.Linear(embed_dims, embed_dims)

    def project_value(self, value, key_padding_mask=None):
        """[N, S, E] -> [N, S, M, C]."""
        value = self.value_proj(value)
        if key_padding_mask is not None:
            value = value.masked_fill(key_padding_mask[..., None], 0.0)
        return value.reshape(value.shape[0], value.shape[1], self.num_heads, -1)

    def query_rows(self, query):
        """[N, Q, E] -> (sampling offsets [N, Q, M, L, P, 2], attention logits [N, Q, M, L*P]), both raw."""
        n, q = query.shape[:2]
        off = self.sampling_offsets(query).reshape(n, q, self.num_heads, self.num_levels, self.num_points, 2)
        return off, self.attention_weights(query).reshape(n, q, self.num_heads, self.num_levels * self.num_points)

    def sample(self, value, offsets, logits, reference_points, spatial_shapes, level_start_index):
        """The reference's softmax, sampling_locations (Z anchors innermost) and op on projected value and raw rows."""
        n, q, m, l, p, _ = offsets.shape
        attn = torch.softmax(logits, -1).reshape(n, q, m, l, p)
        if reference_points.shape[-1] != 2:
            raise ValueError(f"Last dim of reference_points must be 2, but get {reference_points.shape[-1]} instead.")
        d = reference_points.shape[2]
        if p % d != 0:
            raise ValueError(f"num_points {p} must be a multiple of the {d} Z anchors")
        off = (offsets / _normalizer(spatial_shapes).reshape(1, 1, 1, l, 1, 2)).reshape(n, q, m, l, p // d, d, 2)
        loc = (reference_points.reshape(n, q, 1, 1, 1, d, 2) + off).reshape(n, q, m, l, p, 2)
        return ms_deform_attn(value, loc, attn, spatial_shapes, level_start_index, self.im2col_step)

    def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_padding_mask=None,
                reference_points=None, spatial_shapes=None, level_start_index=None, **kwargs):
        if value is None:
            value = query
        if query_pos is not None:
            query = query + query_pos
        if not self.batch_first:
            query, value = query.permute(1, 0, 2), value.permute(1, 0, 2)
        off, logits = self.query_rows(query)
        out = self.sample(self.project_value(value, key_padding_mask), off, logits, reference_points, spatial_shapes,
                          level_start_index)
        return out if self.batch_first else out.permute(1, 0, 2)


def hit_bits_of(bev_mask):
    """bev_mask [cams, B, Q, D] -> the per-query camera bitmask [B, Q] uint8 ops.bevformer.point_sampling returns."""
    hit = (bev_mask != 0).any(-1)
    weights = (2 ** torch.arange(hit.shape[0], device=hit.device, dtype=torch.int32)).reshape(-1, 1, 1)
    return (hit.to(torch.int32) * weights).sum(0).to(torch.uint8)


class SpatialCrossAttention(nn.Module):
    def __init__(self, embed_dims=256, num_cams=6, pc_range=None, dropout=0.1, batch_first=False,
                 deformable_attention=dict(type_name="MSDeformableAttention3D", embed_dims=256, num_levels=4),
                 fused=True, **kwargs):
        super().__init__()
        self.dropout = nn.Dropout(dropout)
        self.pc_range = pc_range
        cfg = copy.deepcopy(deformable_attention)
        self.deformable_attention = ATTENTIONS[cfg.pop("type_name")](**cfg)
        self.embed_dims = embed_dims
        self.num_cams = num_cams
        self.output_proj = nn.Linear(embed_dims, embed_dims)
        self.batch_first = batch_first
        self.fused = bool(fused)

    def _unfused(self, value, off, logits, reference_points_cam, hit, spatial_shapes, level_start_index):
        """Every camera over all Q queries; `hit` [cams, B, Q] masks the misses, cameras are summed in index order."""
        att, cams = self.deformable_attention, self.num_cams
        bs, q = off.shape[:2]
        rep = lambda t: t.unsqueeze(1).expand(bs, cams, *t.shape[1:]).reshape(bs * cams, *t.shape[1:])  # noqa: E731
        ref = reference_points_cam.permute(1, 0, 2, 3, 4).reshape(bs * cams, q, -1, 2)
        out = att.sample(value, rep(off), rep(logits), ref, spatial_shapes, level_start_index)
        out = out.reshape(bs, cams, q, self.embed_dims)
        seen = hit.permute(1, 0, 2).unsqueeze(-1)  # [B, cams, Q, 1]
        zero = out.new_zeros(())
        slots = torch.where(seen[:, 0], out[:, 0], zero)
        for cam in range(1, cams):
            slots = slots + torch.where(seen[:, cam], out[:, cam], zero)
        count = hit.sum(0).clamp(min=1).to(out.dtype)
        return slots / count[..., None]

    def forward(self, query, key, value, residual=None, query_pos=None, key_padding_mask=None, reference_points=None,
                spatial_shapes=None, reference_points_cam=None, bev_mask=None, level_start_index=None, flag="encoder",
                hit_bits=None, **kwargs):
        if self.training:
            raise NotImplementedError("SpatialCrossAttention: inference only")
        query = query.float()
        if key is None:
            key = query
        if value is None:
            value = key
        inp_residual = query if residual is None else residual
        if query_pos is not None:
            query = query + query_pos.float()
        att = self.deformable_attention
        cams, s, bs, _ = value.shape
        if cams != self.num_cams:
            raise RuntimeError(f"SpatialCrossAttention: value has {cams} cameras, the module {self.num_cams}")
        reference_points_cam = reference_points_cam.float()
        d = int(reference_points_cam.shape[3])
        value = att.project_value(value.float().permute(2, 0, 1, 3).reshape(bs * cams, s, self.embed_dims))
        off, logits = att.query_rows(query)
        slots = None
        if self.fused and _ops.sca_supported(int(value.shape[-1]), att.num_levels, att.num_points, cams, d):
            bits = hit_bits if hit_bits is not None else hit_bits_of(bev_mask)
            slots = _ops.spatial_cross_attention_sample(value, off, logits, reference_points_cam, bits, spatial_shapes,
                                                        level_start_index, cams)
        if slots is None:
            slots = self._unfused(value, off, logits, reference_points_cam, (bev_mask != 0).any(-1), spatial_shapes,
                                  level_start_index)
        return self.dropout(self.output_proj(slots)) + inp_residual


class TemporalSelfAttention(nn.Module):
    def __init__(self, embed_dims=256, num_heads=8, num_levels=4, num_points=4, num_bev_queue=2, im2col_step=64,
                 dropout=0.1, batch_first=True, norm_cfg=None, fused=True):
        super().__init__()
        _check_heads(embed_dims, num_heads)
        if num_bev_queue != 2:
            raise ValueError("TemporalSelfAttention: a BEV queue of 2 (one history BEV, the current one)")
        self.norm_cfg = norm_cfg
        self.dropout = nn.Dropout(dropout)
        self.batch_first = batch_first
        self.im2col_step = im2col_step
        self.embed_dims = embed_dims
        self.num_levels = num_levels
        self.num_heads = num_heads
        self.num_points = num_points
        self.num_bev_queue = num_bev_queue
        self.sampling_offsets = nn.Linear(embed_dims * num_bev_queue, num_bev_queue * num_heads * num_levels * num_points * 2)
        self.attention_weights = nn.Linear(embed_dims * num_bev_queue, num_bev_queue * num_heads * num_levels * num_points)
        self.value_proj = nn.Linear(embed_dims, embed_dims)
        self.output_proj = nn.Linear(embed_dims, embed_dims)
        self.fused = bool(fused)

    def _unfused(self, value, off, logits, reference_points, spatial_shapes, level_start_index):
        bs, q, m, nq, l, p, _ = off.shape
        attn = torch.softmax(logits, -1).reshape(bs, q, m, nq, l, p)
        attn = attn.permute(0, 3, 1, 2, 4, 5).reshape(bs * nq, q, m, l, p)
        off = off.permute(0, 3, 1, 2, 4, 5, 6).reshape(bs * nq, q, m, l, p, 2)
        loc = reference_points[:, :, None, :, None, :] + off / _normalizer(spatial_shapes)[None, None, None, :, None, :]
        out = ms_deform_attn(value, loc, attn, spatial_shapes, level_start_index, self.im2col_step)
        return out.reshape(bs, nq, q, self.embed_dims).mean(1)

    def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_padding_mask=None,
                reference_points=None, spatial_shapes=None, level_start_index=None, flag="decoder", **kwargs):
        if self.training:
            raise NotImplementedError("TemporalSelfAttention: inference only")
        if value is None:
            assert self.batch_first
            bs, len_bev, c = query.shape
            value = torch.stack([query, query], 1).reshape(bs * 2, len_bev, c)
        if identity is None:
            identity = query
        if query_pos is not None:
            query = query + query_pos
        if not self.batch_first:
            query, value = query.permute(1, 0, 2), value.permute(1, 0, 2)
        bs, q, _ = query.shape
        s = value.shape[1]
        if reference_points.shape[-1] != 2:
            raise ValueError(f"Last dim of reference_points must be 2, but get {reference_points.shape[-1]} instead.")
        query = torch.cat([value[0::2], query], -1)  # each frame's own history row (the reference: value[:bs])
        value = self.value_proj(value)
        if key_padding_mask is not None:
            value = value.masked_fill(key_padding_mask[..., None], 0.0)
        m, nq, l, p = self.num_heads, self.num_bev_queue, self.num_levels, self.num_points
        value = value.reshape(bs * nq, s, m, -1).float()
        off = self.sampling_offsets(query).reshape(bs, q, m, nq, l, p, 2)
        logits = self.attention_weights(query).reshape(bs, q, m, nq, l * p)
        reference_points = reference_points.float()
        out = None
        if self.fused and _ops.tsa_supported(int(value.shape[-1]), l, p):
            out = _ops.temporal_self_attention_sample(value, off, logits, reference_points, spatial_shapes,
                                                      level_start_index)
        if out is None:
            out = self._unfused(value, off, logits, reference_points, spatial_shapes, level_start_index)
        out = self.output_proj(out)
        if not self.batch_first:
            out = out.permute(1, 0, 2)
        return self.dropout(out) + identity


ATTENTIONS = {"MSDeformableAttention3D": MSDeformableAttention3D, "SpatialCrossAttention": SpatialCrossAttention,
              "TemporalSelfAttention": TemporalSelfAttention}


class FFN(nn.Module):
    def __init__(self, embed_dims=256, feedforward_channels=1024, num_fcs=2, act_cfg=dict(type_name="ReLU"), ffn_drop=0.0,
                 dropout_layer=None, add_identity=True, **kwargs):
        super().__init__()
        assert num_fcs >= 2, f"num_fcs should be no less than 2. got {num_fcs}."
        self.embed_dims = embed_dims
        self.feedforward_channels = feedforward_channels
        self.num_fcs = num_fcs
        self.activate = getattr(nn, dict(act_cfg).get("type_name", "ReLU"))()
        layers, in_channels = [], embed_dims
        for _ in range(num_fcs - 1):
            layers.append(nn.Sequential(nn.Linear(in_channels, feedforward_channels), self.activate, nn.Dropout(ffn_drop)))
            in_channels = feedforward_channels
        layers.append(nn.Linear(feedforward_channels, embed_dims))
        layers.append(nn.Dropout(ffn_drop))
        self.layers = nn.Sequential(*layers)
        if dropout_layer:
            cfg = dict(dropout_layer)
            self.dropout_layer = getattr(nn, cfg.pop("type_name"))(**cfg)
        else:
            self.dropout_layer = nn.Identity()
        self.add_identity = add_identity

    def forward(self, x, identity=None):
        out = self.layers(x)
        if not self.add_identity:
            return self.dropout_layer(out)
        return (x if identity is None else identity) + self.dropout_layer(out)


def _bev_levels(bev_h, bev_w, device):
    """([[bev_h, bev_w]], [0]) int64 on the device, made by fills (no host copy)."""
    return (torch.cat([torch.full((1, 1), bev_h, dtype=torch.int64, device=device),
                       torch.full((1, 1), bev_w, dtype=torch.int64, device=device)], -1),
            torch.zeros((1,), dtype=torch.int64, device=device))


class BEVFormerLayer(nn.Module):
    def __init__(self, attn_cfgs, feedforward_channels, ffn_dropout=0.0, operation_order=None,
                 act_cfg=dict(type_name="ReLU"), norm_cfg=dict(type_name="LayerNorm"), ffn_num_fcs=2, batch_first=True,
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
                cfg.setdefault("fused", fused)
                attention = ATTENTIONS[cfg.pop("type_name")](**cfg)
                attention.operation_name = name
                self.attentions.append(attention)
                index += 1
        self.embed_dims = self.attentions[0].embed_dims
        self.ffns = nn.ModuleList(FFN(embed_dims=self.embed_dims, feedforward_channels=feedforward_channels,
                                      num_fcs=ffn_num_fcs, ffn_drop=ffn_dropout, act_cfg=act_cfg)
                                  for _ in range(operation_order.count("ffn")))
        if dict(norm_cfg).get("type_name", "LayerNorm") != "LayerNorm":
            raise ValueError("BEVFormerLayer: LayerNorm only")
        self.norms = nn.ModuleList(nn.LayerNorm(self.embed_dims, eps=1e-5) for _ in range(operation_order.count("norm")))

    def forward(self, query, key=None, value=None, bev_pos=None, query_pos=None, key_pos=None, attn_masks=None,
                query_key_padding_mask=None, key_padding_mask=None, ref_2d=None, ref_3d=None, bev_h=None, bev_w=None,
                reference_points_cam=None, mask=None, spatial_shapes=None, level_start_index=None, prev_bev=None,
                bev_levels=None, **kwargs):
        norm_index = attn_index = ffn_index = 0
        identity = query
        if attn_masks is None:
            attn_masks = [None] * self.num_attn
        if bev_levels is None:
            bev_levels = _bev_levels(bev_h, bev_w, query.device)
        for layer in self.operation_order:
            if layer == "self_attn":
                query = self.attentions[attn_index](
                    query, prev_bev, prev_bev, identity if self.pre_norm else None, query_pos=bev_pos, key_pos=bev_pos,
                    attn_mask=attn_masks[attn_index], key_padding_mask=query_key_padding_mask, reference_points=ref_2d,
                    spatial_shapes=bev_levels[0], level_start_index=bev_levels[1], **kwargs)
                attn_index += 1
                identity = query
            elif layer == "norm":
                query = self.norms[norm_index](query)
                norm_index += 1
            elif layer == "cross_attn":
                query = self.attentions[attn_index](
                    query, key, value, identity if self.pre_norm else None, query_pos=query_pos, key_pos=key_pos,
                    reference_points=ref_3d, reference_points_cam=reference_points_cam, mask=mask,
                    attn_mask=attn_masks[attn_index], key_padding_mask=key_padding_mask, spatial_shapes=spatial_shapes,
                    level_start_index=level_start_index, **kwargs)
                attn_index += 1
                identity = query
            elif layer == "ffn":
                query = self.ffns[ffn_index](query, identity if self.pre_norm else None)
                ffn_index += 1
        return query


LAYERS = {"BEVFormerLayer": BEVFormerLayer}


class BEVFormerEncoder(nn.Module):
    def __init__(self, transformerlayers, num_layers, point_cloud_range=None, num_points_in_pillar=4,
                 return_intermediate=False, dataset_type="nuscenes", fused=True, **kwargs):
        super().__init__()
        if isinstance(transformerlayers, dict):
            transformerlayers = [copy.deepcopy(transformerlayers) for _ in range(num_layers)]
        else:
            assert isinstance(transformerlayers, list) and len(transformerlayers) == num_layers
            transformerlayers = [copy.deepcopy(c) for c in transformerlayers]
        self.return_intermediate = return_intermediate
        self.num_points_in_pillar = num_points_in_pillar
        self.point_cloud_range = point_cloud_range
        self.layers = nn.ModuleList()
        for cfg in transformerlayers:
            cfg.setdefault("fused", fused)
            self.layers.append(LAYERS[cfg.pop("type_name")](**cfg))
        self._ref_cache = {}

    @staticmethod
    def get_reference_points(H, W, Z=8, num_points_in_pillar=4, dim="3d", bs=1, dtype=torch.float32, device=None):
        """'3d': [bs, D, H*W, 3] pillar anchors in [0, 1] for SCA; '2d': [bs, H*W, 1, 2] BEV points for TSA.  Built
        on the host in float32 as the reference builds them and, for a GPU `device`, sent without a synchronisation."""
        if dim == "3d":
            d = num_points_in_pillar
            zs = torch.linspace(0.5, Z - 0.5, d, dtype=torch.float32).to(dtype).reshape(-1, 1, 1).expand(d, H, W) / Z
            xs = torch.linspace(0.5, W - 0.5, W, dtype=torch.float32).reshape(1, 1, W).to(dtype).expand(d, H, W) / W
            ys = torch.linspace(0.5, H - 0.5, H, dtype=torch.float32).reshape(1, H, 1).to(dtype).expand(d, H, W) / H
            ref = torch.stack((xs, ys, zs), -1).permute(0, 3, 1, 2).flatten(2).permute(0, 2, 1)
            ref = ref[None].repeat(bs, 1, 1, 1)
        elif dim == "2d":
            ref_y, ref_x = torch.meshgrid(torch.linspace(0.5, H - 0.5, H, dtype=torch.float32),
                                          torch.linspace(0.5, W - 0.5, W, dtype=torch.float32), indexing="ij")
            ref_y = ref_y.to(dtype).reshape(-1)[None] / H
            ref_x = ref_x.to(dtype).reshape(-1)[None] / W
            ref = torch.stack((ref_x, ref_y), -1).repeat(bs, 1, 1).unsqueeze(2)
        else:
            raise ValueError(f"dim must be '3d' or '2d', got {dim!r}")
        ref = ref.contiguous()
        if device is not None and torch.device(device).type == "cuda":
            ref = ref.pin_memory().to(device, non_blocking=True)
        return ref

    def _reference_points(self, bev_h, bev_w, bs, dtype, device):
        key = (bev_h, bev_w, bs, dtype, str(device))
        if key not in self._ref_cache:
            z = self.point_cloud_range[5] - self.point_cloud_range[2]
            self._ref_cache = {key: (
                self.get_reference_points(bev_h, bev_w, z, self.num_points_in_pillar, "3d", bs, dtype, device),
                self.get_reference_points(bev_h, bev_w, dim="2d", bs=bs, dtype=dtype, device=device))}
        return self._ref_cache[key]

    @staticmethod
    def _lidar2img(img_metas, device):
        mats = []
        for meta in img_metas:
            m = meta["lidar2img"]
            mats.append(m if isinstance(m, torch.Tensor) else torch.stack([torch.as_tensor(x) for x in m]))
        return torch.stack(mats).to(device=device, dtype=torch.float32)  # (B, N, 4, 4)

    def point_sampling(self, reference_points, point_cloud_range, img_metas, with_hits=False):
        """reference_points [bs, D, Q, 3] -> (reference_points_cam [cams, bs, Q, D, 2], bev_mask [cams, bs, Q, D] bool)
        and, with_hits, the per-query camera bitmask and hit count the kernel writes beside them."""
        ref = reference_points[0].float()
        lidar2img = self._lidar2img(img_metas, ref.device)
        shape = img_metas[0]["img_shape"][0]
        ref_cam, mask, bits, count = _ops.point_sampling(ref, lidar2img, point_cloud_range, int(shape[0]), int(shape[1]))
        mask = mask.bool()
        return (ref_cam, mask, bits, count) if with_hits else (ref_cam, mask)

    def forward(self, bev_query, key, value, *args, bev_h=None, bev_w=None, bev_pos=None, spatial_shapes=None,
                level_start_index=None, valid_ratios=None, prev_bev=None, shift=0.0, **kwargs):
        """bev_query, bev_pos and prev_bev [Q, bs, E]; key, value [cams, S, bs, E]; shift [bs, 2];
        kwargs['img_metas']: per frame 'lidar2img' ([cams, 4, 4], a device tensor to stay free of host copies) and
        'img_shape'.  -> [bs, Q, E] ([num_layers, bs, Q, E] with return_intermediate)."""
        if self.training:
            raise NotImplementedError("BEVFormerEncoder: inference only")
        bs, dev = bev_query.shape[1], bev_query.device
        ref_3d, ref_2d = self._reference_points(bev_h, bev_w, bs, bev_query.dtype, dev)
        reference_points_cam, bev_mask, hit_bits, _ = self.point_sampling(ref_3d, self.point_cloud_range,
                                                                          kwargs["img_metas"], with_hits=True)
        if isinstance(shift, torch.Tensor):
            ref_2d = ref_2d + shift.to(ref_2d.dtype)[:, None, None, :]
        elif shift:
            ref_2d = ref_2d + shift
        bev_query = bev_query.permute(1, 0, 2)
        bev_pos = bev_pos.permute(1, 0, 2)
        _, len_bev, num_bev_level, _ = ref_2d.shape
        if prev_bev is None:
            prev_bev = bev_query
        else:
            prev_bev = prev_bev.permute(1, 0, 2)
            prev_bev = torch.where((prev_bev != 0).any(), prev_bev, bev_query)  # the flag stays on the device
        prev_bev = torch.stack([prev_bev, bev_query], 1).reshape(bs * 2, len_bev, -1)
        hybird_ref_2d = torch.stack([ref_2d, ref_2d], 1).reshape(bs * 2, len_bev, num_bev_level, 2)
        bev_levels = _bev_levels(bev_h, bev_w, dev)
        intermediate = []
        for layer in self.layers:
            output = layer(bev_query, key, value, *args, bev_pos=bev_pos, ref_2d=hybird_ref_2d, ref_3d=ref_3d, bev_h=bev_h,
                           bev_w=bev_w, spatial_shapes=spatial_shapes, level_start_index=level_start_index,
                           reference_points_cam=reference_points_cam, bev_mask=bev_mask, hit_bits=hit_bits,
                           prev_bev=prev_bev, bev_levels=bev_levels, **kwargs)
            bev_query = output
            if self.return_intermediate:
                intermediate.append(output)
        return torch.stack(intermediate) if self.return_intermediate else output
