"""PETR / PETRv2's head at inference on the device ops (paddle3d/models/heads/dense_heads/petr_head.py,
models/layers/petr_transformer.py, models/layers/transformer_layers.py, models/layers/positional_encoding.py:31-121).
The modules have the reference's constructor arguments and state-dict keys, so checkpoint.load_paddle_state_dict places
the head's entries of a PETR `.pdparams` unchanged.

pos2posemb3d(pos, num_pos_feats, temperature)   petr_head.py:63-78
SinePositionalEncoding3D(num_feats, temperature, normalize, scale, eps, offset)     mask [B, N, H, W] -> [B, N, 3 F, H, W]
SELayer(channels), RegLayer(embed_dims, shared_reg_fcs, group_reg_dims)
MultiHeadAttention(embed_dims, num_heads, attn_drop, proj_drop, drop_prob, fused=True)
                                    the self-attention wrapper (transformer_layers.py:304-376).  fused=True without a
                                    mask: the three Linears, ops.bevformer_decoder.multihead_attention (pd3_mha_forward),
                                    out_proj.  Otherwise, or on a refused shape, the same arithmetic in torch.
PETRMultiheadAttention(embed_dims, num_heads, attn_drop, proj_drop, drop_prob, fused=True)
                                    the cross-attention over the camera tokens with a key_padding_mask [B, Nk] or
                                    [B, 1, Nk].  fused=True without an attn_mask: ops.petr.multihead_attention_stream
                                    (pd3_mha_stream_forward: any number of keys, no score tensor: 173 MB to 1.4 GB per
                                    layer and frame never allocated).  Otherwise, or on a refused shape, matmul, add
                                    mask, softmax, matmul in torch.
                                    The layer's, decoder's and head's `fused` reach both attentions; `fused=False` in
                                    an attention's own cfg opts out.  Measured at 900 queries, 8 heads of 32 (DESIGN.md
                                    4.5z): on its own the streamed kernel is faster than torch at 750 keys (1.49 x) and
                                    SLOWER from 1500 keys up (0.82 x; 0.65 x at PETR's 6000, 0.75 x at PETRv2's 12000),
                                    and pd3_mha_forward is 0.90 x at 900 x 900 (4.5y); the eager 6-layer head at B = 1,
                                    which is bound by launches, is all the same faster with both kernels (5.45 ms) than
                                    with torch's attentions (6.03 ms).  Opt out where device time is what counts (a
                                    captured graph, larger batches).
PETRTransformerDecoderLayer(attns, feedforward_channels, ffn_dropout, operation_order, ..., fused=True)
PETRTransformerDecoder(transformerlayers, num_layers, post_norm_cfg, return_intermediate, fused=True)   post-norm
PETRTransformer(decoder_embed_dims, decoder, fused=True)      forward(x [B, N, C, H, W], mask [B, N, H, W], query_embed
                                    [Q, C], pos_embed) -> (out_dec [layers, B, Q, C], memory)
PETRHead(num_classes, in_channels, num_query, transformer, positional_encoding, bbox_coder, with_position, with_multiview,
         depth_num, LID, depth_start, position_level, position_range, group_reg_dims, with_fpe, with_time, with_multi,
         embed_dims=256, fused=True)
                                    position_embeding(feat_shape, pad_shape, masks, img2lidars) is petr_head.py:364-450:
                                    fused=True takes the coordinates from ops.petr.petr_coords3d (one launch), then the
                                    position encoder's 1x1 convolutions in torch.  forward(mlvl_feats, img2lidars,
                                    pad_shape, img_shape=None, timestamp=None) is the inference branch of :575-750;
                                    get_bboxes(preds_dicts) decodes through ops.bevformer_decoder.nms_free_decode with z
                                    moved to the box bottom.

Where this departs from the reference, on purpose:
  * forward takes img2lidars [B, N, 4, 4] as a device tensor (the caller inverts lidar2img, as the reference's export
    mode does), pad_shape (h, w) and img_shape ((h, w) for every camera, or [B][N] pairs) as host integers, and
    timestamp [B, 2 * 6] as a tensor: nothing in it reads a device value on the host.
  * embed_dims is an argument (the reference hard-codes 256); normedlinear and the denoising queries are training
    options and are not implemented (with_denoise gives no mask at inference).

Linear, LayerNorm, the FFN, the 1x1 convolutions, SELayer and the sine encodings are torch.  Inference only; nothing in
the forwards synchronises with the host.
"""
from __future__ import annotations

import copy
import math

import torch
import torch.nn.functional as F
from torch import nn

from .bevformer import FFN, _check_heads
from .bevformer_head import NMSFreeCoder, _PaddleMHA, inverse_sigmoid
from .ops import bevformer_decoder as _dec_ops
from .ops import petr as _ops

__all__ = ["pos2posemb3d", "SinePositionalEncoding3D", "SELayer", "RegLayer", "MultiHeadAttention",
           "PETRMultiheadAttention", "PETRTransformerDecoderLayer", "PETRTransformerDecoder", "PETRTransformer",
           "PETRHead"]


def _dim_t(num_feats, temperature, device):
    dim_t = torch.arange(num_feats, dtype=torch.int32, device=device)
    return temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / num_feats)


def _sincos(pos):
    return torch.stack((pos[..., 0::2].sin(), pos[..., 1::2].cos()), dim=-1).flatten(-2)


def pos2posemb3d(pos, num_pos_feats=128, temperature=10000):
    pos = pos * (2 * math.pi)
    dim_t = _dim_t(num_pos_feats, temperature, pos.device)
    pos_x, pos_y, pos_z = (_sincos(pos[..., i, None] / dim_t) for i in range(3))
    return torch.cat((pos_y, pos_x, pos_z), dim=-1)


class SinePositionalEncoding3D(nn.Module):
    def __init__(self, num_feats, temperature=10000, normalize=False, scale=2 * math.pi, eps=1e-6, offset=0.0,
                 init_cfg=None):
        super().__init__()
        self.num_feats = num_feats
        self.temperature = temperature
        self.normalize = normalize
        self.scale = scale
        self.eps = eps
        self.offset = offset

    def forward(self, mask):
        not_mask = 1 - mask.to(torch.int32)
        n_embed = not_mask.cumsum(1, dtype=torch.float32)
        y_embed = not_mask.cumsum(2, dtype=torch.float32)
        x_embed = not_mask.cumsum(3, dtype=torch.float32)
        if self.normalize:
            n_embed = (n_embed + self.offset) / (n_embed[:, -1:, :, :] + self.eps) * self.scale
            y_embed = (y_embed + self.offset) / (y_embed[:, :, -1:, :] + self.eps) * self.scale
            x_embed = (x_embed + self.offset) / (x_embed[:, :, :, -1:] + self.eps) * self.scale
        dim_t = _dim_t(self.num_feats, self.temperature, mask.device)
        # the reference stacks sin and cos on axis 4, before the feature axis: all sines, then all cosines
        pos_n, pos_x, pos_y = (torch.cat((p[..., 0::2].sin(), p[..., 1::2].cos()), -1)
                               for p in (t[..., None] / dim_t for t in (n_embed, x_embed, y_embed)))
        return torch.cat((pos_n, pos_y, pos_x), dim=4).permute(0, 1, 4, 2, 3)


class _Conv1x1(nn.Conv2d):
    """A 1x1 convolution as a matrix product over the channels, with nn.Conv2d's parameters and state-dict keys.  The
    convolution library picks its algorithm per call, and two runs on the same input then differ in the last bits; the
    matrix product gives the same bits every time, which the guarded memory-safety runs compare."""

    def __init__(self, in_channels, out_channels):
        super().__init__(in_channels, out_channels, kernel_size=1)

    def forward(self, x):
        n, c, h, w = x.shape
        y = torch.matmul(self.weight.reshape(self.out_channels, c), x.reshape(n, c, h * w))
        return (y + self.bias[:, None]).reshape(n, self.out_channels, h, w)


class SELayer(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.conv_reduce = _Conv1x1(channels, channels)
        self.act1 = nn.ReLU()
        self.conv_expand = _Conv1x1(channels, channels)
        self.gate = nn.Sigmoid()

    def forward(self, x, x_se):
        return x * self.gate(self.conv_expand(self.act1(self.conv_reduce(x_se))))


class RegLayer(nn.Module):
    def __init__(self, embed_dims=256, shared_reg_fcs=2, group_reg_dims=(2, 1, 3, 2, 2), drop=0.0):
        super().__init__()
        reg_branch = []
        for _ in range(shared_reg_fcs):
            reg_branch += [nn.Linear(embed_dims, embed_dims), nn.ReLU(), nn.Dropout(drop)]
        self.reg_branch = nn.Sequential(*reg_branch)
        self.task_heads = nn.ModuleList(
            nn.Sequential(nn.Linear(embed_dims, embed_dims), nn.ReLU(), nn.Linear(embed_dims, reg_dim))
            for reg_dim in group_reg_dims)

    def forward(self, x):
        reg_feat = self.reg_branch(x)
        return torch.cat([task_head(reg_feat) for task_head in self.task_heads], -1)


def _attention_core(q, k, v, num_heads, additive=None):
    """paddle.nn.MultiHeadAttention's core in torch on the projected q [B, Nq, E], k, v [B, Nk, E]; `additive` is
    broadcast against the scores [B, M, Nq, Nk]."""
    b, nq, e = q.shape
    d = e // num_heads
    q, k, v = (t.reshape(b, t.shape[1], num_heads, d).permute(0, 2, 1, 3) for t in (q, k, v))
    product = torch.matmul(q * (d ** -0.5), k.transpose(-1, -2))
    if additive is not None:
        product = product + additive
    return torch.matmul(torch.softmax(product, -1), v).permute(0, 2, 1, 3).reshape(b, nq, e)


def _additive(mask, dtype):
    """Paddle's _convert_attention_mask: a boolean mask (true: attend) becomes (cast(mask) - 1.0) * 1e9."""
    return (mask.to(dtype) - 1.0) * 1e9 if mask.dtype == torch.bool else mask.to(dtype)


class _AttentionWrapper(nn.Module):
    """What MultiHeadAttention and PETRMultiheadAttention share: the positional sums and the residual."""

    def __init__(self, embed_dims, num_heads, attn_drop=0.0, proj_drop=0.0, drop_prob=0.0, batch_first=True, fused=True,
                 init_cfg=None, **kwargs):
        super().__init__()
        _check_heads(embed_dims, num_heads)
        self.embed_dims = embed_dims
        self.num_heads = num_heads
        self.batch_first = True  # only batch first, as the reference's layers are built
        self.attn = _PaddleMHA(embed_dims, num_heads)
        self.proj_drop = nn.Dropout(proj_drop)
        self.fused = bool(fused)

    def _inputs(self, query, key, value, identity, query_pos, key_pos):
        if self.training:
            raise NotImplementedError(f"{type(self).__name__}: inference only")
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
        a = self.attn
        return a.q_proj(query).float(), a.k_proj(key).float(), a.v_proj(value).float(), identity


class MultiHeadAttention(_AttentionWrapper):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.dropout_layer = nn.Identity()

    def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_pos=None, attn_mask=None,
                key_padding_mask=None, **kwargs):
        if key_padding_mask is not None:
            raise NotImplementedError("key_padding_mask is not None not support now")
        q, k, v, identity = self._inputs(query, key, value, identity, query_pos, key_pos)
        out = None
        if self.fused and attn_mask is None and _dec_ops.mha_supported(self.attn.head_dim, int(k.shape[1])):
            out = _dec_ops.multihead_attention(q, k, v, self.num_heads)
        if out is None:
            out = _attention_core(q, k, v, self.num_heads, None if attn_mask is None else _additive(~attn_mask, q.dtype))
        return identity + self.dropout_layer(self.proj_drop(self.attn.out_proj(out)))


class PETRMultiheadAttention(_AttentionWrapper):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.dropout = nn.Identity()

    def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_pos=None, attn_mask=None,
                key_padding_mask=None, **kwargs):
        if key_padding_mask is not None and attn_mask is not None:
            raise NotImplementedError("key_padding_mask is not None")
        q, k, v, identity = self._inputs(query, key, value, identity, query_pos, key_pos)
        out = None
        if self.fused and attn_mask is None and _ops.mha_stream_supported(self.attn.head_dim, int(k.shape[1])):
            out = _ops.multihead_attention_stream(q, k, v, self.num_heads, key_padding_mask)
        if out is None:
            additive = None
            if key_padding_mask is not None:
                keep = ~key_padding_mask.to(torch.bool).reshape(q.shape[0], 1, 1, k.shape[1])
                additive = _additive(keep, q.dtype)
            elif attn_mask is not None:
                additive = _additive(~attn_mask, q.dtype)
            out = _attention_core(q, k, v, self.num_heads, additive)
        return identity + self.dropout(self.proj_drop(self.attn.out_proj(out)))


ATTENTIONS = {"MultiHeadAttention": MultiHeadAttention, "PETRMultiheadAttention": PETRMultiheadAttention}


class PETRTransformerDecoderLayer(nn.Module):
    def __init__(self, attns, feedforward_channels, ffn_dropout=0.0, operation_order=None,
                 act_cfg=dict(type_name="ReLU"), norm_cfg=dict(type_name="LayerNorm"), ffn_num_fcs=2, use_recompute=True,
                 batch_first=True, fused=True, **kwargs):
        super().__init__()
        names = {"self_attn", "norm", "ffn", "cross_attn"}
        assert len(operation_order) == 6 and set(operation_order) == names, operation_order
        num_attn = operation_order.count("self_attn") + operation_order.count("cross_attn")
        assert num_attn == len(attns), (num_attn, len(attns))
        self.batch_first = batch_first
        self.num_attn = num_attn
        self.operation_order = tuple(operation_order)
        self.norm_cfg = norm_cfg
        self.pre_norm = operation_order[0] == "norm"
        self.use_recompute = use_recompute
        self.attentions = nn.ModuleList()
        index = 0
        for name in operation_order:
            if name in ("self_attn", "cross_attn"):
                attention = attns[index]
                if isinstance(attention, dict):
                    cfg = copy.deepcopy(attention)
                    # the layer's `fused` reaches both attentions; `fused=False` in an attention's own cfg opts out.
                    # Alone, the kernels are slower on the device than torch's formulation at PETR's shapes, but the
                    # eager head at B = 1 is launch bound and is faster with their one launch each
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
            raise ValueError("PETRTransformerDecoderLayer: LayerNorm only")
        self.norms = nn.ModuleList(nn.LayerNorm(self.embed_dims, eps=1e-5) for _ in range(operation_order.count("norm")))

    def forward(self, query, key=None, value=None, query_pos=None, key_pos=None, attn_masks=None,
                query_key_padding_mask=None, key_padding_mask=None, **kwargs):
        if self.training:
            raise NotImplementedError("PETRTransformerDecoderLayer: inference only")
        kwargs.pop("reg_branch", None)
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


class PETRTransformerDecoder(nn.Module):
    def __init__(self, transformerlayers=None, num_layers=None, post_norm_cfg=dict(type_name="LN"),
                 return_intermediate=False, fused=True):
        super().__init__()
        self.num_layers = num_layers
        self.layers = nn.ModuleList()
        for _ in range(num_layers):
            cfg = copy.deepcopy(transformerlayers)
            cfg.pop("type_name", None)
            cfg.setdefault("fused", fused)
            self.layers.append(PETRTransformerDecoderLayer(**cfg))
        self.embed_dims = self.layers[0].embed_dims
        self.pre_norm = self.layers[0].pre_norm
        self.return_intermediate = return_intermediate
        self.post_norm = nn.LayerNorm(self.embed_dims, eps=1e-5) if post_norm_cfg is not None else None

    def forward(self, query, *args, **kwargs):
        """query [B, Q, E] -> [layers, B, Q, E] with return_intermediate (each after post_norm), else [1, B, Q, E]."""
        if self.training:
            raise NotImplementedError("PETRTransformerDecoder: inference only")
        intermediate = []
        for layer in self.layers:
            query = layer(query, *args, **kwargs)
            if self.return_intermediate:
                intermediate.append(self.post_norm(query) if self.post_norm is not None else query)
        if self.return_intermediate:
            return torch.stack(intermediate)
        return self.post_norm(query)[None] if self.post_norm is not None else query


class PETRTransformer(nn.Module):
    def __init__(self, decoder_embed_dims, encoder=None, decoder=None, init_cfg=None, cross=False, fused=True):
        super().__init__()
        if isinstance(decoder, dict):
            cfg = copy.deepcopy(decoder)
            cfg.pop("type_name", None)
            cfg.setdefault("fused", fused)
            decoder = PETRTransformerDecoder(**cfg)
        self.encoder = encoder
        self.decoder = decoder
        self.embed_dims = decoder_embed_dims
        self.cross = cross

    def forward(self, x, mask, query_embed, pos_embed, reg_branch=None):
        bs, n, c, h, w = x.shape
        memory = x.permute(0, 1, 3, 4, 2).reshape(bs, -1, c)
        pos_embed = pos_embed.permute(0, 1, 3, 4, 2).reshape(bs, -1, c)
        query_embed = query_embed.unsqueeze(0).expand(bs, -1, -1)
        mask = mask.reshape(bs, 1, -1)
        target = torch.zeros_like(query_embed)
        out_dec = self.decoder(query=target, key=memory, value=memory, key_pos=pos_embed, query_pos=query_embed,
                               key_padding_mask=mask, reg_branch=reg_branch)
        memory = memory.reshape(n, h, w, bs, c).permute(3, 0, 4, 1, 2)
        return out_dec, memory


class PETRHead(nn.Module):
    def __init__(self, num_classes, in_channels, num_query=100, num_reg_fcs=2, transformer=None,
                 sync_cls_avg_factor=False, positional_encoding=None, code_weights=None, bbox_coder=None,
                 with_position=True, with_multiview=False, depth_step=0.8, depth_num=64, LID=False, depth_start=1,
                 position_level=0, position_range=[-65, -65, -8.0, 65, 65, 8.0], group_reg_dims=(2, 1, 3, 2, 2),
                 normedlinear=False, with_fpe=False, with_time=False, with_multi=False, with_denoise=False,
                 code_size=10, embed_dims=256, fused=True, **kwargs):
        super().__init__()
        if normedlinear:
            raise NotImplementedError("PETRHead: normedlinear is not supported")
        self.code_size = code_size
        code_weights = (code_weights if code_weights is not None else [1.0] * 8 + [0.2, 0.2])[:code_size]
        self.code_weights = nn.Parameter(torch.tensor(code_weights, dtype=torch.float32), requires_grad=False)
        self.num_query = num_query
        self.num_classes = num_classes
        self.cls_out_channels = num_classes
        self.in_channels = in_channels
        self.num_reg_fcs = num_reg_fcs
        self.embed_dims = embed_dims
        self.depth_step = depth_step
        self.depth_num = depth_num
        self.position_dim = 3 * depth_num
        self.position_range = [float(v) for v in position_range]
        self.LID = LID
        self.depth_start = depth_start
        self.position_level = position_level
        self.with_position = with_position
        self.with_multiview = with_multiview
        self.with_fpe = with_fpe
        self.with_time = with_time
        self.with_multi = with_multi
        self.with_denoise = with_denoise
        self.group_reg_dims = group_reg_dims
        self.fused = bool(fused)
        if isinstance(positional_encoding, dict):
            cfg = copy.deepcopy(positional_encoding)
            cfg.pop("type_name", None)
            positional_encoding = SinePositionalEncoding3D(**cfg)
        self.positional_encoding = positional_encoding
        if isinstance(bbox_coder, dict):
            cfg = copy.deepcopy(bbox_coder)
            cfg.pop("type_name", None)
            cfg.setdefault("fused", fused)
            bbox_coder = NMSFreeCoder(**cfg)
        self.bbox_coder = bbox_coder
        self.pc_range = bbox_coder.point_cloud_range
        if isinstance(transformer, dict):
            cfg = copy.deepcopy(transformer)
            cfg.pop("type_name", None)
            cfg.setdefault("fused", fused)
            transformer = PETRTransformer(**cfg)
        self.transformer = transformer
        self.num_pred = transformer.decoder.num_layers  # the reference hard-codes 6, its configs' num_layers
        self._mask_cache = None
        self._init_layers()

    def _init_layers(self):
        e = self.embed_dims
        self.input_proj = _Conv1x1(self.in_channels, e)
        cls_branch = []
        for _ in range(self.num_reg_fcs):
            cls_branch += [nn.Linear(e, e), nn.LayerNorm(e), nn.ReLU()]
        cls_branch.append(nn.Linear(e, self.cls_out_channels))
        fc_cls = nn.Sequential(*cls_branch)
        if self.with_multi:
            reg_branch = RegLayer(e, self.num_reg_fcs, self.group_reg_dims)
        else:
            reg_branch = []
            for _ in range(self.num_reg_fcs):
                reg_branch += [nn.Linear(e, e), nn.ReLU()]
            reg_branch.append(nn.Linear(e, self.code_size))
            reg_branch = nn.Sequential(*reg_branch)
        self.cls_branches = nn.ModuleList(copy.deepcopy(fc_cls) for _ in range(self.num_pred))
        self.reg_branches = nn.ModuleList(copy.deepcopy(reg_branch) for _ in range(self.num_pred))
        a = e * 3 // 2 if self.with_multiview else e
        self.adapt_pos3d = nn.Sequential(_Conv1x1(a, e * 4 if self.with_multiview else e), nn.ReLU(),
                                         _Conv1x1(e * 4 if self.with_multiview else e, e))
        if self.with_position:
            self.position_encoder = nn.Sequential(_Conv1x1(self.position_dim, e * 4), nn.ReLU(),
                                                  _Conv1x1(e * 4, e))
        self.reference_points = nn.Embedding(self.num_query, 3)
        self.query_embedding = nn.Sequential(nn.Linear(e * 3 // 2, e), nn.ReLU(), nn.Linear(e, e))
        if self.with_fpe:
            self.fpe = SELayer(e)

    def coords3d_torch(self, feat_shape, pad_shape, masks, img2lidars):
        """petr_head.py:369-446 in torch: (inverse_sigmoid(coords3d) [B N, 3 D, H, W], coords_mask [B, N, H, W])."""
        eps = 1e-5
        B, N, _, H, W = feat_shape
        pad_h, pad_w = pad_shape
        dev, r = img2lidars.device, self.position_range
        coords_h = torch.arange(H, dtype=torch.float32, device=dev) * pad_h / H
        coords_w = torch.arange(W, dtype=torch.float32, device=dev) * pad_w / W
        index = torch.arange(0, self.depth_num, 1, dtype=torch.float32, device=dev)
        if self.LID:
            bin_size = (r[3] - self.depth_start) / (self.depth_num * (1 + self.depth_num))
            coords_d = self.depth_start + bin_size * index * (index + 1)
        else:
            bin_size = (r[3] - self.depth_start) / self.depth_num
            coords_d = self.depth_start + bin_size * index
        D = self.depth_num
        coords = torch.stack(torch.meshgrid([coords_w, coords_h, coords_d], indexing="ij")).permute(1, 2, 3, 0)
        coords = torch.cat((coords, torch.ones_like(coords[..., :1])), -1)
        xy = coords[..., :2] * torch.maximum(coords[..., 2:3], torch.ones_like(coords[..., 2:3]) * eps)
        coords = torch.cat((xy, coords[..., 2:]), -1)
        coords = coords.reshape(1, 1, W, H, D, 4, 1)
        m = img2lidars.float().reshape(B, N, 1, 1, 1, 4, 4)
        coords3d = torch.matmul(m, coords).squeeze(-1)[..., :3]
        coords3d = torch.cat([(coords3d[..., i:i + 1] - r[i]) / (r[i + 3] - r[i]) for i in range(3)], -1)
        coords_mask = (coords3d > 1.0) | (coords3d < 0.0)
        coords_mask = coords_mask.to(torch.float32).flatten(-2).sum(-1) > (D * 0.5)
        coords_mask = masks | coords_mask.permute(0, 1, 3, 2)
        coords3d = coords3d.permute(0, 1, 4, 5, 3, 2).reshape(B * N, D * 3, H, W)
        return inverse_sigmoid(coords3d), coords_mask

    def position_embeding(self, feat_shape, pad_shape, masks, img2lidars):
        """feat_shape (B, N, C, H, W) of the feature level, pad_shape (h, w), masks bool [B, N, H, W], img2lidars
        [B, N, 4, 4] -> (position embedding [B, N, E, H, W], coords_mask [B, N, H, W])."""
        B, N, _, H, W = feat_shape
        out = None
        if self.fused and _ops.coords3d_supported(B * N, H, W, self.depth_num):
            out = _ops.petr_coords3d(img2lidars.float(), (H, W), pad_shape, self.depth_num, self.depth_start,
                                     self.position_range, self.LID, token_mask=masks, want_mask=True)
        if out is None:
            coords3d, coords_mask = self.coords3d_torch(feat_shape, pad_shape, masks, img2lidars)
        else:
            coords3d, coords_mask = out[0], out[1].reshape(B, N, H, W)
        emb = self.position_encoder(coords3d)
        return emb.reshape(B, N, self.embed_dims, H, W), coords_mask

    @staticmethod
    def _build_masks(B, N, pad_shape, img_shape, size, device):
        pad_h, pad_w = pad_shape
        masks = torch.ones((B, N, pad_h, pad_w), device=device)
        if img_shape is None:
            img_shape = pad_shape
        if isinstance(img_shape[0], (int, float)):
            masks[:, :, :int(img_shape[0]), :int(img_shape[1])] = 0
        else:
            for b in range(B):
                for n in range(N):
                    masks[b, n, :int(img_shape[b][n][0]), :int(img_shape[b][n][1])] = 0
        return F.interpolate(masks, size=size).to(torch.bool)

    def _masks(self, B, N, pad_shape, img_shape, size, device):
        """The padding masks at feature resolution, bool [B, N, H, W]: petr_head.py:603-621.  They depend on host integers
        only, so the last one built is kept (B * N slice assignments on the padded image and an interpolation else)."""
        shapes = None if img_shape is None else repr(img_shape)
        key = (B, N, tuple(pad_shape), shapes, tuple(size), str(device))
        if self._mask_cache is None or self._mask_cache[0] != key:
            self._mask_cache = (key, self._build_masks(B, N, pad_shape, img_shape, size, device))
        return self._mask_cache[1]

    def forward(self, mlvl_feats, img2lidars, pad_shape, img_shape=None, timestamp=None):
        """mlvl_feats: [B, N, C, H, W] per level; img2lidars [B, N, 4, 4]; pad_shape (h, w) and img_shape as host
        integers; timestamp [B, 2 * 6] (with_time) -> the reference's `outs` dict."""
        if self.training:
            raise NotImplementedError("PETRHead: inference only")
        x = mlvl_feats[self.position_level]
        B, N = int(x.shape[0]), int(x.shape[1])
        feat_shape = tuple(int(s) for s in x.shape)
        pad_shape = (int(pad_shape[0]), int(pad_shape[1]))
        x = self.input_proj(x.flatten(0, 1))
        x = x.reshape(B, N, *x.shape[-3:])
        masks = self._masks(B, N, pad_shape, img_shape, tuple(x.shape[-2:]), x.device)
        if self.with_position:
            pos_embed, _ = self.position_embeding(feat_shape, pad_shape, masks, img2lidars)
            if self.with_fpe:
                pos_embed = self.fpe(pos_embed.flatten(0, 1), x.flatten(0, 1)).reshape(x.shape)
            if self.with_multiview:
                sin_embed = self.positional_encoding(masks)
            else:
                sin_embed = torch.cat([self.positional_encoding(masks[:, i, :, :]).unsqueeze(1) for i in range(N)], 1)
            pos_embed = pos_embed + self.adapt_pos3d(sin_embed.flatten(0, 1)).reshape(x.shape)
        elif self.with_multiview:
            pos_embed = self.adapt_pos3d(self.positional_encoding(masks).flatten(0, 1)).reshape(x.shape)
        else:
            pos_embed = torch.cat([self.positional_encoding(masks[:, i, :, :]).unsqueeze(1) for i in range(N)], 1)
        reference_points = self.reference_points.weight
        query_embeds = self.query_embedding(pos2posemb3d(reference_points, self.embed_dims // 2))
        reference_points = reference_points.unsqueeze(0).expand(B, -1, -1)
        outs_dec, _ = self.transformer(x, masks, query_embeds, pos_embed, self.reg_branches)
        outs_dec = torch.nan_to_num(outs_dec, nan=0.0)
        if self.with_time:
            time_stamp = timestamp.to(x.dtype).reshape(B, -1, 6)
            mean_time_stamp = (time_stamp[:, 1, :] - time_stamp[:, 0, :]).mean(-1)
        pc = self.pc_range
        outputs_classes, outputs_coords = [], []
        for lvl in range(outs_dec.shape[0]):
            reference = inverse_sigmoid(reference_points)
            outputs_class = self.cls_branches[lvl](outs_dec[lvl])
            tmp = self.reg_branches[lvl](outs_dec[lvl]).clone()
            tmp[..., 0:2] = torch.sigmoid(tmp[..., 0:2] + reference[..., 0:2])
            tmp[..., 4:5] = torch.sigmoid(tmp[..., 4:5] + reference[..., 2:3])
            if self.with_time:
                tmp[..., 8:] = tmp[..., 8:] / mean_time_stamp[:, None, None]
            tmp[..., 0:1] = tmp[..., 0:1] * (pc[3] - pc[0]) + pc[0]
            tmp[..., 1:2] = tmp[..., 1:2] * (pc[4] - pc[1]) + pc[1]
            tmp[..., 4:5] = tmp[..., 4:5] * (pc[5] - pc[2]) + pc[2]
            outputs_classes.append(outputs_class)
            outputs_coords.append(tmp)
        return dict(all_cls_scores=torch.stack(outputs_classes), all_bbox_preds=torch.stack(outputs_coords),
                    enc_cls_scores=None, enc_bbox_preds=None, dn_mask_dict=None)

    def get_bboxes(self, preds_dicts, img_metas=None, rescale=False):
        """(boxes [B, max_num, code - 1] with z at the box bottom, scores, labels, count); NMSFreeCoder.to_list turns them
        into the reference's per-frame list."""
        preds = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in preds_dicts.items()}
        return self.bbox_coder.decode(preds, bottom_center=True)
