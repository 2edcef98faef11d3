"""CAPE / CAPE-T's attention layers at inference on the device ops (paddle3d/models/layers/cape_transformer.py).  The
modules have the reference's constructor arguments, attribute names and state-dict keys, so
checkpoint.load_paddle_state_dict places the entries of a CAPE `.pdparams` unchanged.

pos2posemb3d(pos, num_pos_feats, temperature, fused=True)      cape_transformer.py:76-91; on the device through
                                    ops.cape.posemb3d (pd3_cape_posemb3d), else torch
world_posemb3d(ref_points, bound, R, t, num_pos_feats, fused=True)
                                    prepare_emb's un-normalise, + t, R @ and pos2posemb3d (:540-541, :556-559) as one
                                    launch: ref_points [B, Q, 3], R [B, N, 3, 3], t [B, N, 3] -> [B, N, Q, 3 F]
QcR_Modulation(dim), V_R_Modulation(dim), SELayer(channels), MLP(input_dim, hidden_dim, output_dim, num_layers)
CrossAttention(dim, heads, dim_head, qkv_bias, fused=True)
                                    forward(k_g, q_g, k_a, q_a, v, mask) is :200-269.  The five Linears of proj_dict,
                                    then the attention over the keys of all cameras: with the kernel
                                    (ops.cape.cross_view_attention, pd3_cape_cva_forward) no [b, heads, n, Q, K] tensor
                                    and no permuted copy is formed; in torch it is the reference's two einsums, scales,
                                    add, fill, softmax, einsum.  Then proj, skip, prenorm, mlp, postnorm in torch.
CrossViewAttention(num_queries, hidden_dim, qkv_bias, heads, dim_head, conditional, fused=True)
                                    forward(x, modulated_x, lidar_obj_pe, feature, camera_pe, mask, img_embed,
                                    bev_embed, attn_mask) is :725-757; sl_layer can go through
                                    ops.bevformer_decoder.multihead_attention (pd3_mha_forward) when attn_mask is None.

Ego_emb(dim), MLP_Fusion(dim)      :109-162, with the ego matrix (curlidar2prevlidar) as a device tensor argument
CAPETransformer(...)                :288-697 at inference, with and without with_time (see the class); cape_transformer(
                                    config, fused) builds it with the numbers of one of the three configs.
CAPETemporalDNHead(...)             heads/dense_heads/cape_dn_head.py: forward's eval path and get_bboxes (see the class)
CAPE(pts_bbox_head, img_backbone, img_neck), cape_r50_1408x512(), capet_r50_704x256(), capet_vovnet_800x320()
                                    the detector behind any torch.nn.Module as backbone and neck, with the three configs'
                                    numbers.

`fused`: True takes a kernel where its predicate accepts the shape and where it was measured faster than the torch
composition: the cross-view attention up to CVA_FUSED_MAX_KEYS keys (N * K), sl_layer's up to SL_FUSED_MAX_KEYS, the
position embeddings always; "force" takes it wherever the predicate accepts; False is the plain-torch transcription
of the reference, which is also what runs on the CPU.  Inference only; nothing in the forwards synchronises with the
host.
"""
from __future__ import annotations

import copy
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .bevformer_head import NMSFreeCoder, _PaddleMHA, inverse_sigmoid
from .ops import bevformer_decoder as _dec_ops
from .ops import cape as _ops
from .ops import petr as _petr_ops
from .petr_head import PETRHead, RegLayer, _Conv1x1

__all__ = ["pos2posemb3d", "world_posemb3d", "QcR_Modulation", "V_R_Modulation", "SELayer", "MLP", "CrossAttention",
           "CrossViewAttention", "Ego_emb", "MLP_Fusion", "CAPETransformer", "curlidar2prevlidar", "cape_transformer",
           "TRANSFORMER_CONFIGS", "CAPETemporalDNHead", "CAPE", "cape_r50_1408x512", "capet_r50_704x256",
           "capet_vovnet_800x320", "CVA_FUSED_MAX_KEYS", "SL_FUSED_MAX_KEYS"]

# fused=True takes pd3_cape_cva_forward up to this many keys (N * K) and torch above.  Measured on the MI355X against
# core_torch at 900 queries, 8 heads of 64, 6 cameras, b = 2 (tools/prof/cape.py --sweep): the kernel is
# 1.88 x torch at 96 keys and 1.10 x at 192, and SLOWER from 384 keys up (0.60 x; 0.57 x at CAPE-T's 1056 and 1500, 0.59 x
# at CAPE's 4224), so at the three configs' shapes it stays behind fused="force".
CVA_FUSED_MAX_KEYS = 192
# fused=True takes pd3_mha_forward for sl_layer up to this many keys.  Measured at the configs' 900 x 900, 8 heads of 64,
# b = 2: 0.58 x torch; no smaller size was measured, so the default takes it nowhere and fused="force" everywhere.
SL_FUSED_MAX_KEYS = 0


def _check_fused(fused):
    if fused not in (True, False, "force"):
        raise ValueError(f"fused must be True, False or 'force', got {fused!r}")
    return fused


def _on_device(fused, t):
    return bool(fused) and t.is_cuda and t.dtype == torch.float32


def _sincos(pos):
    return torch.stack((pos[..., 0::2].sin(), pos[..., 1::2].cos()), dim=-1).flatten(-2)


def pos2posemb3d(pos, num_pos_feats=128, temperature=10000, fused=True):
    if _on_device(_check_fused(fused), pos) and _ops.posemb3d_supported(num_pos_feats):
        lead = pos.shape[:-1]
        out = _ops.posemb3d(pos.reshape(1, -1, 3), num_pos_feats, temperature=temperature)
        if out is not None:
            return out.reshape(*lead, 3 * num_pos_feats)
    pos = pos * (2 * math.pi)
    dim_t = torch.arange(num_pos_feats, dtype=torch.int32, device=pos.device)
    dim_t = temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / num_pos_feats)
    pos_x, pos_y, pos_z = (_sincos(pos[..., i, None] / dim_t) for i in range(3))
    return torch.cat((pos_y, pos_x, pos_z), dim=-1)


def world_posemb3d(ref_points, bound, R, t, num_pos_feats=128, fused=True):
    """bound: 6 host floats (lo, hi), the reference's `bound` buffer."""
    if _on_device(_check_fused(fused), ref_points) and _ops.posemb3d_supported(num_pos_feats):
        out = _ops.posemb3d(ref_points, num_pos_feats, bound=bound, rot=R, trans=t)
        if out is not None:
            return out
    lo, hi = np.asarray(bound, np.float32).reshape(2, 3)  # host scalars: a copy to the device would synchronise
    span = hi - lo
    world = torch.stack([ref_points[..., c] * float(span[c]) + float(lo[c]) for c in range(3)], -1)
    world = world[:, None] + t[:, :, None]
    world = (R[:, :, None] @ world[..., None]).squeeze(-1)
    return pos2posemb3d(world, num_pos_feats, fused=False)


class _Modulation(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.scale_emb = nn.Sequential(nn.Linear(9, dim), nn.LayerNorm(dim), nn.Sigmoid())


class QcR_Modulation(_Modulation):
    def forward(self, x, R):
        return x[:, None] * self.scale_emb(R.flatten(2))[:, :, None]  # [b, n, Q, d]


class V_R_Modulation(_Modulation):
    def forward(self, feature, R):
        return feature * self.scale_emb(R.flatten(2))[:, :, None]


class SELayer(nn.Module):
    def __init__(self, channels, act_layer=nn.ReLU, gate_layer=nn.Sigmoid):
        super().__init__()
        self.conv_reduce = nn.Linear(channels, channels)
        self.act1 = act_layer()
        self.conv_expand = nn.Linear(channels, channels)
        self.gate = gate_layer()

    def forward(self, x, x_se):
        return x * self.gate(self.conv_expand(self.act1(self.conv_reduce(x_se))))


class MLP(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        h = [hidden_dim] * (num_layers - 1)
        self.layers = nn.ModuleList(nn.Linear(n, k) for n, k in zip([input_dim] + h, h + [output_dim]))

    def forward(self, x):
        for i, layer in enumerate(self.layers):
            x = F.relu(layer(x)) if i < self.num_layers - 1 else layer(x)
        return x


class CrossAttention(nn.Module):
    def __init__(self, dim, heads, dim_head, qkv_bias, norm=nn.LayerNorm, fused=True):
        super().__init__()
        self.heads = heads
        self.dim_head = dim_head
        self.proj_dict = nn.ModuleDict({name: nn.Linear(dim, heads * dim_head, bias=bool(qkv_bias))
                                        for name in ("q_g", "k_g", "q_a", "k_a", "v")})
        self.proj = nn.Linear(heads * dim_head, dim)
        self.prenorm = norm(dim)
        self.mlp = nn.Sequential(nn.Linear(dim, 2 * dim), nn.GELU(), nn.Linear(2 * dim, dim))
        self.postnorm = norm(dim)
        self.scale_a = nn.Parameter(torch.full((heads,), dim_head ** -0.5))
        self.scale_g = nn.Parameter(torch.full((heads,), dim_head ** -0.5))
        self.fused = _check_fused(fused)

    def takes_kernel(self, q_a, num_cams, num_key):
        """Whether forward runs pd3_cape_cva_forward for these projected rows."""
        if not _on_device(self.fused, q_a) or not _ops.cva_supported(self.dim_head, num_cams, num_key, q_a.shape[1]):
            return False
        return self.fused == "force" or num_cams * num_key <= CVA_FUSED_MAX_KEYS

    def core_torch(self, k_g, q_g, k_a, q_a, v, mask):
        """The reference's composition on the projected rows -> [b, Q, heads * dim_head]."""
        b, n, Q, _ = q_g.shape
        K, m, d = k_g.shape[2], self.heads, self.dim_head
        k_g, k_a, v = (t.reshape(b, n, K, m, d).permute(0, 3, 1, 2, 4) for t in (k_g, k_a, v))      # b m n K d
        q_g = q_g.reshape(b, n, Q, m, d).permute(0, 3, 1, 2, 4)                                     # b m n Q d
        q_a = q_a.reshape(b, 1, Q, m, d).permute(0, 3, 1, 2, 4).expand(b, m, n, Q, d)
        dot_g = torch.einsum("bmnqd,bmnkd->bmnqk", q_g, k_g)
        dot_a = torch.einsum("bmnqd,bmnkd->bmnqk", q_a, k_a)
        dot = dot_a * self.scale_a[None, :, None, None, None] + dot_g * self.scale_g[None, :, None, None, None]
        if mask is not None:
            dot = dot.masked_fill(mask[:, None, :, None, :], float("-inf"))
        att = torch.softmax(dot.permute(0, 1, 3, 2, 4).reshape(b, m, Q, n * K), -1)
        a = torch.einsum("bmqk,bmkd->bmqd", att, v.reshape(b, m, n * K, d))
        return a.permute(0, 2, 1, 3).reshape(b, Q, m * d)

    def core(self, k_g, q_g, k_a, q_a, v, mask):
        if self.takes_kernel(q_a, k_g.shape[1], k_g.shape[2]):
            a = _ops.cross_view_attention(q_a, q_g, k_a, k_g, v, self.scale_a, self.scale_g, self.heads, mask)
            if a is not None:
                return a
        return self.core_torch(k_g, q_g, k_a, q_a, v, mask)

    def forward(self, k_g, q_g, k_a, q_a, v, mask):
        """k_g, k_a, v [b, n, K, dim], q_g [b, n, Q, dim], q_a [b, Q, dim], mask bool [b, n, K] or None."""
        if self.training:
            raise NotImplementedError("CrossAttention: inference only")
        skip = q_a
        p = self.proj_dict
        a = self.core(p["k_g"](k_g), p["q_g"](q_g), p["k_a"](k_a), p["q_a"](q_a), p["v"](v), mask)
        z = self.proj(a)
        if skip is not None:
            z = z + skip
        z = self.prenorm(z)
        z = z + self.mlp(z)
        return self.postnorm(z)


class CrossViewAttention(nn.Module):
    def __init__(self, num_queries, hidden_dim, qkv_bias, heads=4, dim_head=32, conditional=True, fused=True):
        super().__init__()
        self.num_queries = num_queries
        self.hidden_dim = hidden_dim
        self.heads = heads
        self.cross_attend = CrossAttention(hidden_dim, heads, dim_head, qkv_bias, fused=fused)
        self.conditional = MLP(hidden_dim, hidden_dim, hidden_dim, 2) if conditional else None
        self.sl_layer = _PaddleMHA(hidden_dim, heads)
        self.norm1 = nn.LayerNorm(hidden_dim)
        self.dropout1 = nn.Dropout(0.1)
        self.fused = _check_fused(fused)

    def self_attention(self, q, k, v, attn_mask=None):
        """paddle.nn.MultiHeadAttention.forward of sl_layer; attn_mask bool [Q, Q] (true: attend) or None."""
        sl = self.sl_layer
        qp, kp, vp = sl.q_proj(q), sl.k_proj(k), sl.v_proj(v)
        m, d = self.heads, self.hidden_dim // self.heads
        out = None
        if attn_mask is None and _on_device(self.fused, qp) and _dec_ops.mha_supported(d, kp.shape[1]) and \
                (self.fused == "force" or kp.shape[1] <= SL_FUSED_MAX_KEYS):
            out = _dec_ops.multihead_attention(qp, kp, vp, m)
        if out is None:
            b, nq, e = qp.shape
            qh, kh, vh = (t.reshape(b, t.shape[1], m, d).permute(0, 2, 1, 3) for t in (qp, kp, vp))
            product = torch.matmul(qh * (d ** -0.5), kh.transpose(-1, -2))
            if attn_mask is not None:
                product = product + (attn_mask.to(product.dtype) - 1.0) * 1e9
            out = torch.matmul(torch.softmax(product, -1), vh).permute(0, 2, 1, 3).reshape(b, nq, e)
        return sl.out_proj(out)

    def forward(self, x, modulated_x, lidar_obj_pe, feature, camera_pe, mask, img_embed, bev_embed, attn_mask=None):
        if self.training:
            raise NotImplementedError("CrossViewAttention: inference only")
        if self.conditional is not None:
            bev_embed = self.conditional(modulated_x) * bev_embed
        k_a, q_a = feature + camera_pe[:, :, None], x + lidar_obj_pe
        updated_x = self.cross_attend(img_embed, bev_embed, k_a, q_a, feature, mask)
        q = updated_x + lidar_obj_pe
        if attn_mask is not None:
            attn_mask = ~attn_mask
        tgt = self.self_attention(q, q, updated_x, attn_mask)
        return self.norm1(updated_x + tgt)


def curlidar2prevlidar(curlidar2curcam, curlidar2prevcam):
    """Ego_emb.get_curlidar2prevlidar (:121-133) on [4, 4] tensors that are already transposed as the reference does
    (`extrinsics[0].T`, `extrinsics[6].T`): inverse(curlidar2curcam) @ curlidar2prevcam.  Once per forward."""
    return torch.linalg.inv_ex(curlidar2curcam).inverse @ curlidar2prevcam


class Ego_emb(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.ego_emb = nn.Sequential(nn.Linear(9, dim), nn.LayerNorm(dim), nn.Sigmoid())

    def forward(self, ego_matrix):
        """ego_matrix: curlidar2prevlidar [4, 4] (or its [3, 3] corner), a device tensor -> [1, 1, dim]."""
        return self.ego_emb(ego_matrix[:3, :3].reshape(1, 1, 9))


class MLP_Fusion(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.dim = dim
        self.proj_k_a = nn.Linear(dim, dim)
        self.proj_k_b = nn.Linear(dim, dim)
        self.proj_v_a = nn.Linear(dim, dim)
        self.proj_v_b = nn.Linear(dim, dim)
        self.fc = nn.Sequential(nn.Linear(dim * 2, dim), nn.LayerNorm(dim), nn.Sigmoid())
        self.ego_emb = Ego_emb(dim)

    def forward(self, a, b, ego_matrix):
        """a, b [bs, Q, dim] (current and previous frame), ego_matrix as Ego_emb takes it (the reference reads it from
        img_metas on every call; here the transformer hands over the one it made for the forward)."""
        k_a, k_b = self.proj_k_a(a), self.proj_k_b(b)
        w = self.fc(torch.cat([k_a, k_b * self.ego_emb(ego_matrix)], -1))
        return w * self.proj_v_a(a), (1 - w) * self.proj_v_b(b)


class CAPETransformer(nn.Module):
    """cape_transformer.py:288-697 at inference.  forward(feature [bs, nc, C, h, w], mask bool [bs, nc, h, w], I_inv [bs,
    nc, 3, 3], R_inv [bs, nc, 3, 3], t [bs, nc, 3, 1] or [bs, nc, 3], pad_shape (h, w) host integers, ego_matrix=None) with
    nc = num_cameras, or 2 * num_cameras under with_time (current cameras first) -> (outs [layers, bs, Q, hidden],
    reference points [bs, Q, 3]); with return_prev_query also the previous frame's queries.  Where it departs from the
    reference on purpose: pad_shape and ego_matrix (curlidar2prevlidar, see the function of that name) are arguments
    instead of img_metas, so nothing in the forward reads a device value on the host or copies one to it, and every
    camera matrix is inverted once per forward (R = inverse(R_inv) here; the caller makes I_inv, R_inv, t and the ego
    matrix).  prepare_for_dn's eval branch tiles the reference points and gives no mask.  dn_query_embedding is
    training-only and kept as parameters so a checkpoint loads strictly.
    position_embeding (:562-622): fused takes the frustum coordinates and coords_mask from ops.petr.petr_coords3d
    (pd3_petr_coords3d) with I_inv in the upper-left of a 4 x 4 whose last column is zero, LID bins and
    cam_position_range; otherwise the reference's torch form."""

    def __init__(self, num_cameras, num_layers, feat_dim, feat_stride, image_height, image_width, bound, with_fpe,
                 depth_start, depth_num, att_layer=None, tf_layer=dict(groups=30, heads=8, hidden_dim=512), scalar=10,
                 noise_scale=1.0, noise_trans=0.0, num_classes=10, with_time=True, fused=True):
        super().__init__()
        self.num_cameras = num_cameras
        self.num_queries = att_layer.num_queries
        self.hidden_dim = att_layer.hidden_dim
        self.feat_dim = feat_dim
        self.with_time = with_time
        self.fused = _check_fused(fused)
        ys, xs = torch.meshgrid(torch.arange(feat_stride / 2, image_height, feat_stride),
                                torch.arange(feat_stride / 2, image_width, feat_stride), indexing="ij")
        self.register_buffer("image_plane", torch.stack([xs, ys, torch.ones_like(xs)], -1).flatten(0, 1).float())
        # image_plane, bound and cam_bound are buffers only because they are entries of the reference's state dict; the
        # forward reads the host copies (bound_host, cam_position_range): a device value never has to come back
        self.register_buffer("bound", torch.tensor(bound, dtype=torch.float32).reshape(2, 3))
        self.bound_host = [float(b) for b in bound]
        self.reference_points = nn.Embedding(self.num_queries, 3)
        nn.init.uniform_(self.reference_points.weight, 0, 1)
        if with_time:
            self.mf = nn.ModuleList(MLP_Fusion(tf_layer["hidden_dim"]) for _ in range(num_layers))
        self.cva_layers = nn.ModuleList(copy.deepcopy(att_layer) for _ in range(num_layers))
        self.cva_layers[0].conditional = None
        self.content_prior = nn.Embedding(self.num_queries, self.hidden_dim)
        self.camera_embedding = nn.Embedding(num_cameras, self.hidden_dim)
        self.bev_embed = MLP(self.hidden_dim * 3 // 2, self.hidden_dim, self.hidden_dim, 2)
        self.feature_linear = nn.Linear(feat_dim, self.hidden_dim)
        self.with_fpe = with_fpe
        if with_fpe:
            self.fpe = SELayer(self.hidden_dim)
        self.depth_start = depth_start
        self.depth_num = depth_num
        self.cam_position_range = [bound[1], -bound[5], depth_start, bound[4], -bound[2], bound[3]]
        self.register_buffer("cam_bound", torch.tensor(self.cam_position_range, dtype=torch.float32).reshape(2, 3))
        self.position_dim = 3 * depth_num
        self.position_encoder = nn.Sequential(_Conv1x1(self.position_dim, self.hidden_dim * 4), nn.ReLU(),
                                              _Conv1x1(self.hidden_dim * 4, self.hidden_dim))
        mlp = lambda: nn.Sequential(nn.Linear(self.hidden_dim * 3 // 2, self.hidden_dim), nn.ReLU(),  # noqa: E731
                                    nn.Linear(self.hidden_dim, self.hidden_dim))
        self.query_embedding = mlp()
        self.dn_query_embedding = mlp()
        self.QcR = QcR_Modulation(self.hidden_dim)
        self.V_R = V_R_Modulation(self.hidden_dim)
        self.num_classes = num_classes
        self.pc_range = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]

    def coords3d(self, I_inv, feat_hw, pad_shape, masks):
        """(coords3d [B * N, 3 * D, H, W] after inverse_sigmoid, coords_mask bool [B, N, H, W]) of :562-618."""
        B, N = I_inv.shape[:2]
        H, W = feat_hw
        pad_h, pad_w = pad_shape
        D = self.depth_num
        if _on_device(self.fused, I_inv) and _petr_ops.coords3d_supported(B * N, H, W, D):
            m = torch.zeros(B * N, 4, 4, dtype=I_inv.dtype, device=I_inv.device)
            m[:, :3, :3] = I_inv.reshape(B * N, 3, 3)
            got = _petr_ops.petr_coords3d(m, (H, W), (pad_h, pad_w), D, self.depth_start, self.cam_position_range, True,
                                          token_mask=masks.reshape(B * N, H, W), want_mask=True)
            if got is not None:
                return got[0], got[1].reshape(B, N, H, W)
        eps, dev = 1e-5, I_inv.device
        coords_h = torch.arange(H, dtype=torch.float32, device=dev) * pad_h / H
        coords_w = torch.arange(W, dtype=torch.float32, device=dev) * pad_w / W
        index = torch.arange(D, dtype=torch.float32, device=dev)
        bin_size = (self.cam_position_range[5] - self.depth_start) / (D * (1 + D))
        coords_d = self.depth_start + bin_size * index * (index + 1)
        coords = torch.stack(torch.meshgrid(coords_w, coords_h, coords_d, indexing="ij"), -1)  # W, H, D, 3
        coords = torch.cat([coords[..., :2] * coords[..., 2:3].clamp(min=eps), coords[..., 2:3]], -1)
        c = torch.matmul(I_inv.reshape(B, N, 1, 1, 1, 3, 3), coords.reshape(1, 1, W, H, D, 3, 1)).squeeze(-1)
        r = self.cam_position_range
        c = torch.stack([(c[..., i] - r[i]) / (r[i + 3] - r[i]) for i in range(3)], -1)
        coords_mask = ((c > 1.0) | (c < 0.0)).to(torch.float32).flatten(-2).sum(-1) > (D * 0.5)
        coords_mask = masks | coords_mask.permute(0, 1, 3, 2)
        c = c.permute(0, 1, 4, 5, 3, 2).reshape(B * N, D * 3, H, W)
        return inverse_sigmoid(c), coords_mask

    def position_embeding(self, img_feats, I_inv, pad_shape, masks):
        B, N, _, H, W = img_feats.shape
        coords3d, coords_mask = self.coords3d(I_inv, (H, W), pad_shape, masks)
        return self.position_encoder(coords3d).reshape(B, N, self.hidden_dim, H, W), coords_mask

    def prepare_emb(self, feature, mask, I_inv, R_inv, t, ref_points, pad_shape, seq_length):
        img_embed, _ = self.position_embeding(feature, I_inv, pad_shape, mask)
        img_embed = img_embed.flatten(-2).permute(0, 1, 3, 2)
        bs, nc, d, h, w = feature.shape
        feature = self.feature_linear(feature.reshape(bs * nc, d, h * w).permute(0, 2, 1)).reshape(bs, nc, h * w, -1)
        if self.with_fpe:
            img_embed = self.fpe(img_embed, feature)
        mask = mask.reshape(bs, nc, -1)
        R = torch.linalg.inv_ex(R_inv).inverse  # inv() reads the factorisation's status on the host
        bev_embed = self.bev_embed(world_posemb3d(ref_points.repeat(seq_length, 1, 1), self.bound_host, R, t,
                                                  self.hidden_dim // 2, fused=self.fused))
        return feature, mask, img_embed, bev_embed, R

    def forward(self, feature, mask, I_inv, R_inv, t, pad_shape, ego_matrix=None, return_prev_query=False):
        if self.training:
            raise NotImplementedError("CAPETransformer: inference only")
        bs, _, d, h, w = feature.shape
        n, f = self.num_cameras, 2 if self.with_time else 1
        feature = feature.reshape(-1, n, d, h, w)
        mask = mask.reshape(-1, n, h, w)
        I_inv, R_inv = I_inv.reshape(-1, n, 3, 3), R_inv.reshape(-1, n, 3, 3)
        t = t.reshape(-1, n, 3)
        x = self.content_prior.weight.unsqueeze(0).repeat(bs, 1, 1)
        ref_points = self.reference_points.weight.unsqueeze(0).repeat(bs, 1, 1)  # prepare_for_dn's eval branch
        lidar_obj_pe = self.query_embedding(pos2posemb3d(ref_points, self.hidden_dim // 2, fused=self.fused))
        cam_pe = self.camera_embedding.weight.repeat(bs, 1, 1)
        feature, mask, img_embed, bev_embed, R = self.prepare_emb(feature, mask, I_inv, R_inv, t, ref_points, pad_shape, f)
        outs, prevs = [], []
        if self.with_time:
            if ego_matrix is None:
                raise RuntimeError("CAPETransformer: with_time needs ego_matrix (curlidar2prevlidar)")
            cur_x = prev_x = x
            lidar_obj_pe = torch.cat([lidar_obj_pe, lidar_obj_pe], 0)
            cam_pe = torch.cat([cam_pe, cam_pe], 0)
            for mf, cva in zip(self.mf, self.cva_layers):
                x = torch.cat([cur_x, prev_x], 0)
                x = cva(x, self.QcR(x, R), lidar_obj_pe, self.V_R(feature, R), cam_pe, mask, img_embed, bev_embed, None)
                cur_x, prev_x = mf(x[:bs], x[bs:], ego_matrix)
                outs.append(cur_x)
                prevs.append(prev_x)
            if return_prev_query:
                return torch.stack(outs), torch.stack(prevs), ref_points
            return torch.stack(outs), ref_points
        for cva in self.cva_layers:
            x = cva(x, self.QcR(x, R), lidar_obj_pe, self.V_R(feature, R), cam_pe, mask, img_embed, bev_embed, None)
            outs.append(x)
        return torch.stack(outs), ref_points


# the transformer blocks of configs/cape/*.yml (image height, width, with_time); everything else is common to the three
TRANSFORMER_CONFIGS = {"cape_r50_1408x512": (512, 1408, False), "capet_r50_704x256": (256, 704, True),
                       "capet_vovnet_800x320": (320, 800, True)}


def cape_transformer(config, fused=True):
    """CAPETransformer with the numbers of configs/cape/<config>*.yml: 6 cameras, 6 layers, 900 queries, hidden 512, 8
    heads of 64, stride-32 features of 256 channels, 64 LID depth bins from 1 m, bound +-61.2, +-61.2, +-10."""
    height, width, with_time = TRANSFORMER_CONFIGS[config]
    att = CrossViewAttention(900, 512, True, heads=8, dim_head=64, conditional=True, fused=fused)
    return CAPETransformer(num_cameras=6, num_layers=6, feat_dim=256, feat_stride=32, image_height=height,
                           image_width=width, bound=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], with_fpe=True, depth_start=1,
                           depth_num=64, att_layer=att, tf_layer=dict(groups=30, heads=8, hidden_dim=512), scalar=10,
                           noise_scale=1.0, with_time=with_time, fused=fused)


class CAPETemporalDNHead(nn.Module):
    """cape_dn_head.py:47-592, 983-1002 at inference.  forward(mlvl_feats, intrinsics [B, nc, 4, 4] or [B, nc, 3, 3],
    extrinsics [B, nc, 4, 4] (lidar2cam: what the reference makes of img_metas as `extrinsics[i].T`), pad_shape (h, w),
    img_shape ((h, w), or [B][nc] pairs, or None), timestamp [B, 12] under with_time, all_levels=False) -> the reference's
    `outs` dict.  The camera matrices (R_inv, t, I_inv and the ego matrix of Ego_emb) are made here once per forward, with
    no read on the host; the previous frame's first camera is extrinsics[:, num_cameras], the reference's hard-coded index
    6.  Only the branches of the last decoder level run unless all_levels is set: get_bboxes reads that level alone.  The
    regression tail (the reference's sigmoid, the division by mean_time_stamp, the pc_range scaling) is torch on the
    device, nan_to_num(outs_dec) is kept.  get_bboxes decodes through bbox_coder (NMSFreeCoder: pd3_nms_free_decode when
    fused) with z moved to the box bottom.  The denoising queries, the losses and the prev-frame auxiliary outputs are
    training-only; with_prev_aux_loss is accepted and changes nothing at inference."""

    def __init__(self, num_classes, in_channels, num_query=100, num_reg_fcs=2, transformer=None, bbox_coder=None,
                 code_weights=None, position_level=0, group_reg_dims=(2, 1, 3, 2, 2), with_time=False, with_multi=False,
                 normedlinear=False, with_prev_aux_loss=False, code_size=10, fused=True, **kwargs):
        super().__init__()
        if normedlinear:
            raise NotImplementedError("CAPETemporalDNHead: normedlinear is not implemented")
        self.num_classes = self.cls_out_channels = num_classes
        self.in_channels = in_channels
        self.num_query = num_query
        self.num_reg_fcs = num_reg_fcs
        self.code_size = code_size
        self.position_level = position_level
        self.with_time = with_time
        self.with_multi = with_multi
        self.with_prev_aux_loss = with_prev_aux_loss
        self.num_pred = 6
        self.fused = _check_fused(fused)
        self.transformer = transformer
        self.embed_dims = getattr(transformer.cva_layers[0], "hidden_dim", 512)
        weights = list(code_weights) if code_weights is not None else [1.0] * 8 + [0.2, 0.2]
        self.code_weights = nn.Parameter(torch.tensor(weights[:code_size], dtype=torch.float32), requires_grad=False)
        if isinstance(bbox_coder, dict):
            cfg = {k: v for k, v in bbox_coder.items() if k not in ("type", "type_name")}
            bbox_coder = NMSFreeCoder(fused=bool(fused), **cfg)
        self.bbox_coder = bbox_coder
        self.pc_range = [float(v) for v in bbox_coder.point_cloud_range]
        e = self.embed_dims
        cls_branch = []
        for _ in range(num_reg_fcs):
            cls_branch += [nn.Linear(e, e), nn.LayerNorm(e), nn.ReLU()]
        fc_cls = nn.Sequential(*cls_branch, nn.Linear(e, num_classes))
        if with_multi:
            reg_branch = RegLayer(e, num_reg_fcs, group_reg_dims)
        else:
            reg_branch = []
            for _ in range(num_reg_fcs):
                reg_branch += [nn.Linear(e, e), nn.ReLU()]
            reg_branch = nn.Sequential(*reg_branch, nn.Linear(e, code_size))
        self.cls_branches = nn.ModuleList(copy.deepcopy(fc_cls) for _ in range(self.num_pred))
        self.reg_branches = nn.ModuleList(copy.deepcopy(reg_branch) for _ in range(self.num_pred))

    def camera_parameters(self, intrinsics, extrinsics):
        """(I_inv, R_inv, t, ego matrix or None) of forward (:453-458, Ego_emb.get_curlidar2prevlidar)."""
        R = extrinsics[:, :, :3, :3]
        R_inv = torch.linalg.inv_ex(R).inverse
        t = R_inv @ extrinsics[:, :, :3, 3:4]
        I_inv = torch.linalg.inv_ex(intrinsics[:, :, :3, :3]).inverse
        ego = None
        if self.with_time:
            ego = curlidar2prevlidar(extrinsics[0, 0], extrinsics[0, self.transformer.num_cameras])
        return I_inv, R_inv, t, ego

    def forward(self, mlvl_feats, intrinsics, extrinsics, pad_shape, img_shape=None, timestamp=None, all_levels=False):
        if self.training:
            raise NotImplementedError("CAPETemporalDNHead: inference only")
        x = mlvl_feats[self.position_level]
        B, N = int(x.shape[0]), int(x.shape[1])
        pad_shape = (int(pad_shape[0]), int(pad_shape[1]))
        masks = PETRHead._build_masks(B, N, pad_shape, img_shape, tuple(x.shape[-2:]), x.device)
        I_inv, R_inv, t, ego = self.camera_parameters(intrinsics.to(x.dtype), extrinsics.to(x.dtype))
        if self.with_time:
            time_stamp = timestamp.to(x.dtype).reshape(B, -1, 6)
            mean_time_stamp = (time_stamp[:, 1, :] - time_stamp[:, 0, :]).mean(-1)
        out = self.transformer(x, masks, I_inv, R_inv, t, pad_shape, ego_matrix=ego)
        outs_dec, reference_points = torch.nan_to_num(out[0], nan=0.0), out[-1]
        reference = inverse_sigmoid(reference_points)
        pc = self.pc_range
        levels = range(outs_dec.shape[0]) if all_levels else [outs_dec.shape[0] - 1]
        outputs_classes, outputs_coords = [], []
        for lvl in levels:
            outputs_classes.append(self.cls_branches[lvl](outs_dec[lvl]))
            tmp = self.reg_branches[lvl](outs_dec[lvl]).clone()
            tmp[..., 0:2] = torch.sigmoid(tmp[..., 0:2] + reference[..., 0:2])
            tmp[..., 4:5] = torch.sigmoid(tmp[..., 4:5] + reference[..., 2:3])
            if self.with_time:
                tmp[..., 8:] = tmp[..., 8:] / mean_time_stamp[:, None, None]
            tmp[..., 0:1] = tmp[..., 0:1] * (pc[3] - pc[0]) + pc[0]
            tmp[..., 1:2] = tmp[..., 1:2] * (pc[4] - pc[1]) + pc[1]
            tmp[..., 4:5] = tmp[..., 4:5] * (pc[5] - pc[2]) + pc[2]
            outputs_coords.append(tmp)
        return dict(all_cls_scores=torch.stack(outputs_classes), all_bbox_preds=torch.stack(outputs_coords),
                    enc_cls_scores=None, enc_bbox_preds=None, dn_mask_dict=None)

    def get_bboxes(self, preds_dicts, img_metas=None, rescale=False):
        """(boxes [B, max_num, code - 1] with z at the box bottom, scores, labels, count); NMSFreeCoder.to_list turns them
        into the reference's per-frame list."""
        preds = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in preds_dicts.items()}
        return self.bbox_coder.decode(preds, bottom_center=True)


class CAPE(nn.Module):
    """models/detection/petr/cape.py at inference: any torch.nn.Module as img_backbone and img_neck (SMOKE's convention:
    the backbone maps [B * nc, 3, H, W] to what the neck takes, the neck returns the list of feature levels; None is the
    identity), then the head and its decode.  forward(img [B, nc, 3, H, W], intrinsics, extrinsics, img_shape=None,
    timestamp=None) -> get_bboxes' tuple; the padded image is img's own size."""

    def __init__(self, pts_bbox_head, img_backbone=None, img_neck=None):
        super().__init__()
        self.img_backbone = img_backbone if img_backbone is not None else nn.Identity()
        self.img_neck = img_neck if img_neck is not None else nn.Identity()
        self.pts_bbox_head = pts_bbox_head

    def extract_feat(self, img):
        B, N = img.shape[:2]
        feats = self.img_neck(self.img_backbone(img.flatten(0, 1)))
        feats = [feats] if isinstance(feats, torch.Tensor) else list(feats)
        return [f.reshape(B, N, *f.shape[1:]) for f in feats]

    def forward(self, img, intrinsics, extrinsics, img_shape=None, timestamp=None):
        pad_shape = tuple(img.shape[-2:])
        outs = self.pts_bbox_head(self.extract_feat(img), intrinsics, extrinsics, pad_shape, img_shape, timestamp)
        return self.pts_bbox_head.get_bboxes(outs)


def _cape_model(config, img_backbone, img_neck, fused):
    with_time = TRANSFORMER_CONFIGS[config][2]
    coder = NMSFreeCoder(point_cloud_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], voxel_size=[0.2, 0.2, 8],
                         post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_num=300, num_classes=10,
                         fused=bool(fused))
    head = CAPETemporalDNHead(num_classes=10, in_channels=256, num_query=900, transformer=cape_transformer(config, fused),
                              bbox_coder=coder, code_weights=[1.0] * 10, with_time=with_time,
                              with_prev_aux_loss=with_time, fused=fused)
    return CAPE(head, img_backbone, img_neck)


def cape_r50_1408x512(img_backbone=None, img_neck=None, fused=True):
    """configs/cape/cape_r50_1408x512_24ep_wocbgs_imagenet_pretrain.yml behind the backbone and the neck; the config's
    backbone is paddle3d_amd.mm_resnet.mm_resnet50_caffe_dcn()."""
    return _cape_model("cape_r50_1408x512", img_backbone, img_neck, fused)


def capet_r50_704x256(img_backbone=None, img_neck=None, fused=True):
    """configs/cape/capet_r50_704x256_24ep_wocbgs_imagenet_pretrain.yml behind the backbone and the neck; the config's
    backbone is paddle3d_amd.mm_resnet.mm_resnet50_caffe_dcn()."""
    return _cape_model("capet_r50_704x256", img_backbone, img_neck, fused)


def capet_vovnet_800x320(img_backbone=None, img_neck=None, fused=True):
    """configs/cape/capet_vovnet_800x320_24ep_wocbgs_load_dd3d_pretrain.yml behind the backbone and the neck."""
    return _cape_model("capet_vovnet_800x320", img_backbone, img_neck, fused)
