"""BEV-LaneDet, the reference's 3D lane model, at inference: lane head and lane post-processing on the device.

Reference: paddle3d/models/detection/bev_lanedet/bev_lanedet.py:50-108 (InstanceEmbeddingOffsetYZ), :143-180
(LaneHeadResidualInstanceWithOffsetZ), :234-299 (FCTransform_, Residual), :302-430 (BEVLaneDet), paddle3d/datasets/
apollo/cluster.py:44-140, post_process.py:26-75, apollo_lane_metric.py:334-336, :355-383; configs/bev_lanedet/
bev_lanedet_apollo_576x1024.yml.  Constructor arguments and state-dict keys are the reference's (bb.*, down.*,
s32transformer.*, s64transformer.*, lane_head.bev_up_new.*, lane_head.head.{neck_new,ms_new,me_new,m_offset_new,m_z}.*,
lane_head_2d.*; BatchNorm's _mean / _variance and the [in, out] Linear weights as checkpoint.py maps them).  The
backbone (ResNet34) is any torch.nn.Module handed in.  lane_head_2d is a training-time auxiliary: it is built with
train=True so that checkpoints load, and never run.

    BEVLaneDet.raw_maps(images)               the [B, 5, H, W] tensor the reference saves per frame (seg LOGIT, emb,
                                              sigmoid(offset), z), on the images' device
    BEVLaneDet.lanes_padded(images, fused)    ops.lanedet.LanePack on the device, no host synchronisation.  fused: True
                                              (LAZY_BY_DEFAULT decides), "lazy" (branch maps + the lazy entry point),
                                              "dense" (the four maps + the from-maps entry point) or False (the plain
                                              torch / NumPy transcription below, which does go through the host)
    BEVLaneDet.test_forward(samples) / forward   per frame the list of [40, 3] lanes the reference's metric consumes, in
                                              its order: exactly one host synchronisation; lanes the device did not fit
                                              (2 or 3 rows) are finished with np.polyfit from the device's points;
                                              frames with a flag set are redone by the transcription (a second transfer,
                                              only then)

On the device path the 3x3 convolution + BatchNorm (+ ReLU) layers behind the backbone run on the F(4x4, 3x3) Winograd
kernel with the norm folded in where conv_kernel asks for it and ops.conv.winograd43_supported holds ("auto":
WINOGRAD_BY_DEFAULT, see DESIGN.md's BEV-LaneDet section), else on torch's convolution; the four branches' first
convolutions share their input and run as one stacked 64 -> 512 launch; the dense final convolutions run on
grouped_conv3x3_small with group_couts (1, nd, 1, 1) where its predicate holds.  Upsampling is torch's `nearest`.
CPU tensors and shapes the kernels refuse (ops.lanedet.lanedet_supported) take the transcription.
"""
from __future__ import annotations

import warnings

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .derived import derived
from .ops import conv as conv_ops
from .ops import lanedet as lane_ops

__all__ = ["Residual", "FCTransform_", "InstanceEmbeddingOffsetYZ", "InstanceEmbedding",
           "LaneHeadResidualInstanceWithOffsetZ", "LaneHeadResidualInstance", "BEVLaneDet", "lanes_numpy",
           "bev_lanedet_apollo_576x1024", "LAZY_BY_DEFAULT", "WINOGRAD_BY_DEFAULT"]

# fused=True takes the dense path: measured, the lazy one is not faster (DESIGN.md's BEV-LaneDet section has the numbers)
LAZY_BY_DEFAULT = False
# conv_kernel="auto": whether the 3x3 + BatchNorm layers take the Winograd kernel (DESIGN.md has the error figures)
WINOGRAD_BY_DEFAULT = False
BRANCHES = ("ms_new", "me_new", "m_offset_new", "m_z")  # seg, emb, offset, z


def _conv_bn(cin, cout, relu=True, bias=False):
    layers = [nn.Conv2d(cin, cout, 3, 1, 1, bias=bias), nn.BatchNorm2d(cout)]
    return layers + [nn.ReLU()] if relu else layers


# ---- 3x3 convolution + BatchNorm (+ ReLU) on the Winograd kernel -------------------------------------------------------
def _is_conv3x3(m):
    return (isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.stride == (1, 1) and m.padding == (1, 1) and
            m.dilation == (1, 1) and m.groups == 1)


def _folded(convs, bns):
    """Weights and biases of conv + BatchNorm pairs (stacked along the output channels) with the norm folded in."""
    ws, bs = [], []
    for conv, bn in zip(convs, bns):
        scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        shift = bn.bias.double() - bn.running_mean.double() * scale
        if conv.bias is not None:
            shift = shift + conv.bias.double() * scale
        ws.append((conv.weight.double() * scale[:, None, None, None]).float())
        bs.append(shift.float())
    return torch.cat(ws), torch.cat(bs).contiguous()


def _winograd_ok(x, cin, cout):
    return x.is_cuda and x.dtype == torch.float32 and conv_ops.winograd43_supported(cin, cout, x.shape[2], x.shape[3])


def _winograd_conv_bn(owner, slot, convs, bns, x, relu):
    """relu?(bn(conv(x))) of one or several pairs that share the input x, as one launch; [B, sum(cout), H, W] (a view of
    a map whose rows are pitch4(W) long)."""
    def build():
        w, b = _folded(convs, bns)
        return conv_ops.pack_winograd43_weight(w), b
    packed = derived(owner, slot, build, sources=(*convs, *bns))
    w = x.shape[3]
    pitch = conv_ops.pitch4(w)
    xp = x.contiguous() if pitch == w else F.pad(x, (0, pitch - w))
    cout = sum(c.out_channels for c in convs)
    return conv_ops.conv3x3_winograd43_bias_relu(xp, packed[0], packed[1], cout, relu=relu, w_valid=w)[:, :, :, :w]


def _run(seq, x, winograd):
    """A Sequential in inference: conv3x3 + BatchNorm (+ ReLU) triples on the Winograd kernel where asked for and
    supported, every other layer as torch runs it."""
    mods = list(seq)
    i = 0
    while i < len(mods):
        m = mods[i]
        if (winograd and _is_conv3x3(m) and i + 1 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm2d) and
                _winograd_ok(x, m.in_channels, m.out_channels)):
            relu = i + 2 < len(mods) and isinstance(mods[i + 2], nn.ReLU)
            x = _winograd_conv_bn(m, "winograd43", (m,), (mods[i + 1],), x, relu)
            i += 3 if relu else 2
            continue
        x = m(x)
        i += 1
    return x


class Residual(nn.Module):
    """bev_lanedet.py:282-299."""

    def __init__(self, module, downsample=None):
        super().__init__()
        self.module, self.downsample, self.relu = module, downsample, nn.ReLU()

    def forward(self, x, winograd=False):
        out = _run(self.module, x, winograd) if isinstance(self.module, nn.Sequential) else self.module(x)
        identity = x if self.downsample is None else self.downsample(x)
        return self.relu(out + identity)


class FCTransform_(nn.Module):
    """bev_lanedet.py:234-279: two Linear + ReLU over the flattened spatial axis, a 1x1 convolution + BatchNorm + ReLU,
    a residual 3x3 convolution + BatchNorm."""

    def __init__(self, image_featmap_size, space_featmap_size):
        super().__init__()
        ic, ih, iw = image_featmap_size
        sc, sh, sw = space_featmap_size
        self.image_featmap_size, self.space_featmap_size = tuple(image_featmap_size), tuple(space_featmap_size)
        self.fc_transform = nn.Sequential(nn.Linear(ih * iw, sh * sw), nn.ReLU(), nn.Linear(sh * sw, sh * sw), nn.ReLU())
        self.conv1 = nn.Sequential(nn.Conv2d(ic, sc, 1, 1, bias=False), nn.BatchNorm2d(sc), nn.ReLU())
        self.residual = Residual(nn.Sequential(nn.Conv2d(sc, sc, 3, 1, 1, bias=False), nn.BatchNorm2d(sc)))

    def forward(self, x, winograd=False):
        b, c = x.shape[:2]
        bev = self.fc_transform(x.reshape(b, c, -1))
        bev = bev.reshape(b, c, self.space_featmap_size[1], self.space_featmap_size[2])
        return self.residual(self.conv1(bev), winograd)


class InstanceEmbeddingOffsetYZ(nn.Module):
    """bev_lanedet.py:50-108: a neck and four branches (seg, emb, offset, z), each 64 -> 128 -> 64 and a final 3x3
    convolution with bias."""

    def __init__(self, ci, co=1):
        super().__init__()
        self.ci, self.co = int(ci), int(co)
        self.neck_new = nn.Sequential(*_conv_bn(ci, 128), *_conv_bn(128, ci))

        def branch(out):
            return nn.Sequential(*_conv_bn(ci, 128), *_conv_bn(128, 64), nn.Conv2d(64, out, 3, 1, 1, bias=True))

        self.ms_new, self.m_offset_new, self.m_z, self.me_new = branch(1), branch(1), branch(1), branch(co)

    def branches(self):
        return [getattr(self, k) for k in BRANCHES]

    def forward(self, x):
        feat = self.neck_new(x)
        return self.ms_new(feat), self.me_new(feat), self.m_offset_new(feat), self.m_z(feat)

    def branch_maps(self, x, winograd=False):
        """The four branches' 64-channel maps after their second convolution, BatchNorm and ReLU (seg, emb, offset,
        z): what the lazy entry point starts from.  The four first convolutions share their input and run stacked."""
        feat = _run(self.neck_new, x, winograd)
        brs = self.branches()
        if winograd and _winograd_ok(feat, self.ci, 4 * 128):
            first = _winograd_conv_bn(self, "first_winograd43", [b[0] for b in brs], [b[1] for b in brs], feat, True)
        else:
            w, bias = derived(self, "first", lambda: _folded([b[0] for b in brs], [b[1] for b in brs]),
                              sources=[b[:2] for b in brs])
            first = F.relu(F.conv2d(feat, w.to(feat.dtype), bias.to(feat.dtype), padding=1))
        return [_run(b[3:6], first[:, 128 * i:128 * (i + 1)], winograd) for i, b in enumerate(brs)]

    def final_maps(self, maps):
        """The four final convolutions densely from branch_maps: seg, emb, offset (logit), z."""
        brs = self.branches()
        x0 = maps[0]
        h, w = x0.shape[2:]
        if (x0.is_cuda and x0.dtype == torch.float32 and self.co <= 4 and
                conv_ops.grouped_small_supported(64, max(self.co, 1), h, w)):
            co = max(self.co, 1)
            counts = (1, self.co, 1, 1)

            def build():
                wt = torch.zeros((4, co, 64, 3, 3), dtype=torch.float32, device=x0.device)
                bs = torch.zeros((4, co), dtype=torch.float32, device=x0.device)
                for g, b in enumerate(brs):
                    wt[g, :counts[g]], bs[g, :counts[g]] = b[6].weight.float(), b[6].bias.float()
                return conv_ops.pack_grouped_weight(wt.reshape(4 * co, 64, 3, 3), 4), bs.reshape(-1).contiguous()
            packed = derived(self, "final_grouped", build, sources=[b[6] for b in brs])
            out = conv_ops.grouped_conv3x3_small(torch.cat(maps, 1), packed[0], packed[1], 4,
                                                 group_couts=counts)
            return tuple(out[:, g * co:g * co + counts[g]] for g in range(4))
        return tuple(b[6](m) for b, m in zip(brs, maps))


class InstanceEmbedding(nn.Module):
    """bev_lanedet.py:111-140 (the 2D auxiliary head's embedding; built for its keys only)."""

    def __init__(self, ci, co=1):
        super().__init__()
        self.neck = nn.Sequential(*_conv_bn(ci, 128), *_conv_bn(128, ci))
        self.ms = nn.Sequential(*_conv_bn(ci, 128), *_conv_bn(128, 64), nn.Conv2d(64, 1, 3, 1, 1, bias=True))
        self.me = nn.Sequential(*_conv_bn(ci, 128), *_conv_bn(128, 64), nn.Conv2d(64, co, 3, 1, 1, bias=True))

    def forward(self, x):
        feat = self.neck(x)
        return self.ms(feat), self.me(feat)


def _up_block(cin, mid, cout, downsample_bias=True, downsample=True):
    return Residual(nn.Sequential(nn.Conv2d(cin, mid, 3, padding=1, bias=False), nn.BatchNorm2d(mid), nn.ReLU(),
                                  nn.Dropout2d(p=0.2), nn.Conv2d(mid, cout, 3, padding=1, bias=False),
                                  nn.BatchNorm2d(cout)),
                    downsample=nn.Conv2d(cin, cout, 1) if downsample else None)


class LaneHeadResidualInstanceWithOffsetZ(nn.Module):
    """bev_lanedet.py:143-180."""

    def __init__(self, output_size, input_channel=256):
        super().__init__()
        self.output_size = tuple(int(s) for s in output_size)
        self.bev_up_new = nn.Sequential(nn.Upsample(scale_factor=2), _up_block(input_channel, 64, 128),
                                        nn.Upsample(size=self.output_size), _up_block(128, 64, 64))
        self.head = InstanceEmbeddingOffsetYZ(64, 2)

    def bev_feat(self, bev_x, winograd=False):
        x = bev_x
        for m in self.bev_up_new:
            x = m(x, winograd) if isinstance(m, Residual) else m(x)
        return x

    def forward(self, bev_x):
        return self.head(self.bev_up_new(bev_x))


class LaneHeadResidualInstance(nn.Module):
    """bev_lanedet.py:183-231 (training-time auxiliary on the image features; built for its keys only)."""

    def __init__(self, output_size, input_channel=256):
        super().__init__()
        self.bev_up = nn.Sequential(nn.Upsample(scale_factor=2), _up_block(input_channel, 64, 128),
                                    nn.Upsample(scale_factor=2), _up_block(128, 64, 32),
                                    nn.Upsample(size=tuple(int(s) for s in output_size)),
                                    _up_block(32, 16, 32, downsample=False))
        self.head = InstanceEmbedding(32, 2)

    def forward(self, bev_x):
        return self.head(self.bev_up(bev_x))


# ---- the plain transcription of the post-processing ------------------------------------------------------------------
def _cluster_numpy(seg, emb, conf, gap):
    """cluster.py:44-109: the selected pixels in row-major order and their centre ids; centres as (mean, count)."""
    ys, xs = np.nonzero(seg >= conf)
    centres, ids = [], []
    for y, x in zip(ys, xs):
        e = emb[:, y, x]
        best, bid = gap + 1, -1
        for i, (c, _) in enumerate(centres):
            d = float(np.sqrt(np.sum((e - c) ** 2))) if len(e) > 1 else float(abs(e[0] - c[0]))
            if d < best:
                best, bid = d, i
        if best < gap:
            c, n = centres[bid]
            centres[bid] = ((c * n + e) / (n + 1), n + 1)
            ids.append(bid)
        else:
            centres.append((e, 1))
            ids.append(len(centres) - 1)
    return ys, xs, np.asarray(ids, np.int64), centres


def lanes_numpy(maps, conf=0.9, emb_margin=6.0, min_cluster_size=15, max_x=103.0, meter_per_pixel=(0.5, 0.5),
                counts=False):
    """The reference's post-processing of one frame's [5 (1 + nd + 2), H, W] maps, transcribed: (canvas uint8 [H, W],
    [(canvas id, points [rows, 3] (x_m, y_m, z), fit [40, 3])]) with np.polyfit for every lane of at least 2 rows.
    counts=True appends (centres, canvas ids): what the kernels' two caps are counted in."""
    maps = np.asarray(maps)
    seg, emb, off, z = maps[0], maps[1:-2], maps[-2], maps[-1]
    h, w = seg.shape
    with np.errstate(all="ignore"):
        ys, xs, ids, centres = _cluster_numpy(seg, emb, conf, emb_margin)
    canvas = np.zeros((h, w), np.uint8)
    for y, x, i in zip(ys, xs, ids):
        if centres[i][1] >= min_cluster_size:
            canvas[y, x] = i + 1
    mx, my = (meter_per_pixel if isinstance(meter_per_pixel, (tuple, list)) else (meter_per_pixel, meter_per_pixel))
    lanes = []
    for cid in np.unique(canvas[canvas > 0]):
        cols, rows, zs = [], [], []
        for y in range(h):
            xo = np.where(canvas[y] == cid)[0]
            if xo.size:
                zs.append(np.mean(z[y][xo]))
                cols.append(np.mean(xo + off[y][xo]))
                rows.append(y + 0.5)
        if len(rows) < 2:
            continue
        xm = (max_x / mx - np.array(rows)[::-1]) * mx
        ym = -(np.array(cols)[::-1] * my - (w / 2) * my)
        zz = np.array(zs)[::-1]
        yy = np.linspace(xm.min(), xm.max(), lane_ops.FIT_SAMPLES)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # polyfit's RankWarning for lanes of 2 or 3 rows, as in the reference
            fx, fz = np.polyfit(xm, -ym, 3), np.polyfit(xm, zz, 3)
        lanes.append((int(cid), np.stack([xm, ym, zz], 1), np.stack([np.poly1d(fx)(yy), yy, np.poly1d(fz)(yy)], 1)))
    if counts:
        return canvas, lanes, (len(centres), int(np.unique(canvas[canvas > 0]).size))
    return canvas, lanes


class BEVLaneDet(nn.Module):
    """bev_lanedet.py:302-430 at inference.  s32 / s64 / bev: the (channels, height, width) of the backbone's output,
    of `down`'s output and of the two transformed maps (the reference hard-codes the defaults)."""

    def __init__(self, backbone, bev_shape, output_2d_shape=None, train=True, fused=True, conv_kernel="auto",
                 s32=(512, 18, 32), s64=(1024, 9, 16), bev=(256, 25, 5), x_range=(3, 103), meter_per_pixel=0.5,
                 post_conf=0.9, post_emb_margin=6.0, post_min_cluster_size=15):
        super().__init__()
        self.bb = backbone
        c32, c64 = s32[0], s64[0]
        self.down = Residual(nn.Sequential(nn.Conv2d(c32, c64, 3, 2, 1), nn.BatchNorm2d(c64), nn.ReLU(),
                                           nn.Conv2d(c64, c64, 3, 1, 1), nn.BatchNorm2d(c64)),
                             downsample=nn.Conv2d(c32, c64, 3, 2, 1))
        self.s32transformer = FCTransform_(s32, bev)
        self.s64transformer = FCTransform_(s64, bev)
        self.lane_head = LaneHeadResidualInstanceWithOffsetZ(bev_shape, input_channel=2 * bev[0])
        self.is_train = bool(train)
        if self.is_train:
            if output_2d_shape is None:
                raise ValueError("BEVLaneDet: train=True builds lane_head_2d (for its checkpoint keys) and needs "
                                 "output_2d_shape; pass it, or train=False")
            self.lane_head_2d = LaneHeadResidualInstance(output_2d_shape, input_channel=c32)
        self.fused, self.conv_kernel = fused, conv_kernel
        self.bev_shape = tuple(int(s) for s in bev_shape)
        self.post = dict(conf=float(post_conf), emb_margin=float(post_emb_margin),
                         min_cluster_size=int(post_min_cluster_size), max_x=float(x_range[1]),
                         meter_per_pixel=(float(meter_per_pixel), float(meter_per_pixel)))

    # ---- the network ---------------------------------------------------------------------------------------------------
    def _winograd(self, fused):
        return bool(fused) and (self.conv_kernel == "winograd43" or (self.conv_kernel == "auto" and WINOGRAD_BY_DEFAULT))

    def bev_feat(self, images, fused=False):
        """The lane head's 64-channel BEV map [B, 64, *bev_shape]."""
        wino = self._winograd(fused)
        s32 = self.bb(images) if self.bb is not None else images
        s64 = self.down(s32, wino)
        bev = torch.cat([self.s64transformer(s64, wino), self.s32transformer(s32, wino)], 1)
        return self.lane_head.bev_feat(bev, wino)

    def raw_maps(self, images, fused=None):
        """[B, 5, H, W]: seg (logit), emb, sigmoid(offset), z -- what test_forward saves per frame."""
        fused = self.fused if fused is None else fused
        head = self.lane_head.head
        feat = self.bev_feat(images, fused)
        if fused and feat.is_cuda:
            seg, emb, off, z = head.final_maps(head.branch_maps(feat, self._winograd(fused)))
        else:
            seg, emb, off, z = head(feat)
        return torch.cat([seg, emb, torch.sigmoid(off), z], 1)

    # ---- lanes -----------------------------------------------------------------------------------------------------------
    def lanes_padded_torch(self, maps):
        """ops.lanedet.LanePack on the maps' device from the transcription (through the host), with the kernels'
        definitions, so that it stands in for their outputs: flag bit 0 for more than MAX_CENTRES centres, bit 1 for
        more than MAX_LANES canvas ids (counted before lanes of fewer than 2 rows are dropped), a flagged frame all
        zero, fit_ok and fit only for lanes of at least 4 rows (test_forward finishes the others from `points`)."""
        host = maps.detach().float().cpu().numpy()
        b, _, h, w = host.shape
        L, K = lane_ops.MAX_LANES, lane_ops.FIT_SAMPLES
        labels = np.zeros((b, h, w), np.uint8)
        ints = {k: np.zeros((b, L), np.int32) for k in ("lane_id", "lane_rows", "fit_ok")}
        num, flags, nsel = (np.zeros(b, np.int32) for _ in range(3))
        points, fit = np.zeros((b, L, h, 3), np.float32), np.zeros((b, L, K, 3), np.float32)
        for i in range(b):
            nsel[i] = int((host[i, 0] >= np.float32(self.post["conf"])).sum())
            canvas, lanes, (centres, ids) = lanes_numpy(host[i], counts=True, **self.post)
            flags[i] = 1 if centres > lane_ops.MAX_CENTRES else (2 if ids > L else 0)
            if flags[i]:
                continue
            labels[i], num[i] = canvas, len(lanes)
            for l, (cid, pts, f) in enumerate(lanes):
                ints["lane_id"][i, l], ints["lane_rows"][i, l], points[i, l, :len(pts)] = cid, len(pts), pts
                if len(pts) >= 4:
                    ints["fit_ok"][i, l], fit[i, l] = 1, f
        t = lambda a: torch.from_numpy(a).to(maps.device)  # noqa: E731
        return lane_ops.LanePack(t(labels), t(num), t(ints["lane_id"]), t(ints["lane_rows"]), t(ints["fit_ok"]),
                                 t(points), t(fit), t(flags), t(nsel))

    def lanes_padded(self, images, fused=None):
        fused = self.fused if fused is None else fused
        lazy = fused == "lazy" or (fused is True and LAZY_BY_DEFAULT)
        head = self.lane_head.head
        h, w = self.bev_shape
        on_device = bool(fused) and images.is_cuda and images.dtype == torch.float32
        if on_device and lane_ops.lanedet_supported(h, w, head.co, 64, batch=images.shape[0]):
            feat = self.bev_feat(images, fused)
            maps = head.branch_maps(feat, self._winograd(fused))
            brs = head.branches()
            if lazy:
                wb = [t for b in brs for t in (b[6].weight, b[6].bias)]
                out = lane_ops.lanedet_head_forward(*maps, *wb, **self.post)
            else:
                seg, emb, off, z = head.final_maps(maps)
                out = lane_ops.lanedet_post_process(seg, emb, off, z, offset_is_logit=True, **self.post)
            if out is not None:
                return out
        return self.lanes_padded_torch(self.raw_maps(images, fused=False))

    def test_forward(self, samples, fused=None):
        """Per frame the list of [40, 3] float64 lanes (X, Y, Z) in increasing canvas id."""
        images = samples["img"]
        fused = self.fused if fused is None else fused
        pack = self.lanes_padded(images, fused)
        b, L, h = pack.points.shape[:3]
        K = lane_ops.FIT_SAMPLES
        small = torch.stack([pack.num_lanes, pack.flags], 1).float()
        blob = torch.cat([small, pack.lane_rows.float(), pack.fit_ok.float(), pack.points.reshape(b, -1),
                          pack.fit.reshape(b, -1)], 1).cpu().numpy()  # the one host synchronisation
        results, redo = [], []
        for i in range(b):
            row = blob[i]
            num, flag = int(row[0]), int(row[1])
            rows, ok = row[2:2 + L].astype(np.int64), row[2 + L:2 + 2 * L]
            points = row[2 + 2 * L:2 + 2 * L + L * h * 3].reshape(L, h, 3)
            fit = row[2 + 2 * L + L * h * 3:].reshape(L, K, 3)
            if flag:
                redo.append(i)
                results.append(None)
                continue
            lanes = []
            for l in range(num):
                if ok[l]:
                    lanes.append(fit[l].astype(np.float64))
                    continue
                p = points[l, :rows[l]].astype(np.float64)
                yy = np.linspace(p[:, 0].min(), p[:, 0].max(), K)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    fx, fz = np.polyfit(p[:, 0], -p[:, 1], 3), np.polyfit(p[:, 0], p[:, 2], 3)
                lanes.append(np.stack([np.poly1d(fx)(yy), yy, np.poly1d(fz)(yy)], 1))
            results.append(lanes)
        if redo:  # more centres or canvas ids than the kernels hold: the transcription, from the maps
            maps = self.raw_maps(images[redo], fused=False).float().cpu().numpy()
            for j, i in enumerate(redo):
                results[i] = [f for _, _, f in lanes_numpy(maps[j], **self.post)[1]]
        return results

    def forward(self, samples, fused=None):
        with torch.no_grad():
            return self.test_forward(samples, fused)


def bev_lanedet_apollo_576x1024(backbone, fused=True):
    """configs/bev_lanedet/bev_lanedet_apollo_576x1024.yml: BEV 200 x 48 at 0.5 m per pixel, x_range (3, 103)."""
    return BEVLaneDet(backbone, bev_shape=(200, 48), output_2d_shape=(144, 256), train=True, fused=fused,
                      x_range=(3, 103), meter_per_pixel=0.5)
