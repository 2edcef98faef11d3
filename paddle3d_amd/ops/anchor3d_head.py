"""BEVFusion's Anchor3DHead at inference on the device (csrc/anchor3d_head.hip, C ABI pd3_anchor3d_head_forward /
pd3_anchor3d_get_bboxes); the arithmetic order is stated in that file's header and restated in
tests/golden/anchor3d_numpy.py.

Reference: paddle3d/models/heads/dense_heads/anchor3d_head.py:146-161, :378-520 (forward_single, get_bboxes,
get_bboxes_single), models/detection/bevfusion/utils.py:92-103, :189-276 (limit_period, box3d_multiclass_nms),
utils/box_coder.py:270-310 (DeltaXYZWLHRBBoxCoder.decode), models/heads/dense_heads/target_assigner/
anchor3d_generator.py:202-304 (AlignedAnchor3DRangeGenerator).

anchor3d_head_forward(feat, cls_weight_packed, cls_bias, reg_weight, reg_bias, dir_weight, dir_bias, anchors, ...)
    the LAZY head: only conv_cls runs densely and only the per-anchor maximum score is written; conv_reg, conv_dir_cls
    and the class scores are evaluated at the <= nms_pre selected anchors.
anchor3d_get_bboxes(cls_score, bbox_pred, dir_cls_pred, anchors, ...)
    the same sequence from existing maps.
Both return (boxes [B, max_num, code_size], scores [B, max_num], labels int32 [B, max_num], counts int32 [B]) on the
device, rows past counts[b] zero, or None when the kernels do not take the shape (`anchor3d_supported`).  float32 only.
Nothing here synchronises with the host; the kernels run on the current stream.
"""
from __future__ import annotations

import ctypes as C

import torch

from ._common import check, gpu_tensor, lib, ptr, stream_ptr, workspace

__all__ = ["anchor3d_supported", "pack_cls_weight", "unpack_cls_weight", "anchor3d_head_forward",
           "anchor3d_get_bboxes", "aligned_anchor3d_grid", "CHUNK_ROWS", "MAX_K"]

_OP = "anchor3d_head"
_UNSUPPORTED = -3
CHUNK_ROWS = 192  # class rows of one chunk of anchors in the dense kernel (kChunkRows)
MAX_K = 1024


def anchor3d_supported(channels, num_classes, num_anchors, code_size, nms_pre, max_num, total_anchors,
                       use_sigmoid_cls=True, use_direction_classifier=True):
    """The kernels' shape predicate.  channels=None: the from-maps form, which has no channel condition.
    total_anchors = H * W * num_anchors; nms_pre <= 0 means no pre-selection."""
    if not (use_sigmoid_cls and use_direction_classifier):
        return False
    if channels is not None and not (channels % 16 == 0 and 16 <= channels <= 512):
        return False
    k = min(nms_pre, total_anchors) if nms_pre > 0 else total_anchors
    return (1 <= num_classes <= 16 and 1 <= num_anchors <= 32 and 7 <= code_size <= 16 and 1 <= k <= MAX_K and
            1 <= max_num <= MAX_K and total_anchors < 2 ** 30)


def _chunks(num_anchors, num_classes):
    """[(first anchor, anchors, first tile)] of the dense kernel's chunks, and the number of tiles."""
    apc = CHUNK_ROWS // num_classes
    full = (apc * num_classes + 15) // 16
    out, t0 = [], 0
    for a0 in range(0, num_anchors, apc):
        na = min(apc, num_anchors - a0)
        out.append((a0, na, t0))
        t0 += full if a0 + apc < num_anchors else (na * num_classes + 15) // 16
    return out, t0


def pack_cls_weight(weight, num_classes):
    """conv_cls's weight [A * nc, C] (or [A * nc, C, 1, 1]) -> [tiles, C / 4, 64] in the MFMA lane order of
    a3d_dense_max_kernel: anchors in chunks of 192 // nc, a chunk's rows zero-padded to whole tiles of 16, lane
    (m = lane & 15, k = lane >> 4) of [tile][s] holding w[row 16 tile + m][channel 4 s + k]."""
    w = weight.reshape(weight.shape[0], -1)
    rows, c = w.shape
    if rows % num_classes or c % 4:
        raise ValueError(f"{_OP}: weight {tuple(weight.shape)} does not hold whole anchors of {num_classes} classes")
    chunks, tiles = _chunks(rows // num_classes, num_classes)
    padded = w.new_zeros((tiles * 16, c))
    for a0, na, t0 in chunks:
        padded[t0 * 16:t0 * 16 + na * num_classes] = w[a0 * num_classes:(a0 + na) * num_classes]
    # [tile, m, s, k] -> [tile, s, k, m]
    return padded.reshape(tiles, 16, c // 4, 4).permute(0, 2, 3, 1).reshape(tiles, c // 4, 64).contiguous()


def unpack_cls_weight(packed, num_anchors, num_classes):
    """The inverse of pack_cls_weight: [A * nc, C]."""
    tiles, s, _ = packed.shape
    padded = packed.reshape(tiles, s, 4, 16).permute(0, 3, 1, 2).reshape(tiles * 16, s * 4)
    chunks, want = _chunks(num_anchors, num_classes)
    if want != tiles:
        raise ValueError(f"{_OP}: {tiles} tiles do not hold {num_anchors} anchors of {num_classes} classes")
    return torch.cat([padded[t0 * 16:t0 * 16 + na * num_classes] for _, na, t0 in chunks]).contiguous()


def aligned_anchor3d_grid(ranges, sizes, rotations, custom_values, featmap_size, scale=1):
    """AlignedAnchor3DRangeGenerator.grid_anchors for one level with reshape_out (align_corner=False, size_per_range):
    float32 [H * W * n_sizes * n_rot, 7 + len(custom_values)], row ((y * W + x) * n_sizes + s) * n_rot + r, columns
    (x, y, z, size, rotation) and zeros in the custom columns (the reference never writes the custom values)."""
    sizes = torch.tensor(sizes, dtype=torch.float32).reshape(-1, 3) * scale
    ranges = [list(r) for r in ranges]
    if len(ranges) != len(sizes):
        if len(ranges) != 1:
            raise ValueError(f"{_OP}: {len(ranges)} ranges for {len(sizes)} sizes")
        ranges = ranges * len(sizes)
    h, w = (int(v) for v in featmap_size[-2:])
    rot = torch.tensor(rotations, dtype=torch.float32)
    out = torch.zeros((h, w, len(sizes), len(rot), 7 + len(custom_values)), dtype=torch.float32)

    def centers(lo, hi, n):
        c = torch.linspace(float(lo), float(hi), n + 1, dtype=torch.float32)
        return (c + (c[1] - c[0]) / 2)[:n]

    for s, (rng, size) in enumerate(zip(ranges, sizes)):
        rng = torch.tensor(rng, dtype=torch.float32)
        out[:, :, s, :, 0] = centers(rng[0], rng[3], w).reshape(1, w, 1)
        out[:, :, s, :, 1] = centers(rng[1], rng[4], h).reshape(h, 1, 1)
        out[:, :, s, :, 2] = centers(rng[2], rng[5], 1)[0]
        out[:, :, s, :, 3:6] = size
        out[:, :, s, :, 6] = rot
    return out.reshape(-1, out.shape[-1])


def _outputs(b, max_num, cs, dev):
    return (torch.empty((b, max_num, cs), dtype=torch.float32, device=dev),
            torch.empty((b, max_num), dtype=torch.float32, device=dev),
            torch.empty((b, max_num), dtype=torch.int32, device=dev),
            torch.empty((b,), dtype=torch.int32, device=dev))


def _cfg(nms_pre, max_num, score_thr, nms_thr, dir_offset, dir_limit_offset):
    return (int(nms_pre), int(max_num), C.c_float(score_thr), C.c_float(nms_thr), C.c_float(dir_offset),
            C.c_float(dir_limit_offset))


def anchor3d_head_forward(feat, cls_weight_packed, cls_bias, reg_weight, reg_bias, dir_weight, dir_bias, anchors,
                          num_classes, nms_pre, max_num, score_thr, nms_thr, dir_offset=0.0, dir_limit_offset=1.0):
    """feat [B, C, H, W]; cls_weight_packed from pack_cls_weight; reg_weight [A * code_size, C(, 1, 1)], dir_weight
    [A * 2, C(, 1, 1)] and the biases as the convolutions hold them; anchors [H * W * A, code_size]."""
    feat = gpu_tensor(_OP, "feat", feat)
    dev = feat.device
    if feat.dim() != 4:
        raise RuntimeError(f"{_OP}: feat must be [B, C, H, W], got {tuple(feat.shape)}")
    b, c, h, w = (int(s) for s in feat.shape)
    nc = int(num_classes)
    anchors = gpu_tensor(_OP, "anchors", anchors, dev=dev)
    if anchors.dim() != 2 or h * w == 0 or anchors.shape[0] % (h * w):
        raise RuntimeError(f"{_OP}: anchors {tuple(anchors.shape)} do not fit a {h} x {w} map")
    a, cs = int(anchors.shape[0]) // (h * w), int(anchors.shape[1])
    if not anchor3d_supported(c, nc, a, cs, int(nms_pre), int(max_num), h * w * a):
        return None
    _, tiles = _chunks(a, nc)
    wp = gpu_tensor(_OP, "cls_weight_packed", cls_weight_packed, dev=dev, shape=(tiles, c // 4, 64))
    cb = gpu_tensor(_OP, "cls_bias", cls_bias, dev=dev, shape=(a * nc,))
    rw = gpu_tensor(_OP, "reg_weight", reg_weight.reshape(reg_weight.shape[0], -1), dev=dev, shape=(a * cs, c))
    rb = gpu_tensor(_OP, "reg_bias", reg_bias, dev=dev, shape=(a * cs,))
    dw = gpu_tensor(_OP, "dir_weight", dir_weight.reshape(dir_weight.shape[0], -1), dev=dev, shape=(a * 2, c))
    db = gpu_tensor(_OP, "dir_bias", dir_bias, dev=dev, shape=(a * 2,))
    L = lib()
    outs = _outputs(b, int(max_num), cs, dev)
    ws = workspace(L.pd3_anchor3d_head_workspace(b, h, w, a, nc, cs, int(nms_pre)), dev)
    st = L.pd3_anchor3d_head_forward(ptr(feat), ptr(wp), ptr(cb), ptr(rw), ptr(rb), ptr(dw), ptr(db), ptr(anchors), b, c,
                                     h, w, a, nc, cs, *_cfg(nms_pre, max_num, score_thr, nms_thr, dir_offset,
                                                            dir_limit_offset),
                                     *(ptr(o) for o in outs), ptr(ws), ws.numel(), stream_ptr(dev))
    if st == _UNSUPPORTED:
        return None
    check(st, f"{_OP}.anchor3d_head_forward")
    return outs


def anchor3d_get_bboxes(cls_score, bbox_pred, dir_cls_pred, anchors, num_classes, nms_pre, max_num, score_thr, nms_thr,
                        dir_offset=0.0, dir_limit_offset=1.0):
    """cls_score [B, A * nc, H, W], bbox_pred [B, A * code_size, H, W], dir_cls_pred [B, A * 2, H, W] (the head's
    three maps), anchors [H * W * A, code_size]."""
    cls_score = gpu_tensor(_OP, "cls_score", cls_score)
    dev = cls_score.device
    nc = int(num_classes)
    if cls_score.dim() != 4 or cls_score.shape[1] % nc:
        raise RuntimeError(f"{_OP}: cls_score must be [B, A * {nc}, H, W], got {tuple(cls_score.shape)}")
    b, ch, h, w = (int(s) for s in cls_score.shape)
    a = ch // nc
    anchors = gpu_tensor(_OP, "anchors", anchors, dev=dev)
    if anchors.dim() != 2 or anchors.shape[0] != h * w * a:
        raise RuntimeError(f"{_OP}: anchors must be [{h * w * a}, code_size], got {tuple(anchors.shape)}")
    cs = int(anchors.shape[1])
    bbox_pred = gpu_tensor(_OP, "bbox_pred", bbox_pred, dev=dev, shape=(b, a * cs, h, w))
    dir_cls_pred = gpu_tensor(_OP, "dir_cls_pred", dir_cls_pred, dev=dev, shape=(b, a * 2, h, w))
    if not anchor3d_supported(None, nc, a, cs, int(nms_pre), int(max_num), h * w * a):
        return None
    L = lib()
    outs = _outputs(b, int(max_num), cs, dev)
    ws = workspace(L.pd3_anchor3d_head_workspace(b, h, w, a, nc, cs, int(nms_pre)), dev)
    st = L.pd3_anchor3d_get_bboxes(ptr(cls_score), ptr(bbox_pred), ptr(dir_cls_pred), ptr(anchors), b, h, w, a, nc, cs,
                                   *_cfg(nms_pre, max_num, score_thr, nms_thr, dir_offset, dir_limit_offset),
                                   *(ptr(o) for o in outs), ptr(ws), ws.numel(), stream_ptr(dev))
    if st == _UNSUPPORTED:
        return None
    check(st, f"{_OP}.anchor3d_get_bboxes")
    return outs
