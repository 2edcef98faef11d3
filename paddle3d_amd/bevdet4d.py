"""BEVDet4D's temporal alignment on the device: every adjacent frame's BEV features warped into the current ego frame
and concatenated behind the current frame, in one HIP launch (csrc/bev_shift.hip, C ABI pd3_bevdet4d_align).

shift_feature(input, trans, rots, bda, bda_adj=None)      BEVDet4D.shift_feature (bevdet4d.py:90-159)
align_concat(bev_feat_list, rots, trans, bda)             extract_img_feat's align + concat (:291-298)
align_concat_sequential(bev_feat, feat_prev, trans_curr, trans_prev, rots_curr, rots_prev, bda)
                                                          extract_img_feat_sequential's (:205-216)

Features are fp32 GPU tensors [B, C, H, W] of any strides with unit-free h / w / c steps -- contiguous NCHW and the
channels-last view LSSViewTransformer.voxel_pooling_v2 returns are read in place.  Poses keep the reference's shapes
(rots [B, N_cam, 3, 3], trans [B, N_cam, 3], bda [B, 3, 3]); camera 0 is used.  Nothing here synchronises with the
host: the transforms are composed on the device.  `view_transformer` is anything with `grid_interval` and
`grid_lower_bound` (x, y first); None means BEVDet4D-R50's grid.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .ops._common import check, host_f32, lib, stream_ptr

__all__ = ["BEVDET4D_NUM_ADJ", "shift_feature", "align_concat", "align_concat_sequential", "align_device"]

BEVDET4D_NUM_ADJ = 8  # configs/bevdet/bevdet4d_r50_depth_nuscenes.yml: num_adj
_OP = "bevdet4d_align"
_MAX_FRAMES = 16


def _grid_params(view_transformer):
    if view_transformer is None:
        from .bevdet import BEVDET4D_GRID

        interval = [BEVDET4D_GRID["x"][2], BEVDET4D_GRID["y"][2]]
        lower = [BEVDET4D_GRID["x"][0], BEVDET4D_GRID["y"][0]]
    else:
        interval = [float(v) for v in list(view_transformer.grid_interval)[:2]]
        lower = [float(v) for v in list(view_transformer.grid_lower_bound)[:2]]
    return host_f32(interval, 2), host_f32(lower, 2)


def _gpu_f32(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"Unsupported device type for {_OP} operator ({what} must be a GPU tensor).")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{_OP}: {what} must be float32, got {t.dtype}")
    return t


def _feature(t, what, shape=None):
    t = _gpu_f32(t, what)
    if t.dim() != 4:
        raise RuntimeError(f"{_OP}: {what} must be [B, C, H, W], got {tuple(t.shape)}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{_OP}: {what} is {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def _mat(t, what, batch, tail):
    """Pose tensor [batch, *tail] with contiguous `tail` (a copy only if the caller's is not)."""
    t = _gpu_f32(t, what)
    if tuple(t.shape) != (batch, *tail):
        raise RuntimeError(f"{_OP}: {what} must be {(batch, *tail)}, got {tuple(t.shape)}")
    inner = t[0] if batch > 0 else t
    if not inner.is_contiguous():
        t = t.contiguous()
    return t


def _cam0(t, what, batch, tail):
    """Camera 0 of a [batch, N_cam, *tail] pose tensor as a [batch, *tail] view."""
    t = _gpu_f32(t, what)
    if t.dim() != 2 + len(tail) or int(t.shape[0]) != batch or tuple(t.shape[2:]) != tuple(tail) or t.shape[1] < 1:
        raise RuntimeError(f"{_OP}: {what} must be [{batch}, N_cam, {', '.join(map(str, tail))}], got "
                           f"{tuple(t.shape)}")
    return _mat(t[:, 0], what, batch, tail)


def _ptrs(ts):
    return C.cast((C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts]), C.c_void_p)


def align_device(feats, rots_cur, trans_cur, rots_adj, trans_adj, bda, bda_adj=None, view_transformer=None,
                 with_current=True, return_grid=False):
    """The operator behind the three entry points.

    feats: list of num_frame feature tensors [B, C, H, W] (feats[0] the current frame; ignored -- may be None --
    when with_current is False).  rots_cur / trans_cur / rots_adj / trans_adj: lists of num_frame - 1 camera-0 poses
    [B, 3, 3] / [B, 3] (views are fine); bda / bda_adj: lists of [B, 3, 3] (bda_adj None: bda).
    Returns out [B, (num_frame - 1 + with_current) * C, H, W] contiguous and, with return_grid, the normalised
    sampling grid [(num_frame - 1) * B, H, W, 2]."""
    nf = len(feats)
    if nf < (1 if with_current else 2) or nf > _MAX_FRAMES:
        raise RuntimeError(f"{_OP}: 1..{_MAX_FRAMES} frames (2.. without the current one), got {nf}")
    ref = feats[0] if with_current else feats[1]
    ref = _feature(ref, "frame feature")
    B, Ch, H, W = (int(s) for s in ref.shape)
    if H < 2 or W < 2:
        raise RuntimeError(f"{_OP}: H and W must be >= 2 (the grid is normalised by W-1, H-1), got {H} x {W}")
    fs = [None if (f == 0 and not with_current) else _feature(t, f"frame {f} feature", (B, Ch, H, W))
          for f, t in enumerate(feats)]
    na = nf - 1
    if any(len(x) != na for x in (rots_cur, trans_cur, rots_adj, trans_adj, bda)) or \
            (bda_adj is not None and len(bda_adj) != na):
        raise RuntimeError(f"{_OP}: one pose per adjacent frame ({na}) expected")
    rc = [_mat(t, "rots (current)", B, (3, 3)) for t in rots_cur]
    tc = [_mat(t, "trans (current)", B, (3,)) for t in trans_cur]
    ra = [_mat(t, "rots (adjacent)", B, (3, 3)) for t in rots_adj]
    ta = [_mat(t, "trans (adjacent)", B, (3,)) for t in trans_adj]
    bd = [_mat(t, "bda", B, (3, 3)) for t in bda]
    bj = None if bda_adj is None else [_mat(t, "bda_adj", B, (3, 3)) for t in bda_adj]
    dev = ref.device
    for t in [x for x in fs if x is not None] + rc + tc + ra + ta + bd + (bj or []):
        if t.device != dev:
            raise RuntimeError(f"{_OP}: all tensors must be on {dev}")
    strides = np.zeros((nf, 4), np.int64)
    for f, t in enumerate(fs):
        if t is not None:
            strides[f] = t.stride()
    pose_strides = np.zeros((max(na, 1), 6), np.int64)
    for a in range(na):
        pose_strides[a] = [rc[a].stride(0), tc[a].stride(0), ra[a].stride(0), ta[a].stride(0), bd[a].stride(0),
                           bj[a].stride(0) if bj is not None else 0]
    interval, lower = _grid_params(view_transformer)
    nout = na + (1 if with_current else 0)
    out = torch.empty((B, nout * Ch, H, W), dtype=torch.float32, device=dev)
    grid = torch.empty((na * B, H, W, 2), dtype=torch.float32, device=dev) if return_grid and na else None
    check(lib().pd3_bevdet4d_align(_ptrs(fs), C.c_void_p(strides.ctypes.data), nf, int(bool(with_current)), B, Ch,
                                   H, W, _ptrs(rc), _ptrs(tc), _ptrs(ra), _ptrs(ta), _ptrs(bd),
                                   _ptrs(bj) if bj is not None else None, C.c_void_p(pose_strides.ctypes.data),
                                   C.c_void_p(interval.ctypes.data), C.c_void_p(lower.ctypes.data),
                                   C.c_void_p(out.data_ptr()),
                                   C.c_void_p(grid.data_ptr()) if grid is not None else None, stream_ptr(dev)), _OP)
    return (out, grid) if return_grid else out


def shift_feature(input, trans, rots, bda, bda_adj=None, view_transformer=None, return_grid=False):
    """BEVDet4D.shift_feature: input [n, C, H, W] of the adjacent frame, trans = [trans_cur, trans_adj] ([n, N_cam,
    3] each), rots = [rots_cur, rots_adj] ([n, N_cam, 3, 3]), bda / bda_adj [n, 3, 3] -> [n, C, H, W]."""
    x = _feature(input, "input")
    n = int(x.shape[0])
    if len(trans) != 2 or len(rots) != 2:
        raise RuntimeError(f"{_OP}: trans and rots are [current, adjacent] pairs")
    return align_device([None, x], [_cam0(rots[0], "rots[0]", n, (3, 3))], [_cam0(trans[0], "trans[0]", n, (3,))],
                        [_cam0(rots[1], "rots[1]", n, (3, 3))], [_cam0(trans[1], "trans[1]", n, (3,))],
                        [bda], None if bda_adj is None else [bda_adj], view_transformer, with_current=False,
                        return_grid=return_grid)


def align_concat(bev_feat_list, rots, trans, bda, view_transformer=None, return_grid=False):
    """extract_img_feat (align_after_view_transfromation): bev_feat_list [current, adj 1 .., adj F-1] of [B, C, H,
    W]; rots / trans: per frame [B, N_cam, 3, 3] / [B, N_cam, 3]; bda [B, 3, 3] -> [B, F*C, H, W] =
    concat([current, shift_feature(adj k, [trans[0], trans[k]], [rots[0], rots[k]], bda) ...], axis=1)."""
    nf = len(bev_feat_list)
    if len(rots) != nf or len(trans) != nf:
        raise RuntimeError(f"{_OP}: rots and trans need one entry per frame ({nf})")
    B = int(_feature(bev_feat_list[0], "bev_feat_list[0]").shape[0])
    r0, t0 = _cam0(rots[0], "rots[0]", B, (3, 3)), _cam0(trans[0], "trans[0]", B, (3,))
    ra = [_cam0(rots[k], f"rots[{k}]", B, (3, 3)) for k in range(1, nf)]
    ta = [_cam0(trans[k], f"trans[{k}]", B, (3,)) for k in range(1, nf)]
    na = nf - 1
    return align_device(list(bev_feat_list), [r0] * na, [t0] * na, ra, ta, [bda] * na, None, view_transformer,
                        return_grid=return_grid)


def align_concat_sequential(bev_feat, feat_prev, trans_curr, trans_prev, rots_curr, rots_prev, bda,
                            view_transformer=None, return_grid=False):
    """extract_img_feat_sequential: bev_feat [1, C, H, W], feat_prev [num_adj, C, H, W]; trans_* [num_adj, N_cam,
    3], rots_* [num_adj, N_cam, 3, 3], bda [num_adj, 3, 3] (the tiled bda_curr) -> [1, (1 + num_adj) * C, H, W] =
    concat([bev_feat, shift_feature(feat_prev, ...).view(1, num_adj * C, H, W)], axis=1)."""
    cur = _feature(bev_feat, "bev_feat")
    prev = _feature(feat_prev, "feat_prev")
    if int(cur.shape[0]) != 1 or tuple(prev.shape[1:]) != tuple(cur.shape[1:]):
        raise RuntimeError(f"{_OP}: bev_feat must be [1, C, H, W] and feat_prev [num_adj, C, H, W], got "
                           f"{tuple(cur.shape)} and {tuple(prev.shape)}")
    na = int(prev.shape[0])
    rc, tc = _cam0(rots_curr, "rots_curr", na, (3, 3)), _cam0(trans_curr, "trans_curr", na, (3,))
    rp, tp = _cam0(rots_prev, "rots_prev", na, (3, 3)), _cam0(trans_prev, "trans_prev", na, (3,))
    bd = _mat(bda, "bda", na, (3, 3))
    # adjacent frame k is entry k of the stacked tensors: batch 1, one view per entry
    one = lambda t, k: t[k:k + 1]  # noqa: E731
    return align_device([cur] + [one(prev, k) for k in range(na)], [one(rc, k) for k in range(na)],
                        [one(tc, k) for k in range(na)], [one(rp, k) for k in range(na)],
                        [one(tp, k) for k in range(na)], [one(bd, k) for k in range(na)], None, view_transformer,
                        return_grid=return_grid)
