"""CaDDN's frustum-to-voxel and map-to-BEV stage on the device (csrc/caddn.hip, contract in include/paddle3d_amd.h).
Inference only.

Common arguments: lidar_to_cam [B, 4, 4], cam_to_img [B, 3, 4], image_shape [B, 2] (H, W of the full-resolution image;
any integer or float dtype, read as int32), grid_size (X, Y, Z), pc_min (3), voxel_size (3) and disc_cfg, the
reference's {"mode": "UD" | "LID" | "SID", "num_bins", "depth_min", "depth_max"}.

frustum_grid(lidar_to_cam, cam_to_img, image_shape, grid_size, pc_min, voxel_size, disc_cfg)
    -> [B, X, Y, Z, 3], FrustumGridGenerator.forward's normalised sampling grid (frustum_grid_generator.py:87-154).
frustum_to_voxel(image_features, depth_logits, lidar_to_cam, cam_to_img, image_shape, grid_size, pc_min, voxel_size,
                 disc_cfg)
    image_features [B, C, h, w], depth_logits [B, D + 1, h, w] -> voxel_features [B, C, Z, Y, X]: FFE's frustum
    features sampled by FrustumToVoxel, without the frustum volume or the grid in memory.
frustum_to_bev_supported(C, C_out, Z)
    whether frustum_to_bev takes the shape (C, C_out multiples of 16 up to 64, Z <= 32).
frustum_to_bev(image_features, depth_logits, lidar_to_cam, cam_to_img, image_shape, grid_size, pc_min, voxel_size,
               disc_cfg, weight, scale, shift)
    weight [C_out, C * Z] (input index c * Z + z), scale / shift [C_out] the folded BatchNorm -> [B, C_out, Y, X]:
    relu(scale * (weight @ voxel) + shift), the voxel volume never in memory.

float32 only, on the GPU.  Nothing here synchronises with the host.  A shape the library does not take raises.
"""
from __future__ import annotations

import torch

from ._common import check, gpu_tensor, host_f32, lib, ptr, stream_ptr, workspace

__all__ = ["frustum_grid", "frustum_to_voxel", "frustum_to_bev", "frustum_to_bev_supported", "DISC_MODES"]

DISC_MODES = {"UD": 0, "LID": 1, "SID": 2}


def _shaped(t, op, what, shape):
    gpu_tensor(op, what, t, dtype=None, contiguous=False)
    if t.dtype != torch.float32:
        raise RuntimeError(f"{op}: {what} must be float32, got {t.dtype}")
    if t.dim() != len(shape) or any(s is not None and int(d) != s for d, s in zip(t.shape, shape)):
        raise RuntimeError(f"{op}: {what} must be {list(shape)}, got {tuple(t.shape)}")
    return t.contiguous()


def _calib(op, lidar_to_cam, cam_to_img, image_shape):
    l2c = _shaped(lidar_to_cam, op, "lidar_to_cam", (None, 4, 4))
    B = int(l2c.shape[0])
    c2i = _shaped(cam_to_img, op, "cam_to_img", (B, 3, 4))
    if not isinstance(image_shape, torch.Tensor) or not image_shape.is_cuda or tuple(image_shape.shape) != (B, 2):
        raise RuntimeError(f"{op}: image_shape must be a [{B}, 2] tensor on the GPU")
    if l2c.device != c2i.device or l2c.device != image_shape.device:
        raise RuntimeError(f"{op}: tensors on different devices")
    return l2c, c2i, image_shape.to(torch.int32).contiguous(), B


def _grid_args(op, grid_size, pc_min, voxel_size, disc_cfg):
    mode = disc_cfg["mode"]
    if mode not in DISC_MODES:
        raise NotImplementedError(f"{op}: discretisation mode {mode!r}")
    X, Y, Z = (int(v) for v in grid_size)
    D = int(disc_cfg["num_bins"])
    if min(X, Y, Z, D) < 1:
        raise RuntimeError(f"{op}: grid {(X, Y, Z)} with {D} bins")
    return (X, Y, Z, host_f32(pc_min, 3), host_f32(voxel_size, 3), DISC_MODES[mode], float(disc_cfg["depth_min"]),
            float(disc_cfg["depth_max"])), D


def frustum_grid(lidar_to_cam, cam_to_img, image_shape, grid_size, pc_min, voxel_size, disc_cfg):
    op = "frustum_grid"
    l2c, c2i, shp, B = _calib(op, lidar_to_cam, cam_to_img, image_shape)
    (X, Y, Z, mn, vs, mode, d0, d1), D = _grid_args(op, grid_size, pc_min, voxel_size, disc_cfg)
    out = torch.empty((B, X, Y, Z, 3), dtype=torch.float32, device=l2c.device)
    check(lib().pd3_frustum_grid(ptr(l2c), ptr(c2i), ptr(shp), B, X, Y, Z, ptr(mn), ptr(vs), mode, d0, d1, D, ptr(out),
                                 stream_ptr(l2c.device)), op)
    return out


def _maps(op, image_features, depth_logits, B, D):
    f = _shaped(image_features, op, "image_features", (B, None, None, None))
    C, h, w = (int(s) for s in f.shape[1:])
    if min(C, h, w) < 1:
        raise RuntimeError(f"{op}: empty image_features {tuple(f.shape)}")
    p = _shaped(depth_logits, op, "depth_logits", (B, D + 1, h, w))
    if p.device != f.device:
        raise RuntimeError(f"{op}: tensors on different devices")
    return f, p, C, h, w


def frustum_to_voxel(image_features, depth_logits, lidar_to_cam, cam_to_img, image_shape, grid_size, pc_min, voxel_size,
                     disc_cfg):
    op = "frustum_to_voxel"
    l2c, c2i, shp, B = _calib(op, lidar_to_cam, cam_to_img, image_shape)
    (X, Y, Z, mn, vs, mode, d0, d1), D = _grid_args(op, grid_size, pc_min, voxel_size, disc_cfg)
    f, p, C, h, w = _maps(op, image_features, depth_logits, B, D)
    out = torch.empty((B, C, Z, Y, X), dtype=torch.float32, device=f.device)
    nbytes = int(lib().pd3_frustum_to_voxel_workspace(B, C, D, h, w))
    ws = workspace(nbytes, f.device)
    check(lib().pd3_frustum_to_voxel(ptr(f), ptr(p), ptr(l2c), ptr(c2i), ptr(shp), B, C, D, h, w, X, Y, Z, ptr(mn),
                                     ptr(vs), mode, d0, d1, ptr(out), ptr(ws), nbytes, stream_ptr(f.device)), op)
    return out


def frustum_to_bev_supported(channels, c_out, grid_z):
    return (int(channels) in (16, 32, 48, 64) and int(c_out) in (16, 32, 48, 64) and 1 <= int(grid_z) <= 32)


def frustum_to_bev(image_features, depth_logits, lidar_to_cam, cam_to_img, image_shape, grid_size, pc_min, voxel_size,
                   disc_cfg, weight, scale, shift):
    op = "frustum_to_bev"
    l2c, c2i, shp, B = _calib(op, lidar_to_cam, cam_to_img, image_shape)
    (X, Y, Z, mn, vs, mode, d0, d1), D = _grid_args(op, grid_size, pc_min, voxel_size, disc_cfg)
    f, p, C, h, w = _maps(op, image_features, depth_logits, B, D)
    wt = _shaped(weight, op, "weight", (None, C * Z))
    CO = int(wt.shape[0])
    sc, sh = _shaped(scale, op, "scale", (CO,)), _shaped(shift, op, "shift", (CO,))
    if CO < 1 or any(t.device != f.device for t in (wt, sc, sh, l2c)):
        raise RuntimeError(f"{op}: weight {tuple(wt.shape)} / tensors on different devices")
    out = torch.empty((B, CO, Y, X), dtype=torch.float32, device=f.device)
    nbytes = int(lib().pd3_frustum_to_bev_workspace(B, C, D, h, w, Z, CO))
    ws = workspace(nbytes, f.device)
    check(lib().pd3_frustum_to_bev(ptr(f), ptr(p), ptr(l2c), ptr(c2i), ptr(shp), B, C, D, h, w, X, Y, Z, ptr(mn),
                                   ptr(vs), mode, d0, d1, ptr(wt), ptr(sc), ptr(sh), CO, ptr(out), ptr(ws), nbytes,
                                   stream_ptr(f.device)), op)
    return out
