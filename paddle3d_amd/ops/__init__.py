"""Op modules with the names and call signatures of the reference's `paddle3d.ops` plugin API
(reference registry: paddle3d/ops/__init__.py:27-104).  Everything here binds the C ABI of
libpaddle3d_amd.so (include/paddle3d_amd.h, include/paddle3d_amd_lanedet.h, include/paddle3d_amd_cape.h, include/paddle3d_amd_dcn.h, include/paddle3d_amd_depthnet.h) through ctypes; nothing has a CPU / PyTorch fallback."""
from . import (anchor3d_head, assign_score_withk, bev_pool_v2, bevformer, bevformer_decoder, caddn, cape, bevdet_postprocess, centerpoint_postprocess, conv, dd3d, deform_conv, depthnet, iassd, iou3d_nms, lanedet,
               ms_deform_attn, petr, pointnet2_ops, pointpillars_scatter, pvrcnn, roi_head, roiaware_pool3d, smoke, sparse_conv3d, squeezeseg, ssd_head, sweeps,
               voxel_encoder, voxelize)

bev_pool_v2_backward = bev_pool_v2  # the reference exposes the backward op as its own module

__all__ = ["voxelize", "pointpillars_scatter", "voxel_encoder", "iou3d_nms", "centerpoint_postprocess",
           "bev_pool_v2", "bev_pool_v2_backward", "bevdet_postprocess", "sparse_conv3d", "sweeps", "conv", "ssd_head",
           "ms_deform_attn", "pointnet2_ops", "roiaware_pool3d", "assign_score_withk", "roi_head", "pvrcnn", "caddn",
           "bevformer", "bevformer_decoder", "petr", "squeezeseg", "anchor3d_head", "iassd", "smoke", "dd3d", "lanedet",
           "cape", "deform_conv", "depthnet"]
