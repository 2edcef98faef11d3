"""Every op shim whose arguments go through ops/_common.gpu_tensor refuses a CPU tensor with the reference's text
(PD_THROW("Unsupported device type for ... operator.")): there is no CPU path.  One public function per shim."""
import pytest
import torch

from paddle3d_amd.ops import (anchor3d_head, assign_score_withk, bevformer, bevformer_decoder, caddn, dd3d, iassd,
                              ms_deform_attn, petr, pointnet2_ops, pvrcnn, roi_head, smoke, squeezeseg)

Z = torch.zeros(2, 3)
RANGE, VOXEL = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0], [0.05, 0.05, 0.1]
CASES = {
    "petr": lambda: petr.multihead_attention_stream(Z, Z, Z, 8),
    "bevformer": lambda: bevformer.point_sampling(Z, Z, [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], 480, 800),
    "bevformer_decoder": lambda: bevformer_decoder.multihead_attention(Z, Z, Z, 8),
    "squeezeseg": lambda: squeezeseg.range_project(Z, Z),
    "smoke": lambda: smoke.smoke_post_process(Z, Z, Z, Z, Z, Z, Z, 50, 0.25),
    "dd3d": lambda: dd3d.dd3d_post_process([Z], [Z], [Z], None, [8], Z, Z),
    "anchor3d_head": lambda: anchor3d_head.anchor3d_get_bboxes(Z, Z, Z, Z, 10, 1000, 500, 0.05, 0.2),
    "farthest_point_sample": lambda: pointnet2_ops.farthest_point_sample(Z, 4),
    "roi_grid_points": lambda: roi_head.roi_grid_points(Z, 6, RANGE, VOXEL, [1]),
    "bev_interpolate": lambda: pvrcnn.bev_interpolate(Z, Z, RANGE, VOXEL, 8),
    "iassd_decode": lambda: iassd.iassd_decode(Z, Z, Z, None, 12),
    "frustum_grid": lambda: caddn.frustum_grid(Z, Z, Z, (4, 4, 2), [2.0, -30.0, -3.0], [0.5, 0.5, 0.5],
                                               dict(mode="LID", num_bins=8, depth_min=2.0, depth_max=46.8)),
    "assign_score_withk": lambda: assign_score_withk.assign_score_withk(Z, Z, Z, Z),
    "ms_deform_attn": lambda: ms_deform_attn.ms_deform_attn(Z, Z, Z, Z, Z, 1),
}


@pytest.mark.parametrize("op", list(CASES))
def test_a_cpu_tensor_is_refused_by_name(op):
    with pytest.raises(RuntimeError) as e:
        CASES[op]()
    assert str(e.value) == f"Unsupported device type for {op} operator."
