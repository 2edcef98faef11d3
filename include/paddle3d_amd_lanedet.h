/* C ABI of BEV-LaneDet's lane head tail and lane post-processing at inference (csrc/lanedet.hip), beside
 * paddle3d_amd.h: the same library, the same conventions (device pointers unless said, statuses 0, PD3_EINVAL (-1),
 * PD3_EWORKSPACE (-2), PD3_EUNSUPPORTED (-3, nothing is launched) or a positive hipError_t).  The rows of these entry
 * points are paddle3d_amd._lib.LANEDET_ENTRY_POINTS.
 *
 * Reference: paddle3d/models/detection/bev_lanedet/bev_lanedet.py:50-108 (the four final 3x3 convolutions), :419-430
 * (test_forward), paddle3d/datasets/apollo/cluster.py:44-140, post_process.py:26-75, apollo_lane_metric.py:355-383.
 * fp32 maps, on `stream`, no host synchronisation, every count on the device, every output element written on every
 * call.  The arithmetic order of every output is in the header of csrc/lanedet.hip; tests/golden/lanedet_numpy.py
 * restates it.
 *
 * Common tail: conf (the threshold on the seg LOGIT, compared in fp32), emb_margin (the clustering gap),
 * min_cluster_size, max_x and meter_per_pixel_x / _y (> 0) of bev_instance2points_with_offset_z ->
 *   labels        uint8 [batch, h, w]              the reference's canvas: centre id + 1 of kept clusters, else 0
 *   num_lanes     int32 [batch]                    lanes with at least 2 rows, in increasing canvas id
 *   lane_id       int32 [batch, 32]                canvas id of each lane (0 past num_lanes)
 *   lane_rows     int32 [batch, 32]                row count of each lane
 *   fit_ok        int32 [batch, 32]                1 when the cubic fit was done here (at least 4 rows)
 *   points        float [batch, 32, h, 3]          (x_m, y_m, z) per row in the reference's (reversed) order, zero past
 *                                                  lane_rows
 *   fit           float [batch, 32, 40, 3]         the (X, Y, Z) samples of apollo_lane_metric.py:376-383, zero where
 *                                                  fit_ok == 0
 *   flags         int32 [batch]                    bit 0: more than 128 centres; bit 1: more than 32 canvas ids
 *   num_selected  int32 [batch]                    pixels with seg >= conf
 * A frame with a non-zero flag has num_lanes 0 and all-zero labels, lane_id, lane_rows, fit_ok, points and fit.
 * PD3_EUNSUPPORTED unless 1 <= nd <= 4, h <= 1024, h * w <= 2^20 and batch <= 65535; batch == 0 is success without a
 * launch; nothing needs an alignment.
 *
 * pd3_lanedet_workspace: bytes of workspace for either entry point (0 for a shape they refuse); needs no GPU.
 * pd3_lanedet_post_process: from the maps test_forward saves: seg [batch, 1, h, w] (logits), emb [batch, nd, h, w],
 *   offset and z [batch, 1, h, w]; offset_is_logit != 0: the sigmoid is applied here.
 * pd3_lanedet_head_forward: the LAZY form.  seg_feat / emb_feat / offset_feat / z_feat: the four branches' maps after
 *   their second convolution, BatchNorm and ReLU [batch, channels, h, pitch] (pitch >= w floats per row, batch_stride
 *   floats between frames: the four pointers may address one stacked map); the final 3x3 weights [1 | nd | 1 | 1,
 *   channels, 3, 3] and biases.  The seg convolution runs densely; emb, offset (with its sigmoid) and z are evaluated at
 *   the selected pixels only.  Also PD3_EUNSUPPORTED unless 1 <= channels <= 128.
 */
#ifndef PADDLE3D_AMD_LANEDET_H_
#define PADDLE3D_AMD_LANEDET_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t pd3_lanedet_workspace(int batch, int h, int w, int nd);
int pd3_lanedet_post_process(const void *seg, const void *emb, const void *offset, const void *z, int offset_is_logit,
                             int batch, int h, int w, int nd, float conf, float emb_margin, int min_cluster_size,
                             double max_x, double meter_per_pixel_x, double meter_per_pixel_y, void *labels,
                             void *num_lanes, void *lane_id, void *lane_rows, void *fit_ok, void *points, void *fit,
                             void *flags, void *num_selected, void *workspace, size_t workspace_bytes, void *stream);
int pd3_lanedet_head_forward(const void *seg_feat, const void *emb_feat, const void *offset_feat, const void *z_feat,
                             int64_t batch_stride, int pitch, int channels, const void *seg_weight,
                             const void *seg_bias, const void *emb_weight, const void *emb_bias,
                             const void *offset_weight, const void *offset_bias, const void *z_weight,
                             const void *z_bias, int batch, int h, int w, int nd, float conf, float emb_margin,
                             int min_cluster_size, double max_x, double meter_per_pixel_x, double meter_per_pixel_y,
                             void *labels, void *num_lanes, void *lane_id, void *lane_rows, void *fit_ok, void *points,
                             void *fit, void *flags, void *num_selected, void *workspace, size_t workspace_bytes,
                             void *stream);

#ifdef __cplusplus
}
#endif

#endif
