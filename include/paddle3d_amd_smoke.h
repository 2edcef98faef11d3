/* C ABI of SMOKE's head and post-processing in libpaddle3d_amd.so: the entry points of csrc/smoke.hip.  They are
 * declared here and listed in paddle3d_amd._lib.SMOKE_ENTRY_POINTS, beside include/paddle3d_amd.h and
 * _lib.ENTRY_POINTS, whose size and blocks tests/test_abi.py pins; tests/test_abi_smoke.py holds these rows to this
 * header in the same way.  The status codes are paddle3d_amd.h's. */
#ifndef PADDLE3D_AMD_SMOKE_H
#define PADDLE3D_AMD_SMOKE_H

#include "paddle3d_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * SMOKE's head and post-processing at inference (csrc/smoke.hip; models/detection/smoke/smoke_predictor.py:78-97,
 * processor.py:45-194, smoke_coder.py:103-383, models/layers/layer_libs.py:36-116, :181-207, layer_norm.py:20-33),
 * fp32, on `stream`, no host synchronisation, every count on the device, every output element written on every call.
 * The arithmetic order of every output is in the header of csrc/smoke.hip; tests/golden/smoke_numpy.py restates it.
 * Statuses: 0, PD3_EINVAL (-1), PD3_EWORKSPACE (-2), PD3_EUNSUPPORTED (-3, nothing is launched), or a positive
 * hipError_t.
 *
 * Common: Ks [batch, 3, 3]; mode 0 (PostProcessor.forward): trans = trans_mat [batch, 3, 3], image_size [2], rows
 * with score <= det_threshold dropped; mode 1 (export_forward): trans = down_ratios [2], image_size unused, all rows;
 * depth_ref [2], dim_ref [num_classes, 3] (all device pointers); reg_channels: five ints on the host -> rows
 * [batch, max_detection, 14] in the reference's column order and descending score, rows past counts[b] zero, counts
 * int32 [batch].  Selection: one exact top-K over the num_classes * feat_h * feat_w peak-tested scores, ties to the
 * lower flat index; a NaN heat has score 0.  PD3_EUNSUPPORTED unless 1 <= max_detection <= min(1024, feat_h * feat_w),
 * 1 <= num_classes <= 16, reg_channels == (1, 2, 3, 2, 2), num_classes * feat_h * feat_w < 2^30 and pred_2d != 0;
 * batch == 0 is success without a launch; nothing needs an alignment.
 * pd3_smoke_head_workspace: bytes of workspace for either entry point (0 for a shape they refuse); needs no GPU.
 * pd3_smoke_head_forward: the LAZY head.  cls_feat / reg_feat: the two branches' 3x3 convolution outputs
 *   [batch, channels, feat_h, pitch] (pitch >= feat_w floats per row, batch_stride floats between frames: the two
 *   pointers may address one stacked map); gamma / beta [channels] of the two norms; cls_tables / reg_tables: NULL
 *   (GroupNorm with `groups` groups: the statistics are computed here, biased variance, epsilon 1e-5, accumulated in
 *   double in a fixed order) or filled [batch, 2, groups] tables (mean, rstd), e.g. BatchNorm's running statistics with
 *   groups == channels; cls_weight [num_classes, channels], reg_weight [10, channels] and the biases.  Only the class
 *   branch runs densely; the regression branch is evaluated at the max_detection selected pixels.  Also
 *   PD3_EUNSUPPORTED unless channels % groups == 0 and channels <= 512.
 * pd3_smoke_post_process: the same selection and decode from SMOKEPredictor's outputs heat [batch, num_classes,
 *   feat_h, feat_w] and regression [batch, 10, feat_h, feat_w].
 * ------------------------------------------------------------------------------------------- */
size_t pd3_smoke_head_workspace(int batch, int feat_h, int feat_w, int num_classes, int max_detection);
int pd3_smoke_head_forward(const void *cls_feat, const void *reg_feat, int64_t batch_stride, int pitch,
                           const void *cls_gamma, const void *cls_beta, const void *reg_gamma, const void *reg_beta,
                           const void *cls_tables, const void *reg_tables, const void *cls_weight,
                           const void *cls_bias, const void *reg_weight, const void *reg_bias, const void *Ks,
                           const void *trans, const void *image_size, const void *depth_ref, const void *dim_ref,
                           int batch, int channels, int groups, int feat_h, int feat_w, int num_classes,
                           const int *reg_channels, int max_detection, float det_threshold, int mode, int pred_2d,
                           void *rows, void *counts, void *workspace, size_t workspace_bytes, void *stream);
int pd3_smoke_post_process(const void *heat, const void *regression, const void *Ks, const void *trans,
                           const void *image_size, const void *depth_ref, const void *dim_ref, int batch, int feat_h,
                           int feat_w, int num_classes, const int *reg_channels, int max_detection,
                           float det_threshold, int mode, int pred_2d, void *rows, void *counts, void *workspace,
                           size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PADDLE3D_AMD_SMOKE_H */
