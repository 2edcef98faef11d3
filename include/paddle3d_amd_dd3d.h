/* C ABI of DD3D's FCOS heads and post-processing in libpaddle3d_amd.so: the entry points of csrc/dd3d.hip.  They are
 * declared here and listed in paddle3d_amd._lib.DD3D_ENTRY_POINTS, beside include/paddle3d_amd.h and
 * _lib.ENTRY_POINTS, whose size and blocks tests/test_abi.py pins (as include/paddle3d_amd_smoke.h does for SMOKE);
 * tests/test_abi_dd3d.py holds these rows to this header in the same way.  The status codes are paddle3d_amd.h's. */
#ifndef PADDLE3D_AMD_DD3D_H
#define PADDLE3D_AMD_DD3D_H

#include "paddle3d_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * DD3D's FCOS heads and post-processing at inference (csrc/dd3d.hip; models/heads/fcos_heads/fcos2d_head.py:160-186,
 * :334-503, fcos3d_head.py:33-108, :268-296, :519-639, models/detection/dd3d/dd3d.py:144-176, :183-212,
 * utils/transform.py:167-246), fp32, on `stream`, no host synchronisation, every count on the device, every output
 * element written on every call.  The arithmetic order of every output and the three definitions (tie order of the
 * selection, no renormalisation of the egocentric quaternion, the NMS semantics) are in the header of csrc/dd3d.hip;
 * tests/golden/dd3d_numpy.py restates them.  Statuses: 0, PD3_EINVAL (-1), PD3_EWORKSPACE (-2), PD3_EUNSUPPORTED
 * (-3, nothing is launched), or a positive hipError_t.
 *
 * Common: per-level arguments are HOST arrays of `levels` device pointers; level_table: `levels` rows of five int64 on
 * the host (H, W, stride, pitch, batch_stride; the last two describe the tower outputs of pd3_dd3d_head_forward and are
 * ignored elsewhere); logits [batch, num_classes, H, W] and centerness [batch, 1, H, W] per level, dense; intrinsics
 * [batch, 3, 3] (inverted here, in double); canon_box_sizes [num_classes, 3]; box3d_classes: num_classes, or 1 for
 * class_agnostic_box3d (the 3D predictors then have one row per quantity); flags: 1 thresh_with_ctr, 2 locations
 * offset "half", 4 scale_depth_by_focal_lengths, 8 predict_allocentric_rot, 16 predict_distance; nms_categories: classes
 * at or above it never survive (the reference's fixed categories = [0 .. 4]).
 * -> rows [batch, R, 20] (pred_boxes 4, scores, scores_3d, pred_classes, fpn_levels, locations 2, pred_boxes3d 10), in
 * NMS order, zero past min(counts[b], R); counts int32 [batch]: the rows the reference keeps (a tie at the post-NMS cut
 * can make it exceed R); R = post_nms_topk, or levels * pre_nms_topk when post_nms_topk <= 0.
 * PD3_EUNSUPPORTED unless 1 <= pre_nms_topk <= 1024, 1 <= levels <= 8, 1 <= num_classes <= 16, num_classes * H * W <
 * 2^30 per level, channels <= 512, nms_thresh > 0 and the NMS sweep's LDS fits; batch == 0 is success without a launch;
 * nothing needs an alignment.
 * pd3_dd3d_workspace: bytes of workspace for either entry point (0 for a shape they refuse); needs no GPU.
 * pd3_dd3d_head_forward: the LAZY form.  box2d_feat / box3d_feat: the box2d and box3d towers' outputs per level
 *   [batch, channels, H, pitch] (pitch >= W floats per row, batch_stride floats between frames, both of a level);
 *   box3d_feat NULL: only_box2d (scores_3d and pred_boxes3d are zero, the order is by scores).  box2d_weight
 *   [4, channels, 3, 3], box2d_bias [4]; box3d_weight [box3d_weight_levels, 11 * box3d_classes, channels, 3, 3] with
 *   the rows quat (4 * box3d_classes), ctr (2 *), depth, size (3 *), conf, each in the reference's channel order
 *   k * box3d_classes + class, and box3d_bias likewise (zeros where a predictor has no bias); box3d_weight_levels: 1, or
 *   `levels` for use_per_level_predictors; scales [levels, 6]: the Scale / Offset values of a level (box2d_reg, proj_ctr,
 *   size, conf, depth scale, depth offset; 1 1 1 1 1 0 without use_scale).  The predictors are evaluated at the selected
 *   entries only.
 * pd3_dd3d_post_process: the same selection, decode and tail from the reference's dense head outputs (scales and ReLU
 *   applied): box2d_reg [batch, 4, H, W] and the five 3D maps per level; the five NULL: only_box2d.
 * ------------------------------------------------------------------------------------------- */
size_t pd3_dd3d_workspace(int batch, int levels, const int64_t *level_table, int num_classes, int pre_nms_topk);
int pd3_dd3d_head_forward(const void *const *logits, const void *const *centerness, const void *const *box2d_feat,
                          const void *const *box3d_feat, const int64_t *level_table, const void *box2d_weight,
                          const void *box2d_bias, const void *box3d_weight, const void *box3d_bias,
                          const void *scales, const void *intrinsics, const void *canon_box_sizes, int batch,
                          int levels, int channels, int num_classes, int box3d_classes, int box3d_weight_levels,
                          int pre_nms_topk, int post_nms_topk, int nms_categories, int flags, float pre_nms_thresh,
                          float nms_thresh, float min_depth, float max_depth, float depth_factor, void *rows,
                          void *counts, void *workspace, size_t workspace_bytes, void *stream);
int pd3_dd3d_post_process(const void *const *logits, const void *const *centerness, const void *const *box2d_reg,
                          const void *const *box3d_quat, const void *const *box3d_ctr,
                          const void *const *box3d_depth, const void *const *box3d_size,
                          const void *const *box3d_conf, const int64_t *level_table, const void *intrinsics,
                          const void *canon_box_sizes, int batch, int levels, int num_classes, int box3d_classes,
                          int pre_nms_topk, int post_nms_topk, int nms_categories, int flags, float pre_nms_thresh,
                          float nms_thresh, float min_depth, float max_depth, float depth_factor, void *rows,
                          void *counts, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PADDLE3D_AMD_DD3D_H */
