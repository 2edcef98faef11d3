/* C ABI of the modulated deformable convolution (csrc/deform_conv.hip), beside paddle3d_amd.h: the same library, the
 * same conventions (device pointers, statuses 0, PD3_EINVAL (-1), PD3_EUNSUPPORTED (-3, nothing is launched) or a
 * positive hipError_t).  The row of this entry point is paddle3d_amd._lib.DCN_ENTRY_POINTS.
 *
 * Reference: paddle.vision.ops.deform_conv2d as paddle3d/models/backbones/mm_resnet.py:32-79 (DeformableConvV2) calls
 * it.  fp32, NCHW, on `stream`, no host synchronisation, no workspace, every output element written on every call.
 * The arithmetic order of every output is in the header of csrc/deform_conv.hip; tests/golden/dcn_numpy.py restates it.
 *
 * pd3_deform_conv2d_forward: x [batch, in_channels, height, width]; offset [batch, 18, Ho, Wo] (channel 2 k: dy of tap
 *   k = ky * 3 + kx, channel 2 k + 1: dx) whose images are offset_batch_stride floats apart, whose rows offset_pitch and
 *   whose channel planes Ho * offset_pitch; mask [batch, 9, Ho, Wo] with a stride and pitch of its own, or NULL
 *   (DCNv1); mask_is_logit != 0: the kernel applies 1 / (1 + expf(-mask)) itself; weight_packed: [out_channels,
 *   in_channels, 3, 3] in the order of ops/deform_conv.py pack_deform_conv_weight, 16-byte aligned; scale and shift
 *   [out_channels] or NULL each (a folded BatchNorm, or a bias as shift); relu != 0: max(., 0) that keeps a NaN ->
 *   y [batch, out_channels, Ho, Wo], Ho = (height + 2 padding - 2 dilation - 1) / stride + 1, Wo likewise.
 *   PD3_EUNSUPPORTED unless in_channels and out_channels are multiples of 16 up to 512, stride is 1 or 2, dilation >= 1,
 *   padding >= 0, height * width < 2^31 and batch * Ho * Wo needs fewer than 2^30 tiles of 64 pixels; an image smaller
 *   than the dilated kernel, a pitch below Wo or a batch stride below the channels' extent is PD3_EINVAL; batch == 0 is
 *   success without a launch.
 */
#ifndef PADDLE3D_AMD_DCN_H_
#define PADDLE3D_AMD_DCN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int pd3_deform_conv2d_forward(const void *x, const void *offset, int64_t offset_batch_stride, int offset_pitch,
                              const void *mask, int64_t mask_batch_stride, int mask_pitch, int mask_is_logit,
                              const void *weight_packed, const void *scale, const void *shift, int relu, int batch,
                              int in_channels, int out_channels, int height, int width, int stride, int padding,
                              int dilation, void *y, void *stream);

#ifdef __cplusplus
}
#endif

#endif
