/* C ABI of BEVDepth's DepthNet kernels (csrc/depthnet.hip), beside paddle3d_amd.h: the same library, the same
 * conventions (device pointers, statuses 0, PD3_EINVAL (-1), PD3_EWORKSPACE (-2), PD3_EUNSUPPORTED (-3, nothing is
 * launched) or a positive hipError_t).  The rows of these entry points are paddle3d_amd._lib.DEPTHNET_ENTRY_POINTS.
 *
 * Reference: paddle3d/models/transformers/bevdet_transformer.py, ASPP.forward (:354-416) in eval mode and the tail of
 * LSSViewTransformerBEVDepth.forward (:740-742).  fp32, NCHW, on `stream`, no host synchronisation, every output element
 * written on every call.  The arithmetic order of every output is in the header of csrc/depthnet.hip;
 * tests/golden/depthnet_numpy.py restates it.
 *
 * pd3_aspp_workspace: bytes of the workspace pd3_aspp_forward needs: the four branches' output
 *   [batch, 4 mid_channels, height, width] and the pooled branch's per-image bias [batch, mid_channels], fp32; 0 for a
 *   shape the kernels do not take.
 *
 * pd3_aspp_forward: x [batch, in_channels, height, width] -> y [batch, mid_channels, height, width], the output of bn1
 *   and the relu (the dropout behind it is the identity in eval mode).
 *     branch_weights: aspp1 .. aspp4's atrous_conv weights, packed by ops/depthnet.py pack_aspp_branches (16-byte
 *       aligned); branch_scale, branch_shift [4 mid_channels]: their folded BatchNorms, branch after branch;
 *     pool_weight_t [in_channels, mid_channels]: global_avg_pool's 1 x 1 weight transposed; pool_scale, pool_shift
 *       [mid_channels]: its folded BatchNorm;
 *     proj_weights: the first 4 mid_channels columns of conv1's weight, packed by pack_aspp_projection (16-byte
 *       aligned); proj_pool_weight_t [mid_channels, mid_channels]: its last mid_channels columns transposed;
 *       proj_scale, proj_shift [mid_channels]: the folded bn1;
 *     dilation1 .. dilation3: the dilations (= paddings) of the three 3 x 3 branches; aspp1 is 1 x 1.
 *   A tap of a dilated kernel that falls outside the image for an output pixel is NOT part of that pixel's sum: for
 *   finite weights that equals zero padding, and an Inf or NaN weight under such a tap does not reach that pixel.
 *   Supported (ops/depthnet.py aspp_supported): in_channels and mid_channels multiples of 16 from 16 to 512,
 *   1 <= dilation <= 65535 each, height * width < 2^31, batch * height * width in fewer than 2^30 tiles of 64 pixels;
 *   anything else is PD3_EUNSUPPORTED.  batch == 0 is success without a launch.  Three launches.
 *
 * pd3_depth_softmax_split: x [batch, depth_channels + context_channels, height, width] ->
 *   depth [batch, depth_channels, height, width] = softmax of the first depth_channels channels over the channel axis,
 *   and tran_feat [batch, height, width, context_channels]: the remaining channels, channels last (the layout
 *   pd3_bev_pool_v2 reads).  depth_channels >= 1, context_channels >= 0, height * width < 2^31.  One launch.
 */
#ifndef PADDLE3D_AMD_DEPTHNET_H_
#define PADDLE3D_AMD_DEPTHNET_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t pd3_aspp_workspace(int batch, int in_channels, int mid_channels, int height, int width);

int pd3_aspp_forward(const void *x, const void *branch_weights, const void *branch_scale, const void *branch_shift,
                     const void *pool_weight_t, const void *pool_scale, const void *pool_shift,
                     const void *proj_weights, const void *proj_pool_weight_t, const void *proj_scale,
                     const void *proj_shift, int batch, int in_channels, int mid_channels, int height, int width,
                     int dilation1, int dilation2, int dilation3, void *y, void *workspace, size_t workspace_bytes,
                     void *stream);

int pd3_depth_softmax_split(const void *x, int batch, int depth_channels, int context_channels, int height, int width,
                            void *depth, void *tran_feat, void *stream);

#ifdef __cplusplus
}
#endif

#endif
