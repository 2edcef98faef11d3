/* C ABI of CAPE / CAPE-T's cross-view attention core and 3D sine position embedding at inference (csrc/cape.hip),
 * beside paddle3d_amd.h: the same library, the same conventions (device pointers unless said, statuses 0, PD3_EINVAL
 * (-1), PD3_EUNSUPPORTED (-3, nothing is launched) or a positive hipError_t).  The rows of these entry points are
 * paddle3d_amd._lib.CAPE_ENTRY_POINTS.
 *
 * Reference: paddle3d/models/layers/cape_transformer.py:200-269 (CrossAttention.forward), :76-91 (pos2posemb3d),
 * :540-557 (prepare_emb's world transform).  fp32, on `stream`, no host synchronisation, no workspace, every output
 * element written on every call.  The arithmetic order of every output is in the header of csrc/cape.hip;
 * tests/golden/cape_numpy.py restates it.
 *
 * pd3_cape_cva_forward: the attention of one decoder layer over the keys of all cameras, from the projected rows to
 *   what self.proj receives, in one launch.  q_a [batch, num_query, num_heads, head_dim], q_g [batch, num_cams,
 *   num_query, num_heads, head_dim], k_a, k_g and v [batch, num_cams, num_key, num_heads, head_dim] (the Linear outputs
 *   viewed per head), mask uint8 [batch, num_cams, num_key] or NULL (non-zero: masked; the score is REPLACED by -inf,
 *   the reference's masked_fill), scale_a and scale_g DEVICE float [num_heads] -> out [batch, num_query, num_heads *
 *   head_dim] = softmax over (camera, key) of scale_a[m] * (q_a . k_a) + scale_g[m] * (q_g[camera] . k_g), times v.  A
 *   query whose keys are all masked gets a NaN row, as the reference's softmax gives; a masked key still multiplies its
 *   zero weight by v, so an Inf or NaN there reaches the output, as in the reference.  An exact two-pass softmax,
 *   glibc's expf, one division per output element.  PD3_EUNSUPPORTED unless head_dim % 16 == 0, head_dim <= 128 and
 *   the five row tensors and out are 16-byte aligned (the mask and the scales need no alignment); num_cams < 1 or
 *   num_key < 1 is PD3_EINVAL; batch == 0 or num_query == 0 is success without a launch.
 * pd3_cape_posemb3d: points [batch, num_query, 3]; bound: 6 HOST floats (lo x, y, z, hi x, y, z) by which the points
 *   are un-normalised first, or NULL; rot [batch, num_views, 3, 3] and trans [batch, num_views, 3] (x = rot (p +
 *   trans)), or both NULL with num_views == 0; dim_t: num_feats HOST floats, the reference's temperature ** (2 * (i // 2)
 *   / num_feats) -> out [batch, num_views, num_query, 3 * num_feats], or [batch, num_query, 3 * num_feats] without
 *   views: sin / cos (glibc's sinf / cosf) of 2 pi x / dim_t, interleaved, in the reference's order (y, x, z).
 *   PD3_EUNSUPPORTED unless num_feats is even and <= 128; an empty output is success without a launch; nothing needs an
 *   alignment.
 */
#ifndef PADDLE3D_AMD_CAPE_H_
#define PADDLE3D_AMD_CAPE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int pd3_cape_cva_forward(const void *q_a, const void *q_g, const void *k_a, const void *k_g, const void *v,
                         const void *mask, const void *scale_a, const void *scale_g, int batch, int num_cams,
                         int num_query, int num_key, int num_heads, int head_dim, void *out, void *stream);
int pd3_cape_posemb3d(const void *points, const float *bound, const void *rot, const void *trans, const float *dim_t,
                      int batch, int num_views, int num_query, int num_feats, void *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif
