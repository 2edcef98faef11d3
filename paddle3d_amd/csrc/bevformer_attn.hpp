// What the BEVFormer attention kernels share (csrc/bevformer.hip: SCA and TSA of the encoder; csrc/bevformer_decoder.hip:
// the decoder's cross-attention): the lane map's dimensions, the group softmax and the walk over the L * P sampled
// points of one source.  The lane map and the arithmetic order are stated in the header of csrc/bevformer.hip.
#pragma once
#include <algorithm>

#include "common.hpp"
#include "libm_exact.hpp"
#include "msda_point.hpp"

namespace pd3 {
namespace bevattn {

using namespace pd3::msda;
namespace lm = pd3::lm;

constexpr int kThreads = 256;
constexpr int kMaxLP = 32;

// Softmax of the group's LP logits into its LDS row `w` (LP floats).  Called by every thread of the workgroup (the
// barriers are block-wide); `active` lanes do the work.  On return w[i] = e_i / sum.
__device__ __forceinline__ void group_softmax(const float* __restrict__ x, int LP, int lane_g, int G, bool active,
                                              float* w) {
  float mx = 0.0f;
  if (active) {
    mx = x[0];
    for (int i = 1; i < LP; ++i) mx = x[i] > mx ? x[i] : mx;
    for (int i = lane_g; i < LP; i += G) w[i] = lm::expf(x[i] - mx);
  }
  __syncthreads();
  float s = 0.0f;
  if (active) {
    s = w[0];
    for (int i = 1; i < LP; ++i) s = s + w[i];
  }
  __syncthreads();
  if (active)
    for (int i = lane_g; i < LP; i += G) w[i] = w[i] / s;
  __syncthreads();
}

struct AttnDims {
  int B, S, M, C, L, Q, P;
  int G, groups;  // lanes per (b, q, m), whole groups per workgroup
};

__device__ __forceinline__ MsdaArgs<float> point_args(const float* value, const int64_t* shapes,
                                                      const int64_t* start, const AttnDims& d) {
  MsdaArgs<float> g;
  g.value = value;
  g.shapes = shapes;
  g.start = start;
  g.loc = nullptr;
  g.attn = nullptr;
  g.B = d.B;
  g.S = d.S;
  g.M = d.M;
  g.C = d.C;
  g.L = d.L;
  g.Q = d.Q;
  g.P = d.P;
  return g;
}

// col[4] of one source (a camera or a queue entry): value batch row vb, reference points ref (x, y pairs, the pair
// of point p at ref[2 * ((p % D) * ref_stride_d + l * ref_stride_l)]).
__device__ __forceinline__ void sample_source(const MsdaArgs<float>& g, int vb, const float* __restrict__ off,
                                              const float* w, const float* __restrict__ ref, int D, int stride_d,
                                              int stride_l, const float* vbase, int64_t MC, float (&col)[4]) {
  for (int l = 0; l < g.L; ++l) {
    const float Wn = (float)g.shapes[2 * l + 1], Hn = (float)g.shapes[2 * l];
    for (int p = 0; p < g.P; ++p) {
      const int i = l * g.P + p;
      const float* r = ref + 2 * ((int64_t)(p % D) * stride_d + (int64_t)l * stride_l);
      const float lx = r[0] + off[2 * i] / Wn;
      const float ly = r[1] + off[2 * i + 1] / Hn;
      const Pt<float> t = ms_point(g, vb, l, lx, ly);
      if (!t.ok) continue;
      ms_sample_add<float, 4>(t, vbase, MC, w[i], col);
    }
  }
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static inline int attn_dims(int batch, int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                            int num_point, AttnDims* d) {
  if (batch < 0 || num_query < 0 || spatial_size < 1 || num_heads < 1 || channels < 1 || num_levels < 1 ||
      num_point < 1)
    return PD3_EINVAL;
  d->B = batch;
  d->S = spatial_size;
  d->M = num_heads;
  d->C = channels;
  d->L = num_levels;
  d->Q = num_query;
  d->P = num_point;
  d->G = std::min(64, std::max(1, channels / 4));
  d->groups = std::min(kThreads / d->G, 64);  // LDS per workgroup stays <= 64 * 2 * kMaxLP floats
  return PD3_OK;
}

}  // namespace bevattn
}  // namespace pd3
