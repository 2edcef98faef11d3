// BEVFormer's encoder attention (paddle3d/models/transformers): the camera projection of the pillar anchors and the
// sampling stage of spatial cross-attention (SCA) and temporal self-attention (TSA), each as one kernel, fp32.
//
// pd3_bevformer_point_sampling       BEVFormerEncoder.point_sampling (encoders.py:120-176)
//   ref_3d [D, Q, 3] in [0, 1], lidar2img [B, cams, 4, 4] (row-major), pc_range[6] (host), img_h, img_w ->
//   reference_points_cam [cams, B, Q, D, 2], bev_mask [cams, B, Q, D] uint8, hit_bits [B, Q] uint8 (bit cam set when
//   any of the D mask bits of that camera is), hit_count [B, Q] uint8.  Per (b, q, d, cam), no fma:
//     x = r_x * (pc[3] - pc[0]) + pc[0], y and z likewise (the differences are formed in fp32 on the host)
//     c_k = ((a_k0*x + a_k1*y) + a_k2*z) + a_k3 for rows k = 0, 1, 2 of the camera's matrix
//     zc = max(c_2, 1e-5f); u = (c_0 / zc) / (float)img_w; v = (c_1 / zc) / (float)img_h
//     mask = c_2 > 1e-5f && v > 0 && v < 1 && u < 1 && u > 0
//   One thread per (b, q); every output element is written.
//
// pd3_bevformer_sca                  SpatialCrossAttention.forward around MSDeformableAttention3D.forward
//                                    (spatial_cross_attention.py:81-212, :310-428) without the rebatch
//   value [B*cams, S, M, C] (projected), offsets [B, Q, M, L, P, 2] and logits [B, Q, M, L*P] (the two Linear outputs on
//   the BEV queries), reference_points_cam, hit_bits, spatial_shapes [L, 2] / level_start_index [L] int64 on the device
//   -> out [B, Q, M*C].  Per (b, q, m), in this order:
//     mx = max_i x_i; e_i = expf(x_i - mx) (glibc's bits, libm_exact.hpp); s = ((e_0 + e_1) + ...); a_i = e_i / s
//     slot = 0; for each camera whose hit bit is set, in index order:
//       col = 0; for l (outer), for p (inner), i = l*P + p:
//         loc = ref_cam[cam, b, q, p % D] + (off_x / (float)W_l, off_y / (float)H_l)
//         the ms_deform_attn point step (msda_point.hpp) against value row b*cams + cam: col = col + val * a_i
//       slot = slot + col
//     out = slot / (float)max(popcount(hit_bits), 1)
//   Cameras that miss cost nothing; out is written once, with no atomics, zeroing or workspace.
//
// pd3_bevformer_tsa                  TemporalSelfAttention.forward's sampling (temporal_self_attention.py:207-272)
//   value [B*2, S, M, C], offsets [B, Q, M, 2, L, P, 2] and logits [B, Q, M, 2, L*P] in the Linear's own layout,
//   reference_points [B*2, Q, L, 2] -> out [B, Q, M*C].  Per (b, q, m): for queue entry j = 0, 1 the softmax above
//   over logits[.., j, :], col_j as above with loc = ref[2b + j, q, l] + off / (W_l, H_l) against value row 2b + j;
//   out = (col_0 + col_1) * 0.5.
//
// Lane map of both attention kernels (the forward of ms_deform_attn.hip): G = min(64, C/4) lanes per (b, q, m), each
// owning 4 channels per step of G*4 and fetching a corner row with 16-B loads; min(256 / G, 64) whole groups per workgroup
// (C = 32: 8 lanes, 32 groups = 16 queries of M = 2).  The group's L*P softmax terms live in LDS: lane j of the group
// evaluates expf for i = j, j + G, ..., every lane then forms the sum in index order, and the same lanes divide.
// Supported shapes (bevformer_supported): C % 4 == 0 with 16-B aligned value and out, L*P <= 32, and for SCA
// cams <= 8 and P % D == 0; anything else returns PD3_EUNSUPPORTED without a launch.  All offsets are 64-bit.
#include "bevformer_attn.hpp"

namespace {

using namespace pd3::bevattn;

constexpr int kMaxCams = 8;

__global__ void __launch_bounds__(kThreads) point_sampling_kernel(const float* __restrict__ ref_3d,
                                                                  const float* __restrict__ lidar2img, float sx,
                                                                  float ox, float sy, float oy, float sz, float oz,
                                                                  float img_h, float img_w, int B, int cams, int Q,
                                                                  int D, float* __restrict__ ref_cam,
                                                                  uint8_t* __restrict__ mask,
                                                                  uint8_t* __restrict__ hit_bits,
                                                                  uint8_t* __restrict__ hit_count) {
  const int64_t bq = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (bq >= (int64_t)B * Q) return;
  const int b = (int)(bq / Q), q = (int)(bq - (int64_t)b * Q);
  const float eps = 1e-5f;
  unsigned bits = 0;
  int count = 0;
  for (int cam = 0; cam < cams; ++cam) {
    const float* a = lidar2img + ((int64_t)b * cams + cam) * 16;
    bool any = false;
    for (int d = 0; d < D; ++d) {
      const float* r = ref_3d + ((int64_t)d * Q + q) * 3;
      const float x = r[0] * sx + ox, y = r[1] * sy + oy, z = r[2] * sz + oz;
      const float c0 = ((a[0] * x + a[1] * y) + a[2] * z) + a[3];
      const float c1 = ((a[4] * x + a[5] * y) + a[6] * z) + a[7];
      const float c2 = ((a[8] * x + a[9] * y) + a[10] * z) + a[11];
      const float zc = (c2 > eps || c2 != c2) ? c2 : eps;  // maximum(c2, eps): a NaN depth stays NaN
      const float u = (c0 / zc) / img_w;
      const float v = (c1 / zc) / img_h;
      const bool m = c2 > eps && v > 0.0f && v < 1.0f && u < 1.0f && u > 0.0f;
      const int64_t o = (((int64_t)cam * B + b) * Q + q) * D + d;
      ref_cam[2 * o] = u;
      ref_cam[2 * o + 1] = v;
      mask[o] = m ? 1 : 0;
      any = any || m;
    }
    if (any) {
      bits |= 1u << cam;
      ++count;
    }
  }
  hit_bits[bq] = (uint8_t)bits;
  hit_count[bq] = (uint8_t)count;
}

__global__ void __launch_bounds__(kThreads) sca_kernel(AttnDims d, int cams, int D, const float* __restrict__ value,
                                                       const int64_t* __restrict__ shapes,
                                                       const int64_t* __restrict__ start,
                                                       const float* __restrict__ offsets,
                                                       const float* __restrict__ logits,
                                                       const float* __restrict__ ref_cam,
                                                       const uint8_t* __restrict__ hit_bits, float* __restrict__ out) {
  extern __shared__ float lds[];
  const int grp = threadIdx.x / d.G, lane_g = threadIdx.x - grp * d.G;
  const int64_t bqm = (int64_t)blockIdx.x * d.groups + grp;
  const bool active = grp < d.groups && bqm < (int64_t)d.B * d.Q * d.M;
  const int LP = d.L * d.P;
  float* w = lds + grp * LP;  // only dereferenced by active lanes
  group_softmax(logits + (active ? bqm : 0) * LP, LP, lane_g, d.G, active, w);
  if (!active) return;
  const int m = (int)(bqm % d.M);
  const int64_t bq = bqm / d.M;
  const int b = (int)(bq / d.Q), q = (int)(bq - (int64_t)b * d.Q);
  const MsdaArgs<float> g = point_args(value, shapes, start, d);
  const float* off = offsets + bqm * LP * 2;
  const unsigned bits = hit_bits[bq] & ((1u << cams) - 1u);
  const float denom = (float)max(__popc(bits), 1);
  const int64_t MC = (int64_t)d.M * d.C;
  for (int c0 = lane_g * 4; c0 < d.C; c0 += d.G * 4) {
    float slot[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const float* vbase = value + (int64_t)m * d.C + c0;
    for (int cam = 0; cam < cams; ++cam) {
      if (!((bits >> cam) & 1u)) continue;
      float col[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      const float* ref = ref_cam + ((((int64_t)cam * d.B + b) * d.Q + q) * D) * 2;
      sample_source(g, b * cams + cam, off, w, ref, D, 1, 0, vbase, MC, col);
#pragma unroll
      for (int j = 0; j < 4; ++j) slot[j] = slot[j] + col[j];
    }
    *reinterpret_cast<float4*>(out + bqm * d.C + c0) =
        make_float4(slot[0] / denom, slot[1] / denom, slot[2] / denom, slot[3] / denom);
  }
}

__global__ void __launch_bounds__(kThreads) tsa_kernel(AttnDims d, const float* __restrict__ value,
                                                       const int64_t* __restrict__ shapes,
                                                       const int64_t* __restrict__ start,
                                                       const float* __restrict__ offsets,
                                                       const float* __restrict__ logits,
                                                       const float* __restrict__ ref_2d, float* __restrict__ out) {
  extern __shared__ float lds[];
  const int grp = threadIdx.x / d.G, lane_g = threadIdx.x - grp * d.G;
  const int64_t bqm = (int64_t)blockIdx.x * d.groups + grp;
  const bool active = grp < d.groups && bqm < (int64_t)d.B * d.Q * d.M;
  const int LP = d.L * d.P;
  float* w = lds + grp * 2 * LP;
  const int64_t row = active ? bqm : 0;
  group_softmax(logits + row * 2 * LP, LP, lane_g, d.G, active, w);
  group_softmax(logits + row * 2 * LP + LP, LP, lane_g, d.G, active, w + LP);
  if (!active) return;
  const int m = (int)(bqm % d.M);
  const int64_t bq = bqm / d.M;
  const int b = (int)(bq / d.Q), q = (int)(bq - (int64_t)b * d.Q);
  const MsdaArgs<float> g = point_args(value, shapes, start, d);
  const int64_t MC = (int64_t)d.M * d.C;
  for (int c0 = lane_g * 4; c0 < d.C; c0 += d.G * 4) {
    float col[2][4] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
    const float* vbase = value + (int64_t)m * d.C + c0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float* off = offsets + (bqm * 2 + j) * LP * 2;
      const float* ref = ref_2d + (((int64_t)(2 * b + j)) * d.Q + q) * d.L * 2;
      sample_source(g, 2 * b + j, off, w + j * LP, ref, 1, 0, 1, vbase, MC, col[j]);
    }
    *reinterpret_cast<float4*>(out + bqm * d.C + c0) =
        make_float4((col[0][0] + col[1][0]) * 0.5f, (col[0][1] + col[1][1]) * 0.5f, (col[0][2] + col[1][2]) * 0.5f,
                    (col[0][3] + col[1][3]) * 0.5f);
  }
}

// The one supported-shape predicate of the two attention kernels (cams = 2, D = 1 for TSA).
bool bevformer_supported(const void* value, const void* out, int C, int L, int P, int cams, int D) {
  return C % 4 == 0 && aligned16(value) && aligned16(out) && (int64_t)L * P <= kMaxLP && cams <= kMaxCams && D >= 1 &&
         P % D == 0;
}

}  // namespace

extern "C" {

int pd3_bevformer_point_sampling(const void* ref_3d, const void* lidar2img, const float* pc_range, int img_h,
                                 int img_w, int batch, int num_cams, int num_query, int num_anchors,
                                 void* reference_points_cam, void* bev_mask, void* hit_bits, void* hit_count,
                                 void* stream) {
  if (batch < 0 || num_query < 0 || num_cams < 1 || num_anchors < 1 || img_h < 1 || img_w < 1 || !pc_range)
    return PD3_EINVAL;
  if (num_cams > kMaxCams) return PD3_EUNSUPPORTED;
  if (batch == 0 || num_query == 0) return PD3_OK;
  if (!ref_3d || !lidar2img || !reference_points_cam || !bev_mask || !hit_bits || !hit_count) return PD3_EINVAL;
  const int64_t blocks = pd3::ceil_div((int64_t)batch * num_query, kThreads);
  if (blocks > 0x7fffffff) return PD3_EUNSUPPORTED;
  hipLaunchKernelGGL(point_sampling_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream,
                     static_cast<const float*>(ref_3d), static_cast<const float*>(lidar2img),
                     pc_range[3] - pc_range[0], pc_range[0], pc_range[4] - pc_range[1], pc_range[1],
                     pc_range[5] - pc_range[2], pc_range[2], (float)img_h, (float)img_w, batch, num_cams, num_query,
                     num_anchors, static_cast<float*>(reference_points_cam), static_cast<uint8_t*>(bev_mask),
                     static_cast<uint8_t*>(hit_bits), static_cast<uint8_t*>(hit_count));
  return pd3::launch_status();
}

int pd3_bevformer_sca(const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                      const void* sampling_offsets, const void* attention_logits, const void* reference_points_cam,
                      const void* hit_bits, int batch, int num_cams, int spatial_size, int num_heads, int channels,
                      int num_levels, int num_query, int num_point, int num_anchors, void* out, void* stream) {
  AttnDims d;
  if (int e = attn_dims(batch, spatial_size, num_heads, channels, num_levels, num_query, num_point, &d)) return e;
  if (num_cams < 1 || num_anchors < 1) return PD3_EINVAL;
  if (!bevformer_supported(value, out, channels, num_levels, num_point, num_cams, num_anchors))
    return PD3_EUNSUPPORTED;
  if ((int64_t)batch * num_cams > 0x7fffffff) return PD3_EUNSUPPORTED;
  if (batch == 0 || num_query == 0) return PD3_OK;
  if (!value || !spatial_shapes || !level_start_index || !sampling_offsets || !attention_logits ||
      !reference_points_cam || !hit_bits || !out)
    return PD3_EINVAL;
  const int64_t blocks = pd3::ceil_div((int64_t)batch * num_query * num_heads, d.groups);
  if (blocks > 0x7fffffff) return PD3_EUNSUPPORTED;
  const size_t lds = (size_t)d.groups * num_levels * num_point * sizeof(float);
  hipLaunchKernelGGL(sca_kernel, dim3((unsigned)blocks), dim3(kThreads), lds, (hipStream_t)stream, d, num_cams,
                     num_anchors, static_cast<const float*>(value), spatial_shapes, level_start_index,
                     static_cast<const float*>(sampling_offsets), static_cast<const float*>(attention_logits),
                     static_cast<const float*>(reference_points_cam), static_cast<const uint8_t*>(hit_bits),
                     static_cast<float*>(out));
  return pd3::launch_status();
}

int pd3_bevformer_tsa(const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                      const void* sampling_offsets, const void* attention_logits, const void* reference_points,
                      int batch, int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                      int num_point, void* out, void* stream) {
  AttnDims d;
  if (int e = attn_dims(batch, spatial_size, num_heads, channels, num_levels, num_query, num_point, &d)) return e;
  if (!bevformer_supported(value, out, channels, num_levels, num_point, 2, 1)) return PD3_EUNSUPPORTED;
  if (batch > 0x3fffffff) return PD3_EUNSUPPORTED;
  if (batch == 0 || num_query == 0) return PD3_OK;
  if (!value || !spatial_shapes || !level_start_index || !sampling_offsets || !attention_logits ||
      !reference_points || !out)
    return PD3_EINVAL;
  const int64_t blocks = pd3::ceil_div((int64_t)batch * num_query * num_heads, d.groups);
  if (blocks > 0x7fffffff) return PD3_EUNSUPPORTED;
  const size_t lds = (size_t)d.groups * 2 * num_levels * num_point * sizeof(float);
  hipLaunchKernelGGL(tsa_kernel, dim3((unsigned)blocks), dim3(kThreads), lds, (hipStream_t)stream, d,
                     static_cast<const float*>(value), spatial_shapes, level_start_index,
                     static_cast<const float*>(sampling_offsets), static_cast<const float*>(attention_logits),
                     static_cast<const float*>(reference_points), static_cast<float*>(out));
  return pd3::launch_status();
}

}  // extern "C"
