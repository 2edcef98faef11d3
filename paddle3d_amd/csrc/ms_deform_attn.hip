// Multi-scale deformable attention, forward and backward: PD_BUILD_OP(ms_deform_attn) and its PD_BUILD_GRAD_OP
// (paddle3d/ops/ms_deform_attn/ms_deform_attn.cc:85-101; per-element arithmetic ms_deform_attn_cuda_kernel.h:37-84
// bilinear, :86-151 its gradient, :220-274 the forward loop).  BEVFormer calls it in all three attention layers.
//
//   value [B, S, M, C], sampling_loc [B, Q, M, L, P, 2] (x, y in [0, 1] of the level), attn_weight [B, Q, M, L, P],
//   spatial_shapes [L, 2] int64 (H, W) and level_start_index [L] int64, both read on the device;
//   out [B, Q, M*C] = out[b, q, m*C + c].  fp32 and fp64 from one templated body.
//
// Arithmetic per output element (b, q, m, c), in this order (-ffp-contract=off, no fma anywhere;
// tests/golden/ms_deform_attn_numpy.py restates it and the fp32 / fp64 outputs equal it bit for bit):
//   col = 0; for l (outer), for p (inner):
//     h = loc_y * H_l - 0.5, w = loc_x * W_l - 0.5          (in T; the reference's double 0.5 rounds the same way)
//     skip unless h > -1 && w > -1 && h < H_l && w < W_l     (floating-point test first: NaN / Inf never get an address)
//     h0 = floorf((float)h), w0 likewise                     (the reference's floorf, also for T = double)
//     lh = h - h0, lw = w - w0, hh = 1 - lh, hw = 1 - lw
//     v1..v4 = corners (h0, w0), (h0, w0+1), (h0+1, w0), (h0+1, w0+1); 0 outside the map or when the value row
//              level_start + y*W_l + x falls outside [0, S) (spatial_shapes / level_start_index are not checked
//              against S by the reference; here such a row is never read).  A level with H_l or W_l outside
//              [1, 2^31 - 1] or |level_start| > 2^62 contributes nothing (its points fail the range test), so the
//              row arithmetic never overflows whatever the device-side tables hold.
//     val = ((w1*v1 + w2*v2) + w3*v3) + w4*v4 with w1 = hh*hw, w2 = hh*lw, w3 = lh*hw, w4 = lh*lw
//     col = col + val * weight
//
// Forward lane map: G lanes per (b, q, m), innermost in the thread index, so a 256-thread workgroup covers whole
// consecutive queries (neighbouring BEV queries share value rows in L2).  fp32 with C % 4 == 0 (and a 16-B aligned
// value): each lane owns 4 channels and fetches a corner row with 16-B loads, G = C/4 lanes per row (C = 32: 8
// lanes, 8 corner rows per wave instruction).  Otherwise one channel per lane.  A lane reads each (q, m, l, p)
// location and weight once (the group's lanes read the same address: one request) and forms the bilinear weights
// once per point for all its channels.  Channels beyond 64 lane groups loop.
//
// Backward (one launch writes all three gradients): Gp = min(64, pow2 >= C) lanes per (b, q, m), one channel per
// lane (c = lane, lane + Gp, ...), so each corner row is one contiguous segment of a wave instruction.
//   grad_value  += w_k * (grad_out * weight) at the four corners: no-return global float atomic adds, corners with
//                  w_k == 0 skipped.  The sum depends on the order the adds arrive in: grad_value may differ in the
//                  last bits from run to run, as the reference's does.  Zeroed in stream order by the entry point.
//   grad_attn   = sum_c grad_out * val, grad_loc = (sum_c (W * gw) * tg, sum_c (H * gh) * tg), tg = grad_out *
//                  weight: per-lane partial sums, then a butterfly across the Gp lanes in a fixed order -- bitwise
//                  reproducible, written once per (b, q, m, l, p) by lane 0 of the group (no atomics, no zeroing).
//                  A point that fails the range test gets 0.
// All offsets are 64-bit.
#include <cmath>

#include "common.hpp"
#include "msda_point.hpp"  // MsdaArgs, Pt, ms_point, load_vec, ms_sample_add: shared with bevformer.hip

namespace {

using namespace pd3::msda;

constexpr int kThreads = 256;

// V channels per lane, G lanes per (b, q, m); V > 1 needs C % V == 0 and an aligned value.
template <typename T, int V>
__global__ void __launch_bounds__(kThreads) ms_deform_attn_fwd(MsdaArgs<T> g, int G, T* out) {
  const int64_t gid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t bqm = gid / G;
  const int lane_g = (int)(gid - bqm * G);
  if (bqm >= (int64_t)g.B * g.Q * g.M) return;
  const int m = (int)(bqm % g.M);
  const int b = (int)(bqm / ((int64_t)g.Q * g.M));
  const int LP = g.L * g.P;
  const T* loc = g.loc + bqm * LP * 2;
  const T* wt = g.attn + bqm * LP;
  const int64_t MC = (int64_t)g.M * g.C;
  for (int c0 = lane_g * V; c0 < g.C; c0 += G * V) {
    T col[V];
#pragma unroll
    for (int j = 0; j < V; ++j) col[j] = (T)0;
    const T* vbase = g.value + (int64_t)m * g.C + c0;
    for (int l = 0; l < g.L; ++l) {
      for (int p = 0; p < g.P; ++p) {
        const int i = l * g.P + p;
        const T lx = loc[2 * i], ly = loc[2 * i + 1], a = wt[i];
        const Pt<T> t = ms_point(g, b, l, lx, ly);
        if (!t.ok) continue;
        ms_sample_add<T, V>(t, vbase, MC, a, col);
      }
    }
    T* o = out + bqm * g.C + c0;
    if constexpr (V == 4 && sizeof(T) == 4) {
      *reinterpret_cast<float4*>(o) = make_float4(col[0], col[1], col[2], col[3]);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = col[j];
    }
  }
}

template <typename T>
__device__ __forceinline__ T group_sum(T x, int Gp) {
  for (int off = Gp >> 1; off > 0; off >>= 1) x = x + __shfl_xor(x, off, Gp);
  return x;
}

__device__ __forceinline__ void atomic_add_nr(float* p, float v) { unsafeAtomicAdd(p, v); }
__device__ __forceinline__ void atomic_add_nr(double* p, double v) { unsafeAtomicAdd(p, v); }

// Gp (power of two, <= 64) lanes per (b, q, m), one channel per lane.  Every lane of a group runs every point so
// the cross-lane sums see the whole group.
template <typename T>
__global__ void __launch_bounds__(kThreads) ms_deform_attn_bwd(MsdaArgs<T> g, int Gp, const T* grad_out,
                                                               T* grad_value, T* grad_loc, T* grad_attn) {
  const int64_t gid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t bqm = gid / Gp;
  const int lane_g = (int)(gid - bqm * Gp);
  // a group never straddles the end: B*Q*M*Gp is the exact thread count rounded up to whole groups
  if (bqm >= (int64_t)g.B * g.Q * g.M) return;
  const int m = (int)(bqm % g.M);
  const int b = (int)(bqm / ((int64_t)g.Q * g.M));
  const int LP = g.L * g.P;
  const T* loc = g.loc + bqm * LP * 2;
  const T* wt = g.attn + bqm * LP;
  const T* go = grad_out + bqm * g.C;
  const int64_t MC = (int64_t)g.M * g.C;
  const int64_t chan0 = (int64_t)m * g.C;
  for (int l = 0; l < g.L; ++l) {
    for (int p = 0; p < g.P; ++p) {
      const int i = l * g.P + p;
      const T lx = loc[2 * i], ly = loc[2 * i + 1], a = wt[i];
      const Pt<T> t = ms_point(g, b, l, lx, ly);
      T sa = (T)0, sx = (T)0, sy = (T)0;
      if (t.ok) {
        for (int c = lane_g; c < g.C; c += Gp) {
          const T top = go[c];
          const T tg = top * a;
          T v[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = t.row[k] >= 0 ? g.value[t.row[k] * MC + chan0 + c] : (T)0;
          // gh / gw as the reference accumulates them, corner by corner
          T gh = (T)0, gw = (T)0;
          if (t.row[0] >= 0) { gh = gh - t.hw * v[0]; gw = gw - t.hh * v[0]; }
          if (t.row[1] >= 0) { gh = gh - t.lw * v[1]; gw = gw + t.hh * v[1]; }
          if (t.row[2] >= 0) { gh = gh + t.hw * v[2]; gw = gw - t.lh * v[2]; }
          if (t.row[3] >= 0) { gh = gh + t.lw * v[3]; gw = gw + t.lh * v[3]; }
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (t.row[k] >= 0 && t.w[k] != (T)0) atomic_add_nr(grad_value + t.row[k] * MC + chan0 + c, t.w[k] * tg);
          const T val = ((t.w[0] * v[0] + t.w[1] * v[1]) + t.w[2] * v[2]) + t.w[3] * v[3];
          sa = sa + top * val;
          sx = sx + ((T)t.Wl * gw) * tg;
          sy = sy + ((T)t.Hl * gh) * tg;
        }
      }
      sa = group_sum(sa, Gp);
      sx = group_sum(sx, Gp);
      sy = group_sum(sy, Gp);
      if (lane_g == 0) {
        grad_attn[bqm * LP + i] = sa;
        grad_loc[(bqm * LP + i) * 2] = sx;
        grad_loc[(bqm * LP + i) * 2 + 1] = sy;
      }
    }
  }
}

int check_dims(int batch, int spatial_size, int num_heads, int channels, int num_levels, int num_query,
               int num_point) {
  if (batch < 0 || num_query < 0 || spatial_size < 1 || num_heads < 1 || channels < 1 || num_levels < 1 ||
      num_point < 1)
    return PD3_EINVAL;
  return PD3_OK;
}

template <typename T>
MsdaArgs<T> make_args(const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                      const void* sampling_loc, const void* attn_weight, int batch, int spatial_size, int num_heads,
                      int channels, int num_levels, int num_query, int num_point) {
  MsdaArgs<T> g;
  g.value = static_cast<const T*>(value);
  g.shapes = spatial_shapes;
  g.start = level_start_index;
  g.loc = static_cast<const T*>(sampling_loc);
  g.attn = static_cast<const T*>(attn_weight);
  g.B = batch;
  g.S = spatial_size;
  g.M = num_heads;
  g.C = channels;
  g.L = num_levels;
  g.Q = num_query;
  g.P = num_point;
  return g;
}

template <typename T>
int fwd(const MsdaArgs<T>& g, void* out, hipStream_t stream) {
  const int64_t bqm = (int64_t)g.B * g.Q * g.M;
  const bool vec4 = sizeof(T) == 4 && g.C % 4 == 0 && (reinterpret_cast<uintptr_t>(g.value) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const int V = vec4 ? 4 : 1;
  const int G = (int)std::min<int64_t>(64, g.C / V);
  const int64_t blocks = pd3::ceil_div(bqm * G, kThreads);
  if (blocks > 0x7fffffff) return PD3_EUNSUPPORTED;
  if constexpr (sizeof(T) == 4) {
    if (vec4) {
      hipLaunchKernelGGL((ms_deform_attn_fwd<T, 4>), dim3((unsigned)blocks), dim3(kThreads), 0, stream, g, G,
                         static_cast<T*>(out));
      return pd3::launch_status();
    }
  }
  hipLaunchKernelGGL((ms_deform_attn_fwd<T, 1>), dim3((unsigned)blocks), dim3(kThreads), 0, stream, g, G,
                       static_cast<T*>(out));
  return pd3::launch_status();
}

template <typename T>
int bwd(const MsdaArgs<T>& g, const void* grad_out, void* grad_value, void* grad_loc, void* grad_attn,
        hipStream_t stream) {
  const int64_t bqm = (int64_t)g.B * g.Q * g.M;
  hipError_t e = hipMemsetAsync(grad_value, 0, (size_t)g.B * g.S * g.M * g.C * sizeof(T), stream);
  if (e != hipSuccess) return (int)e;
  if (bqm == 0) return PD3_OK;
  int Gp = 1;
  while (Gp < g.C && Gp < 64) Gp <<= 1;
  const int64_t blocks = pd3::ceil_div(bqm * Gp, kThreads);
  if (blocks > 0x7fffffff) return PD3_EUNSUPPORTED;
  hipLaunchKernelGGL(ms_deform_attn_bwd<T>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, g, Gp,
                     static_cast<const T*>(grad_out), static_cast<T*>(grad_value), static_cast<T*>(grad_loc),
                     static_cast<T*>(grad_attn));
  return pd3::launch_status();
}

}  // namespace

extern "C" {

int pd3_ms_deform_attn_forward(int dtype, const void* value, const int64_t* spatial_shapes,
                               const int64_t* level_start_index, const void* sampling_loc, const void* attn_weight,
                               int batch, int spatial_size, int num_heads, int channels, int num_levels,
                               int num_query, int num_point, void* out, void* stream) {
  if (dtype != 0 && dtype != 1) return PD3_EINVAL;
  if (int e = check_dims(batch, spatial_size, num_heads, channels, num_levels, num_query, num_point)) return e;
  if (batch == 0 || num_query == 0) return PD3_OK;
  if (!value || !spatial_shapes || !level_start_index || !sampling_loc || !attn_weight || !out) return PD3_EINVAL;
  if (dtype == 0)
    return fwd(make_args<float>(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, batch,
                                spatial_size, num_heads, channels, num_levels, num_query, num_point),
               out, (hipStream_t)stream);
  return fwd(make_args<double>(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, batch,
                               spatial_size, num_heads, channels, num_levels, num_query, num_point),
             out, (hipStream_t)stream);
}

int pd3_ms_deform_attn_backward(int dtype, const void* value, const int64_t* spatial_shapes,
                                const int64_t* level_start_index, const void* sampling_loc, const void* attn_weight,
                                const void* grad_out, int batch, int spatial_size, int num_heads, int channels,
                                int num_levels, int num_query, int num_point, void* grad_value,
                                void* grad_sampling_loc, void* grad_attn_weight, void* stream) {
  if (dtype != 0 && dtype != 1) return PD3_EINVAL;
  if (int e = check_dims(batch, spatial_size, num_heads, channels, num_levels, num_query, num_point)) return e;
  if (batch == 0) return PD3_OK;
  if (!value || !grad_value) return PD3_EINVAL;
  if (num_query > 0 && (!spatial_shapes || !level_start_index || !sampling_loc || !attn_weight || !grad_out ||
                        !grad_sampling_loc || !grad_attn_weight))
    return PD3_EINVAL;
  if (dtype == 0)
    return bwd(make_args<float>(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, batch,
                                spatial_size, num_heads, channels, num_levels, num_query, num_point),
               grad_out, grad_value, grad_sampling_loc, grad_attn_weight, (hipStream_t)stream);
  return bwd(make_args<double>(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, batch,
                               spatial_size, num_heads, channels, num_levels, num_query, num_point),
             grad_out, grad_value, grad_sampling_loc, grad_attn_weight, (hipStream_t)stream);
}

}  // extern "C"
