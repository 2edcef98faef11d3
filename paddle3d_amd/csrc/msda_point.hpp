// The per-point step of multi-scale deformable attention, shared by csrc/ms_deform_attn.hip (the reference's op) and
// csrc/bevformer.hip (the encoder's fused attention): the range test, the corner rows, the bilinear weights, the
// 16-B corner loads and the ((w1*v1 + w2*v2) + w3*v3) + w4*v4 chain.  The arithmetic contract is the one in the
// header of ms_deform_attn.hip; both files compute a sampled point with exactly these operations in this order.
#pragma once
#include <cmath>

#include "common.hpp"

namespace pd3 {
namespace msda {

constexpr int64_t kStartLimit = (int64_t)1 << 62;  // |level_start_index| bound of a level that is read

template <typename T>
struct MsdaArgs {
  const T* value;
  const int64_t* shapes;  // [L, 2] (H, W)
  const int64_t* start;   // [L]
  const T* loc;           // [B, Q, M, L, P, 2]
  const T* attn;          // [B, Q, M, L, P]
  int B, S, M, C, L, Q, P;
};

// One sampling point: the range test, the corners' value-row indices (or -1) and the bilinear weights.
template <typename T>
struct Pt {
  bool ok;
  int64_t row[4];  // value row b*S + level_start + y*W + x, -1 where the corner does not count
  T w[4];
  T hh, hw, lh, lw;
  int Hl, Wl;
};

template <typename T>
__device__ __forceinline__ Pt<T> ms_point(const MsdaArgs<T>& g, int b, int l, T lx, T ly) {
  Pt<T> t;
  const int64_t Hl = g.shapes[2 * l], Wl = g.shapes[2 * l + 1], s0 = g.start[l];
  // a level outside these limits is skipped whole; inside them s0 + y*W + x cannot overflow int64
  const bool level_ok = Hl >= 1 && Hl <= INT32_MAX && Wl >= 1 && Wl <= INT32_MAX && s0 >= -kStartLimit &&
                        s0 <= kStartLimit;
  t.Hl = level_ok ? (int)Hl : 0;
  t.Wl = level_ok ? (int)Wl : 0;
  const T h = ly * (T)t.Hl - (T)0.5;
  const T w = lx * (T)t.Wl - (T)0.5;
  t.ok = level_ok && h > (T)-1 && w > (T)-1 && h < (T)t.Hl && w < (T)t.Wl;
  for (int k = 0; k < 4; ++k) t.row[k] = -1;
  if (!t.ok) {
    t.w[0] = t.w[1] = t.w[2] = t.w[3] = t.hh = t.hw = t.lh = t.lw = (T)0;
    return t;
  }
  const int h0 = (int)floorf((float)h), w0 = (int)floorf((float)w);
  t.lh = h - (T)h0;
  t.lw = w - (T)w0;
  t.hh = (T)1 - t.lh;
  t.hw = (T)1 - t.lw;
  t.w[0] = t.hh * t.hw;
  t.w[1] = t.hh * t.lw;
  t.w[2] = t.lh * t.hw;
  t.w[3] = t.lh * t.lw;
  const int64_t base = (int64_t)b * g.S;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t y = h0 + (k >> 1), x = w0 + (k & 1);
    const int64_t r = s0 + y * Wl + x;
    if (y >= 0 && y < Hl && x >= 0 && x < Wl && r >= 0 && r < g.S) t.row[k] = base + r;
  }
  return t;
}

template <typename T, int V>
struct Vec {
  T v[V];
};

template <typename T, int V>
__device__ __forceinline__ Vec<T, V> load_vec(const T* p) {
  Vec<T, V> r;
  if constexpr (V == 4 && sizeof(T) == 4) {
    const float4 f = *reinterpret_cast<const float4*>(p);
    r.v[0] = f.x;
    r.v[1] = f.y;
    r.v[2] = f.z;
    r.v[3] = f.w;
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) r.v[j] = p[j];
  }
  return r;
}

// col += bilinear(point) * a for the V channels at vbase (value + m*C + c0; MC = M*C floats per value row).
// The caller has tested t.ok.
template <typename T, int V>
__device__ __forceinline__ void ms_sample_add(const Pt<T>& t, const T* vbase, int64_t MC, T a, T (&col)[V]) {
  Vec<T, V> v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (t.row[k] >= 0) {
      v[k] = load_vec<T, V>(vbase + t.row[k] * MC);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) v[k].v[j] = (T)0;
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const T val = ((t.w[0] * v[0].v[j] + t.w[1] * v[1].v[j]) + t.w[2] * v[2].v[j]) + t.w[3] * v[3].v[j];
    col[j] = col[j] + val * a;
  }
}

}  // namespace msda
}  // namespace pd3
