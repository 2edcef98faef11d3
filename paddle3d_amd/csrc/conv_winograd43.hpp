// Shared pieces of the F(4x4, 3x3) kernels (conv_winograd43.hip: the packed form; conv_winograd43_pp.hip: the ping-pong
// form of round 4; conv_winograd43_ppv.hip: the ping-pong form fed with a precomputed V): tile constants, the transform
// steps, the MFMA stream, the output step, the tile decode and the entry points' common checks.  What only the two
// ping-pong forms share is in conv_winograd43_pp.hpp.
#pragma once
#include "../../include/paddle3d_amd.h"
#include "common.hpp"
#include "lds_dma.hpp"

#include <type_traits>

namespace pd3 {

typedef float w4_f32x4 __attribute__((ext_vector_type(4)));
typedef float w4_f32x2 __attribute__((ext_vector_type(2)));

constexpr int kW4Ci = 4;                  // input channels per trip (= MFMA K)
constexpr int kW4TR = 2, kW4TC = 16;      // tile rows / columns per workgroup (4x4 outputs each)
constexpr int kW4Cs = 36;                 // components per element
constexpr int kW4RawR = 4 * kW4TR + 2;    // 10 staged input rows
constexpr int kW4RawW = 4 * kW4TC + 8;    // 72 staged input columns: x0-4 .. x0+67
constexpr int kW4RawPl = kW4RawR * kW4RawW;                  // 720
constexpr int kW4Vsz = kW4TR * kW4Ci * kW4TC * kW4Cs;        // 4608 floats
constexpr int kW4RawSz = kW4Ci * kW4RawPl;                   // 2880 floats
constexpr int kW4XN4 = kW4RawSz / 4;                         // 720 float4

// B^T applied to six values (one column or one row of the patch)
__device__ __forceinline__ void w4_in(const float d0, const float d1, const float d2, const float d3, const float d4,
                                      const float d5, float (&t)[6]) {
  const float a = __builtin_fmaf(-4.f, d2, d4), b = __builtin_fmaf(-4.f, d1, d3);
  const float c = d4 - d2, e = d3 - d1;
  t[0] = __builtin_fmaf(4.f, d0, __builtin_fmaf(-5.f, d2, d4));
  t[1] = a + b;
  t[2] = a - b;
  t[3] = __builtin_fmaf(2.f, e, c);
  t[4] = __builtin_fmaf(-2.f, e, c);
  t[5] = __builtin_fmaf(4.f, d1, __builtin_fmaf(-5.f, d3, d5));
}

// A^T applied to six values -> four
__device__ __forceinline__ void w4_out(const float m0, const float m1, const float m2, const float m3, const float m4,
                                       const float m5, float (&s)[4]) {
  const float p = m1 + m2, q = m1 - m2, r = m3 + m4, u = m3 - m4;
  s[0] = m0 + p + r;
  s[1] = __builtin_fmaf(2.f, u, q);
  s[2] = __builtin_fmaf(4.f, r, p);
  s[3] = __builtin_fmaf(8.f, u, q) + m5;
}

// w4_in on both halves of a register pair at once (v_pk_add_f32 / v_pk_fma_f32: one issue slot each on gfx950 when the
// pair lies adjacent as it is, tools/hwcheck/lane_swap_pk_rates.hip): every half sees w4_in's operations, in their order
__device__ __forceinline__ w4_f32x2 w4_fma2(const float k, const w4_f32x2 x, const w4_f32x2 y) {
  return __builtin_elementwise_fma((w4_f32x2){k, k}, x, y);
}
__device__ __forceinline__ void w4_in2(const w4_f32x2 d0, const w4_f32x2 d1, const w4_f32x2 d2, const w4_f32x2 d3,
                                       const w4_f32x2 d4, const w4_f32x2 d5, w4_f32x2 (&t)[6]) {
  const w4_f32x2 a = w4_fma2(-4.f, d2, d4), b = w4_fma2(-4.f, d1, d3);
  const w4_f32x2 c = d4 - d2, e = d3 - d1;
  t[0] = w4_fma2(4.f, d0, w4_fma2(-5.f, d2, d4));
  t[1] = a + b;
  t[2] = a - b;
  t[3] = w4_fma2(2.f, e, c);
  t[4] = w4_fma2(-2.f, e, c);
  t[5] = w4_fma2(4.f, d1, w4_fma2(-5.f, d3, d5));
}

// (lo[i], hi[i]) of this lane and of lane ^ 16 -> (own lo, partner's lo) on the lanes of an even row of 16, (partner's hi,
// own hi) on those of an odd row: ONE v_permlane16_swap_b32 per value (8 cycles of issue, where the two DPP moves and two
// selects of a lane ^ 1 pairing take 16).  Spelled out, and the nine of a transform as one block: this compiler's
// __builtin_amdgcn_permlane16_swap hands back its FIRST result for both (measured: lane 0 got (own lo, own lo)), and inside
// inline assembly the two wait states between a VALU write of an operand and the swap that reads it are ours to keep --
// one s_nop 1 in front of the block (8 cycles, once) covers whatever wrote the operands last; the swaps themselves touch
// disjoint registers.
__device__ __forceinline__ void w4_swap_halves9(float (&lo)[9], float (&hi)[9]) {
  asm volatile(
      "s_nop 1\n\t"
      "v_permlane16_swap_b32 %0, %9\n\t"
      "v_permlane16_swap_b32 %1, %10\n\t"
      "v_permlane16_swap_b32 %2, %11\n\t"
      "v_permlane16_swap_b32 %3, %12\n\t"
      "v_permlane16_swap_b32 %4, %13\n\t"
      "v_permlane16_swap_b32 %5, %14\n\t"
      "v_permlane16_swap_b32 %6, %15\n\t"
      "v_permlane16_swap_b32 %7, %16\n\t"
      "v_permlane16_swap_b32 %8, %17"
      : "+v"(lo[0]), "+v"(lo[1]), "+v"(lo[2]), "+v"(lo[3]), "+v"(lo[4]), "+v"(lo[5]), "+v"(lo[6]), "+v"(lo[7]), "+v"(lo[8]),
        "+v"(hi[0]), "+v"(hi[1]), "+v"(hi[2]), "+v"(hi[3]), "+v"(hi[4]), "+v"(hi[5]), "+v"(hi[6]), "+v"(hi[7]), "+v"(hi[8]));
}

// (w4_lds_barrier, the workgroup barrier that orders LDS traffic only: lds_dma.hpp)

// V = B^T d B of a thread pair's patch -- lanes l and l ^ 16 of a wave, half hf = (l >> 4) & 1 -- from the six rows of this
// lane's three columns (r01[r] = d[r][3 hf + 0, 1], r2[r] = d[r][3 hf + 2]) to the lane's 18 components at v.  Row pass on
// this lane's three columns (columns 0 and 1 as a register pair), halves swapped between the pair, column pass on this
// lane's three rows; components (row, nu) -> 6 row + nu.
__device__ inline void w4_pair_transform(const w4_f32x2 (&r01)[6], const float (&r2)[6], float* v) {
  w4_f32x2 t01[6];  // (B^T d)[row][my columns 0, 1]
  float t2[6];      // (B^T d)[row][my column 2]
  w4_in2(r01[0], r01[1], r01[2], r01[3], r01[4], r01[5], t01);
  w4_in(r2[0], r2[1], r2[2], r2[3], r2[4], r2[5], t2);
  // the hf = 0 lane runs the column pass for rows 0..2, the hf = 1 lane for rows 3..5; what a lane lacks are the other
  // three columns of its rows, i.e. the partner's rows 0..2 (hf = 0) or 3..5 (hf = 1) of ITS columns: rows a and 3 + a
  // trade places between the two lanes, one swap per column
  float f[9], l[9];  // [3 a + b] -> columns 0..2 / 3..5 of row 3 hf + a of B^T d
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    f[3 * a] = t01[a][0], f[3 * a + 1] = t01[a][1], f[3 * a + 2] = t2[a];
    l[3 * a] = t01[3 + a][0], l[3 * a + 1] = t01[3 + a][1], l[3 * a + 2] = t2[3 + a];
  }
  w4_swap_halves9(f, l);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float o[6];
    w4_in(f[3 * a], f[3 * a + 1], f[3 * a + 2], l[3 * a], l[3 * a + 1], l[3 * a + 2], o);
    *reinterpret_cast<w4_f32x2*>(v + a * 6 + 0) = (w4_f32x2){o[0], o[1]};
    *reinterpret_cast<w4_f32x2*>(v + a * 6 + 2) = (w4_f32x2){o[2], o[3]};
    *reinterpret_cast<w4_f32x2*>(v + a * 6 + 4) = (w4_f32x2){o[4], o[5]};
  }
}

// N groups of 4 components (9 per trip of 4 input channels): b128 reads feed four MFMAs each; the reads run two groups
// ahead of their MFMAs (ring of three).  B of group g is read from vptr(g).  A is either an array of N float4 already
// in registers, or a functor g -> LDS address, read through a second ring.  hook() runs behind group HOOK's MFMAs (none
// by default).  FIRST: the stream opens the sum -- the MFMAs of its first trip take a zero C operand (an inline constant)
// instead of reading acc[], which nobody then has to clear: 0 + a * b either way.
struct w4_no_hook {
  __device__ __forceinline__ void operator()() const {}
};
template <int N, int HOOK = -1, bool FIRST = false, class UA, class VP, class F = w4_no_hook>
__device__ __forceinline__ void w4_mfma_stream(w4_f32x4 (&acc)[36], const UA& ua, const VP& vptr, const F& hook = F()) {
  constexpr bool kRing = !std::is_array<UA>::value;
  w4_f32x4 a[3], b[3];
  auto load = [&](const int g) {
    if constexpr (kRing) a[g % 3] = *reinterpret_cast<const w4_f32x4*>(ua(g));
    b[g % 3] = *reinterpret_cast<const w4_f32x4*>(vptr(g));
  };
  load(0);
  load(1);
#pragma unroll
  for (int g = 0; g < N; ++g) {
    if (g + 2 < N) load(g + 2);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float av;
      if constexpr (kRing) av = a[g % 3][j];
      else av = ua[g][j];
      const w4_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
      acc[(g % 9) * 4 + j] =
          __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[g % 3][j], FIRST && g < 9 ? zero : acc[(g % 9) * 4 + j], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (g == HOOK) {
      hook();
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// Output step: Y = A^T M A in registers, + bias, ReLU, zeros from column wv on, one non-temporal float4 store per output
// row (16 lanes = 256 contiguous bytes).  The lane holds all 36 components of tile (oy, ox) for channels co0 + r (acc[c][r],
// bias bv[r]).
// RELU: 1 / 0 when the caller knows it at compile time, -1: the runtime flag `relu`.  WHOLE: the caller vouches for
// wv == w, h % 8 == 0 and w % 64 == 0 -- no column is masked and no store is skipped, so neither is tested.  The general
// form (-1, false) computes the same values: the fast paths only drop selects that would not have changed anything.
template <int RELU = -1, bool WHOLE = false>
__device__ __forceinline__ void w4_output_step(const w4_f32x4 (&acc)[36], const w4_f32x4 bv, const int n, const int cout,
                                               const int co0, const int oy, const int ox, const int h, const int w,
                                               const int wv, const int relu, const int64_t plane,
                                               float* __restrict__ out) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float s[4][6];  // A^T M: column j of M through the row pass
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      float c4[4];
      w4_out(acc[0 * 6 + j][r], acc[1 * 6 + j][r], acc[2 * 6 + j][r], acc[3 * 6 + j][r], acc[4 * 6 + j][r],
             acc[5 * 6 + j][r], c4);
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k][j] = c4[k];
    }
    float* o = out + ((int64_t)n * cout + co0 + r) * plane + (int64_t)oy * w + ox;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float y4[4];
      w4_out(s[k][0], s[k][1], s[k][2], s[k][3], s[k][4], s[k][5], y4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        y4[j] += bv[r];
        if (RELU < 0 ? relu != 0 : RELU != 0) y4[j] = fmaxf(y4[j], 0.f);
        if (!WHOLE && ox + j >= wv) y4[j] = 0.f;
      }
      if (WHOLE || (oy + k < h && ox < w))  // partial tiles at the border (w % 4 == 0: a quad is in or out)
        __builtin_nontemporal_store((w4_f32x4){y4[0], y4[1], y4[2], y4[3]},
                                    reinterpret_cast<w4_f32x4*>(o + (int64_t)k * w));
    }
  }
}

// XCD-aware tile order (see conv_winograd.hip): pixel tile pt lives on XCD pt % 8 with all its `groups` channel groups
// (cg: this workgroup's).  A workgroup whose pt is not below the layer's pixel tiles has nothing to do.
struct w4_tile {
  int cg, pt, n, y0, x0;
};
__device__ __forceinline__ w4_tile w4_decode_block(const int groups, const int h, const int w) {
  const int tiles_x = (w + 4 * kW4TC - 1) / (4 * kW4TC), tiles_y = (h + 4 * kW4TR - 1) / (4 * kW4TR);
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int pt = (slot / groups) * 8 + xcd;
  const int tx = pt % tiles_x, ty = (pt / tiles_x) % tiles_y;
  return {slot % groups, pt, pt / (tiles_x * tiles_y), ty * 4 * kW4TR, tx * 4 * kW4TC};
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// What every entry point asks of (input, packed U, output) and of the layer's shape; the limits that differ (channel
// multiples, 32-bit offsets) are the entry point's own.
inline int w4_check_args(const void* in, const void* u, const void* out, int batch, int cin, int cout, int h, int w,
                         int w_valid, int cin_multiple, int cout_multiple) {
  if (!in || !u || !out || batch <= 0 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0 || w_valid <= 0 || w_valid > w)
    return PD3_EINVAL;
  if (cin % cin_multiple != 0 || cout % cout_multiple != 0 || w % 4 != 0) return PD3_EUNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(in) % 16 != 0 || reinterpret_cast<uintptr_t>(u) % 16 != 0 ||
      reinterpret_cast<uintptr_t>(out) % 16 != 0)
    return PD3_EINVAL;
  return PD3_OK;
}

// can the output step take its WHOLE form?
inline bool w4_whole(int h, int w, int w_valid) { return w_valid == w && h % (4 * kW4TR) == 0 && w % (4 * kW4TC) == 0; }

// pixel tiles of a layer (-> *ptiles) and the workgroups of a launch that gives each of them `groups` channel groups: pixel
// tiles rounded up to whole rounds of the 8 XCDs
inline int64_t w4_grid(int batch, int h, int w, int groups, int64_t* ptiles) {
  *ptiles = (int64_t)batch * ceil_div(h, 4 * kW4TR) * ceil_div(w, 4 * kW4TC);
  return (*ptiles + 7) / 8 * 8 * groups;
}

}  // namespace pd3
