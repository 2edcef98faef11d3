// What the two ping-pong forms of the F(4x4, 3x3) kernels share (conv_winograd43_pp.hip, conv_winograd43_ppv.hip): the slot
// constants, the LDS addressing of a multiply slot's operands and the fetch of a slot's U.
#pragma once
#include "conv_winograd43.hpp"

namespace pd3 {

constexpr int kPpKT = 2;                                   // trips per slot
constexpr int kPpCi = kPpKT * kW4Ci;                       // 8 input channels per slot
constexpr int kPpVsz = kPpCi * kW4TC * kW4Cs;              // 4608 floats per (tile row, slot): [8 ci][16 tiles][36]
constexpr int kPpUHalf = 9 * 64 * 4;                       // 2304 floats: U of one trip for one wave (9 float4 per lane)
constexpr int kPpUsz = kPpKT * 4 * kPpUHalf;               // 18432 floats per slot: [trip][cb][q][lane][4]

// (pp_dma, 64 lanes x 16 bytes from global memory straight into LDS: lds_dma.hpp)

// MFMA operands of group g = 9 trip + q of a multiply slot: B = V[(trip * 4 + k) ci][tile][component] (bbase: the lane's
// (k, tile) = (lane >> 4, lane & 15)); A = U of (co, ci) = (lane & 15, lane >> 4), float4 q of the lane's 36 components at
// Us[((trip * 4 + cb) * 9 + q) * 256 + 4 lane]
__device__ __forceinline__ int pp_bbase(int lane) { return ((lane >> 4) * kW4TC + (lane & 15)) * kW4Cs; }
__device__ __forceinline__ const float* pp_vptr(const float* V, int bbase, int g) {
  return V + (g / 9) * (kW4Ci * kW4TC * kW4Cs) + bbase + (g % 9) * 4;
}
__device__ __forceinline__ const float* pp_uptr(const float* Us, int cb, int lane, int g) {
  return Us + (((g / 9) * 4 + cb) * 9 + (g % 9)) * 256 + lane * 4;
}

// half hh of U slot `slot` (counted from u, whose `bytes` bytes hold whole slots) for wave cb: 9 KB, contiguous in global
// memory and in LDS alike
__device__ __forceinline__ void pp_fetch_u(const float* u, unsigned bytes, float* Us, int cb, int lane, int slot, int hh) {
  const int blk = (hh * 4 + cb) * kPpUHalf;
  const unsigned so = __builtin_amdgcn_readfirstlane((unsigned)((slot * kPpUsz + blk) * 4));
#pragma unroll
  for (int q = 0; q < 9; ++q) pp_dma(u, bytes, Us + blk + q * 256, lane * 16, so + (unsigned)(q * 1024));
}

}  // namespace pd3
