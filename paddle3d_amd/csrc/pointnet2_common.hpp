// Pieces shared by the pointnet2 kernels (pointnet2.hip, pointnet2_stack.hip).
#pragma once
#include "common.hpp"

namespace pd3 {
namespace pn2 {

// ((dx*dx + dy*dy) + dz*dz) with dx = x2 - x1; the build has -ffp-contract=off, so no FMA.
__device__ __forceinline__ float dist3(float x1, float y1, float z1, float x2, float y2, float z2) {
  const float dx = x2 - x1, dy = y2 - y1, dz = z2 - z1;
  return (dx * dx + dy * dy) + dz * dz;
}

// Number of set lanes of `mask` below the calling lane: the slot of this lane's hit among the wave's hits, so the
// wave places its hits in lane (index) order.
__device__ __forceinline__ int ballot_rank(uint64_t mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

}  // namespace pn2
}  // namespace pd3
