// Global memory straight into LDS (buffer_load_dwordx4 ... lds) and the barrier that goes with it; shared by the F(4x4, 3x3)
// ping-pong kernels (conv_winograd43_pp.hpp) and the grouped final convolutions (conv3x3.hip).
#pragma once

namespace pd3 {

// Workgroup barrier that orders LDS traffic only.  __syncthreads() makes the compiler drain vmcnt as well -- a pending
// buffer_load ... lds counts as a store to LDS -- which puts the full latency of every fetch in flight in front of the
// barrier.  The kernels that use this wait for exactly the fetches a barrier has to publish (explicit s_waitcnt vmcnt(N))
// and let the others travel across it (LDS-DMA requests stay in flight across s_barrier).
__device__ __forceinline__ void w4_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// 64 lanes x 16 bytes from base + voff + soff to lds .. lds + 1023 (buffer_load_dwordx4 ... lds: no staging registers, no
// store pass; bytes from `bytes` on read as zeros; a lane that is masked out fetches nothing and writes nothing)
__device__ __forceinline__ void pp_dma(const float* base, unsigned bytes, float* lds, unsigned voff, unsigned soff) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, (int)bytes, 0x00020000);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds, 16, (int)voff, (int)soff, 0, 0);
}

}  // namespace pd3
