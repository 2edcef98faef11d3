// 3x3 / stride 1 / pad 1 convolution + bias + ReLU by Winograd F(4x4, 3x3) on the fp32 matrix cores, NCHW in
// and out, fully fused (same layers as conv_winograd.hip; reference: second_backbone.py:72-120 and
// center_head.py:43-220, cuDNN in the reference).
//
//   Y(4x4) = A^T [ sum_ci (G g G^T) (.) (B^T d B) ] A,   d = the 6x6 input patch of a 4x4 output tile
// 36 independent GEMMs M[xi] = U[xi] V[xi]: 4x fewer multiplies than the direct form (F(2x2,3x3): 2.25x) for
// 1.5x the transform work per pixel.  fp32 throughout; the transform constants (4, 5, 8, 1/24 ...) cost about one
// decimal digit against the direct form (measured ~1e-5 absolute for |y| ~ 1.5), far inside the 1e-3 contract.
//
// Workgroup = 32 output channels x 32 tiles (2 tile rows x 16 tile columns = 8 x 64 output pixels) x all 36
// components; K walks 4 input channels per trip = one K step of v_mfma_f32_16x16x4_f32:
//   U trip : pre-transformed on the host, packed [2 co blocks][4 ci][16 co][36 xi] -> linear copy to LDS;
//   raw X  : [4 ci][10 rows][72 cols], aligned float4 loads from column x0-4, zero outside the image;
//   V trip : a PAIR of lanes transforms one (channel, tile) patch: lane h takes columns 3h..3h+2 through the
//            row pass, the halves are swapped with one DPP quad_perm per value, lane h then runs the column
//            pass for rows 3h..3h+2 and writes its 18 components to LDS as [2 tile rows][4 ci][16 tile cols][36];
//   MFMA   : wave w owns co block (w & 1) and tile row (w >> 1) for all 36 components (36 accumulator quads);
//            the 36-float component axis is read with conflict-free ds_read_b128 (36 l mod 64 are 16 distinct
//            multiples of 4), 9 + 9 reads for 36 MFMAs, reads running two groups ahead of their MFMAs;
//   epilogue: one lane holds all 36 components of its (co, tile): A^T M A in registers, + bias, ReLU, one float4
//            store per output row (16 lanes = 256 contiguous bytes).
// Two workgroups per CU (47 KB LDS); the next trip's global loads are issued before the MFMA block.
#include "../../include/paddle3d_amd.h"
#include "common.hpp"
#include "conv_winograd43.hpp"

namespace pd3 {

// CB = 16-channel blocks per workgroup.  CB = 2: 256 threads, two workgroups per CU.  CB = 4: 512 threads, one
// workgroup per CU -- every transformed patch then feeds 64 output channels (half the transform work per
// MFMA) and the two waves of a SIMD run their MFMA phases together, back to back on the matrix pipe; waves
// 0-3 transform while waves 4-7 park the (twice as large) U slice.
template <int CB>
__global__ __launch_bounds__(128 * CB, CB == 2 ? 2 : 1) void conv3x3_winograd43_kernel(const float* __restrict__ x,
                                                                    const float* __restrict__ up,
                                                                    const float* __restrict__ bias,
                                                                    float* __restrict__ out, int cin, int cout,
                                                                    int h, int w, int wv, int relu, int ptiles) {
  // w = row pitch of input and output (a multiple of 4), wv <= w the valid width: output columns >= wv are
  // written as zeros (and the caller guarantees the same of the input), i.e. they are the next layer's padding
  constexpr int THREADS = 128 * CB;
  constexpr int CO = 16 * CB;                       // output channels per workgroup
  constexpr int USZ = CB * kW4Ci * 16 * kW4Cs;      // floats of one U trip
  constexpr int UN4 = USZ / 4;                      // CB = 2: 1152, CB = 4: 2304 float4
  constexpr int UT0 = CB == 2 ? 0 : 256;            // first of the 256 threads that move U
  constexpr int UPT = (UN4 + 255) / 256;            // 5 (tail repeats the last one) / 9
  constexpr int XPT = (kW4XN4 + THREADS - 1) / THREADS;  // 3 / 2
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NBUF = CB == 4 ? 2 : 1;              // CB = 4: U and V double-buffered (see the trip loop)
  float* Us = smem;                                  // [NBUF][USZ]
  float* Vs = smem + NBUF * USZ;                     // [NBUF][kW4Vsz]
  float* Raw = Vs + NBUF * kW4Vsz;
  float *Ucur = Us, *Vcur = Vs, *Unext = Us, *Vnext = Vs;  // buffers of the trip being multiplied / prepared
  const int lane = lane_id(), wave = wave_id();
  const w4_tile tl = w4_decode_block(cout / CO, h, w);
  if (tl.pt >= ptiles) return;
  const int ct = tl.cg, n = tl.n, y0 = tl.y0, x0 = tl.x0;
  const int chunks = cin / kW4Ci;
  const int64_t plane = (int64_t)h * w;
  const float* xin = x + (int64_t)n * cin * plane;
  const w4_f32x4* usrc = reinterpret_cast<const w4_f32x4*>(up) + (int64_t)ct * chunks * UN4;

  // staging pattern of the raw patch (identical for every trip)
  int gofs[XPT], ldst[XPT];
  unsigned live = 0;
#pragma unroll
  for (int i = 0; i < XPT; ++i) {
    const int e = min((int)threadIdx.x + i * THREADS, kW4XN4 - 1);
    const int ci = e / (kW4RawR * (kW4RawW / 4)), rem = e - ci * (kW4RawR * (kW4RawW / 4));
    const int r = rem / (kW4RawW / 4), c4 = rem - r * (kW4RawW / 4);
    const int gy = y0 - 1 + r, gx = x0 - 4 + c4 * 4;  // a float4 is entirely inside or outside (w % 4 == 0)
    const bool ok = gy >= 0 && gy < h && gx >= 0 && gx < w;
    gofs[i] = ok ? (int)(ci * plane + (int64_t)gy * w + gx) : 0;
    live |= ok ? (1u << i) : 0u;
    ldst[i] = e * 4;
  }
  const bool moves_u = (int)threadIdx.x >= UT0;  // wave-uniform
  int uofs[UPT];
#pragma unroll
  for (int i = 0; i < UPT; ++i) uofs[i] = min(max((int)threadIdx.x - UT0, 0) + i * 256, UN4 - 1);
  const bool transforms = threadIdx.x < 256;     // wave-uniform
  // transform assignment: lanes l and l ^ 16 of wave ci (0..3) own patch (ci, tile); half hf = columns / rows 3hf..3hf+2.
  // A 32-lane half of the wave covers one tile row x 16 tiles x both halves (conv_winograd43_pp.hip has the LDS banks)
  const int hf = (lane >> 4) & 1;
  const int pci = wave & 3, ptile = (lane >> 5) * 16 + (lane & 15);
  const int rsrc = pci * kW4RawPl + (4 * (ptile >> 4)) * kW4RawW + 4 * (ptile & 15) + 3 + 3 * hf;
  const int vdst = (((ptile >> 4) * kW4Ci + pci) * kW4TC + (ptile & 15)) * kW4Cs + 18 * hf;
  // MFMA operand bases
  const int cb = wave % CB, tb = wave / CB;
  const int abase = ((cb * kW4Ci + (lane >> 4)) * 16 + (lane & 15)) * kW4Cs;
  const int bbase = ((tb * kW4Ci + (lane >> 4)) * kW4TC + (lane & 15)) * kW4Cs;

  w4_f32x4 acc[36];
#pragma unroll
  for (int c = 0; c < 36; ++c) acc[c] = (w4_f32x4){0.f, 0.f, 0.f, 0.f};

  w4_f32x4 xr[XPT], ur[UPT];

#define W4_FETCH_X(cc)                                                                   \
  {                                                                                      \
    const float* xc_ = xin + (int64_t)(cc) * kW4Ci * plane;                              \
    _Pragma("unroll") for (int i = 0; i < XPT; ++i)                                      \
        xr[i] = *reinterpret_cast<const w4_f32x4*>(xc_ + gofs[i]);                       \
  }
#define W4_FETCH_U(cc)                                                                   \
  if (CB == 2 || moves_u) {                                                              \
    const w4_f32x4* uc_ = usrc + (int64_t)(cc) * UN4;                                    \
    _Pragma("unroll") for (int i = 0; i < UPT; ++i) ur[i] = uc_[uofs[i]];                \
  }
#define W4_STASH_X()                                                                     \
  {                                                                                      \
    _Pragma("unroll") for (int i = 0; i < XPT; ++i) {                                    \
      const bool on_ = (live >> i) & 1u;                                                 \
      const w4_f32x4 z_ = {0.f, 0.f, 0.f, 0.f};                                          \
      *reinterpret_cast<w4_f32x4*>(Raw + ldst[i]) = on_ ? xr[i] : z_;                    \
    }                                                                                    \
  }
#define W4_STASH_U()                                                                     \
  if (CB == 2 || moves_u) {                                                              \
    _Pragma("unroll") for (int i = 0; i < UPT; ++i)                                      \
        *reinterpret_cast<w4_f32x4*>(Unext + uofs[i] * 4) = ur[i];                       \
  }
  // V = B^T d B of the pair's patch, from Raw to Vnext
  auto transform = [&]() {
    if (CB == 2 || transforms) {
      w4_f32x2 r01[6];
      float r2[6];
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        r01[r] = (w4_f32x2){Raw[rsrc + r * kW4RawW], Raw[rsrc + r * kW4RawW + 1]};
        r2[r] = Raw[rsrc + r * kW4RawW + 2];
      }
      w4_pair_transform(r01, r2, Vnext + vdst);
    }
  };
  // one trip: 9 groups of 4 components
  auto multiply = [&]() {
    w4_mfma_stream<9>(
        acc, [&](int g) { return Ucur + abase + g * 4; }, [&](int g) { return Vcur + bbase + g * 4; });
  };

  // The U slice of a trip is 37 KB (CB = 4): its loads back-pressure at issue for ~1700 cycles (the L2 -> CU
  // path delivers ~16 B/clk), and a wave issues in order -- so they are issued where their waves have slack, right
  // after parking the previous slice during the other waves' transform, not in front of the MFMA phase.
  W4_FETCH_X(0)
  W4_FETCH_U(0)
  W4_STASH_X()
  __syncthreads();
  transform();
  W4_STASH_U()
  if (chunks > 1) W4_FETCH_U(1)
  if (CB == 4 && chunks > 1) W4_FETCH_X(1)
  __syncthreads();
  if (CB == 4) {
    // 64-channel form.  Wave w and wave w + 4 share a SIMD and take turns on its pipes inside a trip:
    //   waves 0-3:  transform(c+1) -> V[next]           then  MFMA(c)
    //   waves 4-7:  MFMA(c)                             then  park U(c+1) -> U[next], issue the loads of U(c+2)
    // so one wave of every SIMD feeds the matrix pipe while its partner runs the VALU / LDS chain (a wave issues
    // in order and does not overlap its own MFMAs with its own VALU work; two waves of a SIMD do).  Two barriers
    // per trip: after the raw patch of trip c+1 is staged, and at the end.  (The first round-2 attempt at such a
    // ping-pong gave every group its own transform and lost: the chain then ran twice per trip.)
    for (int cc = 0; cc < chunks; ++cc) {
      const bool more = cc + 1 < chunks;
      Ucur = Us + (cc & 1) * USZ;
      Vcur = Vs + (cc & 1) * kW4Vsz;
      Unext = Us + ((cc + 1) & 1) * USZ;
      Vnext = Vs + ((cc + 1) & 1) * kW4Vsz;
      if (more) {
        W4_STASH_X()  // X(cc + 1), fetched a trip ago
        if (cc + 2 < chunks) W4_FETCH_X(cc + 2)
      }
      __syncthreads();
      if (transforms) {
        if (more) transform();
        __builtin_amdgcn_s_setprio(1);
        multiply();
        __builtin_amdgcn_s_setprio(0);
      } else {
        __builtin_amdgcn_s_setprio(1);
        multiply();
        __builtin_amdgcn_s_setprio(0);
        if (more) W4_STASH_U()
        if (cc + 2 < chunks) W4_FETCH_U(cc + 2)
      }
      __syncthreads();
    }
  } else {
    // steady state (no conditionals around the activation loads); last trip peeled
    for (int cc = 0; cc + 1 < chunks; ++cc) {
      W4_FETCH_X(cc + 1)
      __builtin_amdgcn_sched_barrier(0);  // keep the loads in flight ahead of the MFMA block
      __builtin_amdgcn_s_setprio(1);  // the matrix phase outranks the co-resident waves' transform VALU
      multiply();
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      __syncthreads();  // every wave is done with U and V of this trip
      W4_STASH_X()
      __syncthreads();
      transform();
      W4_STASH_U()
      if (cc + 2 < chunks) W4_FETCH_U(cc + 2)
      __syncthreads();
    }
    multiply();
  }
#undef W4_FETCH_X
#undef W4_FETCH_U
#undef W4_STASH_X
#undef W4_STASH_U

  // epilogue: lane: tile column lane & 15, channels 4 (lane >> 4) + r of the co block
  w4_f32x4 bv = {0.f, 0.f, 0.f, 0.f};
  const int co0 = ct * CO + cb * 16 + 4 * (lane >> 4);
  if (bias) {
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[r] = bias[co0 + r];
  }
  w4_output_step(acc, bv, n, cout, co0, y0 + 4 * tb, x0 + 4 * (lane & 15), h, w, wv, relu, plane, out);
}

}  // namespace pd3

using namespace pd3;

template <int CB>
static int launch_wino43(const float* x, const float* u_packed, const float* bias, int batch, int cin, int cout,
                         int h, int w, int wv, int relu, float* out, hipStream_t s) {
  constexpr size_t lds = (size_t)((CB == 4 ? 2 : 1) * (CB * kW4Ci * 16 * kW4Cs + kW4Vsz) + kW4RawSz) * sizeof(float);
  int64_t ptiles;
  const int64_t nwg = w4_grid(batch, h, w, cout / (16 * CB), &ptiles);
  if (nwg >= (int64_t)1 << 31) return PD3_EUNSUPPORTED;
  const int rc = launch_lds(conv3x3_winograd43_kernel<CB>, (unsigned)nwg, 128 * CB, lds, s, x, u_packed, bias, out, cin,
                            cout, h, w, wv, relu, (int)ptiles);
  return rc ? rc : launch_status();
}

// channels_per_tile selects the workgroup shape the weights were packed for: 32 (two workgroups per CU) or 64
extern "C" int pd3_conv3x3_winograd43_bias_relu(const float* x, const float* u_packed, const float* bias,
                                                int batch, int cin, int cout, int h, int w, int w_valid,
                                                int relu, float* out, int channels_per_tile, void* stream) {
  if (channels_per_tile != 32 && channels_per_tile != 64) return PD3_EINVAL;
  const int st = w4_check_args(x, u_packed, out, batch, cin, cout, h, w, w_valid, kW4Ci, channels_per_tile);
  if (st != PD3_OK) return st;
  if ((int64_t)cin * h * w >= (int64_t)1 << 31) return PD3_EUNSUPPORTED;  // 32-bit staging offsets
  hipStream_t s = static_cast<hipStream_t>(stream);
  return channels_per_tile == 64 ? launch_wino43<4>(x, u_packed, bias, batch, cin, cout, h, w, w_valid, relu, out, s)
                                 : launch_wino43<2>(x, u_packed, bias, batch, cin, cout, h, w, w_valid, relu, out, s);
}
