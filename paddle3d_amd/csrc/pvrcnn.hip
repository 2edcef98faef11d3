// PV-RCNN's set abstraction on the device: one scale of StackSAModuleMSG.forward (models/common/pointnet2_stack/
// pointnet2_modules.py:31-120) as one kernel, from the ball query to the max pool over nsample, with no
// [M, *, nsample] tensor and no idx in global memory; and interpolate_from_bev_features (models/point_encoders/
// voxel_set_abstraction.py:32-67, 180-213) for all frames in one launch, reading the NCHW map in place.
//
// stack_sa_pool.  The scale's mlp is Conv2d(3 + C -> C1) / BN / ReLU, Conv2d(C1 -> C2) / BN / ReLU.  The first
// convolution is linear in [d; f], so the caller forms features_in = features @ W1[:, 3:]^T once over the n source rows
// and passes w_pos = W1[:, :3]:
//
//   h[s, j]      = relu(scale1[j] * (features_in[row_s, j] + ((w_pos[j,0] * dx + w_pos[j,1] * dy) + w_pos[j,2] * dz))
//                       + shift1[j])                                                                  (no FMA)
//   pooled[m, c] = max_s relu(scale2[c] * (sum_j w2[c, j] * h[s, j]) + shift2[c])                     (no FMA outside the sum)
//
// with row_s = start(frame) + idx[s], idx exactly pd3_ball_query_stack's row (csrc/pointnet2_stack.hip: the frame scan,
// d2 < r2, a NaN is no hit, the first nsample hits in index order), d = xyz[row_s] - new_xyz; a row without a hit
// has features 0 and d 0 (h[j] = relu(shift1[j]), the reference's zeroed grouped tensor).  The sum over j is an
// ascending-j fp32 fmaf chain from 0: what v_mfma_f32_16x16x4_f32 computes, so a VALU fmaf loop gives the same bits
// and the result depends neither on the tiling nor on where a row sits in the launch.  relu(v) = v > 0 ? v : +0 (a NaN
// stays); the max keeps a NaN once it has met one (pd3_voxel_pool's conventions).
//
// One wave per query; a wave walks the queries q = w, w + W, ... of the launch's W waves, so the w2 fragments, scales
// and shifts it holds in registers are loaded once per wave, not once per query.  Query phase: ball_query_stack_kernel's
// (64 of the frame's points per step, __ballot + mbcnt place the hits); a hit lane has the point in registers and
// leaves its row and d in the wave's LDS.  Then per tile of 16 slots: layer 1 with lanes as (sample group g = lane / C1,
// channel j = lane % C1) writes h as a [16, C1] tile into the wave's LDS (row stride C1 + 4 floats: the A-fragment
// reads of 16 rows x 4 consecutive j touch 64 different banks); layer 2 is C1 / 4 steps of
// __builtin_amdgcn_mfma_f32_16x16x4f32 with the 16 slots as M and C2 / 16 independent accumulator tiles as N
// (A[i = lane & 15][k = lane >> 4] = h[i][4 * step + k], B[k][n = lane & 15] = w2[16 * tile + n][4 * step + k];
// D: column lane & 15, rows 4 * (lane >> 4) + reg).  Slots of a tile behind the hits repeat slot 0, which a max does
// not see; the loop ends at the hit count (one slot for a row without a hit).  The max over the slots is over a
// lane's four rows, then __shfl_xor 16 and 32.  Lanes 0..15 store the row, 64 contiguous bytes per accumulator tile.
// The wave's LDS is written and read by that wave alone: a wavefront-scope fence and wave barrier order the phases.
//
// bev_interpolate.  A thread per (keypoint, channel), the channel fastest (the stores of a wave are contiguous):
//   xs = ((x - range_min_x) / voxel_x) / stride, ys likewise (true divisions);
//   x0 = floor(xs), x1 = x0 + 1, both clipped to [0, W - 1] (y to [0, H - 1]) before the weights are formed;
//   wa = (x1 - xs) * (y1 - ys), wb = (x1 - xs) * (ys - y0), wc = (xs - x0) * (y1 - ys), wd = (xs - x0) * (ys - y0);
//   out = ((Ia * wa + Ib * wb) + Ic * wc) + Id * wd, Ia = bev[b, :, y0, x0], Ib = [y1, x0], Ic = [y0, x1], Id = [y1, x1].
// b = the keypoint's first column; not an integer of [0, B): the row is zeros (the reference's mask == k drops it).  A floor outside int32 saturates and a NaN is 0, as in pd3_roi_grid_points.
//
// No FMA but the MFMA chain (-ffp-contract=off), no atomics, 64-bit offsets.
// tests/golden/pv_rcnn_numpy.py restates both in the same order; bev_interpolate equals it bit for bit, and so does
// stack_sa_pool against the restatement's fp32 fmaf-chain form.
#include "common.hpp"
#include "head_math.hpp"
#include "pointnet2_common.hpp"

#include <cmath>

namespace {

using pd3::pn2::ballot_rank;
using pd3::relu_keep_nan;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / pd3::kWave;
constexpr int kMaxBatch = kThreads;  // one count per thread of the prefix
constexpr int kMaxSample = 64;       // a row of idx is one wave's lanes
constexpr int kMaxBlocks = 4096;     // 16 per CU: the waves walk the rest of the queries

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float max_keep_nan(float acc, float v) { return (v > acc || v != v) ? v : acc; }

// The wave's LDS stores before, its LDS loads after.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Inclusive prefix of cnt[0..B) into s[0..B) (B <= kThreads); clamp: negative counts read as 0.  Every thread of the
// workgroup calls it.  (As in pointnet2_stack.hip.)
__device__ void block_prefix(const int* __restrict__ cnt, int B, bool clamp, int64_t* s) {
  const int t = threadIdx.x;
  int64_t v = 0;
  if (t < B) {
    const int c = cnt[t];
    v = clamp && c < 0 ? 0 : c;
  }
  s[t] = v;
  __syncthreads();
  for (int o = 1; o < B; o <<= 1) {
    const int64_t a = t >= o && t < B ? s[t - o] : 0;
    __syncthreads();
    s[t] += a;
    __syncthreads();
  }
}

// The reference's frame scan over an inclusive prefix.
__device__ __forceinline__ int frame_of(int64_t row, const int64_t* incl, int B) {
  for (int k = 0; k < B - 1; ++k)
    if (row < incl[k]) return k;
  return B - 1;
}

template <int C1, int C2>
__global__ __launch_bounds__(kThreads) void stack_sa_pool_kernel(
    const float* __restrict__ new_xyz, const int* __restrict__ new_xyz_batch_cnt, const float* __restrict__ xyz,
    const int* __restrict__ xyz_batch_cnt, const float* __restrict__ features_in, const float* __restrict__ w_pos,
    const float* __restrict__ scale1, const float* __restrict__ shift1, const float* __restrict__ w2,
    const float* __restrict__ scale2, const float* __restrict__ shift2, int B, int m, int n, float r2, int nsample,
    float* __restrict__ pooled) {
  static_assert(C1 == 16 || C1 == 32 || C1 == 64, "lanes are (64 / C1 sample groups) x C1 channels");
  static_assert(C2 == 16 || C2 == 32 || C2 == 64, "C2 / 16 accumulator tiles");
  constexpr int G = 64 / C1;    // sample groups of layer 1
  constexpr int NT = C2 / 16;   // accumulator tiles
  constexpr int KS = C1 / 4;    // MFMA steps
  constexpr int HS = C1 + 4;    // row stride of the h tile
  __shared__ int64_t rows[kMaxBatch], pts[kMaxBatch];
  __shared__ int64_t s_row[kWaves][kMaxSample];
  __shared__ float s_d[kWaves][3][kMaxSample];
  __shared__ float s_h[kWaves][16 * HS];
  block_prefix(new_xyz_batch_cnt, B, false, rows);
  block_prefix(xyz_batch_cnt, B, true, pts);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t stride = (int64_t)gridDim.x * kWaves;
  int64_t q = (int64_t)blockIdx.x * kWaves + wave;
  if (q >= m) return;  // whole waves leave; no block barrier below

  // what the lane keeps for every query: layer 1's channel j, layer 2's fragments of w2 and channels 16 * t + (lane & 15)
  const int j1 = lane % C1, g1 = lane / C1;
  const float p0 = w_pos[3 * j1], p1 = w_pos[3 * j1 + 1], p2 = w_pos[3 * j1 + 2];
  const float sc1 = scale1[j1], sh1 = shift1[j1];
  const int col = lane & 15, kq = lane >> 4;
  float bw[NT][KS], sc2[NT], sh2[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    sc2[t] = scale2[16 * t + col], sh2[t] = shift2[16 * t + col];
#pragma unroll
    for (int k = 0; k < KS; ++k) bw[t][k] = w2[(16 * t + col) * C1 + 4 * k + kq];
  }
  int64_t* my_row = s_row[wave];
  float* my_h = s_h[wave];

  for (; q < m; q += stride) {
    // ---- query: the first nsample hits of the frame's points, rows of xyz and their offsets from the query, into LDS
    const int f = frame_of(q, rows, B);
    const int64_t s0 = f ? pts[f - 1] : 0, e0 = pts[f];
    const int64_t start = s0 < n ? s0 : n, len = (e0 < n ? e0 : n) - start;
    const float* cq = new_xyz + q * 3;
    const float nx = cq[0], ny = cq[1], nz = cq[2];
    const float* p = xyz + start * 3;
    int cnt = 0;
    for (int64_t base = 0; base < len && cnt < nsample; base += 64) {
      const int64_t k = base + lane;
      bool hit = false;
      float dx = 0.f, dy = 0.f, dz = 0.f;
      if (k < len) {
        dx = p[3 * k] - nx, dy = p[3 * k + 1] - ny, dz = p[3 * k + 2] - nz;
        hit = (dx * dx + dy * dy) + dz * dz < r2;  // the squares of ball_query_stack_kernel's (new - x)
      }
      const uint64_t mask = __ballot(hit);
      if (mask == 0) continue;
      const int pos = cnt + ballot_rank(mask);
      if (hit && pos < nsample) {
        my_row[pos] = start + k;
        s_d[wave][0][pos] = dx;
        s_d[wave][1][pos] = dy;
        s_d[wave][2][pos] = dz;
      }
      cnt += __popcll(mask);
    }
    if (cnt > nsample) cnt = nsample;
    wave_lds_sync();

    const int lim = cnt < 1 ? 1 : cnt;
    float best[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) best[t] = 0.f;  // every term is >= +0 (or a NaN): 0 is neutral for the max
    for (int t0 = 0; t0 < lim; t0 += 16) {
      // ---- layer 1: group g over the tile's slots g, g + G, ...; slots behind the hits are slot 0 again
#pragma unroll
      for (int i = g1; i < 16; i += G) {
        float fv = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
        if (cnt > 0) {
          const int ss = t0 + i < cnt ? t0 + i : 0;
          if (features_in) fv = features_in[my_row[ss] * C1 + j1];
          dx = s_d[wave][0][ss], dy = s_d[wave][1][ss], dz = s_d[wave][2][ss];
        }
        my_h[i * HS + j1] = relu_keep_nan(sc1 * (fv + ((p0 * dx + p1 * dy) + p2 * dz)) + sh1);
      }
      wave_lds_sync();
      // ---- layer 2: [16 slots, C1] x [C1, C2] as C1 / 4 MFMA steps into C2 / 16 accumulator tiles
      f32x4 acc[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < KS; ++k) {
        const float a = my_h[col * HS + 4 * k + kq];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bw[t][k], acc[t], 0, 0, 0);
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) best[t] = max_keep_nan(best[t], relu_keep_nan(sc2[t] * acc[t][r] + sh2[t]));
      }
      wave_lds_sync();  // the tile is read before the next one is written
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      best[t] = max_keep_nan(best[t], __shfl_xor(best[t], 16));
      best[t] = max_keep_nan(best[t], __shfl_xor(best[t], 32));
      if (kq == 0) pooled[q * C2 + 16 * t + col] = best[t];
    }
  }
}

// ---- bev_interpolate ------------------------------------------------------------------------------------------------
// float -> int32 as astype('int32') of an in-range value; out of range saturates, a NaN is 0
__device__ __forceinline__ int to_i32(float f) {
  if (f != f) return 0;
  if (f >= 2147483648.f) return INT32_MAX;
  if (f <= -2147483648.f) return INT32_MIN;
  return (int)f;
}

__device__ __forceinline__ int clip(int64_t v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }

__global__ __launch_bounds__(256) void bev_interpolate_kernel(const float* __restrict__ keypoints,
                                                              const float* __restrict__ bev, int64_t total, int B,
                                                              int C, int H, int W, float min_x, float min_y,
                                                              float voxel_x, float voxel_y, float stride,
                                                              float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int64_t row = t / C;
  const int c = (int)(t - row * C);
  const float* kp = keypoints + row * 4;
  const int b = to_i32(kp[0]);
  if (b < 0 || b >= B || (float)b != kp[0]) {  // the reference's mask is keypoints[:, 0] == k
    out[t] = 0.f;
    return;
  }
  const float xs = ((kp[1] - min_x) / voxel_x) / stride, ys = ((kp[2] - min_y) / voxel_y) / stride;
  const int64_t fx = to_i32(floorf(xs)), fy = to_i32(floorf(ys));
  const int x0 = clip(fx, W - 1), x1 = clip(fx + 1, W - 1), y0 = clip(fy, H - 1), y1 = clip(fy + 1, H - 1);
  const float ax = (float)x1 - xs, bx = xs - (float)x0, ay = (float)y1 - ys, by = ys - (float)y0;
  const float wa = ax * ay, wb = ax * by, wc = bx * ay, wd = bx * by;
  const float* im = bev + ((int64_t)b * C + c) * H * W;
  const float Ia = im[(int64_t)y0 * W + x0], Ib = im[(int64_t)y1 * W + x0], Ic = im[(int64_t)y0 * W + x1],
              Id = im[(int64_t)y1 * W + x1];
  out[t] = ((Ia * wa + Ib * wb) + Ic * wc) + Id * wd;
}

template <int C1>
int launch_stack_sa_pool(int c2, dim3 grid, hipStream_t s, const float* new_xyz, const int* new_cnt, const float* xyz,
                         const int* cnt, const float* features_in, const float* w_pos, const float* scale1,
                         const float* shift1, const float* w2, const float* scale2, const float* shift2, int B, int m,
                         int n, float r2, int nsample, float* pooled) {
#define PD3_STACK_SA_POOL(C2)                                                                                        \
  hipLaunchKernelGGL((stack_sa_pool_kernel<C1, C2>), grid, dim3(kThreads), 0, s, new_xyz, new_cnt, xyz, cnt,         \
                     features_in, w_pos, scale1, shift1, w2, scale2, shift2, B, m, n, r2, nsample, pooled)
  if (c2 == 16)
    PD3_STACK_SA_POOL(16);
  else if (c2 == 32)
    PD3_STACK_SA_POOL(32);
  else
    PD3_STACK_SA_POOL(64);
#undef PD3_STACK_SA_POOL
  return pd3::launch_status();
}

}  // namespace

extern "C" {

int pd3_stack_sa_pool(const float* new_xyz, const int* new_xyz_batch_cnt, const float* xyz, const int* xyz_batch_cnt,
                      const float* features_in, const float* w_pos, const float* scale1, const float* shift1,
                      const float* w2, const float* scale2, const float* shift2, int batch, int m, int n, int c1,
                      int c2, float radius, int nsample, float* pooled, void* stream) {
  if (batch < 0 || m < 0 || n < 0 || c1 < 1 || c2 < 1 || nsample < 1) return PD3_EINVAL;
  if ((c1 != 16 && c1 != 32 && c1 != 64) || (c2 != 16 && c2 != 32 && c2 != 64) || nsample > kMaxSample)
    return PD3_EUNSUPPORTED;
  if (m == 0) return PD3_OK;
  if (batch == 0 || !new_xyz || !new_xyz_batch_cnt || !xyz_batch_cnt || !w_pos || !scale1 || !shift1 || !w2 ||
      !scale2 || !shift2 || !pooled || (n > 0 && !xyz))
    return PD3_EINVAL;
  if (batch > kMaxBatch) return PD3_EUNSUPPORTED;
  const float r2 = radius * radius;
  const int64_t blocks = pd3::ceil_div(m, kWaves);
  const dim3 grid((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks));
  hipStream_t s = (hipStream_t)stream;
#define PD3_ARGS                                                                                                     \
  c2, grid, s, new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, features_in, w_pos, scale1, shift1, w2, scale2,      \
      shift2, batch, m, n, r2, nsample, pooled
  if (c1 == 16) return launch_stack_sa_pool<16>(PD3_ARGS);
  if (c1 == 32) return launch_stack_sa_pool<32>(PD3_ARGS);
  return launch_stack_sa_pool<64>(PD3_ARGS);
#undef PD3_ARGS
}

int pd3_bev_interpolate(const float* keypoints, const float* bev, int64_t m, int batch, int channels, int h, int w,
                        float range_min_x, float range_min_y, float voxel_x, float voxel_y, float stride, float* out,
                        void* stream) {
  if (m < 0 || batch < 0 || channels < 0 || h < 0 || w < 0) return PD3_EINVAL;
  const int64_t total = m * channels;
  if (total == 0) return PD3_OK;
  if (!keypoints || !out) return PD3_EINVAL;
  if (batch > 0 && (h == 0 || w == 0)) return PD3_EINVAL;  // a frame to read and no cell in it
  if (batch > 0 && !bev) return PD3_EINVAL;
  const int64_t blocks = pd3::ceil_div(total, 256);
  if (blocks > INT32_MAX) return PD3_EUNSUPPORTED;
  hipLaunchKernelGGL(bev_interpolate_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, keypoints, bev,
                     total, batch, channels, h, w, range_min_x, range_min_y, voxel_x, voxel_y, stride, out);
  return pd3::launch_status();
}

}  // extern "C"
