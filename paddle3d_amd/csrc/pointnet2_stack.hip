// pointnet2 stack ops: the custom operators PV-RCNN's StackSAModuleMSG and Voxel R-CNN's NeighborVoxelSAModuleMSG call.
//
//   ball_query_stack          PD_BUILD_OP(ball_query_stack), pointnet2_stack/ball_query_stack.cc:73,
//                             ball_query_gpu_stack.cu:26-81
//   voxel_query_wrapper       PD_BUILD_OP(voxel_query_wrapper), pointnet2/voxel_query.cc:78, voxel_query_gpu.cu:11-93
//   grouping_operation_stack  PD_BUILD_OP / PD_BUILD_GRAD_OP(grouping_operation_stack),
//                             pointnet2_stack/group_points_stack.cc:117-130, group_points_gpu_stack.cu:26-131
//
// Rows of a stacked batch belong to frames by counts that stay on the device.  Every workgroup loads the counts into
// LDS and forms their inclusive prefix there (kMaxBatch frames at most; more is PD3_EUNSUPPORTED).  A row's frame is
// the reference's scan (ball_query_gpu_stack.cu:37-42): the first k < B - 1 with row < cnt[0] + ... + cnt[k], else
// B - 1; a frame with count 0 is never picked, rows past the total go to frame B - 1.  Prefix sums are 64-bit.
// tests/golden/pointnet2_stack_numpy.py restates every op in the same order; the device results equal it bit for bit
// (the backward up to the order of its float atomics).
//
// ball_query_stack: one wave per query, 64 of the frame's points per step, __ballot + mbcnt place the hits in index
// order, the wave leaves at nsample hits.  Hit: ((new_x - x)^2 + (new_y - y)^2) + (new_z - z)^2 < r2 (a NaN is no
// hit).  The frame's point range is [sum of the earlier counts, + its count), negative counts read as 0 and the range
// is clamped into [0, N) (the reference reads outside xyz there).  Indices are local to the frame.
//
// voxel_query: one wave per query, lanes over the flattened (2zr+1)(2yr+1)(2xr+1) window in (dz, dy, dx) order, 64
// cells per step, __ballot + mbcnt, the wave leaves at nsample hits (the reference scans on, but its cnt2 is unused).
// Hit: !(((x - new_x)^2 + (y - new_y)^2) + (z - new_z)^2 > r2): the sphere's surface and a NaN distance are hits.
// Cells outside the grid, a batch index outside [0, B), point_indices < 0 and point_indices >= N are skipped.
// Indices are rows of xyz.
//
// Both queries: unused slots repeat the first hit; a row without a hit is [-1, 0, 0, ...] (the reference starts
// from paddle::full(0) and writes idx[0] = -1).
//
// grouping forward: a thread per (row, sample) reads its index once and serves every channel, 16-byte feature reads
// when C % 4 == 0.  out[m, c, s] = features[start(frame(m)) + idx[m, s], c]; a global row outside [0, N) reads as 0.
// Backward: grad_features zeroed in stream order, then a thread per (row, sample, channel), channel fastest, adds
// with float atomics: one wave-instruction adds to whole feature rows (last bits may vary from run to run, as the
// reference's do).  A global row outside [0, N) adds nothing.
//
// All offsets are 64-bit.
#include "common.hpp"
#include "pointnet2_common.hpp"

namespace {

using pd3::pn2::ballot_rank;
using pd3::pn2::dist3;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / pd3::kWave;
constexpr int kMaxBatch = kThreads;  // one count per thread of the prefix

// Inclusive prefix of cnt[0..B) into s[0..B) (B <= kThreads); clamp: negative counts read as 0.  Every thread of the
// workgroup calls it.
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

// Fill of a query row after its hits: slots [cnt, nsample) repeat `first`, a row without a hit is [-1, 0, ...].
__device__ __forceinline__ void fill_row(int* out, int cnt, int first, int nsample, int lane) {
  for (int l = (cnt < nsample ? cnt : nsample) + lane; l < nsample; l += 64) out[l] = cnt == 0 && l == 0 ? -1 : first;
}

// ---- ball_query_stack ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ball_query_stack_kernel(const float* __restrict__ new_xyz,
                                                                    const int* __restrict__ new_xyz_batch_cnt,
                                                                    const float* __restrict__ xyz,
                                                                    const int* __restrict__ xyz_batch_cnt, int B,
                                                                    int m, int n, float r2, int nsample,
                                                                    int* __restrict__ idx) {
  __shared__ int64_t rows[kMaxBatch], pts[kMaxBatch];
  block_prefix(new_xyz_batch_cnt, B, false, rows);
  block_prefix(xyz_batch_cnt, B, true, pts);
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (q >= m) return;  // whole waves leave
  const int f = frame_of(q, rows, B);
  const int64_t s0 = f ? pts[f - 1] : 0, e0 = pts[f];
  const int64_t start = s0 < n ? s0 : n, len = (e0 < n ? e0 : n) - start;
  const float* c = new_xyz + q * 3;
  const float nx = c[0], ny = c[1], nz = c[2];
  const float* p = xyz + start * 3;
  int* out = idx + q * nsample;
  int cnt = 0, first = 0;
  for (int64_t base = 0; base < len && cnt < nsample; base += 64) {
    const int64_t k = base + lane;
    bool hit = false;
    if (k < len) {
      const float x = p[3 * k], y = p[3 * k + 1], z = p[3 * k + 2];
      hit = dist3(x, y, z, nx, ny, nz) < r2;  // (new_x - x)^2 ... as ball_query_gpu_stack.cu:64-66
    }
    const uint64_t mask = __ballot(hit);
    if (mask == 0) continue;
    if (cnt == 0) first = (int)base + __ffsll((unsigned long long)mask) - 1;
    const int pos = cnt + ballot_rank(mask);
    if (hit && pos < nsample) out[pos] = (int)k;
    cnt += __popcll(mask);
  }
  fill_row(out, cnt, first, nsample, lane);
}

// ---- voxel_query ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void voxel_query_kernel(const float* __restrict__ new_xyz,
                                                               const float* __restrict__ xyz,
                                                               const int* __restrict__ new_coords,
                                                               const int* __restrict__ point_indices, int m, int n,
                                                               int B, int Z, int Y, int X, float r2, int nsample,
                                                               int zr, int yr, int xr, int* __restrict__ idx) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (q >= m) return;
  const float* c = new_xyz + q * 3;
  const float nx = c[0], ny = c[1], nz = c[2];
  const int* co = new_coords + q * 4;
  const int b = co[0], cz = co[1], cy = co[2], cx = co[3];
  int* out = idx + q * nsample;
  const int wx = 2 * xr + 1, wyx = (2 * yr + 1) * wx, win = zr < 0 ? 0 : (2 * zr + 1) * wyx;
  int cnt = 0, first = 0;
  if (b >= 0 && b < B) {
    const int* grid = point_indices + (int64_t)b * Z * Y * X;
    for (int base = 0; base < win && cnt < nsample; base += 64) {
      const int w = base + lane;
      bool hit = false;
      int ni = -1;
      if (w < win) {
        const int64_t z = (int64_t)cz + w / wyx - zr, y = (int64_t)cy + (w % wyx) / wx - yr,
                      x = (int64_t)cx + w % wx - xr;
        if (z >= 0 && z < Z && y >= 0 && y < Y && x >= 0 && x < X) {
          ni = grid[(z * Y + y) * X + x];
          if (ni >= 0 && ni < n) {
            const float px = xyz[3 * (int64_t)ni], py = xyz[3 * (int64_t)ni + 1], pz = xyz[3 * (int64_t)ni + 2];
            hit = !(dist3(nx, ny, nz, px, py, pz) > r2);  // (x_per - new_x)^2 ... as voxel_query_gpu.cu:60-64
          }
        }
      }
      const uint64_t mask = __ballot(hit);
      if (mask == 0) continue;
      if (cnt == 0) first = __shfl(ni, __ffsll((unsigned long long)mask) - 1);
      const int pos = cnt + ballot_rank(mask);
      if (hit && pos < nsample) out[pos] = ni;
      cnt += __popcll(mask);
    }
  }
  fill_row(out, cnt, first, nsample, lane);
}

// ---- grouping_operation_stack --------------------------------------------------------------------------------------
template <bool kVec4>
__global__ __launch_bounds__(kThreads) void group_stack_fwd_kernel(const float* __restrict__ features,
                                                                   const int* __restrict__ features_batch_cnt,
                                                                   const int* __restrict__ idx,
                                                                   const int* __restrict__ idx_batch_cnt, int B,
                                                                   int n, int C, int nsample, int64_t pairs,
                                                                   float* __restrict__ out) {
  __shared__ int64_t rows[kMaxBatch], feats[kMaxBatch];
  block_prefix(idx_batch_cnt, B, false, rows);
  block_prefix(features_batch_cnt, B, false, feats);
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= pairs) return;
  const int64_t row = e / nsample, s = e - row * nsample;
  const int f = frame_of(row, rows, B);
  const int64_t g = (f ? feats[f - 1] : 0) + idx[e];
  const bool ok = g >= 0 && g < n;
  const float* src = features + (ok ? g : 0) * C;
  float* dst = out + row * C * nsample + s;
  int c = 0;
  if constexpr (kVec4) {
    for (; c + 4 <= C; c += 4) {
      const float4 v = ok ? *reinterpret_cast<const float4*>(src + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      dst[(int64_t)c * nsample] = v.x;
      dst[(int64_t)(c + 1) * nsample] = v.y;
      dst[(int64_t)(c + 2) * nsample] = v.z;
      dst[(int64_t)(c + 3) * nsample] = v.w;
    }
  }
  for (; c < C; ++c) dst[(int64_t)c * nsample] = ok ? src[c] : 0.f;
}

__global__ __launch_bounds__(kThreads) void group_stack_bwd_kernel(const float* __restrict__ grad_out,
                                                                   const int* __restrict__ idx,
                                                                   const int* __restrict__ idx_batch_cnt,
                                                                   const int* __restrict__ features_batch_cnt, int B,
                                                                   int n, int C, int nsample, int64_t total,
                                                                   float* __restrict__ grad_features) {
  __shared__ int64_t rows[kMaxBatch], feats[kMaxBatch];
  block_prefix(idx_batch_cnt, B, false, rows);
  block_prefix(features_batch_cnt, B, false, feats);
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  const int64_t e = t / C, c = t - e * C;  // e = row * nsample + s
  const int64_t row = e / nsample, s = e - row * nsample;
  const int f = frame_of(row, rows, B);
  const int64_t g = (f ? feats[f - 1] : 0) + idx[e];
  if (g < 0 || g >= n) return;
  unsafeAtomicAdd(grad_features + g * C + c, grad_out[(row * C + c) * nsample + s]);
}

}  // namespace

extern "C" {

int pd3_ball_query_stack(const float* new_xyz, const int* new_xyz_batch_cnt, const float* xyz,
                         const int* xyz_batch_cnt, int batch, int m, int n, float radius, int nsample, int* idx,
                         void* stream) {
  if (batch < 0 || m < 0 || n < 0 || nsample < 1) return PD3_EINVAL;
  if (m == 0) return PD3_OK;
  if (batch == 0 || !new_xyz || !new_xyz_batch_cnt || !xyz_batch_cnt || !idx || (n > 0 && !xyz)) return PD3_EINVAL;
  if (batch > kMaxBatch) return PD3_EUNSUPPORTED;
  const float r2 = radius * radius;
  hipLaunchKernelGGL(ball_query_stack_kernel, dim3((unsigned)pd3::ceil_div(m, kWaves)), dim3(kThreads), 0,
                     (hipStream_t)stream, new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, batch, m, n, r2, nsample,
                     idx);
  return pd3::launch_status();
}

int pd3_voxel_query(const float* new_xyz, const float* xyz, const int* new_coords, const int* point_indices, int m,
                    int n, int batch, int z, int y, int x, float radius, int nsample, int z_range, int y_range,
                    int x_range, int* idx, void* stream) {
  if (m < 0 || n < 0 || batch < 0 || z < 0 || y < 0 || x < 0 || nsample < 1) return PD3_EINVAL;
  if (m == 0) return PD3_OK;
  if (batch == 0 || !new_xyz || !new_coords || !idx || (n > 0 && !xyz)) return PD3_EINVAL;
  if ((int64_t)batch * z * y * x > 0 && !point_indices) return PD3_EINVAL;
  // a negative range is an empty loop in the reference: no cell, every row without a hit
  const bool empty = z_range < 0 || y_range < 0 || x_range < 0;
  if (!empty && (2 * (int64_t)z_range + 1) * (2 * (int64_t)y_range + 1) * (2 * (int64_t)x_range + 1) > INT32_MAX - 64)
    return PD3_EUNSUPPORTED;
  if (empty) z_range = y_range = x_range = -1;  // window of 0 cells below
  const float r2 = radius * radius;
  hipLaunchKernelGGL(voxel_query_kernel, dim3((unsigned)pd3::ceil_div(m, kWaves)), dim3(kThreads), 0,
                     (hipStream_t)stream, new_xyz, xyz, new_coords, point_indices, m, n, batch, z, y, x, r2, nsample,
                     z_range, y_range, x_range, idx);
  return pd3::launch_status();
}

int pd3_group_points_stack(const float* features, const int* features_batch_cnt, const int* idx,
                           const int* idx_batch_cnt, int batch, int n, int channels, int m, int nsample, float* out,
                           void* stream) {
  if (batch < 0 || n < 0 || channels < 0 || m < 0 || nsample < 1) return PD3_EINVAL;
  const int64_t pairs = (int64_t)m * nsample;
  if (pairs == 0 || channels == 0) return PD3_OK;
  if (batch == 0 || !features_batch_cnt || !idx || !idx_batch_cnt || !out || (n > 0 && !features)) return PD3_EINVAL;
  if (batch > kMaxBatch) return PD3_EUNSUPPORTED;
  const int64_t blocks = pd3::ceil_div(pairs, kThreads);
  if (blocks > INT32_MAX) return PD3_EUNSUPPORTED;
  // 16-byte rows: C % 4 == 0 and a 16-byte aligned base
  const bool vec4 = channels % 4 == 0 && ((uintptr_t)features & 15) == 0;
  if (vec4)
    hipLaunchKernelGGL(group_stack_fwd_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream,
                       features, features_batch_cnt, idx, idx_batch_cnt, batch, n, channels, nsample, pairs, out);
  else
    hipLaunchKernelGGL(group_stack_fwd_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream,
                       features, features_batch_cnt, idx, idx_batch_cnt, batch, n, channels, nsample, pairs, out);
  return pd3::launch_status();
}

int pd3_group_points_stack_grad(const float* grad_out, const int* idx, const int* idx_batch_cnt,
                                const int* features_batch_cnt, int batch, int n, int channels, int m, int nsample,
                                float* grad_features, void* stream) {
  if (batch < 0 || n < 0 || channels < 0 || m < 0 || nsample < 1) return PD3_EINVAL;
  if (n == 0 || channels == 0) return PD3_OK;
  if (!grad_features) return PD3_EINVAL;
  const int64_t total = (int64_t)m * nsample * channels;
  if (total > 0 && (batch == 0 || !grad_out || !idx || !idx_batch_cnt || !features_batch_cnt)) return PD3_EINVAL;
  if (batch > kMaxBatch) return PD3_EUNSUPPORTED;
  const int64_t blocks = pd3::ceil_div(total, kThreads);
  if (blocks > INT32_MAX) return PD3_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(grad_features, 0, (size_t)n * channels * sizeof(float), s) != hipSuccess)
    return pd3::launch_status();
  if (total == 0) return PD3_OK;
  hipLaunchKernelGGL(group_stack_bwd_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, grad_out, idx,
                     idx_batch_cnt, features_batch_cnt, batch, n, channels, nsample, total, grad_features);
  return pd3::launch_status();
}

}  // extern "C"
