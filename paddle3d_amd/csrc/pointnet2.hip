// pointnet2 batch ops and points_in_boxes: the custom operators IA-SSD calls.
//
//   farthest_point_sample   PD_BUILD_OP(farthest_point_sample), pointnet2/sampling.cc:62, sampling_gpu.cu:37-149
//   gather_operation        PD_BUILD_OP / PD_BUILD_GRAD_OP(gather_operation), gather_points.cc:100-110,
//                           gather_points_gpu.cu:25, 69
//   ball_query_batch        PD_BUILD_OP(ball_query_batch), pointnet2_batch/ball_query_batch.cc:61,
//                           ball_query_gpu_batch.cu:20-61
//   grouping_operation_batch  PD_BUILD_OP / PD_BUILD_GRAD_OP(grouping_operation_batch), group_points_batch.cc:95-106,
//                           group_points_gpu_batch.cu:25, 74
//   points_in_boxes_gpu     PD_BUILD_OP(points_in_boxes_gpu), roiaware_pool3d/box_utils.cc:65, box_utils_gpu.cu:28-78
//
// Every distance is ((dx*dx + dy*dy) + dz*dz) in fp32 with dx = x2 - x1 in the reference's operand order; the build
// has -ffp-contract=off, so no FMA.  tests/golden/pointnet2_numpy.py restates every op in the same order and the
// device results equal it bit for bit (the backward ops up to the order of their float atomics).
//
// FPS (one workgroup per frame).  Each lane owns the points k = tid + c*T, c = 0, 1, ... (T = threads of
// the workgroup) and keeps their running minimum distance in VGPRs.  Per iteration: every lane updates its own points
// and keeps its first maximum (strict >, c ascending), forms a 64-bit key = (distance bits << 32) | ~order(k), the wave
// max-reduces the keys with __shfl_xor, the wave's winning lane publishes {key, x, y, z} to an LDS slot of the
// iteration's parity, one barrier, and every wave reduces the slots itself.  The centre's coordinates travel with the
// key: no dependent global load per iteration.  order(k) = (bitrev_L(k mod bs) << 22) | (k >> L), bs = 2^L =
// min(2^floor(log2 n), 1024) the reference's thread count: the reference's per-thread scan and its left-biased tree
// pick, among equal maximum distances, the smallest (bitrev_L(k mod bs), k).  T = 1024 whenever n > 1024 (then
// bs = T, so a lane's own points are in the reference's order); for n <= 1024 a lane owns one point.
//   Register tier (R = 1, 2, 4, 8, 16 points per lane, n <= 16384): coordinates and minima in VGPRs for the whole run.
//   General tier (n <= 2^24): the minima of the first 64 slots per lane (n <= 65536) in VGPRs, the rest in the caller's
//   workspace; coordinates re-read from global memory (L2) every iteration.
//
// ball_query_batch: one wave per query, 64 consecutive points per step, __ballot + mbcnt place each hit in index
// order, the wave leaves once nsample hits are found.  Rows without a hit are 0 (the reference leaves them undefined).
//
// gather / grouping forward: a thread per (point, sample) reads its index once and serves every channel; stores are
// coalesced along npoint*nsample.  Indices outside [0, N) read as 0.  Backward: grad_points zeroed in stream order,
// then float atomic adds (last bits may vary from run to run, as the reference's do); indices outside [0, N) add
// nothing.  gather_operation is grouping with nsample = 1.
//
// points_in_boxes: a thread per point, boxes staged in LDS 256 at a time with cosf / sinf(-rz) (glibc's bits,
// libm_exact.hpp); the first box in index order that holds the point wins, -1 otherwise.  The z test and the
// |local| < d / 2.0 + MARGIN tests in double, local_x / local_y in fp32, as box_utils_gpu.cu:28-45 has them.
//
// All offsets are 64-bit.
#include <cmath>

#include "common.hpp"
#include "libm_exact.hpp"
#include "pointnet2_common.hpp"

namespace {

using pd3::pn2::dist3;

constexpr int kFpsThreads = 1024;
constexpr int kFpsWaves = kFpsThreads / pd3::kWave;
constexpr int kFpsRegMax = 16;   // register tier: points per lane (n <= 16384)
constexpr int kFpsGenRegs = 64;  // general tier: minima per lane kept in VGPRs (n <= 65536 without workspace)
constexpr int kFpsMaxN = 1 << 24;

struct FpsSlot {
  uint64_t key;
  float x, y, z, pad;
};

__device__ __forceinline__ uint32_t fps_order(uint32_t k, int lg) {
  const uint32_t t = k & ((1u << lg) - 1u);
  const uint32_t rank = lg ? (__brev(t) >> (32 - lg)) : 0u;
  return ~((rank << 22) | (k >> lg));
}

__device__ __forceinline__ uint32_t fps_index(uint64_t key, int lg) {
  const uint32_t o = ~(uint32_t)key;
  const uint32_t rank = o >> 22, q = o & 0x3FFFFFu;
  const uint32_t t = lg ? (__brev(rank) >> (32 - lg)) : 0u;
  return (q << lg) | t;
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t w = __shfl_xor(v, o);
    v = w > v ? w : v;
  }
  return v;
}

// R: points (register tier) or minima (general tier) per lane held in VGPRs.
template <int R, bool kGeneral>
__global__ __launch_bounds__(kFpsThreads) void fps_kernel(const float* __restrict__ xyz, int n, int m, int lg,
                                                          float* __restrict__ ws, int64_t ws_per_frame,
                                                          int* __restrict__ idxs) {
  __shared__ FpsSlot slots[2][kFpsWaves];
  const int T = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = T >> 6;
  const float* p = xyz + (int64_t)blockIdx.x * n * 3;
  int* out = idxs + (int64_t)blockIdx.x * m;
  const int C = (n + T - 1) / T;  // slots in use per lane
  float t[R];
  float px[kGeneral ? 1 : R], py[kGeneral ? 1 : R], pz[kGeneral ? 1 : R];
#pragma unroll
  for (int c = 0; c < R; ++c) {
    const int k = c * T + tid;
    const bool ok = k < n;
    t[c] = ok ? 1e10f : -1.f;  // -1: no point; fminf(d, -1) stays -1 and never wins
    if constexpr (!kGeneral) {
      px[c] = ok ? p[3 * (int64_t)k] : 0.f;
      py[c] = ok ? p[3 * (int64_t)k + 1] : 0.f;
      pz[c] = ok ? p[3 * (int64_t)k + 2] : 0.f;
    }
  }
  float* wt = nullptr;
  if constexpr (kGeneral) {
    wt = ws + (int64_t)blockIdx.x * ws_per_frame;
    for (int c = R; c < C; ++c) {
      const int k = c * T + tid;
      if (k < n) wt[(int64_t)(c - R) * T + tid] = 1e10f;
    }
  }
  float cx = p[0], cy = p[1], cz = p[2];
  if (tid == 0) out[0] = 0;
  for (int j = 1; j < m; ++j) {
    float best = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
    int bc = 0;
    // general tier: the lane's coordinate offset is re-derived every iteration, so the compiler cannot hoist 64
    // per-slot addresses out of the j loop (they would not fit next to the 64 minima)
    uint32_t off0 = 3u * (uint32_t)tid;
    if constexpr (kGeneral) asm volatile("" : "+v"(off0));
#pragma unroll
    for (int c = 0; c < R; ++c) {
      if (kGeneral && c >= C) continue;  // uniform; no early exit, so the loop unrolls and t[] stays in VGPRs
      float x, y, z;
      if constexpr (kGeneral) {
        const bool ok = c * T + tid < n;
        const uint32_t o = off0 + 3u * (uint32_t)(c * T);  // < 3 * 2^24: 32-bit offsets from the frame's base
        x = ok ? p[o] : 0.f;
        y = ok ? p[o + 1] : 0.f;
        z = ok ? p[o + 2] : 0.f;
      } else {
        x = px[c];
        y = py[c];
        z = pz[c];
      }
      t[c] = fminf(dist3(cx, cy, cz, x, y, z), t[c]);
      if (t[c] > best) {
        best = t[c];
        bc = c;
        bx = x;
        by = y;
        bz = z;
      }
    }
    if constexpr (kGeneral) {
      for (int c = R; c < C; ++c) {
        const int k = c * T + tid;
        if (k >= n) break;
        const float x = p[3 * (int64_t)k], y = p[3 * (int64_t)k + 1], z = p[3 * (int64_t)k + 2];
        float* tp = wt + (int64_t)(c - R) * T + tid;
        const float d2 = fminf(dist3(cx, cy, cz, x, y, z), *tp);
        *tp = d2;
        if (d2 > best) {
          best = d2;
          bc = c;
          bx = x;
          by = y;
          bz = z;
        }
      }
    }
    const uint64_t key =
        best >= 0.f ? ((uint64_t)__float_as_uint(best) << 32) | fps_order((uint32_t)(bc * T + tid), lg) : 0ull;
    const uint64_t wmax = wave_max_u64(key);
    const uint64_t hit = __ballot(key == wmax);
    FpsSlot* s = slots[j & 1];
    if (lane == __ffsll((unsigned long long)hit) - 1) s[wave] = FpsSlot{key, bx, by, bz, 0.f};
    __syncthreads();
    FpsSlot win = s[0];
    for (int w = 1; w < W; ++w) {
      const FpsSlot o = s[w];
      if (o.key > win.key) win = o;
    }
    cx = win.x;
    cy = win.y;
    cz = win.z;
    if (tid == 0) out[j] = (int)fps_index(win.key, lg);
  }
}

template <int R>
void launch_fps_reg(const float* xyz, int b, int n, int m, int lg, int threads, int* idxs, hipStream_t s) {
  hipLaunchKernelGGL((fps_kernel<R, false>), dim3(b), dim3(threads), 0, s, xyz, n, m, lg, nullptr, (int64_t)0, idxs);
}

int fps_lg(int n) {  // floor(log2 n) of the reference's opt_n_threads, capped at 10
  int lg = 31 - __builtin_clz((unsigned)n);
  return lg > 10 ? 10 : lg;
}

int64_t fps_ws_per_frame(int n) {  // floats of workspace per frame in the general tier
  const int64_t C = ((int64_t)n + kFpsThreads - 1) / kFpsThreads;
  return C > kFpsGenRegs ? (C - kFpsGenRegs) * kFpsThreads : 0;
}

// ---- gather / grouping ------------------------------------------------------------------------------------------
constexpr int kGroupThreads = 256;

__global__ __launch_bounds__(kGroupThreads) void group_fwd_kernel(const float* __restrict__ points,
                                                                  const int* __restrict__ idx, int C, int n,
                                                                  int64_t pairs, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * kGroupThreads + threadIdx.x;
  if (e >= pairs) return;
  const int64_t b = blockIdx.y;
  const int k = idx[b * pairs + e];
  const bool ok = k >= 0 && k < n;
  const float* src = points + b * C * (int64_t)n + (ok ? k : 0);
  float* dst = out + b * C * pairs + e;
  int c = 0;
  for (; c + 4 <= C; c += 4) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = ok ? src[(int64_t)(c + u) * n] : 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) dst[(int64_t)(c + u) * pairs] = v[u];
  }
  for (; c < C; ++c) dst[(int64_t)c * pairs] = ok ? src[(int64_t)c * n] : 0.f;
}

__global__ __launch_bounds__(kGroupThreads) void group_bwd_kernel(const float* __restrict__ grad_out,
                                                                  const int* __restrict__ idx, int C, int n,
                                                                  int64_t pairs, float* __restrict__ grad_points) {
  const int64_t e = (int64_t)blockIdx.x * kGroupThreads + threadIdx.x;
  if (e >= pairs) return;
  const int64_t b = blockIdx.y;
  const int k = idx[b * pairs + e];
  if (k < 0 || k >= n) return;
  const float* src = grad_out + b * C * pairs + e;
  float* dst = grad_points + b * C * (int64_t)n + k;
  for (int c = 0; c < C; ++c) unsafeAtomicAdd(dst + (int64_t)c * n, src[(int64_t)c * pairs]);
}

int group_fwd(const float* points, const int* idx, int b, int c, int n, int64_t pairs, float* out, hipStream_t s) {
  if (b == 0 || c == 0 || pairs == 0) return PD3_OK;
  const int64_t blocks = pd3::ceil_div(pairs, kGroupThreads);
  if (blocks > INT32_MAX || b > 65535) return PD3_EUNSUPPORTED;
  hipLaunchKernelGGL(group_fwd_kernel, dim3((unsigned)blocks, b), dim3(kGroupThreads), 0, s, points, idx, c, n, pairs,
                     out);
  return pd3::launch_status();
}

int group_bwd(const float* grad_out, const int* idx, int b, int c, int n, int64_t pairs, float* grad_points,
              hipStream_t s) {
  if (b == 0 || c == 0 || n == 0) return PD3_OK;
  const int64_t blocks = pd3::ceil_div(pairs, kGroupThreads);
  if (blocks > INT32_MAX || b > 65535) return PD3_EUNSUPPORTED;
  if (hipMemsetAsync(grad_points, 0, (size_t)b * c * n * sizeof(float), s) != hipSuccess) return pd3::launch_status();
  if (pairs == 0) return PD3_OK;
  hipLaunchKernelGGL(group_bwd_kernel, dim3((unsigned)blocks, b), dim3(kGroupThreads), 0, s, grad_out, idx, c, n,
                     pairs, grad_points);
  return pd3::launch_status();
}

// ---- ball_query_batch --------------------------------------------------------------------------------------------
constexpr int kBqThreads = 256;
constexpr int kBqWaves = kBqThreads / pd3::kWave;

__global__ __launch_bounds__(kBqThreads) void ball_query_kernel(const float* __restrict__ new_xyz,
                                                                const float* __restrict__ xyz, int n, int m,
                                                                float r2, int nsample, int* __restrict__ idx) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * kBqWaves + (threadIdx.x >> 6);
  if (q >= m) return;  // whole waves leave
  const int64_t b = blockIdx.y;
  const float* c = new_xyz + (b * m + q) * 3;
  const float nx = c[0], ny = c[1], nz = c[2];
  const float* p = xyz + b * n * 3;
  int* out = idx + (b * m + q) * nsample;
  int cnt = 0, first = 0;
  for (int base = 0; base < n && cnt < nsample; base += 64) {
    const int k = base + lane;
    bool hit = false;
    if (k < n) {
      const float x = p[3 * (int64_t)k], y = p[3 * (int64_t)k + 1], z = p[3 * (int64_t)k + 2];
      hit = dist3(x, y, z, nx, ny, nz) < r2;  // (new_x - x)^2 ... as ball_query_gpu_batch.cu:42-43
    }
    const uint64_t mask = __ballot(hit);
    if (mask == 0) continue;
    if (cnt == 0) first = base + __ffsll((unsigned long long)mask) - 1;
    const int pos = cnt + pd3::pn2::ballot_rank(mask);
    if (hit && pos < nsample) out[pos] = k;
    cnt += __popcll(mask);
  }
  for (int l = (cnt < nsample ? cnt : nsample) + lane; l < nsample; l += 64) out[l] = first;
}

// ---- points_in_boxes ---------------------------------------------------------------------------------------------
constexpr int kPibThreads = 256;
constexpr float kPibMargin = 1e-5f;  // box_utils_gpu.cu:27, a float promoted to double in the tests

struct PibBox {
  double hz, hx, hy;  // dz / 2.0, dx / 2.0 + MARGIN, dy / 2.0 + MARGIN
  float cx, cy, cz, cosa, sina, pad;
};

__global__ __launch_bounds__(kPibThreads) void points_in_boxes_kernel(const float* __restrict__ pts,
                                                                      const float* __restrict__ boxes, int npts,
                                                                      int nboxes, int64_t row_stride,
                                                                      int64_t batch_stride, int* __restrict__ out) {
  __shared__ PibBox sb[kPibThreads];
  const int64_t b = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * kPibThreads + threadIdx.x;
  const bool active = i < npts;
  float x = 0.f, y = 0.f, z = 0.f;
  if (active) {
    x = pts[(b * npts + i) * 3];
    y = pts[(b * npts + i) * 3 + 1];
    z = pts[(b * npts + i) * 3 + 2];
  }
  int found = -1;
  const float* bb = boxes + b * batch_stride;
  for (int base = 0; base < nboxes; base += kPibThreads) {
    const int cnt = nboxes - base < kPibThreads ? nboxes - base : kPibThreads;
    __syncthreads();  // the previous chunk is consumed
    if ((int)threadIdx.x < cnt) {
      const float* r = bb + (int64_t)(base + threadIdx.x) * row_stride;
      PibBox s;
      s.cx = r[0];
      s.cy = r[1];
      s.cz = r[2];
      s.hx = (double)r[3] / 2.0 + (double)kPibMargin;
      s.hy = (double)r[4] / 2.0 + (double)kPibMargin;
      s.hz = (double)r[5] / 2.0;
      s.cosa = pd3::lm::cosf(-r[6]);
      s.sina = pd3::lm::sinf(-r[6]);
      s.pad = 0.f;
      sb[threadIdx.x] = s;
    }
    __syncthreads();
    if (active && found < 0) {
      for (int k = 0; k < cnt; ++k) {
        const PibBox& s = sb[k];
        if ((double)fabsf(z - s.cz) > s.hz) continue;
        const float sx = x - s.cx, sy = y - s.cy;
        const float lx = sx * s.cosa + sy * (-s.sina);
        const float ly = sx * s.sina + sy * s.cosa;
        if ((double)fabsf(lx) < s.hx && (double)fabsf(ly) < s.hy) {
          found = base + k;
          break;
        }
      }
    }
  }
  if (active) out[b * npts + i] = found;
}

}  // namespace

extern "C" {

size_t pd3_farthest_point_sample_workspace(int batch, int n, int tier) {
  if (batch < 0 || n < 0 || n > kFpsMaxN) return 0;
  const bool general = tier == 2 || (tier == 0 && n > kFpsRegMax * kFpsThreads);
  return general ? (size_t)batch * (size_t)fps_ws_per_frame(n) * sizeof(float) : 0;
}

int pd3_farthest_point_sample(const float* xyz, int batch, int n, int m, int tier, void* workspace,
                              size_t workspace_bytes, int* idxs, void* stream) {
  if (batch < 0 || n < 0 || tier < 0 || tier > 2) return PD3_EINVAL;
  if (batch == 0 || m <= 0) return PD3_OK;
  if (n == 0 || !xyz || !idxs) return PD3_EINVAL;
  if (n > kFpsMaxN || batch > INT32_MAX / 2) return PD3_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int lg = fps_lg(n);
  const bool general = tier == 2 || (tier == 0 && n > kFpsRegMax * kFpsThreads);
  if (!general) {
    if (n > kFpsRegMax * kFpsThreads) return PD3_EUNSUPPORTED;
    const int threads = n > kFpsThreads ? kFpsThreads : (int)pd3::ceil_div(n, 64) * 64;
    const int per = (int)pd3::ceil_div(n, kFpsThreads);
    if (per <= 1) launch_fps_reg<1>(xyz, batch, n, m, lg, threads, idxs, s);
    else if (per <= 2) launch_fps_reg<2>(xyz, batch, n, m, lg, threads, idxs, s);
    else if (per <= 4) launch_fps_reg<4>(xyz, batch, n, m, lg, threads, idxs, s);
    else if (per <= 8) launch_fps_reg<8>(xyz, batch, n, m, lg, threads, idxs, s);
    else launch_fps_reg<16>(xyz, batch, n, m, lg, threads, idxs, s);
    return pd3::launch_status();
  }
  const int64_t per_frame = fps_ws_per_frame(n);
  if (per_frame > 0 && (!workspace || workspace_bytes < (size_t)batch * per_frame * sizeof(float)))
    return PD3_EWORKSPACE;
  // n > 1024 here or T = 1024 anyway: a lane's slots stay in the reference's order only with T = bs (see header)
  const int threads = n > kFpsThreads ? kFpsThreads : (int)pd3::ceil_div(n, 64) * 64;
  hipLaunchKernelGGL((fps_kernel<kFpsGenRegs, true>), dim3(batch), dim3(threads), 0, s, xyz, n, m, lg,
                     (float*)workspace, per_frame, idxs);
  return pd3::launch_status();
}

int pd3_gather_points(const float* points, const int* idx, int batch, int channels, int n, int npoints, float* out,
                      void* stream) {
  if (batch < 0 || channels < 0 || n < 0 || npoints < 0) return PD3_EINVAL;
  if (batch > 0 && channels > 0 && npoints > 0 && (!idx || !out || (n > 0 && !points))) return PD3_EINVAL;
  return group_fwd(points, idx, batch, channels, n, npoints, out, (hipStream_t)stream);
}

int pd3_gather_points_grad(const float* grad_out, const int* idx, int batch, int channels, int n, int npoints,
                           float* grad_points, void* stream) {
  if (batch < 0 || channels < 0 || n < 0 || npoints < 0) return PD3_EINVAL;
  if (batch > 0 && channels > 0 && n > 0 && (!grad_points || (npoints > 0 && (!idx || !grad_out))))
    return PD3_EINVAL;
  return group_bwd(grad_out, idx, batch, channels, n, npoints, grad_points, (hipStream_t)stream);
}

int pd3_group_points_batch(const float* points, const int* idx, int batch, int channels, int n, int npoints,
                           int nsample, float* out, void* stream) {
  if (batch < 0 || channels < 0 || n < 0 || npoints < 0 || nsample < 0) return PD3_EINVAL;
  const int64_t pairs = (int64_t)npoints * nsample;
  if (batch > 0 && channels > 0 && pairs > 0 && (!idx || !out || (n > 0 && !points))) return PD3_EINVAL;
  return group_fwd(points, idx, batch, channels, n, pairs, out, (hipStream_t)stream);
}

int pd3_group_points_batch_grad(const float* grad_out, const int* idx, int batch, int channels, int n, int npoints,
                                int nsample, float* grad_points, void* stream) {
  if (batch < 0 || channels < 0 || n < 0 || npoints < 0 || nsample < 0) return PD3_EINVAL;
  const int64_t pairs = (int64_t)npoints * nsample;
  if (batch > 0 && channels > 0 && n > 0 && (!grad_points || (pairs > 0 && (!idx || !grad_out))))
    return PD3_EINVAL;
  return group_bwd(grad_out, idx, batch, channels, n, pairs, grad_points, (hipStream_t)stream);
}

int pd3_ball_query_batch(const float* new_xyz, const float* xyz, int batch, int n, int m, float radius, int nsample,
                         int* idx, void* stream) {
  if (batch < 0 || n < 0 || m < 0 || nsample < 0) return PD3_EINVAL;
  if (batch == 0 || m == 0 || nsample == 0) return PD3_OK;
  if (!new_xyz || !idx || (n > 0 && !xyz)) return PD3_EINVAL;
  if (batch > 65535) return PD3_EUNSUPPORTED;
  const float r2 = radius * radius;
  hipLaunchKernelGGL(ball_query_kernel, dim3((unsigned)pd3::ceil_div(m, kBqWaves), batch), dim3(kBqThreads), 0,
                     (hipStream_t)stream, new_xyz, xyz, n, m, r2, nsample, idx);
  return pd3::launch_status();
}

int pd3_points_in_boxes(const float* pts, const float* boxes, int batch, int npts, int nboxes, int64_t box_row_stride,
                        int64_t box_batch_stride, int* box_idx_of_points, void* stream) {
  if (batch < 0 || npts < 0 || nboxes < 0 || box_row_stride < 7 || box_batch_stride < 0) return PD3_EINVAL;
  if (batch == 0 || npts == 0) return PD3_OK;
  if (!pts || !box_idx_of_points || (nboxes > 0 && !boxes)) return PD3_EINVAL;
  if (batch > 65535) return PD3_EUNSUPPORTED;
  hipLaunchKernelGGL(points_in_boxes_kernel, dim3((unsigned)pd3::ceil_div(npts, kPibThreads), batch),
                     dim3(kPibThreads), 0, (hipStream_t)stream, pts, boxes, npts, nboxes, box_row_stride,
                     box_batch_stride, box_idx_of_points);
  return pd3::launch_status();
}

}  // extern "C"
