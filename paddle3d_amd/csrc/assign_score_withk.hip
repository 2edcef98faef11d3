// assign_score_withk and its gradient: PAConv's weight-bank assembly (PD_BUILD_OP / PD_BUILD_GRAD_OP
// (assign_score_withk), assign_score_withk/assign_score_withk_cuda.cc:265-274, CPU kernels :32-158).
//
//   scores [B, N, K, M], points [B, N, M, O], centers [B, N, M, O], knn_idx [B, N, K] int64 -> output [B, O, N].
//   kn = knn_idx[b, n, k].  All fp32, plain IEEE operations without FMA contraction (-ffp-contract=off), in the
//   reference CPU kernels' order:
//   forward        acc = +0; for k, for m: acc = acc + points[b, kn, m, o] * s; acc = acc - centers[b, n, m, o] * s
//                  (s = scores[b, n, k, m]; each product and sum rounded on its own)
//   grad_scores    acc = +0; for o: acc = acc + (points[b, kn, m, o] - centers[b, n, m, o]) * grad_out[b, o, n]
//   grad_points    acc = +0; for every (n, k) with kn == j, (n, k) ascending: acc = acc + scores[b, n, k, m] *
//                  grad_out[b, o, n]  (the order of the reference's single writer per (b, m, o))
//   grad_centers   acc = +0; for k: acc = acc - scores[b, n, k, m] * grad_out[b, o, n]
//   tests/golden/assign_score_withk_numpy.py restates the same contract; the device results equal it bit for bit.
//
// Departures from the reference:
//   - kn outside [0, N) is range-tested as int64 (the reference truncates it to int and reads out of bounds): points
//     reads as 0 there, so the forward still subtracts c * s, grad_scores reads p = 0 and grad_points gets nothing.
//   - Offsets are 64-bit (the reference's int products overflow at B * N * M * O >= 2^31).
//   - fp32 only (the reference allocates its outputs as FLOAT32 whatever the input type: no fp64 contract exists).
//   - aggregate is SUM; the reference's dead AVG / MAX branches are not reproduced.
//   - The CUDA kernel adds p * s - c * s as one term (possibly contracted to an fma) with float atomics; this file
//     follows the CPU kernels and uses no atomics, so every output is bitwise reproducible.
//
// Lane maps (wave = 64 lanes):
//   forward       a lane per (n, o), lanes along o: the neighbour row points[b, kn, m, o0:o0+64] is one 256-B segment,
//                 kn and s are wave-uniform (scalar loads), the (k, m) chain stays in the lane's registers.  A block
//                 computes 64 n x 64 o; the tile goes through LDS and is stored along n (output is [B, O, N]).
//   transpose     grad_out [B, O, N] -> goT [B, N, O] in the workspace, once per backward (64 x 64 LDS tiles).
//   inverse index keys kn (out of range: N) and values n*K + k go through the batched stable radix sort
//                 (radix_sort.hpp); segment starts seg[b, j] = first sorted position with key >= j, j = 0..N.
//   grad_points   a wave per (b, j, 64-wide o-slice), lanes along o, one accumulator per m (8 per pass): a gather
//                 of goT rows over j's segment.  The same wave then computes grad_centers of row n = j.
//   grad_scores   a block per (b, n): the K*M chains run along o, so (p - c) * g for 32 o at a time is staged in LDS
//                 (rows padded to 33 floats: conflict-free both ways) and each thread carries one chain across the
//                 chunks.  More than 256 chains take several passes.
//   Blocks go to the XCDs so that one XCD works through one (frame, o-slice) window at a time (the gathered 64-wide
//   slice of a frame's table is N*M*64*4 B, 2 MB at PAConv's shapes, inside the XCD's 4 MiB L2): speed only.
#include "common.hpp"
#include "radix_sort.hpp"
#include "scan.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / pd3::kWave;
constexpr int kTile = 64;   // forward: n and o per block; transpose tile edge; o per backward wave
constexpr int kMC = 8;      // m per unrolled step / accumulators per pass
constexpr int kOC = 32;     // grad_scores: o per LDS chunk
constexpr int kChains = kThreads;  // grad_scores: chains per pass

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// window of `tiles` work tiles: consecutive tiles (one (frame, o-slice) after another) stay on one XCD
static inline int window_size(int64_t tiles, int64_t per_pair) {
  const int64_t even = pd3::ceil_div(tiles, 8);
  return (int)(per_pair < even ? per_pair : even);
}

// ---- forward ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void asw_forward_kernel(const float* __restrict__ scores,
                                                               const float* __restrict__ points,
                                                               const float* __restrict__ centers,
                                                               const int64_t* __restrict__ knn, int N, int K, int M,
                                                               int O, int tiles_n, int oslices, int tiles, int win,
                                                               float* __restrict__ out) {
  __shared__ float tile[kTile][kTile + 1];
  const int t = pd3::sp_window_tile(blockIdx.x, tiles, win);
  if (t < 0) return;
  const int pair = t / tiles_n, nt = t - pair * tiles_n;
  const int b = pair / oslices, os = pair - b * oslices;
  const int lane = pd3::lane_id(), wave = uniform(pd3::wave_id());
  const int o = os * kTile + lane;
  const bool ok = o < O;
  const int64_t MO = (int64_t)M * O;
  const float* pts = points + (int64_t)b * N * MO + o;
  constexpr int kPerWave = kTile / kWaves;
  for (int i = 0; i < kPerWave; ++i) {
    const int nl = wave * kPerWave + i, n = nt * kTile + nl;
    float acc = 0.f;
    if (n < N) {
      const int64_t row = (int64_t)b * N + n;
      const int64_t* kr = knn + row * K;
      const float* cr = centers + row * MO + o;
      for (int k = 0; k < K; ++k) {
        const int64_t kn = kr[k];
        const bool in = kn >= 0 && kn < N;
        const float* pr = pts + (in ? kn : 0) * MO;
        const float* s = scores + (row * K + k) * M;
        int m = 0;
        for (; m + kMC <= M; m += kMC) {
          float p[kMC], c[kMC];
#pragma unroll
          for (int j = 0; j < kMC; ++j) {
            p[j] = ok && in ? pr[(int64_t)(m + j) * O] : 0.f;
            c[j] = ok ? cr[(int64_t)(m + j) * O] : 0.f;
          }
#pragma unroll
          for (int j = 0; j < kMC; ++j) {
            const float sv = s[m + j];
            acc = acc + p[j] * sv;
            acc = acc - c[j] * sv;
          }
        }
        for (; m < M; ++m) {
          const float p = ok && in ? pr[(int64_t)m * O] : 0.f;
          const float c = ok ? cr[(int64_t)m * O] : 0.f;
          const float sv = s[m];
          acc = acc + p * sv;
          acc = acc - c * sv;
        }
      }
    }
    tile[lane][nl] = acc;
  }
  __syncthreads();
  const int n = nt * kTile + lane;
  for (int i = 0; i < kPerWave; ++i) {
    const int ol = wave * kPerWave + i, oo = os * kTile + ol;
    if (oo < O && n < N) out[((int64_t)b * O + oo) * N + n] = tile[ol][lane];
  }
}

// ---- backward: grad_out [B, O, N] -> [B, N, O] --------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void asw_transpose_kernel(const float* __restrict__ in, int N, int O,
                                                                 int tiles_n, int tiles_o, float* __restrict__ outT) {
  __shared__ float tile[kTile][kTile + 1];
  const int per_frame = tiles_n * tiles_o;
  const int b = blockIdx.x / per_frame, r = blockIdx.x - b * per_frame;
  const int ot = r / tiles_n, nt = r - ot * tiles_n;
  const int lane = pd3::lane_id(), wave = pd3::wave_id();
  constexpr int kPerWave = kTile / kWaves;
  const float* src = in + (int64_t)b * O * N;
  for (int i = 0; i < kPerWave; ++i) {
    const int ol = wave * kPerWave + i, o = ot * kTile + ol, n = nt * kTile + lane;
    tile[ol][lane] = o < O && n < N ? src[(int64_t)o * N + n] : 0.f;
  }
  __syncthreads();
  float* dst = outT + (int64_t)b * N * O;
  for (int i = 0; i < kPerWave; ++i) {
    const int nl = wave * kPerWave + i, n = nt * kTile + nl, o = ot * kTile + lane;
    if (n < N && o < O) dst[(int64_t)n * O + o] = tile[lane][nl];
  }
}

// ---- backward: inverse index --------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void asw_keys_kernel(const int64_t* __restrict__ knn, int64_t total, int N,
                                                            uint32_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int64_t kn = knn[i];
  keys[i] = kn >= 0 && kn < N ? (uint32_t)kn : (uint32_t)N;  // out of range: past the last segment
}

// seg[b, j] = first position of frame b's sorted keys with key >= j (j = 0..N; seg[b, N] = in-range entries)
__global__ __launch_bounds__(kThreads) void asw_segments_kernel(const uint32_t* __restrict__ skeys, int NK, int N,
                                                                int batch, int* __restrict__ seg) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= (int64_t)batch * NK) return;
  const int b = (int)(g / NK), i = (int)(g - (int64_t)b * NK);
  const uint32_t* k = skeys + (int64_t)b * NK;
  int* s = seg + (int64_t)b * (N + 1);
  const int64_t key = k[i], prev = i ? (int64_t)k[i - 1] : -1;
  for (int64_t j = prev + 1; j <= key; ++j) s[j] = i;
  if (i == NK - 1)
    for (int64_t j = key + 1; j <= N; ++j) s[j] = NK;
}

// ---- backward: grad_points (gather over the inverse index) and grad_centers ---------------------------------------
__global__ __launch_bounds__(kThreads) void asw_bwd_points_kernel(const float* __restrict__ goT,
                                                                  const float* __restrict__ scores,
                                                                  const uint32_t* __restrict__ sval,
                                                                  const int* __restrict__ seg, int N, int K, int M,
                                                                  int O, int tiles_r, int oslices, int tiles, int win,
                                                                  float* __restrict__ grad_points,
                                                                  float* __restrict__ grad_centers) {
  const int t = pd3::sp_window_tile(blockIdx.x, tiles, win);
  if (t < 0) return;
  const int pair = t / tiles_r, rt = t - pair * tiles_r;
  const int b = pair / oslices, os = pair - b * oslices;
  const int lane = pd3::lane_id(), wave = uniform(pd3::wave_id());
  const int r = rt * kWaves + wave;
  if (r >= N) return;  // whole waves leave
  const int o = os * kTile + lane;
  const bool ok = o < O;
  const float* gT = goT + (int64_t)b * N * O + o;
  const float* sc = scores + (int64_t)b * N * K * M;
  const int64_t out_row = ((int64_t)b * N + r) * M * O + o;
  if (grad_points) {
    const uint32_t* sv = sval + (int64_t)b * N * K;
    const int s0 = seg[(int64_t)b * (N + 1) + r], s1 = seg[(int64_t)b * (N + 1) + r + 1];
    for (int m0 = 0; m0 < M; m0 += kMC) {
      const int mc = M - m0 < kMC ? M - m0 : kMC;
      float acc[kMC];
#pragma unroll
      for (int j = 0; j < kMC; ++j) acc[j] = 0.f;
      for (int e = s0; e < s1; ++e) {
        const uint32_t v = sv[e];  // n * K + k
        const uint32_t n = v / (uint32_t)K;
        const float g = ok ? gT[(int64_t)n * O] : 0.f;
        const float* s = sc + (int64_t)v * M + m0;
#pragma unroll
        for (int j = 0; j < kMC; ++j)
          if (j < mc) acc[j] = acc[j] + s[j] * g;
      }
#pragma unroll
      for (int j = 0; j < kMC; ++j)
        if (j < mc && ok) grad_points[out_row + (int64_t)(m0 + j) * O] = acc[j];
    }
  }
  if (grad_centers) {
    const float g = ok ? gT[(int64_t)r * O] : 0.f;
    const float* sr = sc + (int64_t)r * K * M;
    for (int m0 = 0; m0 < M; m0 += kMC) {
      const int mc = M - m0 < kMC ? M - m0 : kMC;
      float acc[kMC];
#pragma unroll
      for (int j = 0; j < kMC; ++j) acc[j] = 0.f;
      for (int k = 0; k < K; ++k) {
        const float* s = sr + (int64_t)k * M + m0;
#pragma unroll
        for (int j = 0; j < kMC; ++j)
          if (j < mc) acc[j] = acc[j] - s[j] * g;
      }
#pragma unroll
      for (int j = 0; j < kMC; ++j)
        if (j < mc && ok) grad_centers[out_row + (int64_t)(m0 + j) * O] = acc[j];
    }
  }
}

// ---- backward: grad_scores ----------------------------------------------------------------------------------------
// Dynamic LDS: min(K*M, kChains) rows of kOC + 1 floats.
__global__ __launch_bounds__(kThreads) void asw_bwd_scores_kernel(const float* __restrict__ goT,
                                                                  const float* __restrict__ points,
                                                                  const float* __restrict__ centers,
                                                                  const int64_t* __restrict__ knn, int N, int K,
                                                                  int M, int O, int tiles, int win,
                                                                  float* __restrict__ grad_scores) {
  extern __shared__ float E[];  // [rows][kOC + 1]: (p - c) * g of one o-chunk
  const int t = pd3::sp_window_tile(blockIdx.x, tiles, win);
  if (t < 0) return;
  const int64_t row = t;  // b * N + n
  const int b = (int)(row / N);
  const int64_t MO = (int64_t)M * O;
  const int KM = K * M;
  const int64_t* kr = knn + row * K;
  const float* pts = points + (int64_t)b * N * MO;
  const float* cr = centers + row * MO;
  const float* g = goT + row * O;
  float* out = grad_scores + row * KM;
  const int col = threadIdx.x % kOC, sub = threadIdx.x / kOC;  // staging: kThreads / kOC rows per step
  constexpr int kRowsPerStep = kThreads / kOC;
  for (int q0 = 0; q0 < KM; q0 += kChains) {
    const int rows = KM - q0 < kChains ? KM - q0 : kChains;
    float acc = 0.f;
    for (int o0 = 0; o0 < O; o0 += kOC) {
      const int cols = O - o0 < kOC ? O - o0 : kOC;
      const int o = o0 + col;
      const float gv = col < cols ? g[o] : 0.f;
      for (int rr = sub; rr < rows; rr += kRowsPerStep) {
        const int q = q0 + rr, k = q / M, m = q - k * M;
        float e = 0.f;
        if (col < cols) {
          const int64_t kn = kr[k];
          const float p = kn >= 0 && kn < N ? pts[kn * MO + (int64_t)m * O + o] : 0.f;
          const float c = cr[(int64_t)m * O + o];
          e = (p - c) * gv;
        }
        E[rr * (kOC + 1) + col] = e;
      }
      __syncthreads();
      if ((int)threadIdx.x < rows) {
        const float* er = E + threadIdx.x * (kOC + 1);
        for (int c = 0; c < cols; ++c) acc = acc + er[c];
      }
      __syncthreads();
    }
    if ((int)threadIdx.x < rows) out[q0 + threadIdx.x] = acc;
  }
}

struct BwdLayout {
  pd3::RadixPlan plan;
  size_t bytes;
};

// Workspace carve-out, in this order: goT, keys a/b, values a/b, seg, hist, partial.
static BwdLayout bwd_layout(int batch, int n, int k, int o) {
  BwdLayout L;
  const int64_t NK = (int64_t)n * k;
  L.plan = pd3::radix_plan((uint32_t)n, NK > 0 ? NK : 1);
  const int64_t hist = (int64_t)pd3::radix_hist_ints(L.plan);
  const size_t sizes[] = {(size_t)batch * n * o * sizeof(float),
                          (size_t)batch * NK * sizeof(uint32_t),
                          (size_t)batch * NK * sizeof(uint32_t),
                          (size_t)batch * NK * sizeof(uint32_t),
                          (size_t)batch * NK * sizeof(uint32_t),
                          (size_t)batch * (n + 1) * sizeof(int),
                          (size_t)batch * hist * sizeof(int),
                          (size_t)batch * pd3::scan_num_tiles(hist) * sizeof(int)};
  L.bytes = 0;
  for (size_t s : sizes) L.bytes = pd3::align_up(L.bytes + s, 256);
  return L;
}

static bool dims_ok(int batch, int n, int k, int m, int o) {
  return batch >= 0 && n >= 0 && k >= 0 && m >= 0 && o >= 0;
}

}  // namespace

extern "C" {

int pd3_assign_score_withk_forward(const float* scores, const float* points, const float* centers,
                                   const int64_t* knn_idx, int batch, int n, int k, int m, int o, float* output,
                                   void* stream) {
  if (!dims_ok(batch, n, k, m, o)) return PD3_EINVAL;
  if ((int64_t)batch * n * k >= (int64_t)INT32_MAX + 1) return PD3_EUNSUPPORTED;
  const int64_t outs = (int64_t)batch * n * o;
  if (outs == 0) return PD3_OK;
  if (!output) return PD3_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (k == 0 || m == 0) {  // no term: +0 everywhere
    if (hipMemsetAsync(output, 0, (size_t)outs * sizeof(float), s) != hipSuccess) return pd3::launch_status();
    return PD3_OK;
  }
  if (!scores || !points || !centers || !knn_idx) return PD3_EINVAL;
  const int64_t tiles_n = pd3::ceil_div(n, kTile), oslices = pd3::ceil_div(o, kTile);
  const int64_t tiles = (int64_t)batch * oslices * tiles_n;
  const int win = window_size(tiles, tiles_n);
  const int64_t grid = pd3::sp_window_grid(tiles, win);
  if (tiles > INT32_MAX / 2 || grid > INT32_MAX) return PD3_EUNSUPPORTED;
  hipLaunchKernelGGL(asw_forward_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, scores, points, centers,
                     knn_idx, n, k, m, o, (int)tiles_n, (int)oslices, (int)tiles, win, output);
  return pd3::launch_status();
}

size_t pd3_assign_score_withk_backward_workspace(int batch, int n, int k, int o) {
  if (batch < 0 || n < 0 || k < 0 || o < 0) return 0;
  return bwd_layout(batch, n, k, o).bytes;
}

int pd3_assign_score_withk_backward(const float* grad_out, const float* scores, const float* points,
                                    const float* centers, const int64_t* knn_idx, int batch, int n, int k, int m,
                                    int o, float* grad_scores, float* grad_points, float* grad_centers,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!dims_ok(batch, n, k, m, o)) return PD3_EINVAL;
  if ((int64_t)batch * n * k >= (int64_t)INT32_MAX + 1) return PD3_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)batch * n;
  const int64_t nkm = rows * k * m, nmo = rows * m * o;
  if (rows == 0 || m == 0) return PD3_OK;  // every output is empty
  if (o == 0) {  // grad_scores: sums over no o; grad_points / grad_centers are empty
    if (grad_scores && nkm && hipMemsetAsync(grad_scores, 0, (size_t)nkm * sizeof(float), s) != hipSuccess)
      return pd3::launch_status();
    return PD3_OK;
  }
  if (k == 0) {  // grad_scores empty; nothing gathers into grad_points; grad_centers sums no k
    grad_scores = nullptr;
    if (grad_points) {
      if (hipMemsetAsync(grad_points, 0, (size_t)nmo * sizeof(float), s) != hipSuccess) return pd3::launch_status();
      grad_points = nullptr;
    }
  }
  if (!grad_scores && !grad_points && !grad_centers) return PD3_OK;
  if (!grad_out || !workspace || (k > 0 && (!scores || !knn_idx))) return PD3_EINVAL;
  if (grad_scores && (!points || !centers)) return PD3_EINVAL;
  if (batch > 65535) return PD3_EUNSUPPORTED;  // the radix sort's grid.y
  const BwdLayout L = bwd_layout(batch, n, k, o);
  if (workspace_bytes < L.bytes) return PD3_EWORKSPACE;
  const int64_t NK = (int64_t)n * k;
  const int64_t tiles_n = pd3::ceil_div(n, kTile), tiles_o = pd3::ceil_div(o, kTile);
  const int64_t tr_blocks = (int64_t)batch * tiles_n * tiles_o;
  const int64_t tiles_r = pd3::ceil_div(n, kWaves), pc_tiles = (int64_t)batch * tiles_o * tiles_r;
  if (tr_blocks > INT32_MAX || pc_tiles > INT32_MAX / 2 || rows > INT32_MAX / 2) return PD3_EUNSUPPORTED;

  pd3::Carver cv(workspace);
  float* goT = cv.take<float>((size_t)batch * n * o);
  uint32_t* keys_a = cv.take<uint32_t>((size_t)batch * NK);
  uint32_t* keys_b = cv.take<uint32_t>((size_t)batch * NK);
  uint32_t* vals_a = cv.take<uint32_t>((size_t)batch * NK);
  uint32_t* vals_b = cv.take<uint32_t>((size_t)batch * NK);
  int* seg = cv.take<int>((size_t)batch * (n + 1));
  const int64_t hist_n = (int64_t)pd3::radix_hist_ints(L.plan);
  int* hist = cv.take<int>((size_t)batch * hist_n);
  int* partial = cv.take<int>((size_t)batch * pd3::scan_num_tiles(hist_n));

  hipLaunchKernelGGL(asw_transpose_kernel, dim3((unsigned)tr_blocks), dim3(kThreads), 0, s, grad_out, n, o,
                     (int)tiles_n, (int)tiles_o, goT);
  const uint32_t* sval = nullptr;
  if (grad_points) {
    const int64_t total = (int64_t)batch * NK;
    hipLaunchKernelGGL(asw_keys_kernel, dim3((unsigned)pd3::ceil_div(total, kThreads)), dim3(kThreads), 0, s,
                       knn_idx, total, n, keys_a);
    const int cur = pd3::enqueue_radix_sort(keys_a, vals_a, keys_b, vals_b, NK, NK, batch, L.plan, true, hist,
                                            partial, s);
    sval = cur ? vals_b : vals_a;
    hipLaunchKernelGGL(asw_segments_kernel, dim3((unsigned)pd3::ceil_div(total, kThreads)), dim3(kThreads), 0, s,
                       cur ? keys_b : keys_a, (int)NK, n, batch, seg);
  }
  if (grad_points || grad_centers) {
    const int win = window_size(pc_tiles, tiles_r);
    const int64_t grid = pd3::sp_window_grid(pc_tiles, win);
    if (grid > INT32_MAX) return PD3_EUNSUPPORTED;
    hipLaunchKernelGGL(asw_bwd_points_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, goT, scores, sval, seg, n,
                       k, m, o, (int)tiles_r, (int)tiles_o, (int)pc_tiles, win, grad_points, grad_centers);
  }
  if (grad_scores) {
    const int64_t km = (int64_t)k * m;
    const int lds_rows = (int)(km < kChains ? km : kChains);
    const int win = window_size(rows, n);
    const int64_t grid = pd3::sp_window_grid(rows, win);
    if (km > INT32_MAX || grid > INT32_MAX) return PD3_EUNSUPPORTED;
    hipLaunchKernelGGL(asw_bwd_scores_kernel, dim3((unsigned)grid), dim3(kThreads),
                       (size_t)lds_rows * (kOC + 1) * sizeof(float), s, goT, points, centers, knn_idx, n, k, m, o,
                       (int)rows, win, grad_scores);
  }
  return pd3::launch_status();
}

}  // extern "C"
