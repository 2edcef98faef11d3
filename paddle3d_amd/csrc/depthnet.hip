// BEVDepth's DepthNet kernels (reference paddle3d/models/transformers/bevdet_transformer.py): ASPP.forward (:354-416) in
// eval mode and the tail of LSSViewTransformerBEVDepth.forward (:740-742).  fp32, NCHW, 64-bit offsets.
//
// pd3_aspp_forward: x [N, Cin, H, W] -> y [N, Cmid, H, W] in three launches; `ws` is the workspace
//   [N, 4 Cmid, H, W] (the four branches, branch after branch: what the reference concatenates) + bias [N, Cmid].
//   1. aspp_pool_kernel, one workgroup per image n:
//        s_c     = the sum of x[n, c, :]: lane l of a wave adds the elements i = l, l + 64, l + 128, ... in ascending order
//                  (plain adds from +0), then part[l] += part[l + s] for s = 32, 16, 8, 4, 2, 1; the sum is part[0]
//        mean_c  = s_c / (float)(H W)                                                         one IEEE division
//        g_m     = fmaf(mean_Cin-1, wg[m, Cin-1], ... fmaf(mean_0, wg[m, 0], +0)), * pool_scale[m], + pool_shift[m], relu
//        bias_no = fmaf(g_Cmid-1, w1[o, 4 Cmid + Cmid-1], ... fmaf(g_0, w1[o, 4 Cmid], +0)) * proj_scale[o]
//      The pooled branch is constant over an image (bilinear upsampling of a 1 x 1 map with align_corners=True), so
//      behind conv1 it is this per-image vector; it is never broadcast to [N, Cmid, H, W].
//   2. aspp_gemm_kernel<NTW, false>, the four convolution branches (1 x 1, and 3 x 3 at the three dilations with padding =
//      dilation), per output (n, b, o, y, x):
//        acc = +0; for the taps (ky, kx) in ascending order whose input pixel (y + (ky - 1) d_b, x + (kx - 1) d_b) lies
//        inside the image ONLY, and per tap for c = 0 .. Cin - 1 ascending: acc = fmaf(x[n, c, yy, xx], w_b[o, c, ky, kx], acc)
//        ws[n, b Cmid + o, y, x] = relu(acc * branch_scale[b Cmid + o] + branch_shift[b Cmid + o])   a rounding each
//      A tap outside the image is not part of the sum: it equals zero padding for finite weights, and an Inf or NaN
//      weight under it does not reach that pixel.
//   3. aspp_gemm_kernel<NTW, true>, the projection:
//        acc = fmaf chain over j = 0 .. 4 Cmid - 1 ascending of ws[n, j, y, x] * w1[o, j] from +0
//        y[n, o, y, x] = relu(((acc * proj_scale[o]) + bias_no) + proj_shift[o])                     a rounding each
//   relu(r) = r > 0 ? r : (r is a NaN ? r : +0).  Nothing depends on N, the tile, the pixel's place in it or the stream.
//
//   Both GEMM kernels: the pixels of the whole batch are numbered p = n H W + y W + x and cut into tiles of 64; a
//   workgroup (four waves) owns one tile and a group of 64 NTW output channels (NTW = 1, 2 or 4 MFMA tiles of 16 per
//   wave; grid.y walks the groups) of ALL four branches, one branch after the other in the same accumulators.  Every
//   product is v_mfma_f32_16x16x4_f32, whose result is the k-ordered fp32 fmaf chain.
//     * per pixel of the tile a 28-bit mask says which (branch, tap) pairs are in range (bit 0: the 1 x 1 branch, bit
//       1 + 9 (b - 1) + 3 ky + kx: branch b's tap).  A pair that no pixel of the tile has in range is SKIPPED: at 16 x 44
//       with dilation 18 that is six of nine taps everywhere.  The pairs left form the tile's work list.
//     * a pair some pixels lack is computed with those pixels' operands zeroed, and the accumulator rows of those pixels
//       are put back to what they held before the pair: the tap is not part of their sum, whatever the weight.
//     * per pair the channels are walked in chunks of 16.  Wave w fetches the chunk for pixels 16 w .. 16 w + 15 (lane
//       (m, kk): channels 16 t + 4 ks + kk, ks = 0 .. 3, 16 consecutive pixels per channel) and stores one float4 to the
//       chunk's LDS buffer (two buffers, one barrier per chunk); every wave reads the four pixel tiles' float4 and
//       multiplies them into its own NTW channel tiles: an input value is fetched once per workgroup, for the 64 NTW
//       channels of its group, and a weight by exactly one wave.  The next chunk's weights and inputs are fetched before
//       the current chunk's MFMAs.
//   Packed weights (ops/depthnet.py): [pair or 1][K / 16][Cout / 16][64][4]: lane (col, kk) of chunk t, channel tile nt
//   holds in element ks w[16 nt + col][16 t + 4 ks + kk] of that pair's [Cout, K] matrix.
//   Padded pixels (p >= N H W) fetch +0 and are never stored.  Stores are float4 when H W % 4 == 0.
//
// pd3_depth_softmax_split: x [BN, D + C, H, W] -> depth [BN, D, H, W], tran_feat [BN, H, W, C] in ONE launch; a workgroup
//   (one wave) owns 64 consecutive pixels of one image, a lane one pixel:
//        m = x_0; for d = 1 .. D - 1: m = x_d > m ? x_d : m                    (a NaN in x_0 stays, another is never taken)
//        e_d = expf(x_d - m), glibc's bits (libm_exact.hpp);  s = ((e_0 + e_1) + ...) ascending from +0;  depth_d = e_d / s
//   (two passes over the logits; a NaN logit makes its whole column NaN), and the C context channels go through a
//   64 x 64 LDS tile so that both the reads (pixel-major) and the writes (channel-major) are coalesced.
//
// No FMA but the chains named above (-ffp-contract=off).
#include "../../include/paddle3d_amd_depthnet.h"
#include "common.hpp"
#include "libm_exact.hpp"

namespace {

using namespace pd3;
namespace lm = pd3::lm;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kPixels = 16 * kWaves;  // a workgroup's pixel tile
constexpr int kPairs = 28;            // 1 + 3 * 9 (branch, tap) pairs
constexpr int kMaxC = 512;
constexpr int kMaxDil = 65535;

__device__ __forceinline__ float relu_nan(float q) { return q > 0.0f ? q : (q != q ? q : 0.0f); }

// ---- 1. the pooled branch as a per-image bias ---------------------------------------------------------------------------
struct PoolArgs {
  const float* x;
  const float* wg_t;   // [Cin, Cmid]
  const float* gs;     // pool_scale
  const float* gb;     // pool_shift
  const float* w1p_t;  // [Cmid, Cmid]: w1[o, 4 Cmid + m] at [m, o]
  const float* s1;     // proj_scale
  float* bias;         // [N, Cmid]
  int64_t HW;
  int Cin, Cmid;
};

__global__ void __launch_bounds__(kThreads) aspp_pool_kernel(PoolArgs a) {
  __shared__ float s_mean[kMaxC];
  __shared__ float s_g[kMaxC];
  const int lane = lane_id(), wv = wave_id();
  const int64_t n = blockIdx.x;
  const float* xn = a.x + n * a.Cin * a.HW;
  for (int c = wv; c < a.Cin; c += kWaves) {
    const float* xc = xn + c * a.HW;
    float part = 0.0f;
    for (int64_t i = lane; i < a.HW; i += kWave) part = part + xc[i];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) part = part + __shfl_down(part, s, kWave);
    if (lane == 0) s_mean[c] = part / (float)a.HW;
  }
  __syncthreads();
  for (int m = threadIdx.x; m < a.Cmid; m += kThreads) {
    float acc = 0.0f;
    for (int c = 0; c < a.Cin; ++c) acc = fmaf(s_mean[c], a.wg_t[(int64_t)c * a.Cmid + m], acc);
    float q = acc * a.gs[m];
    q = q + a.gb[m];
    s_g[m] = relu_nan(q);
  }
  __syncthreads();
  for (int o = threadIdx.x; o < a.Cmid; o += kThreads) {
    float acc = 0.0f;
    for (int m = 0; m < a.Cmid; ++m) acc = fmaf(s_g[m], a.w1p_t[(int64_t)m * a.Cmid + o], acc);
    a.bias[n * a.Cmid + o] = acc * a.s1[o];
  }
}

// ---- 2., 3. the branches and the projection ---------------------------------------------------------------------------------
struct GemmArgs {
  const float* x;      // [N, K, H, W]
  const float* wp;     // packed
  const float* scale;  // [branches * Cout]
  const float* shift;
  const float* bias;   // PROJ: [N, Cout]
  float* y;            // [N, branches * Cout, H, W]
  int64_t total;       // N * H * W
  int K, Cout, H, W;
  int d1, d2, d3;
  int vec;
};

__device__ __forceinline__ void pair_decode(int pair, int d1, int d2, int d3, int& b, int& dy, int& dx) {
  if (pair == 0) {
    b = 0, dy = 0, dx = 0;
    return;
  }
  const int q = pair - 1;
  b = 1 + q / 9;
  const int k = q - (b - 1) * 9, ky = k / 3, kx = k - ky * 3;
  const int d = b == 1 ? d1 : (b == 2 ? d2 : d3);
  dy = (ky - 1) * d, dx = (kx - 1) * d;
}

template <int NTW, bool PROJ>
__global__ void __launch_bounds__(kThreads) aspp_gemm_kernel(GemmArgs a) {
  constexpr int NP = PROJ ? 1 : kPairs;
  __shared__ uint32_t s_mask[kPixels];
  __shared__ int s_item[kPairs], s_dy[kPairs], s_dx[kPairs];  // item: pair | branch << 8 | last of its branch << 16 | partial << 17
  __shared__ int s_count;
  __shared__ f32x4 s_a[2][kWaves][kWave];
  const int lane = lane_id(), wv = wave_id(), col = lane & 15, g = lane >> 4;
  const int64_t p0 = (int64_t)blockIdx.x * kPixels;
  const int64_t HW = (int64_t)a.H * a.W;
  // ---- per pixel: which pairs are in range --------------------------------------------------------------------------------
  if (threadIdx.x < kPixels) {
    const int64_t p = p0 + threadIdx.x;
    uint32_t mask = 0;
    if (p < a.total) {
      const int64_t hw = p % HW;
      const int y = (int)(hw / a.W), x = (int)(hw - (int64_t)y * a.W);
      for (int pair = 0; pair < NP; ++pair) {
        int b, dy, dx;
        pair_decode(pair, a.d1, a.d2, a.d3, b, dy, dx);
        const int yy = y + dy, xx = x + dx;
        if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) mask |= 1u << pair;
      }
    }
    s_mask[threadIdx.x] = mask;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t any = 0, all = 0xffffffffu;
    for (int i = 0; i < kPixels; ++i) any |= s_mask[i], all &= s_mask[i];
    int cnt = 0;
    for (int pair = 0; pair < NP; ++pair) {
      if (!((any >> pair) & 1u)) continue;
      int b, dy, dx;
      pair_decode(pair, a.d1, a.d2, a.d3, b, dy, dx);
      s_item[cnt] = pair | (b << 8) | (((all >> pair) & 1u) ? 0 : 1 << 17);
      s_dy[cnt] = dy, s_dx[cnt] = dx;
      ++cnt;
    }
    for (int i = 0; i < cnt; ++i)
      if (i == cnt - 1 || ((s_item[i + 1] >> 8) & 0xff) != ((s_item[i] >> 8) & 0xff)) s_item[i] |= 1 << 16;
    s_count = cnt;  // >= 1 per branch: a tile has a real pixel, whose centre taps are in range
  }
  __syncthreads();
  const int cnt = s_count;
  // ---- this lane's fetching pixel (16 wv + col) and this wave's channel tiles -------------------------------------------
  const int ps = 16 * wv + col;
  const float* xs = a.x;
  bool pv = false;
  int py = 0, px = 0;
  {
    const int64_t p = p0 + ps;
    if (p < a.total) {
      const int64_t n = p / HW, hw = p - n * HW;
      pv = true;
      py = (int)(hw / a.W), px = (int)(hw - (int64_t)py * a.W);
      xs += n * a.K * HW;
    }
  }
  const int CT = a.Cout >> 4, NT = a.K >> 4;
  const int nt0 = ((int)blockIdx.y * kWaves + wv) * NTW;  // tiles nt0 .. nt0 + NTW - 1, those below CT
  const auto fetch_x = [&](int item, int t) {
    const int yy = py + s_dy[item], xx = px + s_dx[item];
    const bool ok = pv && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
    const float* xc = xs + (int64_t)(16 * t + g) * HW + ((int64_t)yy * a.W + xx);  // formed, read only when ok
    f32x4 r;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) r[ks] = ok ? xc[(int64_t)(4 * ks) * HW] : 0.0f;
    return r;
  };
  const auto fetch_w = [&](int item, int t, f32x4 (&w)[NTW]) {
    const int pair = s_item[item] & 0xff;
    const f32x4* p = reinterpret_cast<const f32x4*>(a.wp) + (((int64_t)pair * NT + t) * CT) * kWave + lane;
#pragma unroll
    for (int i = 0; i < NTW; ++i) w[i] = nt0 + i < CT ? p[(int64_t)(nt0 + i) * kWave] : f32x4{0.f, 0.f, 0.f, 0.f};
  };
  f32x4 acc[kWaves][NTW], keep[kWaves][NTW];
#pragma unroll
  for (int mt = 0; mt < kWaves; ++mt)
#pragma unroll
    for (int i = 0; i < NTW; ++i) acc[mt][i] = keep[mt][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 wcur[NTW], wnext[NTW];
  fetch_w(0, 0, wcur);
  s_a[0][wv][lane] = fetch_x(0, 0);
  __syncthreads();
  int item = 0, t = 0;
  for (int s = 0;; ++s) {
    const int buf = s & 1;
    int item_n = item, t_n = t + 1;
    if (t_n == NT) t_n = 0, ++item_n;
    const bool more = item_n < cnt;  // uniform
    f32x4 xn = {0.f, 0.f, 0.f, 0.f};
    if (more) {
      fetch_w(item_n, t_n, wnext);
      xn = fetch_x(item_n, t_n);
    }
    const int info = s_item[item];
    const bool partial = (info >> 17) & 1;  // uniform
    if (nt0 < CT) {                          // wave-uniform
      if (t == 0 && partial) {
#pragma unroll
        for (int mt = 0; mt < kWaves; ++mt)
#pragma unroll
          for (int i = 0; i < NTW; ++i) keep[mt][i] = acc[mt][i];
      }
#pragma unroll
      for (int mt = 0; mt < kWaves; ++mt) {
        const f32x4 av = s_a[buf][mt][lane];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
          for (int i = 0; i < NTW; ++i)
            acc[mt][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ks], wcur[i][ks], acc[mt][i], 0, 0, 0);
        }
      }
      if (t == NT - 1) {
        if (partial) {  // the pixels that lack this pair: their rows are what they were before it
          const int pair = info & 0xff;
#pragma unroll
          for (int mt = 0; mt < kWaves; ++mt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const bool has = (s_mask[16 * mt + 4 * g + r] >> pair) & 1u;
#pragma unroll
              for (int i = 0; i < NTW; ++i) acc[mt][i][r] = has ? acc[mt][i][r] : keep[mt][i][r];
            }
          }
        }
        if ((info >> 16) & 1) {  // the branch is complete: scale, shift, (bias,) relu, store; lane (col, g) holds pixels
          const int b = (info >> 8) & 0xff;  // 16 mt + 4 g + r of channel 16 nt + col
          const int64_t planes = (int64_t)(PROJ ? 1 : 4) * a.Cout;
#pragma unroll
          for (int i = 0; i < NTW; ++i) {
            if (nt0 + i < CT) {
              const int o = 16 * (nt0 + i) + col;
              const float sc = a.scale[b * a.Cout + o], sh = a.shift[b * a.Cout + o];
#pragma unroll
              for (int mt = 0; mt < kWaves; ++mt) {
                const int64_t p = p0 + 16 * mt + 4 * g;
                if (a.vec) {  // H W % 4 == 0: the four pixels are in one image together, 16-byte aligned
                  if (p < a.total) {
                    const int64_t n = p / HW, hw = p - n * HW;
                    const float bs = PROJ ? a.bias[n * a.Cout + o] : 0.0f;
                    f32x4 v;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                      float q = acc[mt][i][r] * sc;
                      if (PROJ) q = q + bs;
                      q = q + sh;
                      v[r] = relu_nan(q);
                    }
                    *reinterpret_cast<f32x4*>(a.y + (n * planes + (int64_t)b * a.Cout + o) * HW + hw) = v;
                  }
                } else {
#pragma unroll
                  for (int r = 0; r < 4; ++r) {
                    const int64_t pq = p + r;
                    if (pq < a.total) {
                      const int64_t n = pq / HW, hw = pq - n * HW;
                      float q = acc[mt][i][r] * sc;
                      if (PROJ) q = q + a.bias[n * a.Cout + o];
                      q = q + sh;
                      a.y[(n * planes + (int64_t)b * a.Cout + o) * HW + hw] = relu_nan(q);
                    }
                  }
                }
              }
            }
#pragma unroll
            for (int mt = 0; mt < kWaves; ++mt) acc[mt][i] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
        }
      }
    }
    if (!more) break;  // uniform; no barrier follows
    s_a[buf ^ 1][wv][lane] = xn;
#pragma unroll
    for (int i = 0; i < NTW; ++i) wcur[i] = wnext[i];
    item = item_n, t = t_n;
    __syncthreads();  // chunk s + 1 is written; every wave has read chunk s
  }
}

template <int NTW, bool PROJ>
int launch_gemm(const GemmArgs& a, int64_t tiles, hipStream_t stream) {
  const int groups = (a.Cout / 16 + kWaves * NTW - 1) / (kWaves * NTW);
  hipLaunchKernelGGL((aspp_gemm_kernel<NTW, PROJ>), dim3((unsigned)tiles, (unsigned)groups), dim3(kThreads), 0, stream, a);
  return pd3::launch_status();
}

// The channel tiles per wave: the largest of 4, 2, 1 that still gives the grid two workgroups per CU (256 CUs), the
// smallest where none does.  An output's chain is the same in every form.
int gemm_tiles_per_wave(int64_t tiles, int cout) {
  const int CT = cout / 16;
  for (int ntw = 4; ntw > 1; ntw >>= 1) {
    const int groups = (CT + kWaves * ntw - 1) / (kWaves * ntw);
    if (CT >= kWaves * ntw && tiles * groups >= 512) return ntw;
  }
  return 1;
}

template <bool PROJ>
int launch_gemm_any(const GemmArgs& a, int64_t tiles, hipStream_t stream) {
  switch (gemm_tiles_per_wave(tiles, a.Cout)) {
    case 4:
      return launch_gemm<4, PROJ>(a, tiles, stream);
    case 2:
      return launch_gemm<2, PROJ>(a, tiles, stream);
    default:
      return launch_gemm<1, PROJ>(a, tiles, stream);
  }
}

bool aspp_shape_ok(int batch, int cin, int cmid, int h, int w) {
  if (cin % 16 != 0 || cmid % 16 != 0 || cin < 16 || cmid < 16 || cin > kMaxC || cmid > kMaxC) return false;
  if ((int64_t)h * w > 0x7fffffff) return false;
  const int64_t per = (int64_t)h * w;
  if (batch > 0 && per > ((int64_t)1 << 36) / batch) return false;
  return (per * batch + kPixels - 1) / kPixels < (int64_t)1 << 30;
}

// ---- the softmax / channels-last tail -----------------------------------------------------------------------------------
struct TailArgs {
  const float* x;
  float* depth;
  float* feat;
  int64_t HW;
  int D, C;
};

__global__ void __launch_bounds__(kWave) depth_softmax_split_kernel(TailArgs a) {
  __shared__ uint64_t etab[32];  // expf's table (libm_exact.hpp expf_with)
  __shared__ float s_t[kWave][kWave + 1];
  lm::exp2f_tab_fill(etab);
  __syncthreads();
  const auto tab = [&](int i) { return etab[i]; };
  const int lane = threadIdx.x;
  const int64_t n = blockIdx.y, hw0 = (int64_t)blockIdx.x * kWave, hw = hw0 + lane;
  const int live = (int)(a.HW - hw0 < kWave ? a.HW - hw0 : kWave);  // pixels of this tile
  const float* xn = a.x + n * (a.D + a.C) * a.HW;
  if (lane < live) {
    const float* xp = xn + hw;
    float* dp = a.depth + n * a.D * a.HW + hw;
    float m = xp[0];
    for (int d = 1; d < a.D; ++d) {
      const float v = xp[d * a.HW];
      m = v > m ? v : m;
    }
    float s = 0.0f;
    for (int d = 0; d < a.D; ++d) {
      const float e = lm::expf_with(xp[d * a.HW] - m, tab);
      s = s + e;
      dp[d * a.HW] = e;
    }
    for (int d = 0; d < a.D; ++d) dp[d * a.HW] = dp[d * a.HW] / s;  // this lane's own stores
  }
  const float* xc = xn + a.D * a.HW;
  float* fo = a.feat + (n * a.HW + hw0) * a.C;
  for (int c0 = 0; c0 < a.C; c0 += kWave) {
    const int cc = a.C - c0 < kWave ? a.C - c0 : kWave;
    __syncthreads();
    if (lane < live)
      for (int c = 0; c < cc; ++c) s_t[c][lane] = xc[(int64_t)(c0 + c) * a.HW + hw];
    __syncthreads();
    if (lane < cc)
      for (int p = 0; p < live; ++p) fo[(int64_t)p * a.C + c0 + lane] = s_t[lane][p];
  }
}

}  // namespace

extern "C" {

size_t pd3_aspp_workspace(int batch, int in_channels, int mid_channels, int height, int width) {
  if (batch < 1 || height < 1 || width < 1 || !aspp_shape_ok(batch, in_channels, mid_channels, height, width)) return 0;
  const size_t per = (size_t)height * width;
  return ((size_t)batch * 4 * mid_channels * per + (size_t)batch * mid_channels) * sizeof(float);
}

int pd3_aspp_forward(const void* x, const void* branch_weights, const void* branch_scale, const void* branch_shift,
                     const void* pool_weight_t, const void* pool_scale, const void* pool_shift, const void* proj_weights,
                     const void* proj_pool_weight_t, const void* proj_scale, const void* proj_shift, int batch,
                     int in_channels, int mid_channels, int height, int width, int dilation1, int dilation2, int dilation3,
                     void* y, void* workspace, size_t workspace_bytes, void* stream) {
  if (batch < 0 || in_channels < 1 || mid_channels < 1 || height < 1 || width < 1) return PD3_EINVAL;
  if (!aspp_shape_ok(batch, in_channels, mid_channels, height, width)) return PD3_EUNSUPPORTED;
  for (int d : {dilation1, dilation2, dilation3})
    if (d < 1 || d > kMaxDil) return PD3_EUNSUPPORTED;
  if (batch == 0) return PD3_OK;
  if (!x || !branch_weights || !branch_scale || !branch_shift || !pool_weight_t || !pool_scale || !pool_shift ||
      !proj_weights || !proj_pool_weight_t || !proj_scale || !proj_shift || !y || !workspace)
    return PD3_EINVAL;
  if ((reinterpret_cast<uintptr_t>(branch_weights) & 15) != 0 || (reinterpret_cast<uintptr_t>(proj_weights) & 15) != 0 ||
      (reinterpret_cast<uintptr_t>(workspace) & 15) != 0)
    return PD3_EINVAL;
  if (workspace_bytes < pd3_aspp_workspace(batch, in_channels, mid_channels, height, width)) return PD3_EWORKSPACE;
  const hipStream_t st = (hipStream_t)stream;
  const int64_t per = (int64_t)height * width, total = per * batch;
  const int64_t tiles = (total + kPixels - 1) / kPixels;
  float* ws = static_cast<float*>(workspace);
  float* bias = ws + (int64_t)batch * 4 * mid_channels * per;

  PoolArgs pa;
  pa.x = static_cast<const float*>(x);
  pa.wg_t = static_cast<const float*>(pool_weight_t);
  pa.gs = static_cast<const float*>(pool_scale), pa.gb = static_cast<const float*>(pool_shift);
  pa.w1p_t = static_cast<const float*>(proj_pool_weight_t);
  pa.s1 = static_cast<const float*>(proj_scale);
  pa.bias = bias;
  pa.HW = per, pa.Cin = in_channels, pa.Cmid = mid_channels;
  hipLaunchKernelGGL(aspp_pool_kernel, dim3((unsigned)batch), dim3(kThreads), 0, st, pa);
  int status = pd3::launch_status();
  if (status != PD3_OK) return status;

  GemmArgs ga;
  ga.x = static_cast<const float*>(x);
  ga.wp = static_cast<const float*>(branch_weights);
  ga.scale = static_cast<const float*>(branch_scale), ga.shift = static_cast<const float*>(branch_shift);
  ga.bias = nullptr;
  ga.y = ws;
  ga.total = total;
  ga.K = in_channels, ga.Cout = mid_channels, ga.H = height, ga.W = width;
  ga.d1 = dilation1, ga.d2 = dilation2, ga.d3 = dilation3;
  ga.vec = per % 4 == 0 ? 1 : 0;  // the workspace is 16-byte aligned
  status = launch_gemm_any<false>(ga, tiles, st);
  if (status != PD3_OK) return status;

  GemmArgs gp = ga;
  gp.x = ws;
  gp.wp = static_cast<const float*>(proj_weights);
  gp.scale = static_cast<const float*>(proj_scale), gp.shift = static_cast<const float*>(proj_shift);
  gp.bias = bias;
  gp.y = static_cast<float*>(y);
  gp.K = 4 * mid_channels;
  gp.vec = (per % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0) ? 1 : 0;
  return launch_gemm_any<true>(gp, tiles, st);
}

int pd3_depth_softmax_split(const void* x, int batch, int depth_channels, int context_channels, int height, int width,
                            void* depth, void* tran_feat, void* stream) {
  if (batch < 0 || depth_channels < 1 || context_channels < 0 || height < 1 || width < 1) return PD3_EINVAL;
  const int64_t per = (int64_t)height * width;
  if (per > 0x7fffffff || batch > 65535 || (int64_t)depth_channels + context_channels > 0x7fffffff) return PD3_EUNSUPPORTED;
  if (batch == 0) return PD3_OK;
  if (!x || !depth || (context_channels > 0 && !tran_feat)) return PD3_EINVAL;
  TailArgs a;
  a.x = static_cast<const float*>(x);
  a.depth = static_cast<float*>(depth);
  a.feat = static_cast<float*>(tran_feat);
  a.HW = per, a.D = depth_channels, a.C = context_channels;
  hipLaunchKernelGGL(depth_softmax_split_kernel, dim3((unsigned)((per + kWave - 1) / kWave), (unsigned)batch),
                     dim3(kWave), 0, (hipStream_t)stream, a);
  return pd3::launch_status();
}

}  // extern "C"
