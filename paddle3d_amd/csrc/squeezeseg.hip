// SqueezeSegV3 (paddle3d/models/backbones/sac.py, models/segmentation/squeezesegv3/squeezesegv3.py,
// transforms/reader.py LoadSemanticKITTIRange + transforms/normalize.py NormalizeRangeImage): the spatially-adaptive
// convolution block up to its 1x1 layer as one kernel, and the reader's range projection for a whole batch, fp32.
//
// pd3_sac_isk_forward                SACISKBlock.forward (sac.py:186-197) from xyz and feature to the first MLP layer
//   xyz [N, 3, H, W], feature [N, C, H, W] (NCHW); the 7x7 attention convolution's weight [9C, 3, 7, 7] packed as w1p,
//   its folded BatchNorm s_a, t_a [9C] (t_a = (bias - mean) * s_a + beta: this convolution has a bias); the 1x1 weight
//   [C, 9C] packed as w2p with s_m, t_m [C] -> Y [N, C, H, W].  With j = c * 9 + ky * 3 + kx (F.unfold's channel) and
//   tap = ci * 49 + ky7 * 7 + kx7, per pixel (n, y, x), in this order:
//     a_j  = fmaf(X_147, w_j,147, ... fmaf(X_1, w_j1, fmaf(X_0, w_j0, +0)))      ascending tap; X_tap = xyz[n, ci, y +
//            ky7 - 3, x + kx7 - 3] or +0 outside the image (it takes part as fmaf(+0, w, .), so an Inf weight gives the
//            NaN the zero-padded convolution gives); tap 147 is the padding of K to 148: X = +0, w = +0
//     z_j  = a_j * s_a[j] + t_a[j]                                                two roundings
//     g_j  = 1 / (1 + expf(-z_j))                                                 glibc's expf bits (libm_exact.hpp), one
//                                                                                 IEEE division
//     p_j  = u_j * g_j,  u_j = feature[n, c, y + ky - 1, x + kx - 1] or +0 outside the image
//     y_o  = fmaf(p_{9C-1}, v_o,9C-1, ... fmaf(p_1, v_o1, fmaf(p_0, v_o0, +0)))  ONE chain, ascending j
//     Y_o  = r > 0 ? r : (r is a NaN ? r : +0),  r = y_o * s_m[o] + t_m[o]        two roundings; relu, a NaN stays
//   Nothing above depends on N, H, W, the tile, the pixel's place in it, the grid or the stream.  Every product is
//   v_mfma_f32_16x16x4_f32, whose result is the k-ordered fp32 fmaf chain (csrc/petr.hip relies on the same).
//   A wave owns 16 consecutive x of one (n, y); a workgroup is four such waves (segments 4 b .. 4 b + 3 in (n, y, x
//   tile) order).  Lane (col = lane & 15, g = lane >> 4).
//     * the im2col of the wave's xyz halo is the B operand of the first product and does not depend on j: lane (pixel
//       col, g) keeps X_{4 s + g}, s = 0 .. 36, in 37 registers for the whole kernel;
//     * the j are walked in tiles of 16 (9C / 16 of them).  The first product is computed transposed, A^T = W1 X^T (the
//       j as M, the pixels as N; a * b commutes, so the chain is a_j's): MFMA row m holds j = 16 T + 4 (m & 3) + (m >> 2),
//       so that lane (pixel col, g) ends with j = 16 T + 4 r + g in accumulator register r -- which is the A operand of
//       the second product when its MFMA step r takes the four j = 16 T + 4 r + (0 .. 3): the chain over j is ascending
//       and z, g, u and p never leave the lane's registers.  Neither U, A nor P exists in memory or LDS;
//     * the [16 pixels, C] accumulators stay in registers: C / 16 MFMA tiles of 4 values per lane (64 at C = 256).
//     * with fewer than 768 segments and C >= 128 (the 64 x 128 stage of one frame is 512 segments on 1024 SIMDs) two
//       waves share a segment: each repeats the first product and owns half the output channels.  An output's chain is
//       the same in both forms, so the choice, which depends on N, H and W, changes no bit.
//   Packed weights (ops/squeezeseg.py pack_sac_attention_weight / pack_sac_mlp_weight):
//     w1p [9C / 16][37][64]:      lane (m, k) of step s of tile T holds w[16 T + 4 (m & 3) + (m >> 2)][4 s + k] (0 for
//                                 tap 147)
//     w2p [9C / 16][4][C / 16][64]: lane (col, k) of step r, output tile ot holds v[16 ot + col][16 T + 4 r + k]
//   so every weight fetch of a wave is 64 consecutive floats.  The next tile's w1p is fetched before the current tile's
//   MFMAs; the current tile's w2p and u before its first product.  LDS: expf's table, 256 bytes.
//   Padded pixels (x >= W) load +0 everywhere and are never stored.  No address outside the inputs is formed for a
//   load.  Supported (sac_isk_supported): C % 16 == 0, 16 <= C <= 256, any H, W >= 1 with N * H * ceil(W / 16) below
//   2^30.  Anything else: PD3_EUNSUPPORTED without a launch.  Stores are float4 when W % 4 == 0 and Y is 16-byte
//   aligned, single floats otherwise.
//
// pd3_range_project                  LoadSemanticKITTIRange.__call__ + NormalizeRangeImage for B frames at once
//   points [P, 4] (x, y, z, remission; the frames concatenated), offsets int32 [B + 1] on the device (frame b is rows
//   offsets[b] .. offsets[b + 1] - 1), H, W, the two inclinations in degrees, mean[5], std[5] host doubles, a uint64
//   [B, H, W] workspace -> image [B, 5, H, W] (range, x, y, z, remission, normalised), proj_idx int32 [B, H, W] (the
//   point's index inside its frame), proj_mask uint8 [B, H, W], proj_y, proj_x int32 [P].  Per point:
//     depth = sqrtf((x * x + y * y) + z * z)                                      fp32, np.linalg.norm's bits
//     fx = (0.5 * (-atan2((double)y, (double)x) / pi + 1.0)) * W                  fp64 from the fp32 inputs
//     fy = (1.0 - (asin(q) + |lower|) / fov) * H,  q = (double)z / (double)depth clipped to [-1, 1]
//          (upper = up_deg / 180 * pi, lower = down_deg / 180 * pi, fov = upper - lower, host doubles)
//     px = max(0, min(W - 1, floor(fx))), py likewise with H
//   The reference computes these in float32 with NumPy's vectorised arctan2 / arcsin, whose bits no libm restates; the
//   fp64 form is the well-defined one, and the golden scans keep every coordinate away from an integer.  A pixel takes
//   the point with the smallest depth and, among equal depths, the smallest index: a 64-bit atomicMin on (depth bits <<
//   32) | index, exact in any order (the reference's argsort(depth)[::-1] + last write wins, where that is defined).
//   An empty pixel holds -1 in all five channels and in proj_idx before the normalisation (float)((double)(float)
//   ((double)v - mean_c) / std_c), NumPy's in-place -= and /= of a float64 array on a float32 image.  proj_mask =
//   proj_idx > 0: the reference's own form, which masks out the pixel of point 0 as well.  A point with a non-finite
//   coordinate or zero depth, or outside every frame, takes no pixel and gets proj_y = proj_x = -1 (the reference
//   raises); no address is formed from it.  Three launches: the workspace's fill, the points, the pixels; nothing
//   depends on a buffer's previous contents.
//
// No FMA but the MFMA chains (-ffp-contract=off), 64-bit offsets.
#include "../../include/paddle3d_amd.h"
#include "common.hpp"
#include "libm_exact.hpp"

#include <cmath>

namespace {

using namespace pd3;
namespace lm = pd3::lm;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kSacThreads = 256;
constexpr int kSacWaves = kSacThreads / kWave;
constexpr int kSacSteps = 37;  // 148 taps / 4
constexpr int kSacTaps = 147;
constexpr int kSacMaxC = 256;

template <int CT, int OS>  // C / 16; the waves that share a segment's output channels
__global__ void __launch_bounds__(kSacThreads) sac_isk_kernel(const float* __restrict__ xyz,
                                                              const float* __restrict__ feat,
                                                              const float* __restrict__ w1p,
                                                              const float* __restrict__ s_a,
                                                              const float* __restrict__ t_a,
                                                              const float* __restrict__ w2p,
                                                              const float* __restrict__ s_m,
                                                              const float* __restrict__ t_m, float* __restrict__ out,
                                                              int H, int W, int XT, int64_t segments, int vec) {
  constexpr int C = 16 * CT, NT = 9 * CT, CTP = CT / OS;
  __shared__ uint64_t etab[32];  // expf's table (libm_exact.hpp expf_with)
  lm::exp2f_tab_fill(etab);
  __syncthreads();
  const auto tab = [&](int i) { return etab[i]; };
  const int lane = lane_id(), col = lane & 15, g = lane >> 4;
  const int64_t unit = (int64_t)blockIdx.x * kSacWaves + wave_id();
  const int64_t seg = unit / OS;
  const int ot0 = (int)(unit % OS) * CTP;  // this wave's output tiles: ot0 .. ot0 + CTP - 1
  if (seg >= segments) return;  // wave-uniform; no barrier follows
  const int xt = (int)(seg % XT);
  const int64_t row = seg / XT;  // n * H + y
  const int y = (int)(row % H);
  const int64_t n = row / H;
  const int64_t HW = (int64_t)H * W;
  const int x = xt * 16 + col;
  const bool live = x < W;
  // ---- the im2col of the xyz halo, as the B operand: lane (pixel col, g) holds X_{4 s + g} --------------------------
  float xs[kSacSteps];
  {
    const float* xb = xyz + n * 3 * HW;
#pragma unroll
    for (int s = 0; s < kSacSteps; ++s) {
      const int tap = 4 * s + g;
      const int ci = tap / 49, rem = tap - ci * 49;
      const int ky = rem / 7, kx = rem - ky * 7;
      const int yy = y + ky - 3, xx = x + kx - 3;
      const bool ok = live && tap < kSacTaps && yy >= 0 && yy < H && xx >= 0 && xx < W;
      xs[s] = ok ? xb[ci * HW + (int64_t)yy * W + xx] : 0.0f;
    }
  }
  const float* fb = feat + n * C * HW;
  f32x4 oacc[CTP];
#pragma unroll
  for (int ot = 0; ot < CTP; ++ot) oacc[ot] = f32x4{0.f, 0.f, 0.f, 0.f};
  float w1[kSacSteps], w1n[kSacSteps];
  const auto fetch_w1 = [&](int t, float (&w)[kSacSteps]) {  // behind the last tile: zeros, no load
    const float* p = w1p + ((int64_t)(t < NT ? t : 0) * kSacSteps) * kWave + lane;
#pragma unroll
    for (int s = 0; s < kSacSteps; ++s) w[s] = t < NT ? p[s * kWave] : 0.0f;
  };
  fetch_w1(0, w1);
  for (int t = 0; t < NT; ++t) {
    // this tile's second-product weights, its u, s_a, t_a; the next tile's first-product weights
    float w2[4][CTP], u[4], sa[4], ta[4];
    {
      const float* p = w2p + ((int64_t)t * 4 * CT + ot0) * kWave + lane;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int ot = 0; ot < CTP; ++ot) w2[r][ot] = p[(r * CT + ot) * kWave];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = 16 * t + 4 * r + g;
      const int c = j / 9, k9 = j - c * 9;
      const int ky = k9 / 3, kx = k9 - ky * 3;
      const int yy = y + ky - 1, xx = x + kx - 1;
      const bool ok = live && yy >= 0 && yy < H && xx >= 0 && xx < W;
      u[r] = ok ? fb[c * HW + (int64_t)yy * W + xx] : 0.0f;
      sa[r] = s_a[j];
      ta[r] = t_a[j];
    }
    fetch_w1(t + 1, w1n);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < kSacSteps; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[s], xs[s], acc, 0, 0, 0);
    float p[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float z = acc[r] * sa[r] + ta[r];
      const float e = lm::expf_with(-z, tab);
      const float gate = 1.0f / (1.0f + e);
      p[r] = u[r] * gate;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int ot = 0; ot < CTP; ++ot) oacc[ot] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[r], w2[r][ot], oacc[ot], 0, 0, 0);
    }
#pragma unroll
    for (int s = 0; s < kSacSteps; ++s) w1[s] = w1n[s];
  }
  // ---- folded BatchNorm, relu, store: lane (col, g) holds pixels 4 g + r of channel 16 ot + col ----------------------
  const int x0 = xt * 16 + 4 * g;
  float* ob = out + n * C * HW + (int64_t)y * W + x0;
#pragma unroll
  for (int ot = 0; ot < CTP; ++ot) {
    const int o = 16 * (ot0 + ot) + col;
    const float sm = s_m[o], tm = t_m[o];
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float q = oacc[ot][r] * sm + tm;
      v[r] = q > 0.0f ? q : (q != q ? q : 0.0f);
    }
    float* dst = ob + o * HW;
    if (vec) {  // W % 4 == 0: the four pixels are inside the row together
      if (x0 < W) *reinterpret_cast<f32x4*>(dst) = v;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (x0 + r < W) dst[r] = v[r];
    }
  }
}

template <int CT, int OS>
int launch_sac_split(const float* xyz, const float* feat, const float* w1p, const float* s_a, const float* t_a,
               const float* w2p, const float* s_m, const float* t_m, float* out, int H, int W, int XT, int64_t segments,
               int vec, hipStream_t stream) {
  const unsigned blocks = (unsigned)((segments * OS + kSacWaves - 1) / kSacWaves);
  hipLaunchKernelGGL((sac_isk_kernel<CT, OS>), dim3(blocks), dim3(kSacThreads), 0, stream, xyz, feat, w1p, s_a, t_a, w2p, s_m,
                     t_m, out, H, W, XT, segments, vec);
  return pd3::launch_status();
}

// One wave per segment fills the device's 1024 SIMDs from 1024 segments on; below 3/4 of that, from C = 128 on, two
// waves share a segment: each repeats the attention product (37 of the tile's 37 + C / 4 MFMAs) and owns half the
// output channels.  Every output's chain is the same either way: the split changes no bit.
constexpr int64_t kSacSplitBelow = 768;

template <int CT>
int launch_sac(const float* xyz, const float* feat, const float* w1p, const float* s_a, const float* t_a,
               const float* w2p, const float* s_m, const float* t_m, float* out, int H, int W, int XT, int64_t segments,
               int vec, hipStream_t stream) {
  if constexpr (CT >= 8 && CT % 2 == 0) {
    if (segments < kSacSplitBelow)
      return launch_sac_split<CT, 2>(xyz, feat, w1p, s_a, t_a, w2p, s_m, t_m, out, H, W, XT, segments, vec, stream);
  }
  return launch_sac_split<CT, 1>(xyz, feat, w1p, s_a, t_a, w2p, s_m, t_m, out, H, W, XT, segments, vec, stream);
}

bool sac_isk_supported(int64_t N, int C, int H, int W) {
  if (C < 16 || C > kSacMaxC || C % 16 != 0 || H < 1 || W < 1 || N < 0) return false;
  return N * H * ((W + 15) / 16) <= 0x7fffffff / 2;
}

// ---- range projection --------------------------------------------------------------------------------------------
constexpr int kProjThreads = 256;
constexpr uint64_t kProjEmpty = ~0ull;

struct ProjCfg {
  int B, H, W;
  int64_t P;
  double lower_abs, fov;
  double mean[5], std[5];
};

__global__ void __launch_bounds__(kProjThreads) range_fill_kernel(uint64_t* __restrict__ ws, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kProjThreads + threadIdx.x;
  if (i < n) ws[i] = kProjEmpty;
}

__global__ void __launch_bounds__(kProjThreads) range_points_kernel(ProjCfg c, const float* __restrict__ points,
                                                                    const int32_t* __restrict__ offsets,
                                                                    uint64_t* __restrict__ ws,
                                                                    int32_t* __restrict__ proj_y,
                                                                    int32_t* __restrict__ proj_x) {
  const int64_t p = (int64_t)blockIdx.x * kProjThreads + threadIdx.x;
  if (p >= c.P) return;
  int py = -1, px = -1;
  // the frame: the first b with offsets[b + 1] > p, when offsets[b] <= p
  int lo = 0, hi = c.B;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)offsets[mid + 1] <= p) lo = mid + 1; else hi = mid;
  }
  const float x = points[4 * p], y = points[4 * p + 1], z = points[4 * p + 2];
  const float depth = sqrtf((x * x + y * y) + z * z);
  const bool finite = __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
  if (lo < c.B && (int64_t)offsets[lo] <= p && finite && depth > 0.0f) {
    const double kPi = 3.141592653589793;
    double fx = -atan2((double)y, (double)x) / kPi;
    fx = fx + 1.0;
    fx = 0.5 * fx;
    fx = floor(fx * (double)c.W);
    double q = (double)z / (double)depth;
    q = q > 1.0 ? 1.0 : (q < -1.0 ? -1.0 : q);
    double fy = (asin(q) + c.lower_abs) / c.fov;
    fy = 1.0 - fy;
    fy = floor(fy * (double)c.H);
    fx = fx > (double)(c.W - 1) ? (double)(c.W - 1) : fx;
    fy = fy > (double)(c.H - 1) ? (double)(c.H - 1) : fy;
    px = fx > 0.0 ? (int)fx : 0;
    py = fy > 0.0 ? (int)fy : 0;
    const uint64_t key = ((uint64_t)lm::f2u(depth) << 32) | (uint32_t)(p - offsets[lo]);
    atomicMin(reinterpret_cast<unsigned long long*>(ws + ((int64_t)lo * c.H + py) * c.W + px), (unsigned long long)key);
  }
  proj_y[p] = py;
  proj_x[p] = px;
}

__global__ void __launch_bounds__(kProjThreads) range_pixels_kernel(ProjCfg c, const float* __restrict__ points,
                                                                    const int32_t* __restrict__ offsets,
                                                                    const uint64_t* __restrict__ ws,
                                                                    float* __restrict__ image,
                                                                    int32_t* __restrict__ proj_idx,
                                                                    uint8_t* __restrict__ proj_mask) {
  const int64_t HW = (int64_t)c.H * c.W;
  const int64_t i = (int64_t)blockIdx.x * kProjThreads + threadIdx.x;
  if (i >= c.B * HW) return;
  const int64_t b = i / HW, hw = i - b * HW;
  const uint64_t key = ws[i];
  float v[5] = {-1.0f, -1.0f, -1.0f, -1.0f, -1.0f};
  int32_t idx = -1;
  if (key != kProjEmpty) {
    const int64_t p = (int64_t)offsets[b] + (int64_t)(uint32_t)key;
    if (p >= 0 && p < c.P) {  // always: the key came from point p of this frame
      idx = (int32_t)(uint32_t)key;
      v[0] = lm::u2f((uint32_t)(key >> 32));
      v[1] = points[4 * p], v[2] = points[4 * p + 1], v[3] = points[4 * p + 2], v[4] = points[4 * p + 3];
    }
  }
#pragma unroll
  for (int ch = 0; ch < 5; ++ch) {
    const float d = (float)((double)v[ch] - c.mean[ch]);
    image[(b * 5 + ch) * HW + hw] = (float)((double)d / c.std[ch]);
  }
  proj_idx[i] = idx;
  proj_mask[i] = idx > 0 ? 1 : 0;  // the reference's `proj_idx > 0`: point 0's pixel is masked out too
}

}  // namespace

extern "C" {

int pd3_sac_isk_forward(const void* xyz, const void* feature, const void* attn_weight_packed, const void* attn_scale,
                        const void* attn_shift, const void* mlp_weight_packed, const void* mlp_scale,
                        const void* mlp_shift, int batch, int channels, int height, int width, void* out,
                        void* stream) {
  if (batch < 0 || channels < 1 || height < 0 || width < 0) return PD3_EINVAL;
  if (!sac_isk_supported(batch, channels, height, width)) return PD3_EUNSUPPORTED;
  if (batch == 0) return PD3_OK;
  if (!xyz || !feature || !attn_weight_packed || !attn_scale || !attn_shift || !mlp_weight_packed || !mlp_scale ||
      !mlp_shift || !out)
    return PD3_EINVAL;
  const int XT = (width + 15) / 16;
  const int64_t segments = (int64_t)batch * height * XT;
  const int vec = (width % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) ? 1 : 0;
  const float* xf = static_cast<const float*>(xyz);
  const float* ff = static_cast<const float*>(feature);
  const float* w1 = static_cast<const float*>(attn_weight_packed);
  const float* sa = static_cast<const float*>(attn_scale);
  const float* ta = static_cast<const float*>(attn_shift);
  const float* w2 = static_cast<const float*>(mlp_weight_packed);
  const float* sm = static_cast<const float*>(mlp_scale);
  const float* tm = static_cast<const float*>(mlp_shift);
  float* of = static_cast<float*>(out);
  const hipStream_t st = (hipStream_t)stream;
#define PD3_SAC_CASE(CT) \
  case CT:               \
    return launch_sac<CT>(xf, ff, w1, sa, ta, w2, sm, tm, of, height, width, XT, segments, vec, st)
  switch (channels / 16) {
    PD3_SAC_CASE(1);
    PD3_SAC_CASE(2);
    PD3_SAC_CASE(3);
    PD3_SAC_CASE(4);
    PD3_SAC_CASE(5);
    PD3_SAC_CASE(6);
    PD3_SAC_CASE(7);
    PD3_SAC_CASE(8);
    PD3_SAC_CASE(9);
    PD3_SAC_CASE(10);
    PD3_SAC_CASE(11);
    PD3_SAC_CASE(12);
    PD3_SAC_CASE(13);
    PD3_SAC_CASE(14);
    PD3_SAC_CASE(15);
    PD3_SAC_CASE(16);
  }
#undef PD3_SAC_CASE
  return PD3_EUNSUPPORTED;
}

int pd3_range_project(const void* points, int64_t num_points, const void* offsets, int batch, int height, int width,
                      double fov_up_deg, double fov_down_deg, const double* mean, const double* std, void* image,
                      void* proj_idx, void* proj_mask, void* proj_y, void* proj_x, void* workspace,
                      size_t workspace_bytes, void* stream) {
  if (num_points < 0 || batch < 0 || height < 1 || width < 1 || !mean || !std) return PD3_EINVAL;
  const double kPi = 3.141592653589793;
  const double upper = fov_up_deg / 180.0 * kPi, lower = fov_down_deg / 180.0 * kPi;
  const double fov = upper - lower;
  if (!(fov > 0.0) || !(fov < 1e300)) return PD3_EINVAL;
  for (int i = 0; i < 5; ++i)
    if (!(mean[i] == mean[i]) || !(std[i] == std[i])) return PD3_EINVAL;
  const int64_t pixels = (int64_t)batch * height * width;
  const int64_t pix_blocks = (pixels + kProjThreads - 1) / kProjThreads;
  const int64_t pt_blocks = (num_points + kProjThreads - 1) / kProjThreads;
  if (pix_blocks > 0x7fffffff || pt_blocks > 0x7fffffff || num_points > 0x7fffffff) return PD3_EUNSUPPORTED;
  if (workspace_bytes < (size_t)pixels * sizeof(uint64_t)) return PD3_EWORKSPACE;
  if (num_points > 0 && (!points || !proj_y || !proj_x)) return PD3_EINVAL;
  if (batch == 0 && num_points == 0) return PD3_OK;
  if (!offsets) return PD3_EINVAL;
  if (pixels > 0 && (!image || !proj_idx || !proj_mask || !workspace ||
                     (reinterpret_cast<uintptr_t>(workspace) & 7) != 0))
    return PD3_EINVAL;
  ProjCfg c;
  c.B = batch, c.H = height, c.W = width, c.P = num_points;
  c.lower_abs = fabs(lower), c.fov = fov;
  for (int i = 0; i < 5; ++i) c.mean[i] = mean[i], c.std[i] = std[i];
  const hipStream_t st = (hipStream_t)stream;
  uint64_t* ws = static_cast<uint64_t*>(workspace);
  const float* pf = static_cast<const float*>(points);
  const int32_t* off = static_cast<const int32_t*>(offsets);
  if (pixels > 0) hipLaunchKernelGGL(range_fill_kernel, dim3((unsigned)pix_blocks), dim3(kProjThreads), 0, st, ws, pixels);
  if (num_points > 0)
    hipLaunchKernelGGL(range_points_kernel, dim3((unsigned)pt_blocks), dim3(kProjThreads), 0, st, c, pf, off, ws,
                       static_cast<int32_t*>(proj_y), static_cast<int32_t*>(proj_x));
  if (pixels > 0)
    hipLaunchKernelGGL(range_pixels_kernel, dim3((unsigned)pix_blocks), dim3(kProjThreads), 0, st, c, pf, off, ws,
                       static_cast<float*>(image), static_cast<int32_t*>(proj_idx), static_cast<uint8_t*>(proj_mask));
  return pd3::launch_status();
}

}  // extern "C"
