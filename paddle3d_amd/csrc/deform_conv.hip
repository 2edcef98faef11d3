// Modulated deformable convolution (paddle.vision.ops.deform_conv2d: DCNv2 with a mask, DCNv1 without; the conv2 of
// nine bottlenecks of CAPE's ResNet-50, paddle3d/models/backbones/mm_resnet.py:32-79), forward, fp32, NCHW, 3 x 3,
// groups = deformable_groups = 1, as ONE kernel: the sampled columns [N, 9 Cin, Ho, Wo] never exist in memory.
//
// pd3_deform_conv2d_forward
//   x [N, Cin, H, W]; offset [N, 18, Ho, Wo] (channel 2 k is dy of tap k = ky * 3 + kx, channel 2 k + 1 its dx) and mask
//   [N, 9, Ho, Wo] or NULL, each with a batch stride and a row pitch of its own (channel planes Ho * pitch apart: the two
//   parts of one 27-channel map are passed as views); the weight [Cout, Cin, 3, 3] packed as wp; scale, shift [Cout] or
//   NULL each -> y [N, Cout, Ho, Wo], Ho = (H + 2 pad - 2 dil - 1) / stride + 1.  With j = c * 9 + k, per output value
//   (n, o, ho, wo), in this order:
//     m_k  = 1 without a mask, mask[n, k, ho, wo] with one, 1 / (1 + expf(-mask[n, k, ho, wo])) when mask_is_logit:
//            glibc's expf bits (libm_exact.hpp), one IEEE division
//     h    = (float)(ho * stride - pad + ky * dil) + dy,   w = (float)(wo * stride - pad + kx * dil) + dx
//     val  = +0 unless h > -1 && w > -1 && h < H && w < W (a NaN or huge offset fails the test; the test comes before any
//            float -> int conversion, so no address outside x is ever formed); otherwise with hl = floorf(h), lh = h - hl,
//            hh = 1 - lh (and wl, lw, hw likewise), v1 .. v4 = x[n, c, hl, wl], [hl, wl + 1], [hl + 1, wl], [hl + 1,
//            wl + 1], each +0 where the corner lies outside [0, H - 1] x [0, W - 1]:
//            val = (((hh * hw) * v1 + (hh * lw) * v2) + (lh * hw) * v3) + (lh * lw) * v4      no FMA, seven roundings
//     p_j  = val * m_k                                                                       (an out-of-range sample of a
//            finite mask is +0 and takes part as fmaf(+0, weight, .): an Inf weight there gives the NaN 0 * Inf gives)
//     y_o  = fmaf(p_{9Cin-1}, w_o,9Cin-1, ... fmaf(p_1, w_o1, fmaf(p_0, w_o0, +0)))           ONE chain, ascending j
//     r    = y_o, * scale[o] where scale is given, + shift[o] where shift is given             a rounding each
//     Y    = relu ? (r > 0 ? r : (r is a NaN ? r : +0)) : r                                   a NaN stays
//   Nothing above depends on N, the tile, the pixel's place in it, the grid or the stream.  Every product is
//   v_mfma_f32_16x16x4_f32, whose result is the k-ordered fp32 fmaf chain (csrc/petr.hip, csrc/squeezeseg.hip).
//
//   Work: the output pixels of the whole batch are numbered p = (n * Ho + ho) * Wo + wo and cut into tiles of 64; a
//   workgroup (four waves) owns one tile and a group of 64 * NTW output channels (NTW = 1, 2 or 4 MFMA tiles of 16 per
//   wave; grid.y walks the groups).
//     * once per workgroup, per (pixel, tap): the four coefficients hh * hw .. lh * lw, the four corner offsets inside a
//       channel plane (-1: the corner is +0) and m_k go to LDS (21 KB) -- they do not depend on the channel;
//     * the j are walked in chunks of 16.  Wave w samples the chunk for pixels 16 w .. 16 w + 15: lane (m, kk) computes
//       p_j for j = 16 t + 4 ks + kk, ks = 0 .. 3, and stores them as one float4 at [w][lane] of the chunk's LDS buffer
//       (4 KB, two buffers, one barrier per chunk).  That float4 is the A operand of the four MFMA steps of pixel tile w
//       for EVERY wave: each wave reads the four pixel tiles' float4 and multiplies them into its own NTW channel tiles,
//       so a sampled value is computed once per workgroup and a weight is fetched by exactly one wave of it: per layer
//       the weight crosses L2 once per 64 pixels (0.6 GB at CAPE's stage 3, not the 2.5 GB of a wave per 16 pixels);
//     * the next chunk's weights (NTW float4 per lane, 64 lanes x 16 bytes consecutive) and samples are fetched before
//       the current chunk's MFMAs; accumulators: 4 x NTW tiles of 4 registers.
//   NTW is chosen from the shape alone so that the grid has about two workgroups per CU where the layer allows (a
//   smaller NTW repeats the sampling in more workgroups); an output's chain is the same in every form, so the choice
//   changes no bit.
//   Packed weight (ops/deform_conv.py pack_deform_conv_weight) wp [9 Cin / 16][Cout / 16][64][4]: lane (col, kk) of
//   chunk t, channel tile nt holds in element ks w[16 nt + col][16 t + 4 ks + kk] (w viewed as [Cout, 9 Cin]).
//   Padded pixels (p >= N Ho Wo) sample +0 and are never stored.  Stores are float4 when Ho * Wo % 4 == 0 and y is
//   16-byte aligned, single floats otherwise.
//   Supported (deform_conv2d_supported): Cin % 16 == 0, Cout % 16 == 0, 16 <= Cin, Cout <= 512, stride 1 or 2, dil >= 1,
//   pad >= 0, H * W below 2^31 and fewer than 2^30 pixel tiles.  Anything else: PD3_EUNSUPPORTED without a launch.
//
// No FMA but the MFMA chains (-ffp-contract=off), 64-bit offsets.
#include "../../include/paddle3d_amd_dcn.h"
#include "common.hpp"
#include "libm_exact.hpp"

#include <cmath>

namespace {

using namespace pd3;
namespace lm = pd3::lm;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kDcnThreads = 256;
constexpr int kDcnWaves = kDcnThreads / kWave;
constexpr int kDcnPixels = 16 * kDcnWaves;  // a workgroup's pixel tile
constexpr int kDcnTaps = 9;
constexpr int kDcnMaxC = 512;

struct DcnArgs {
  const float* x;
  const float* offset;
  const float* mask;
  const float* wp;
  const float* scale;
  const float* shift;
  float* y;
  int64_t off_batch, mask_batch, total;  // total = N * Ho * Wo
  int off_pitch, mask_pitch;
  int Cin, Cout, H, W, Ho, Wo, stride, pad, dil;
  int mask_is_logit, relu, vec;
};

template <int NTW>
__global__ void __launch_bounds__(kDcnThreads) deform_conv_kernel(DcnArgs a) {
  __shared__ uint64_t etab[32];  // expf's table (libm_exact.hpp expf_with)
  __shared__ f32x4 s_coef[kDcnTaps][kDcnPixels];
  __shared__ i32x4 s_off[kDcnTaps][kDcnPixels];
  __shared__ float s_m[kDcnTaps][kDcnPixels];
  __shared__ f32x4 s_a[2][kDcnWaves][kWave];
  lm::exp2f_tab_fill(etab);
  __syncthreads();
  const auto tab = [&](int i) { return etab[i]; };
  const int lane = lane_id(), wv = wave_id(), col = lane & 15, g = lane >> 4;
  const int64_t p0 = (int64_t)blockIdx.x * kDcnPixels;
  const int64_t HoWo = (int64_t)a.Ho * a.Wo, HW = (int64_t)a.H * a.W;
  // ---- per (pixel, tap): coefficients, corner offsets, modulation ------------------------------------------------------
  for (int e = threadIdx.x; e < kDcnTaps * kDcnPixels; e += kDcnThreads) {
    const int ps = e % kDcnPixels, k = e / kDcnPixels;
    const int64_t p = p0 + ps;
    f32x4 cf = {0.f, 0.f, 0.f, 0.f};
    i32x4 of = {-1, -1, -1, -1};
    float m = 0.0f;
    if (p < a.total) {
      const int64_t n = p / HoWo, hw = p - n * HoWo;
      const int ho = (int)(hw / a.Wo), wo = (int)(hw - (int64_t)ho * a.Wo);
      const int ky = k / 3, kx = k - ky * 3;
      const float* ob = a.offset + n * a.off_batch + (int64_t)ho * a.off_pitch + wo;
      const int64_t oplane = (int64_t)a.Ho * a.off_pitch;
      const float dy = ob[(2 * k) * oplane], dx = ob[(2 * k + 1) * oplane];
      m = 1.0f;
      if (a.mask) {
        m = a.mask[n * a.mask_batch + ((int64_t)k * a.Ho + ho) * a.mask_pitch + wo];
        if (a.mask_is_logit) {
          const float ex = lm::expf_with(-m, tab);
          m = 1.0f / (1.0f + ex);
        }
      }
      const float h = (float)((int64_t)ho * a.stride - a.pad + (int64_t)ky * a.dil) + dy;
      const float w = (float)((int64_t)wo * a.stride - a.pad + (int64_t)kx * a.dil) + dx;
      if (h > -1.0f && w > -1.0f && h < (float)a.H && w < (float)a.W) {
        const float hl = floorf(h), wl = floorf(w);
        const float lh = h - hl, lw = w - wl;
        const float hh = 1.0f - lh, hw_ = 1.0f - lw;
        const int ih = (int)hl, iw = (int)wl;  // in [-1, H - 1] x [-1, W - 1]
        const bool t_ok = ih >= 0, b_ok = ih + 1 <= a.H - 1, l_ok = iw >= 0, r_ok = iw + 1 <= a.W - 1;
        const int64_t base = (int64_t)ih * a.W + iw;  // a corner inside the image is below H * W < 2^31
        cf = f32x4{hh * hw_, hh * lw, lh * hw_, lh * lw};
        of = i32x4{t_ok && l_ok ? (int)base : -1, t_ok && r_ok ? (int)(base + 1) : -1,
                   b_ok && l_ok ? (int)(base + a.W) : -1, b_ok && r_ok ? (int)(base + a.W + 1) : -1};
      }
    }
    s_coef[k][ps] = cf;
    s_off[k][ps] = of;
    s_m[k][ps] = m;
  }
  // ---- this lane's sampling pixel (16 wv + col) and this wave's channel tiles ------------------------------------------
  const int ps = 16 * wv + col;
  const float* xs = a.x;
  {
    const int64_t p = p0 + ps;
    if (p < a.total) xs += (p / HoWo) * a.Cin * HW;
  }
  const int CT = a.Cout >> 4, NT = (9 * a.Cin) >> 4;
  const int nt0 = ((int)blockIdx.y * kDcnWaves + wv) * NTW;  // tiles nt0 .. nt0 + NTW - 1, those below CT
  const auto sample = [&](int t) {
    f32x4 r;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int j = 16 * t + 4 * ks + g;
      const int c = j / 9, k = j - c * 9;
      const f32x4 cf = s_coef[k][ps];
      const i32x4 of = s_off[k][ps];
      const float m = s_m[k][ps];
      const float* xc = xs + c * HW;
      const float v1 = of[0] >= 0 ? xc[of[0]] : 0.0f;
      const float v2 = of[1] >= 0 ? xc[of[1]] : 0.0f;
      const float v3 = of[2] >= 0 ? xc[of[2]] : 0.0f;
      const float v4 = of[3] >= 0 ? xc[of[3]] : 0.0f;
      float val = cf[0] * v1;
      val = val + cf[1] * v2;
      val = val + cf[2] * v3;
      val = val + cf[3] * v4;
      r[ks] = val * m;
    }
    return r;
  };
  const auto fetch_w = [&](int t, f32x4 (&w)[NTW]) {
    const f32x4* p = reinterpret_cast<const f32x4*>(a.wp) + ((int64_t)t * CT) * kWave + lane;
#pragma unroll
    for (int i = 0; i < NTW; ++i) w[i] = nt0 + i < CT ? p[(int64_t)(nt0 + i) * kWave] : f32x4{0.f, 0.f, 0.f, 0.f};
  };
  f32x4 acc[kDcnWaves][NTW];
#pragma unroll
  for (int mt = 0; mt < kDcnWaves; ++mt)
#pragma unroll
    for (int i = 0; i < NTW; ++i) acc[mt][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 wcur[NTW], wnext[NTW];
  fetch_w(0, wcur);
  __syncthreads();  // the tables
  s_a[0][wv][lane] = sample(0);
  __syncthreads();
  for (int t = 0; t < NT; ++t) {
    const int buf = t & 1;
    const bool more = t + 1 < NT;  // uniform
    f32x4 pn = {0.f, 0.f, 0.f, 0.f};
    if (more) {
      fetch_w(t + 1, wnext);
      pn = sample(t + 1);
    }
    if (nt0 < CT) {  // wave-uniform
#pragma unroll
      for (int mt = 0; mt < kDcnWaves; ++mt) {
        const f32x4 av = s_a[buf][mt][lane];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
          for (int i = 0; i < NTW; ++i)
            acc[mt][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ks], wcur[i][ks], acc[mt][i], 0, 0, 0);
        }
      }
    }
    if (more) {
      s_a[buf ^ 1][wv][lane] = pn;
#pragma unroll
      for (int i = 0; i < NTW; ++i) wcur[i] = wnext[i];
    }
    __syncthreads();  // chunk t + 1 is written; every wave has read chunk t
  }
  if (nt0 >= CT) return;  // no barrier follows
  // ---- scale, shift, relu, store: lane (col, g) holds pixels 16 mt + 4 g + r of channel 16 nt + col -----------------------
#pragma unroll
  for (int i = 0; i < NTW; ++i) {
    if (nt0 + i >= CT) break;
    const int o = 16 * (nt0 + i) + col;
    const float sc = a.scale ? a.scale[o] : 1.0f, sh = a.shift ? a.shift[o] : 0.0f;
#pragma unroll
    for (int mt = 0; mt < kDcnWaves; ++mt) {
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float q = acc[mt][i][r];
        if (a.scale) q = q * sc;
        if (a.shift) q = q + sh;
        if (a.relu) q = q > 0.0f ? q : (q != q ? q : 0.0f);
        v[r] = q;
      }
      const int64_t p = p0 + 16 * mt + 4 * g;
      if (a.vec) {  // Ho * Wo % 4 == 0: the four pixels are in one image together, 16-byte aligned
        if (p < a.total) {
          const int64_t n = p / HoWo, hw = p - n * HoWo;
          *reinterpret_cast<f32x4*>(a.y + (n * a.Cout + o) * HoWo + hw) = v;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t q = p + r;
          if (q < a.total) {
            const int64_t n = q / HoWo, hw = q - n * HoWo;
            a.y[(n * a.Cout + o) * HoWo + hw] = v[r];
          }
        }
      }
    }
  }
}

template <int NTW>
int launch_dcn(const DcnArgs& a, int64_t tiles, hipStream_t stream) {
  const int groups = (a.Cout / 16 + kDcnWaves * NTW - 1) / (kDcnWaves * NTW);
  hipLaunchKernelGGL((deform_conv_kernel<NTW>), dim3((unsigned)tiles, (unsigned)groups), dim3(kDcnThreads), 0, stream, a);
  return pd3::launch_status();
}

// The channel tiles per wave: the largest of 4, 2, 1 that still gives the grid two workgroups per CU (256 CUs), the
// smallest where none does.  A smaller value repeats the sampling in more workgroups and keeps fewer accumulators.
int dcn_tiles_per_wave(int64_t tiles, int cout) {
  const int CT = cout / 16;
  for (int ntw = 4; ntw > 1; ntw >>= 1) {
    const int groups = (CT + kDcnWaves * ntw - 1) / (kDcnWaves * ntw);
    if (CT >= kDcnWaves * ntw && tiles * groups >= 512) return ntw;
  }
  return 1;
}

}  // namespace

extern "C" {

int pd3_deform_conv2d_forward(const void* x, const void* offset, int64_t offset_batch_stride, int offset_pitch,
                              const void* mask, int64_t mask_batch_stride, int mask_pitch, int mask_is_logit,
                              const void* weight_packed, const void* scale, const void* shift, int relu, int batch,
                              int in_channels, int out_channels, int height, int width, int stride, int padding,
                              int dilation, void* y, void* stream) {
  if (batch < 0 || in_channels < 1 || out_channels < 1 || height < 1 || width < 1) return PD3_EINVAL;
  if (in_channels % 16 != 0 || out_channels % 16 != 0 || in_channels > kDcnMaxC || out_channels > kDcnMaxC)
    return PD3_EUNSUPPORTED;
  if ((stride != 1 && stride != 2) || dilation < 1 || padding < 0) return PD3_EUNSUPPORTED;
  if ((int64_t)height * width > 0x7fffffff) return PD3_EUNSUPPORTED;
  const int64_t span = 2 * (int64_t)dilation + 1;
  const int64_t eh = (int64_t)height + 2 * (int64_t)padding - span, ew = (int64_t)width + 2 * (int64_t)padding - span;
  if (eh < 0 || ew < 0) return PD3_EINVAL;  // no output pixel
  const int64_t Ho = eh / stride + 1, Wo = ew / stride + 1;
  if (Ho > 0x7fffffff || Wo > 0x7fffffff) return PD3_EUNSUPPORTED;
  const int64_t per = Ho * Wo;
  if (per > (int64_t)1 << 40 || (batch > 0 && per > ((int64_t)1 << 40) / batch)) return PD3_EUNSUPPORTED;
  const int64_t total = per * batch;
  const int64_t tiles = (total + kDcnPixels - 1) / kDcnPixels;
  if (tiles >= (int64_t)1 << 30) return PD3_EUNSUPPORTED;
  if (batch == 0) return PD3_OK;
  if (!x || !offset || !weight_packed || !y) return PD3_EINVAL;
  if (offset_pitch < Wo || offset_batch_stride < 18 * Ho * (int64_t)offset_pitch) return PD3_EINVAL;
  if (mask && (mask_pitch < Wo || mask_batch_stride < 9 * Ho * (int64_t)mask_pitch)) return PD3_EINVAL;
  if ((reinterpret_cast<uintptr_t>(weight_packed) & 15) != 0) return PD3_EINVAL;
  DcnArgs a;
  a.x = static_cast<const float*>(x);
  a.offset = static_cast<const float*>(offset);
  a.mask = static_cast<const float*>(mask);
  a.wp = static_cast<const float*>(weight_packed);
  a.scale = static_cast<const float*>(scale);
  a.shift = static_cast<const float*>(shift);
  a.y = static_cast<float*>(y);
  a.off_batch = offset_batch_stride, a.mask_batch = mask ? mask_batch_stride : 0, a.total = total;
  a.off_pitch = offset_pitch, a.mask_pitch = mask ? mask_pitch : 0;
  a.Cin = in_channels, a.Cout = out_channels, a.H = height, a.W = width, a.Ho = (int)Ho, a.Wo = (int)Wo;
  a.stride = stride, a.pad = padding, a.dil = dilation;
  a.mask_is_logit = mask && mask_is_logit ? 1 : 0, a.relu = relu ? 1 : 0;
  a.vec = (per % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0) ? 1 : 0;
  const hipStream_t st = (hipStream_t)stream;
  switch (dcn_tiles_per_wave(tiles, out_channels)) {
    case 4:
      return launch_dcn<4>(a, tiles, st);
    case 2:
      return launch_dcn<2>(a, tiles, st);
    default:
      return launch_dcn<1>(a, tiles, st);
  }
}

}  // extern "C"
