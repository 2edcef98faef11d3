// SMOKE's head and post-processing at inference for gfx950: GroupNorm statistics, the class branch down to the clipped
// heat map, and nms_hm + select_topk + select_point_of_interest + SMOKECoder's decode + the threshold of a whole batch
// in one workgroup per frame, every count on the device.
// (reference: paddle3d/models/detection/smoke/smoke_predictor.py:78-97, processor.py:45-194, smoke_coder.py:103-347,
//  :350-383, paddle3d/models/layers/layer_libs.py:36-116, :181-207, layers/layer_norm.py:20-33.)
//
// The reference evaluates both branches densely (two 3x3 convolutions, two GroupNorms, two 1x1 convolutions, the
// channel-wise activations) and then runs some sixty small ops on max_detection pixels.  Here the head is LAZY: the
// regression branch's normalised map and its ten outputs are evaluated at the max_detection selected pixels only, from
// the 3x3 convolution's output.  pd3_smoke_post_process is the same selection and decode from existing maps.
//
// Arithmetic order (fp32 unless said, every operation rounded on its own, -ffp-contract=off;
// tests/golden/smoke_numpy.py restates it):
//   tables         per (frame, group): the n = (C / G) * H * W values of the group in index order i = (c * H + y) * W + x;
//                  thread t of 1024 adds the values i = t, t + 1024, .. in that order into a double; the 1024 doubles are
//                  folded by halves (p[t] += p[t + s], s = 512, 256, .. 1); m = sum / n; a second pass in the same order
//                  over (x - m) * (x - m) in double gives the biased variance v; mean = (float)m,
//                  rstd = (float)(1 / sqrt(v + 1e-5)) -- one rounding each.  No atomics; a frame's tables depend on
//                  nothing but that frame.
//   norm(x, c)     ((x - mean[g]) * rstd[g]) * gamma[c] + beta[c], g = c / (C / G): the reference's form, four roundings;
//                  relu(v) = v > 0 ? v : +0, a NaN stays
//   conv1x1(row)   fmaf(f[C-1], w[C-1], ... fmaf(f[0], w[0], +0)) + bias[row]            ascending channel
//   heat           s = 1 / (1 + expf(-logit)), expf with glibc's bits (libm_exact.hpp); s < lo ? lo : (s > hi ? hi : s)
//                  with lo = 1e-4f, hi = (float)(1 - 1e-4): a NaN stays
//   selection      score(c, y, x) = heat unless an in-map 3x3 neighbour is larger (then 0); key = bits(1.0f) - bits(score);
//                  the K = max_detection smallest (key, flat index c * H * W + y * W + x) pairs in that order: the
//                  reference's two-stage topk selects the same entries in the same order when ties go to the lower
//                  index.  The two places where this is a DEFINITION and not parity: (1) that tie order -- the reference
//                  leaves it to its framework; (2) a NaN heat has score 0 and a NaN neighbour suppresses nothing -- the
//                  reference's heat * (hmax == heat) differs between frameworks there.  (A heat outside (0, 1], which
//                  sigmoid_hm's clip never gives, also has score 0: every key is bits(1.0f) - bits of a score in [0, 1].)
//   regression     lazy: r[j] = conv1x1 of relu(norm(column)) for the ten rows; then r[3..5] = sigmoid(r) - 0.5f,
//                  nrm = sqrtf(r6 * r6 + r7 * r7), d = nrm < 1e-12f ? 1e-12f : nrm (a NaN stays), r6 /= d, r7 /= d
//   inverses       of K and trans_mat once per frame, in double by the adjugate (cofactors / determinant), rounded to fp32
//   mat3(M, p)     ((M[r][0] * p0 + M[r][1] * p1) + M[r][2] * p2) per row
//   decode         depth = r0 * depth_ref[1] + depth_ref[0]; (px, py) = (r1 + x, r2 + y);
//                  forward: q = mat3(Tinv, (px, py, 1)) * depth (per component); export: q = (dr0 * px, dr1 * py, 1) * depth;
//                  loc = mat3(Kinv, q); (l, h, w) = expf(r3..5) * dim_ref[cls]; loc.y = loc.y + h / 2;
//                  ray = atanf(loc.x / (loc.z + 1e-7f)); alpha = atanf(r6 / (r7 + 1e-7f)) - (r7 >= 0 ? P/2 : -P/2),
//                  P = 3.14159f; roty = alpha + ray; roty > P: roty - 2P; roty < -P: roty + 2P (one wrap; atanf with
//                  glibc's bits); box (x0, y0, x1, y1) = (x - r8 / 2, y - r9 / 2, x + r8 / 2, y + r9 / 2);
//                  forward: mat3(Tinv, (x0, y0, 1))[0:2], mat3(Tinv, (x1, y1, 1))[0:2], x clipped to [0, image_size[0]],
//                  y to [0, image_size[1]] (a NaN stays); export: (dr0 * x0, dr1 * y0, dr0 * x1, dr1 * y1)
//   row            (cls, alpha, x0, y0, x1, y1, h, w, l, loc.x, loc.y, loc.z, roty, score); forward: rows with
//                  score > det_threshold (a prefix, the rows are in descending score), the rest zero; export: all K rows
// Nothing depends on the frame's place in the batch, on the grid or on the stream.
//
// Launches:
//   a. smoke_stats_kernel   grid (G, B, branches), 1024 threads: the tables of both branches in one launch
//   b. smoke_class_kernel   grid (ceil(H * W / 64), B), one pixel per thread, the C-channel column read once
//   c. smoke_select_kernel  grid (B), 1024 threads: keys (the 3x3 peak test applied while the heat map is read), the
//      exact top-K (block_topk.hpp), the ten regression values (lazy: thread = (entry, row)), the decode, rows, count
// No atomics but the histogram's in LDS, no host synchronisation, 64-bit offsets.
#include "../../include/paddle3d_amd.h"
#include "block_topk.hpp"
#include "common.hpp"
#include "head_math.hpp"
#include "libm_exact.hpp"

#include <algorithm>

namespace {

using namespace pd3;

constexpr int kMaxC = 512, kMaxClasses = 16, kMaxK = 1024, kReg = 10, kCols = 14;
constexpr int kStatThreads = 1024, kClassThreads = 64;
constexpr float kPi = 3.14159f;  // the reference's PI

struct SmokeShape {
  int B, C, G, H, W, HW, nc, K, pitch, mode;
  int64_t bstride;  // floats between two frames of a 3x3 output
  float thr;
};

struct SmokeCam {
  const float *Ks, *trans, *image_size, *depth_ref, *dim_ref;
};

// ---- a. tables: grid (G, B, branches) ---------------------------------------------------------------------------------
__device__ __forceinline__ double stats_fold(double v, double* p) {
  const int t = threadIdx.x;
  p[t] = v;
  __syncthreads();
  for (int s = kStatThreads / 2; s > 0; s >>= 1) {
    if (t < s) p[t] += p[t + s];
    __syncthreads();
  }
  const double r = p[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kStatThreads) void smoke_stats_kernel(const float* __restrict__ f0,
                                                                   const float* __restrict__ f1, SmokeShape sh,
                                                                   float* __restrict__ t0, float* __restrict__ t1) {
  __shared__ double part[kStatThreads];
  const int g = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const float* f = blockIdx.z ? f1 : f0;
  float* tab = blockIdx.z ? t1 : t0;
  if (!tab) return;  // the whole block: this branch's tables were given
  const int cpg = sh.C / sh.G;
  const int64_t plane = (int64_t)sh.H * sh.pitch;
  const float* x = f + (int64_t)b * sh.bstride + (int64_t)g * cpg * plane;
  const int n = cpg * sh.HW;  // <= 512 * HW < 2^31: C * H * W is checked on the host
  // rows without padding: the group is n contiguous floats (the same values in the same order, without the divisions)
  const bool flat = sh.pitch == sh.W;
  const auto at = [&](int i) {
    if (flat) return (double)x[i];
    const int c = i / sh.HW, p = i - c * sh.HW, y = p / sh.W;
    return (double)x[(int64_t)c * plane + (int64_t)y * sh.pitch + (p - y * sh.W)];
  };
  double s = 0.0;
#pragma unroll 8
  for (int i = t; i < n; i += kStatThreads) s += at(i);
  const double m = stats_fold(s, part) / (double)n;
  double q = 0.0;
#pragma unroll 8
  for (int i = t; i < n; i += kStatThreads) {
    const double d = at(i) - m;
    q += d * d;
  }
  const double v = stats_fold(q, part) / (double)n;
  if (t == 0) {
    tab[((int64_t)b * 2 + 0) * sh.G + g] = (float)m;
    tab[((int64_t)b * 2 + 1) * sh.G + g] = (float)(1.0 / sqrt(v + 1e-5));
  }
}

// ---- b. class branch: grid (ceil(HW / 64), B), 64 threads ----------------------------------------------------------
template <int NCMAX>
__global__ __launch_bounds__(kClassThreads) void smoke_class_kernel(const float* __restrict__ feat,
                                                          const float* __restrict__ tables,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, const float* __restrict__ w,
                                                          const float* __restrict__ bias, SmokeShape sh,
                                                          float* __restrict__ heat) {
  __shared__ uint64_t etab[32];
  __shared__ float4 prm[kMaxC];  // mean, rstd, gamma, beta of a channel
  const int b = blockIdx.y;
  lm::exp2f_tab_fill(etab);
  const int cpg = sh.C / sh.G;
  for (int c = threadIdx.x; c < sh.C; c += blockDim.x) {
    const int g = c / cpg;
    prm[c] = make_float4(tables[((int64_t)b * 2 + 0) * sh.G + g], tables[((int64_t)b * 2 + 1) * sh.G + g], gamma[c],
                         beta[c]);
  }
  __syncthreads();
  const auto tab = [&](int i) { return etab[i]; };
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= sh.HW) return;
  const int y = pix / sh.W, xx = pix - y * sh.W;
  const int64_t plane = (int64_t)sh.H * sh.pitch;
  const float* fp = feat + (int64_t)b * sh.bstride + (int64_t)y * sh.pitch + xx;
  float acc[NCMAX];
#pragma unroll
  for (int k = 0; k < NCMAX; ++k) acc[k] = 0.0f;
#pragma unroll 8
  for (int c = 0; c < sh.C; ++c) {
    const float4 p = prm[c];
    const float v = relu_keep_nan(((fp[(int64_t)c * plane] - p.x) * p.y) * p.z + p.w);
#pragma unroll
    for (int k = 0; k < NCMAX; ++k)
      if (k < sh.nc) acc[k] = fmaf(v, w[k * sh.C + c], acc[k]);
  }
  const float lo = 1e-4f, hi = (float)(1 - 1e-4);
#pragma unroll
  for (int k = 0; k < NCMAX; ++k)
    if (k < sh.nc) {
      const float s = sigmoid_exact(acc[k] + bias[k], tab);
      heat[((int64_t)b * sh.nc + k) * sh.HW + pix] = s < lo ? lo : (s > hi ? hi : s);
    }
}

// ---- c. selection and decode: grid (B), kTopkThreads ----------------------------------------------------------------
__device__ __forceinline__ float clip_keep_nan(float v, float hi) { return v < 0.0f ? 0.0f : (v > hi ? hi : v); }

template <bool LAZY>
__global__ __launch_bounds__(kTopkThreads) void smoke_select_kernel(const float* __restrict__ heat,
                                                                    const float* __restrict__ reg_map,
                                                                    const float* __restrict__ feat,
                                                                    const float* __restrict__ tables,
                                                                    const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta,
                                                                    const float* __restrict__ w,
                                                                    const float* __restrict__ bias, SmokeCam cam,
                                                                    SmokeShape sh, uint32_t* __restrict__ keys,
                                                                    float* __restrict__ regs, float* __restrict__ rows,
                                                                    int32_t* __restrict__ counts) {
  __shared__ unsigned long long list[kTopkMaxK];
  __shared__ int hist[kTopkHistWords];
  __shared__ int scr[kTopkScratch];
  __shared__ uint64_t etab[32];
  __shared__ float inv[2][9];
  const int b = blockIdx.x, t = threadIdx.x;
  const int N = sh.nc * sh.HW, K = sh.K;
  lm::exp2f_tab_fill(etab);
  if (t == 64) inverse3(cam.Ks + (int64_t)b * 9, inv[0]);
  if (t == 128 && sh.mode == 0) inverse3(cam.trans + (int64_t)b * 9, inv[1]);
  const auto tab = [&](int i) { return etab[i]; };
  // keys: the 3x3 peak test while the heat map is read
  const float* hm = heat + (int64_t)b * N;
  uint32_t* kb = keys + (int64_t)b * N;
  for (int i = t; i < N; i += kTopkThreads) {
    const int c = i / sh.HW, p = i - c * sh.HW, y = p / sh.W, x = p - y * sh.W;
    const float* pl = hm + (int64_t)c * sh.HW;
    const float h = pl[p];
    bool peak = h > 0.0f && h <= 1.0f;  // a score outside (0, 1], a NaN included, is 0
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int yy = y + dy, xx = x + dx;
        if (yy >= 0 && yy < sh.H && xx >= 0 && xx < sh.W && pl[yy * sh.W + xx] > h) peak = false;
      }
    kb[i] = kScoreKeyOne - __float_as_uint(peak ? h : 0.0f);
  }
  __syncthreads();  // the block's keys are in memory
  const auto key = [&](int i) { return kb[i]; };
  const auto visit = [&](auto f) {
#pragma unroll 4
    for (int i = t; i < N; i += kTopkThreads) f(kb[i]);
  };
  const TopkCut cut = N > K ? block_topk_cut(K, kScoreKeyBits, hist, scr, visit) : TopkCut{kScoreKeyAll, 0};
  block_topk_compact(cut, N, key, [](int i, int) { return (uint32_t)i; }, list, scr);
  block_topk_sort(list, K);
  // the ten regression values of every entry
  float* rg = regs + (int64_t)b * K * kReg;
  if constexpr (LAZY) {
    const int cpg = sh.C / sh.G;
    const int64_t plane = (int64_t)sh.H * sh.pitch;
    const float* tb = tables + (int64_t)b * 2 * sh.G;
    for (int e = t; e < K * kReg; e += kTopkThreads) {
      const int k = e / kReg, j = e - k * kReg;
      const int i = min((int)(uint32_t)list[k], N - 1);  // (always inside: exactly K entries are taken)
      const int p = i % sh.HW, y = p / sh.W, x = p - y * sh.W;
      const float* fp = feat + (int64_t)b * sh.bstride + (int64_t)y * sh.pitch + x;
      const float* wr = w + (int64_t)j * sh.C;
      float acc = 0.0f;
#pragma unroll 4
      for (int c = 0; c < sh.C; ++c) {
        const int g = c / cpg;
        const float v = relu_keep_nan(((fp[(int64_t)c * plane] - tb[g]) * tb[sh.G + g]) * gamma[c] + beta[c]);
        acc = fmaf(v, wr[c], acc);
      }
      rg[e] = acc + bias[j];
    }
  } else {
    for (int e = t; e < K * kReg; e += kTopkThreads) {
      const int k = e / kReg, j = e - k * kReg;
      const int i = min((int)(uint32_t)list[k], N - 1);
      rg[e] = reg_map[((int64_t)b * kReg + j) * sh.HW + i % sh.HW];
    }
  }
  __syncthreads();  // the block's regression values are in memory
  bool kept = false;
  if (t < K) {
    const unsigned long long ent = list[t];
    const int i = min((int)(uint32_t)ent, N - 1);
    const float score = __uint_as_float(kScoreKeyOne - (uint32_t)(ent >> 32));
    const int cls = i / sh.HW, p = i - cls * sh.HW, yi = p / sh.W, xi = p - yi * sh.W;
    const float xs = (float)xi, ys = (float)yi;
    float r[kReg];
#pragma unroll
    for (int j = 0; j < kReg; ++j) r[j] = rg[t * kReg + j];
    if constexpr (LAZY) {
#pragma unroll
      for (int j = 3; j < 6; ++j) r[j] = sigmoid_exact(r[j], tab) - 0.5f;
      const float nrm = sqrtf(r[6] * r[6] + r[7] * r[7]);
      const float d = nrm < 1e-12f ? 1e-12f : nrm;
      r[6] = r[6] / d;
      r[7] = r[7] / d;
    }
    const float depth = r[0] * cam.depth_ref[1] + cam.depth_ref[0];
    const float px = r[1] + xs, py = r[2] + ys;
    const float* Ki = inv[0];
    const float* Ti = inv[1];
    float q0, q1, q2, dr0 = 1.0f, dr1 = 1.0f;
    if (sh.mode == 0) {
      q0 = mat3_row(Ti, 0, px, py, 1.0f);
      q1 = mat3_row(Ti, 1, px, py, 1.0f);
      q2 = mat3_row(Ti, 2, px, py, 1.0f);
    } else {
      dr0 = cam.trans[0];
      dr1 = cam.trans[1];
      q0 = dr0 * px;
      q1 = dr1 * py;
      q2 = 1.0f;
    }
    q0 = q0 * depth;
    q1 = q1 * depth;
    q2 = q2 * depth;
    const float lx = mat3_row(Ki, 0, q0, q1, q2);
    float ly = mat3_row(Ki, 1, q0, q1, q2);
    const float lz = mat3_row(Ki, 2, q0, q1, q2);
    const float* dref = cam.dim_ref + cls * 3;
    const float dl = lm::expf_with(r[3], tab) * dref[0];
    const float dh = lm::expf_with(r[4], tab) * dref[1];
    const float dw = lm::expf_with(r[5], tab) * dref[2];
    ly = ly + dh / 2.0f;
    const float ray = lm::atanf(lx / (lz + 1e-7f));
    float alpha = lm::atanf(r[6] / (r[7] + 1e-7f));
    alpha = alpha - (r[7] >= 0.0f ? kPi / 2.0f : -kPi / 2.0f);
    float roty = alpha + ray;
    if (roty > kPi)
      roty = roty - 2.0f * kPi;
    else if (roty < -kPi)
      roty = roty - (-2.0f * kPi);
    float x0 = xs - r[8] / 2.0f, y0 = ys - r[9] / 2.0f, x1 = xs + r[8] / 2.0f, y1 = ys + r[9] / 2.0f;
    if (sh.mode == 0) {
      const float a0 = mat3_row(Ti, 0, x0, y0, 1.0f), a1 = mat3_row(Ti, 1, x0, y0, 1.0f);
      const float b0 = mat3_row(Ti, 0, x1, y1, 1.0f), b1 = mat3_row(Ti, 1, x1, y1, 1.0f);
      x0 = clip_keep_nan(a0, cam.image_size[0]);
      y0 = clip_keep_nan(a1, cam.image_size[1]);
      x1 = clip_keep_nan(b0, cam.image_size[0]);
      y1 = clip_keep_nan(b1, cam.image_size[1]);
    } else {
      x0 = dr0 * x0;
      y0 = dr1 * y0;
      x1 = dr0 * x1;
      y1 = dr1 * y1;
    }
    kept = sh.mode != 0 || score > sh.thr;
    const float out[kCols] = {(float)cls, alpha, x0, y0, x1, y1, dh, dw, dl, lx, ly, lz, roty, score};
    float* ro = rows + ((int64_t)b * K + t) * kCols;
#pragma unroll
    for (int j = 0; j < kCols; ++j) ro[j] = kept ? out[j] : 0.0f;
  }
  const int count = __syncthreads_count(kept ? 1 : 0);
  if (t == 0) counts[b] = count;
}

struct SmokeWorkspace {
  float *tab_cls, *tab_reg, *heat, *regs;
  uint32_t* keys;
  size_t bytes;
};

SmokeWorkspace smoke_carve(void* base, const SmokeShape& sh) {
  Carver c(base);
  SmokeWorkspace w;
  const size_t B = (size_t)sh.B;
  w.tab_cls = c.take<float>(B * 2 * kMaxC);
  w.tab_reg = c.take<float>(B * 2 * kMaxC);
  w.heat = c.take<float>(B * sh.nc * sh.HW);
  w.keys = c.take<uint32_t>(B * sh.nc * sh.HW);
  w.regs = c.take<float>(B * sh.K * kReg);
  w.bytes = c.off;
  return w;
}

// PD3_OK with `sh` filled, PD3_EINVAL or PD3_EUNSUPPORTED.  channels < 0: the from-maps form (no channel predicate).
int smoke_shape(int batch, int channels, int groups, int feat_h, int feat_w, int pitch, int64_t bstride,
                int num_classes, const int* reg_channels, int max_detection, float det_threshold, int mode, int pred_2d,
                SmokeShape& sh) {
  if (batch < 0 || feat_h <= 0 || feat_w <= 0 || num_classes <= 0 || channels == 0 || !reg_channels ||
      (mode != 0 && mode != 1))
    return PD3_EINVAL;
  const int64_t hw = (int64_t)feat_h * feat_w;
  if (channels > 0) {
    if (groups <= 0 || pitch < feat_w || bstride < (int64_t)channels * feat_h * pitch) return PD3_EINVAL;
    if (channels > kMaxC || channels % groups != 0 || (int64_t)channels * feat_h * pitch >= (int64_t)1 << 31)
      return PD3_EUNSUPPORTED;
  }
  const int want[5] = {1, 2, 3, 2, 2};
  for (int i = 0; i < 5; ++i)
    if (reg_channels[i] != want[i]) return PD3_EUNSUPPORTED;
  if (!pred_2d || num_classes > kMaxClasses || max_detection < 1 || max_detection > kMaxK || max_detection > hw ||
      num_classes * hw >= (int64_t)1 << 30 || batch > 65535)
    return PD3_EUNSUPPORTED;
  sh.B = batch;
  sh.C = channels;
  sh.G = groups;
  sh.H = feat_h;
  sh.W = feat_w;
  sh.HW = (int)hw;
  sh.nc = num_classes;
  sh.K = max_detection;
  sh.pitch = pitch;
  sh.bstride = bstride;
  sh.mode = mode;
  sh.thr = det_threshold;
  return PD3_OK;
}

}  // namespace

extern "C" size_t pd3_smoke_head_workspace(int batch, int feat_h, int feat_w, int num_classes, int max_detection) {
  SmokeShape sh;
  const int reg[5] = {1, 2, 3, 2, 2};
  if (batch <= 0 ||
      smoke_shape(batch, -1, 0, feat_h, feat_w, feat_w, 0, num_classes, reg, max_detection, 0.f, 0, 1, sh) != PD3_OK)
    return 0;
  return smoke_carve(nullptr, sh).bytes;
}

extern "C" int pd3_smoke_head_forward(const void* cls_feat, const void* reg_feat, int64_t batch_stride, int pitch,
                                      const void* cls_gamma, const void* cls_beta, const void* reg_gamma,
                                      const void* reg_beta, const void* cls_tables, const void* reg_tables,
                                      const void* cls_weight, const void* cls_bias, const void* reg_weight,
                                      const void* reg_bias, const void* Ks, const void* trans, const void* image_size,
                                      const void* depth_ref, const void* dim_ref, int batch, int channels, int groups,
                                      int feat_h, int feat_w, int num_classes, const int* reg_channels,
                                      int max_detection, float det_threshold, int mode, int pred_2d, void* rows,
                                      void* counts, void* workspace, size_t workspace_bytes, void* stream) {
  if (channels <= 0) return PD3_EINVAL;
  SmokeShape sh;
  const int st = smoke_shape(batch, channels, groups, feat_h, feat_w, pitch, batch_stride, num_classes, reg_channels,
                             max_detection, det_threshold, mode, pred_2d, sh);
  if (st != PD3_OK) return st;
  if (batch == 0) return PD3_OK;
  if (!cls_feat || !reg_feat || !cls_gamma || !cls_beta || !reg_gamma || !reg_beta || !cls_weight || !cls_bias ||
      !reg_weight || !reg_bias || !Ks || !trans || !depth_ref || !dim_ref || (mode == 0 && !image_size) || !rows ||
      !counts || !workspace)
    return PD3_EINVAL;
  const SmokeWorkspace w = smoke_carve(workspace, sh);
  if (workspace_bytes < w.bytes) return PD3_EWORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float* cf = static_cast<const float*>(cls_feat);
  const float* rf = static_cast<const float*>(reg_feat);
  const float* ct = static_cast<const float*>(cls_tables);
  const float* rt = static_cast<const float*>(reg_tables);
  if (!ct || !rt) {
    smoke_stats_kernel<<<dim3(sh.G, sh.B, 2), kStatThreads, 0, s>>>(cf, rf, sh, ct ? nullptr : w.tab_cls,
                                                                   rt ? nullptr : w.tab_reg);
    if (!ct) ct = w.tab_cls;
    if (!rt) rt = w.tab_reg;
  }
  // 64 pixels per workgroup: at KITTI's 30720 pixels a frame's 480 waves spread over every CU instead of 120
  const dim3 grid((sh.HW + kClassThreads - 1) / kClassThreads, sh.B);
  const float* cg = static_cast<const float*>(cls_gamma);
  const float* cb = static_cast<const float*>(cls_beta);
  const float* cw = static_cast<const float*>(cls_weight);
  const float* cbi = static_cast<const float*>(cls_bias);
  if (sh.nc <= 4)
    smoke_class_kernel<4><<<grid, kClassThreads, 0, s>>>(cf, ct, cg, cb, cw, cbi, sh, w.heat);
  else
    smoke_class_kernel<kMaxClasses><<<grid, kClassThreads, 0, s>>>(cf, ct, cg, cb, cw, cbi, sh, w.heat);
  const SmokeCam cam{static_cast<const float*>(Ks), static_cast<const float*>(trans),
                     static_cast<const float*>(image_size), static_cast<const float*>(depth_ref),
                     static_cast<const float*>(dim_ref)};
  smoke_select_kernel<true><<<sh.B, kTopkThreads, 0, s>>>(
      w.heat, nullptr, rf, rt, static_cast<const float*>(reg_gamma), static_cast<const float*>(reg_beta),
      static_cast<const float*>(reg_weight), static_cast<const float*>(reg_bias), cam, sh, w.keys, w.regs,
      static_cast<float*>(rows), static_cast<int32_t*>(counts));
  return launch_status();
}

extern "C" int pd3_smoke_post_process(const void* heat, const void* regression, const void* Ks, const void* trans,
                                      const void* image_size, const void* depth_ref, const void* dim_ref, int batch,
                                      int feat_h, int feat_w, int num_classes, const int* reg_channels,
                                      int max_detection, float det_threshold, int mode, int pred_2d, void* rows,
                                      void* counts, void* workspace, size_t workspace_bytes, void* stream) {
  SmokeShape sh;
  const int st = smoke_shape(batch, -1, 0, feat_h, feat_w, feat_w, 0, num_classes, reg_channels, max_detection,
                             det_threshold, mode, pred_2d, sh);
  if (st != PD3_OK) return st;
  if (batch == 0) return PD3_OK;
  if (!heat || !regression || !Ks || !trans || !depth_ref || !dim_ref || (mode == 0 && !image_size) || !rows ||
      !counts || !workspace)
    return PD3_EINVAL;
  const SmokeWorkspace w = smoke_carve(workspace, sh);
  if (workspace_bytes < w.bytes) return PD3_EWORKSPACE;
  const SmokeCam cam{static_cast<const float*>(Ks), static_cast<const float*>(trans),
                     static_cast<const float*>(image_size), static_cast<const float*>(depth_ref),
                     static_cast<const float*>(dim_ref)};
  smoke_select_kernel<false><<<sh.B, kTopkThreads, 0, static_cast<hipStream_t>(stream)>>>(
      static_cast<const float*>(heat), static_cast<const float*>(regression), nullptr, nullptr, nullptr, nullptr,
      nullptr, nullptr, cam, sh, w.keys, w.regs, static_cast<float*>(rows), static_cast<int32_t*>(counts));
  return launch_status();
}
