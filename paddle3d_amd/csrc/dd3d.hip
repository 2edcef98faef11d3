// DD3D's FCOS heads and post-processing at inference for gfx950: candidate selection per (level, image), the 3x3
// predictors evaluated LAZILY at the selected entries only, FCOS2DInference's and FCOS3DInference's decode, the per-image
// concatenation, class-wise NMS and the post-NMS cut of a whole batch, every count on the device.
// (reference: paddle3d/models/heads/fcos_heads/fcos2d_head.py:160-186, :334-503, fcos3d_head.py:33-108, :268-296,
//  :519-639, paddle3d/models/detection/dd3d/dd3d.py:144-176, :183-212, paddle3d/utils/transform.py:167-246,
//  paddle3d/models/losses/disentangled_box3d_loss.py:36-60.)
//
// The reference evaluates 59 predictor channels densely over five levels (box2d_reg 4, quat 4 nc, ctr 2 nc, depth nc,
// size 3 nc, conf nc at nc = 5), transposes each, and then runs per level and image a chain of small ops with several
// host synchronisations; at most pre_nms_topk (pixel, class) entries per level and image are ever used.  Here the head
// is LAZY: the 4 + 11 predictor channels of an entry are evaluated at its pixel from the two towers' outputs.
// pd3_dd3d_post_process is the same selection, decode and tail from the reference's dense head outputs.
//
// Arithmetic order (fp32, every operation rounded on its own, -ffp-contract=off; tests/golden/dd3d_numpy.py restates it):
//   sigmoid(x)     1 / (1 + expf(-x)), expf with glibc's bits (libm_exact.hpp)
//   score          sl = sigmoid(logit), sc = sigmoid(centerness), s = sl * sc; candidate iff s > pre_nms_thresh
//                  (thresh_with_ctr) or sl > pre_nms_thresh (else), and s is no NaN
//   selection      per (level, image): key = bits(1.0f) - bits(s); the min(candidates, pre_nms_topk) smallest (key, flat
//                  index pixel * nc + class) pairs.  DEFINITION: ties go to the lower flat index (the reference's
//                  topk(sorted=False) leaves it open); a NaN score is no candidate
//   conv3x3(o)     lazy: acc = +0; for c ascending, ky = 0..2, kx = 0..2 with the tap inside the map:
//                  acc = fmaf(f[c][y + ky - 1][x + kx - 1], w[o][c][ky][kx], acc); v = acc + bias[o] (taps outside are
//                  zero padding: they leave acc as it is)
//   predictors     lazy: box2d_reg v * scale_box2d, then relu (v > 0 ? v : +0, a NaN stays); ctr v * scale_ctr;
//                  size v * scale_size; conf v * scale_conf; depth v * scale_depth + offset_depth; quat as it is.  The 3D
//                  rows are those of the entry's class: row k * ncp + class of each predictor (ncp = 1: class agnostic)
//   locations      (x * stride, y * stride) as floats, + stride / 2 (integer division) with offset "half"
//   box            (lx - r0, ly - r1, lx + r2, ly + r3); score = sqrtf(s)
//   inv_intrinsics once per frame, in double by the adjugate (cofactors / determinant), rounded to fp32
//   mat3(M, p)     ((M[r][0] * p0 + M[r][1] * p1) + M[r][2] * p2) per row
//   norm4 / norm3  sqrtf(((a * a + b * b) + c * c) + d * d), sqrtf((a * a + b * b) + c * c)
//   quat           n = norm4(q), d = n < 1e-7f ? 1e-7f : n (a NaN stays), q = q / d; q = q / norm4(q)
//   depth          ps = sqrtf(Ki[0][0] * Ki[0][0] + Ki[1][1] * Ki[1][1]); depth = depth / (ps * factor)
//                  (scale_depth_by_focal_lengths); depth = depth / max(norm3(mat3(Ki, (lx, ly, 1))), 1e-7f)
//                  (predict_distance); depth < min ? min : (depth > max ? max : depth) (a NaN stays)
//   proj_ctr       (c0 + lx, c1 + ly)
//   egocentric     R = quaternion_to_matrix(q) with two_s = 2 / (((r r + i i) + j j) + k k) and the nine entries as
//                  the reference writes them; ray = mat3(Ki, (cx, cy, 1)), z = ray / norm3(ray); y = (0 - z1 * z0,
//                  1 - z1 * z1, 0 - z1 * z2), y = y / norm3(y); x = cross(y, z) = (y1 z2 - y2 z1, y2 z0 - y0 z2,
//                  y0 z1 - y1 z0); M[r][c] = (x[r] * R[0][c] + y[r] * R[1][c]) + z[r] * R[2][c]; matrix_to_quaternion:
//                  0.5f * sqrtf(max(t, 0)) with t = ((1 + m00) + m11) + m22, ((1 + m00) - m11) - m22,
//                  ((1 - m00) + m11) - m22, ((1 - m00) - m11) + m22 (t > 0 ? t : 0), the signs by _copysign from
//                  m21 - m12, m02 - m20, m10 - m01 ((a < 0) != (b < 0) ? -a : a).  DEFINITION: the reference
//                  renormalises all quaternions of a (level, image) when any norm is off by more than 1e-3
//                  (fcos3d_head.py:60-65); the device never does -- a product of two rotations cannot trip that test
//                  in fp32, and a NaN row stays NaN
//   size           e = expf(v + v), th = 1 - 2 / (1 + e) (tanh), (th + 1) * canon_box_sizes[class][k]
//   scores_3d      score * sigmoid(conf); without a 3D head scores_3d and pred_boxes3d are zero
//   tail           per image the entries of all levels with class < nms_categories (the reference passes
//                  categories = [0..4] to its NMS whatever num_classes is: other classes never survive), ordered by
//                  descending scores_3d (scores without a 3D head), ties to the lower level, then the lower flat index;
//                  a NaN scores_3d orders last.  NMS: area = (x1 - x0) * (y1 - y0), iw = min(ax1, bx1) - max(ax0, bx0),
//                  ih likewise, inter = (iw > 0 ? iw : 0) * (ih > 0 ? ih : 0), iou = inter / ((a + b) - inter); a
//                  pair suppresses iff it has the same class and iou > nms_thresh.  DEFINITION: greedy per class in
//                  descending score, output in descending score (Paddle core's source is not in the reference tree).
//                  post-NMS: if more than post_nms_topk > 0 rows survive, thresh = the post_nms_topk-th largest 2D
//                  score of them and the rows with score >= thresh stay, in NMS order; counts[b] is their number
//                  (ties at thresh can make it exceed post_nms_topk), rows holds the first min(counts[b], R) of them
//   row            20 floats: pred_boxes 4, scores, scores_3d, pred_classes, fpn_levels, locations 2, pred_boxes3d 10
//                  (quat 4, proj_ctr 2, depth, size 3); rows past the count are zero
// Nothing depends on the frame's place in the batch, on the grid or on the stream.
//
// Launches:
//   a. dd_keys_kernel     grid (ceil(max HW / 256), levels, B): the keys of every (pixel, class)
//   b. dd_select_kernel   grid (levels, B), kTopkThreads: the exact top-K (block_topk.hpp), the per-(level, image) count
//   c. dd_decode_kernel   grid (ceil(K / 16), levels, B), 256 threads: 16 lanes per entry, lane j evaluates predictor
//                         row j (lazy) or fetches it from the maps; lane 0 of the group decodes and writes the candidate
//   d. dd_rank_kernel     grid (ceil(levels * K / 256), B): every candidate's rank among the image's candidates by
//                         counting (the sort keys are distinct), the rows in NMS order, the image's total
//   e. dd_nms_mask_kernel grid (cb, cb, B), one wave: the upper triangle of the class-aware suppression bit matrix
//   f. nms_sweep_kernel   (nms_kernels.hpp) grid (B)
//   g. dd_finish_kernel   grid (B), kTopkThreads: the post-NMS cut (block_topk_cut on the 2D scores), rows and counts
// No atomics but the histogram's in LDS, no host synchronisation, 64-bit offsets.
#include "../../include/paddle3d_amd.h"
#include "block_topk.hpp"
#include "common.hpp"
#include "head_math.hpp"
#include "libm_exact.hpp"
#include "nms_kernels.hpp"

#include <algorithm>

namespace {

using namespace pd3;

constexpr uint32_t kNoKey = 0xFFFFFFFFu;  // no candidate: above 2^kScoreKeyBits, never counted, never taken
constexpr int kMaxLevels = 8, kMaxC = 512, kMaxClasses = 16, kRow = 20, kVals = 15;
constexpr int kGroup = 16, kDecodeThreads = 256, kRankThreads = 256, kKeyThreads = 256;
constexpr size_t kLdsBytes = 160 * 1024;  // LDS of a gfx950 CU
constexpr int kFlagCtr = 1, kFlagHalf = 2, kFlagFocal = 4, kFlagAllo = 8, kFlagDist = 16;

struct DdLevel {
  int H, W, stride, pitch;
  int64_t bstride;   // floats between two frames of a tower output
  int64_t key_off;   // keys of the lower levels of one image
  const float *logits, *ctr;
  const float *f2d, *f3d;  // lazy: the towers' outputs
  const float *m[6];       // from maps: box2d_reg, quat, ctr, depth, size, conf
};

struct DdLevels {
  DdLevel lv[kMaxLevels];
};

struct DdCfg {
  int B, L, nc, ncp, wl, C, K, P, R, cap, cats, flags, has3d;
  int64_t kpi;  // keys per image
  float thr, nms_thr, min_depth, max_depth, factor;
};

struct DdWeights {
  const float *w2d, *b2d, *w3d, *b3d, *scales, *intrinsics, *canon;
};

// ---- a. keys: grid (ceil(max HW / 256), levels, B) ------------------------------------------------------------------
__global__ __launch_bounds__(kKeyThreads) void dd_keys_kernel(DdLevels lvs, DdCfg cf, uint32_t* __restrict__ keys) {
  __shared__ uint64_t etab[32];
  lm::exp2f_tab_fill(etab);
  __syncthreads();
  const auto tab = [&](int i) { return etab[i]; };
  const DdLevel& lv = lvs.lv[blockIdx.y];
  const int b = blockIdx.z, HW = lv.H * lv.W;
  const int p = blockIdx.x * kKeyThreads + threadIdx.x;
  if (p >= HW) return;
  const float sc = sigmoid_exact(lv.ctr[(int64_t)b * HW + p], tab);
  uint32_t* kb = keys + (int64_t)b * cf.kpi + lv.key_off + (int64_t)p * cf.nc;
  const float* lg = lv.logits + (int64_t)b * cf.nc * HW + p;
  for (int c = 0; c < cf.nc; ++c) {
    const float sl = sigmoid_exact(lg[(int64_t)c * HW], tab);
    const float s = sl * sc;
    const bool cand = ((cf.flags & kFlagCtr) ? s > cf.thr : sl > cf.thr) && s == s;
    kb[c] = cand ? kScoreKeyOne - __float_as_uint(s) : kNoKey;
  }
}

// ---- b. selection: grid (levels, B), kTopkThreads -------------------------------------------------------------------
__global__ __launch_bounds__(kTopkThreads) void dd_select_kernel(DdLevels lvs, DdCfg cf,
                                                                 const uint32_t* __restrict__ keys,
                                                                 unsigned long long* __restrict__ sel,
                                                                 int32_t* __restrict__ lcount) {
  __shared__ unsigned long long list[kTopkMaxK];
  __shared__ int hist[kTopkHistWords];
  __shared__ int scr[kTopkScratch];
  const DdLevel& lv = lvs.lv[blockIdx.x];
  const int l = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int N = cf.nc * lv.H * lv.W, K = cf.K;
  const uint32_t* kb = keys + (int64_t)b * cf.kpi + lv.key_off;
  int mine = 0;
  for (int i = t; i < N; i += kTopkThreads) mine += kb[i] != kNoKey ? 1 : 0;
  int ncand;
  block_exclusive_scan<kTopkThreads>(mine, scr, ncand);
  const auto key = [&](int i) { return kb[i]; };
  const auto visit = [&](auto f) {
#pragma unroll 4
    for (int i = t; i < N; i += kTopkThreads) f(kb[i]);
  };
  // (uniform) more candidates than K: the radix select, whose precondition that is; else every candidate is taken
  const TopkCut cut = ncand > K ? block_topk_cut(K, kScoreKeyBits, hist, scr, visit) : TopkCut{kScoreKeyAll, 0};
  block_topk_compact(cut, N, key, [](int i, int) { return (uint32_t)i; }, list, scr);
  block_topk_sort(list, K);
  if (t < K) sel[((int64_t)b * cf.L + l) * K + t] = list[t];
  if (t == 0) lcount[b * cf.L + l] = min(ncand, K);
}

// ---- c. predictors and decode: grid (ceil(K / 16), levels, B), 256 threads ----------------------------------------------
__device__ __forceinline__ float norm3(float a, float b, float c) { return sqrtf((a * a + b * b) + c * c); }
__device__ __forceinline__ float norm4(float a, float b, float c, float d) {
  return sqrtf(((a * a + b * b) + c * c) + d * d);
}
__device__ __forceinline__ float sqrt_positive_part(float x) { return sqrtf(x > 0.0f ? x : 0.0f); }
__device__ __forceinline__ float copysign_ref(float a, float b) { return ((a < 0.0f) != (b < 0.0f)) ? -a : a; }

// predictor j - 4 of the 3D head -> (map, channel inside it) for class row cc of ncp
__device__ __forceinline__ void row3d(int r, int ncp, int cc, int& map, int& ch, int& packed) {
  if (r < 4) {
    map = 1, ch = r * ncp + cc, packed = ch;
  } else if (r < 6) {
    map = 2, ch = (r - 4) * ncp + cc, packed = 4 * ncp + ch;
  } else if (r == 6) {
    map = 3, ch = cc, packed = 6 * ncp + ch;
  } else if (r < 10) {
    map = 4, ch = (r - 7) * ncp + cc, packed = 7 * ncp + ch;
  } else {
    map = 5, ch = cc, packed = 10 * ncp + ch;
  }
}

template <bool LAZY>
__global__ __launch_bounds__(kDecodeThreads) void dd_decode_kernel(DdLevels lvs, DdCfg cf, DdWeights wt,
                                                                   const unsigned long long* __restrict__ sel,
                                                                   const int32_t* __restrict__ lcount,
                                                                   float* __restrict__ cand,
                                                                   unsigned long long* __restrict__ skey) {
  __shared__ uint64_t etab[32];
  __shared__ float inv[9];
  __shared__ float vals[kDecodeThreads / kGroup][kGroup];
  const int l = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
  const int cnt = lcount[b * cf.L + l];
  const int e0 = blockIdx.x * (kDecodeThreads / kGroup);
  if (e0 >= cnt) return;  // the whole block
  const DdLevel& lv = lvs.lv[l];
  lm::exp2f_tab_fill(etab);
  if (t == 64 && cf.has3d) inverse3(wt.intrinsics + (int64_t)b * 9, inv);
  const auto tab = [&](int i) { return etab[i]; };
  const int g = t / kGroup, j = t % kGroup, k = e0 + g;
  const bool live = k < cnt;
  const int HW = lv.H * lv.W, N = cf.nc * HW;
  const unsigned long long ent = live ? sel[((int64_t)b * cf.L + l) * cf.K + k] : 0ull;
  const int idx = min((int)(uint32_t)ent, N - 1);  // (always inside: only taken entries are live)
  const int pix = idx / cf.nc, cls = idx - pix * cf.nc, y = pix / lv.W, x = pix - y * lv.W;
  const int nvals = cf.has3d ? kVals : 4;
  if (live && j < nvals) {
    const int cc = cf.ncp > 1 ? cls : 0;
    int map = 0, ch = j, packed = j;
    if (j >= 4) row3d(j - 4, cf.ncp, cc, map, ch, packed);
    float v;
    if constexpr (LAZY) {
      const float* f = (j < 4 ? lv.f2d : lv.f3d) + (int64_t)b * lv.bstride;
      const int64_t plane = (int64_t)lv.H * lv.pitch;
      const int64_t wrow = j < 4 ? j : (int64_t)(cf.wl > 1 ? l : 0) * 11 * cf.ncp + packed;
      const float* w = (j < 4 ? wt.w2d : wt.w3d) + wrow * cf.C * 9;
      const float bias = (j < 4 ? wt.b2d : wt.b3d)[wrow];
      // the nine taps' offsets inside a channel plane, clamped into the map, and whether each lies inside it: the loop
      // over the channels is then free of branches (a tap outside is loaded from the clamped place and left out by a
      // select), so the loads of several channels are in flight while the chain of fmaf advances
      int off[9];
      bool in[9];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int yy = y + ky - 1, xx = x + kx - 1;
          in[ky * 3 + kx] = yy >= 0 && yy < lv.H && xx >= 0 && xx < lv.W;
          off[ky * 3 + kx] = min(max(yy, 0), lv.H - 1) * lv.pitch + min(max(xx, 0), lv.W - 1);
        }
      float acc = 0.0f;
#pragma unroll 4
      for (int c = 0; c < cf.C; ++c) {
        const float* fc = f + (int64_t)c * plane;
        const float* wc = w + c * 9;
        float fv[9], wv[9];
#pragma unroll
        for (int k9 = 0; k9 < 9; ++k9) fv[k9] = fc[off[k9]], wv[k9] = wc[k9];
#pragma unroll
        for (int k9 = 0; k9 < 9; ++k9) acc = in[k9] ? fmaf(fv[k9], wv[k9], acc) : acc;
      }
      v = acc + bias;
      const float* sc = wt.scales + l * 6;
      if (j < 4)
        v = relu_keep_nan(v * sc[0]);
      else if (map == 2)
        v = v * sc[1];
      else if (map == 4)
        v = v * sc[2];
      else if (map == 5)
        v = v * sc[3];
      else if (map == 3)
        v = v * sc[4] + sc[5];
    } else {
      const int per[6] = {4, 4, 2, 1, 3, 1};  // channels of a map per class row
      const int chans = per[map] * (map ? cf.ncp : 1);
      v = lv.m[map][((int64_t)b * chans + ch) * HW + pix];
    }
    vals[g][j] = v;
  }
  __syncthreads();
  if (!live || j != 0) return;
  const float* v = vals[g];
  const float s = __uint_as_float(kScoreKeyOne - (uint32_t)(ent >> 32));
  const float score = sqrtf(s);
  const int half = (cf.flags & kFlagHalf) ? lv.stride / 2 : 0;
  const float lx = (float)(x * lv.stride + half), ly = (float)(y * lv.stride + half);
  float out[kRow];
  out[0] = lx - v[0];
  out[1] = ly - v[1];
  out[2] = lx + v[2];
  out[3] = ly + v[3];
  out[4] = score;
  out[6] = (float)cls;
  out[7] = (float)l;
  out[8] = lx;
  out[9] = ly;
  float s3 = 0.0f;
  if (cf.has3d) {
    const float* Ki = inv;
    float q0 = v[4], q1 = v[5], q2 = v[6], q3 = v[7];
    const float n1 = norm4(q0, q1, q2, q3);
    const float d1 = n1 < 1e-7f ? 1e-7f : n1;
    q0 = q0 / d1, q1 = q1 / d1, q2 = q2 / d1, q3 = q3 / d1;
    const float n2 = norm4(q0, q1, q2, q3);
    q0 = q0 / n2, q1 = q1 / n2, q2 = q2 / n2, q3 = q3 / n2;
    float depth = v[10];
    if (cf.flags & kFlagFocal) {
      const float ps = sqrtf(Ki[0] * Ki[0] + Ki[4] * Ki[4]);
      depth = depth / (ps * cf.factor);
    }
    if (cf.flags & kFlagDist) {
      const float nr = norm3(mat3_row(Ki, 0, lx, ly, 1.0f), mat3_row(Ki, 1, lx, ly, 1.0f), mat3_row(Ki, 2, lx, ly, 1.0f));
      depth = depth / (nr < 1e-7f ? 1e-7f : nr);
    }
    depth = depth < cf.min_depth ? cf.min_depth : (depth > cf.max_depth ? cf.max_depth : depth);
    const float cx = v[8] + lx, cy = v[9] + ly;
    if (cf.flags & kFlagAllo) {
      const float r = q0, i = q1, jj = q2, kk = q3;
      const float two_s = 2.0f / (((r * r + i * i) + jj * jj) + kk * kk);
      const float R[9] = {1.0f - two_s * (jj * jj + kk * kk), two_s * (i * jj - kk * r), two_s * (i * kk + jj * r),
                          two_s * (i * jj + kk * r), 1.0f - two_s * (i * i + kk * kk), two_s * (jj * kk - i * r),
                          two_s * (i * kk - jj * r), two_s * (jj * kk + i * r), 1.0f - two_s * (i * i + jj * jj)};
      float z[3] = {mat3_row(Ki, 0, cx, cy, 1.0f), mat3_row(Ki, 1, cx, cy, 1.0f), mat3_row(Ki, 2, cx, cy, 1.0f)};
      const float nz = norm3(z[0], z[1], z[2]);
      z[0] = z[0] / nz, z[1] = z[1] / nz, z[2] = z[2] / nz;
      float yv[3] = {0.0f - z[1] * z[0], 1.0f - z[1] * z[1], 0.0f - z[1] * z[2]};
      const float ny = norm3(yv[0], yv[1], yv[2]);
      yv[0] = yv[0] / ny, yv[1] = yv[1] / ny, yv[2] = yv[2] / ny;
      const float xv[3] = {yv[1] * z[2] - yv[2] * z[1], yv[2] * z[0] - yv[0] * z[2], yv[0] * z[1] - yv[1] * z[0]};
      float M[9];
#pragma unroll
      for (int rr = 0; rr < 3; ++rr)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[rr * 3 + c] = (xv[rr] * R[c] + yv[rr] * R[3 + c]) + z[rr] * R[6 + c];
      const float m00 = M[0], m11 = M[4], m22 = M[8];
      const float o0 = 0.5f * sqrt_positive_part(((1.0f + m00) + m11) + m22);
      const float ax = 0.5f * sqrt_positive_part(((1.0f + m00) - m11) - m22);
      const float ay = 0.5f * sqrt_positive_part(((1.0f - m00) + m11) - m22);
      const float az = 0.5f * sqrt_positive_part(((1.0f - m00) - m11) + m22);
      q0 = o0;
      q1 = copysign_ref(ax, M[7] - M[5]);
      q2 = copysign_ref(ay, M[2] - M[6]);
      q3 = copysign_ref(az, M[3] - M[1]);
    }
    out[10] = q0, out[11] = q1, out[12] = q2, out[13] = q3;
    out[14] = cx, out[15] = cy, out[16] = depth;
    const float* cb = wt.canon + cls * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float e = lm::expf_with(v[11 + a] + v[11 + a], tab);
      const float th = 1.0f - 2.0f / (1.0f + e);
      out[17 + a] = (th + 1.0f) * cb[a];
    }
    s3 = score * sigmoid_exact(v[14], tab);
  } else {
#pragma unroll
    for (int a = 10; a < kRow; ++a) out[a] = 0.0f;
  }
  out[5] = s3;
  const int64_t pos = (int64_t)b * cf.cap + (int64_t)l * cf.K + k;
  float* ro = cand + pos * kRow;
#pragma unroll
  for (int a = 0; a < kRow; ++a) ro[a] = out[a];
  const float order = cf.has3d ? s3 : score;
  const uint32_t k31 = order != order ? 0x7FFFFFFFu : kScoreKeyOne - __float_as_uint(order);
  skey[pos] = cls < cf.cats ? ((unsigned long long)k31 << 33) | ((unsigned long long)l << 30) | (unsigned long long)idx
                            : ~0ull;
}

// ---- d. rank by counting: grid (ceil(cap / 256), B) ------------------------------------------------------------------
__global__ __launch_bounds__(kRankThreads) void dd_rank_kernel(DdCfg cf, const int32_t* __restrict__ lcount,
                                                               const float* __restrict__ cand,
                                                               const unsigned long long* __restrict__ skey,
                                                               float* __restrict__ srow, int32_t* __restrict__ total) {
  __shared__ unsigned long long tile[kRankThreads];
  const int b = blockIdx.y, t = threadIdx.x;
  const int pos = blockIdx.x * kRankThreads + t;
  const int l = pos / cf.K, k = pos - l * cf.K;
  const unsigned long long* sk = skey + (int64_t)b * cf.cap;
  unsigned long long my = ~0ull;
  if (l < cf.L && k < lcount[b * cf.L + l]) my = sk[pos];
  // (uniform) block 0 always walks: it counts the image's total
  if (!__syncthreads_or(my != ~0ull ? 1 : 0) && blockIdx.x != 0) return;
  int rank = 0, all = 0;
  for (int l2 = 0; l2 < cf.L; ++l2) {
    const int c2 = lcount[b * cf.L + l2];
    for (int k0 = 0; k0 < c2; k0 += kRankThreads) {
      const unsigned long long mine = k0 + t < c2 ? sk[(int64_t)l2 * cf.K + k0 + t] : ~0ull;
      tile[t] = mine;
      all += __syncthreads_count(mine != ~0ull ? 1 : 0);  // the barrier that publishes the tile counts it as well
      const int n = min(kRankThreads, c2 - k0);
#pragma unroll 4
      for (int u = 0; u < n; ++u) rank += tile[u] < my ? 1 : 0;
      __syncthreads();
    }
  }
  if (blockIdx.x == 0 && t == 0) total[b] = all;
  if (my == ~0ull) return;
  const float* src = cand + ((int64_t)b * cf.cap + pos) * kRow;
  float* dst = srow + ((int64_t)b * cf.cap + rank) * kRow;
#pragma unroll
  for (int a = 0; a < kRow; ++a) dst[a] = src[a];
}

// ---- e. bit matrix: grid (cb, cb, B), 64 threads ------------------------------------------------------------------------
__device__ __forceinline__ float iou_xyxy(const float* a, const float* b) {
  const float aa = (a[2] - a[0]) * (a[3] - a[1]), ab = (b[2] - b[0]) * (b[3] - b[1]);
  const float iw = fminf(a[2], b[2]) - fmaxf(a[0], b[0]), ih = fminf(a[3], b[3]) - fmaxf(a[1], b[1]);
  const float inter = (iw > 0.0f ? iw : 0.0f) * (ih > 0.0f ? ih : 0.0f);
  return inter / ((aa + ab) - inter);
}

__global__ __launch_bounds__(64) void dd_nms_mask_kernel(const float* __restrict__ srow,
                                                         const int32_t* __restrict__ total, int cap, int cb_cap,
                                                         float thresh, unsigned long long* __restrict__ mask) {
  __shared__ float col[64 * 5];
  const int b = blockIdx.z, row_blk = blockIdx.y, col_blk = blockIdx.x, lane = threadIdx.x;
  const int n = min(total[b], cap);
  if (col_blk < row_blk || row_blk * 64 >= n || col_blk * 64 >= n) return;
  const float* rows = srow + (int64_t)b * cap * kRow;
  const int col_size = min(n - col_blk * 64, 64), row_size = min(n - row_blk * 64, 64);
  if (lane < col_size) {
    const float* r = rows + (int64_t)(col_blk * 64 + lane) * kRow;
#pragma unroll
    for (int a = 0; a < 4; ++a) col[lane * 5 + a] = r[a];
    col[lane * 5 + 4] = r[6];
  }
  __syncthreads();
  if (lane >= row_size) return;
  const float* r = rows + (int64_t)(row_blk * 64 + lane) * kRow;
  const float me[4] = {r[0], r[1], r[2], r[3]};
  const float cls = r[6];
  unsigned long long bits = 0ull;
  for (int i = row_blk == col_blk ? lane + 1 : 0; i < col_size; ++i)
    if (col[i * 5 + 4] == cls && iou_xyxy(me, col + i * 5) > thresh) bits |= 1ull << i;
  mask[((int64_t)b * cap + row_blk * 64 + lane) * cb_cap + col_blk] = bits;
}

// ---- g. post-NMS cut and rows: grid (B), kTopkThreads -------------------------------------------------------------------
__global__ __launch_bounds__(kTopkThreads) void dd_finish_kernel(DdCfg cf, const float* __restrict__ srow,
                                                                 const int32_t* __restrict__ keep,
                                                                 const int32_t* __restrict__ nkeep,
                                                                 float* __restrict__ rows, int32_t* __restrict__ counts) {
  __shared__ int hist[kTopkHistWords];
  __shared__ int scr[kTopkScratch];
  __shared__ uint32_t best;
  const int b = blockIdx.x, t = threadIdx.x;
  const int nk = min(nkeep[b], cf.cap);
  const int32_t* kp = keep + (int64_t)b * cf.cap;
  const float* sr = srow + (int64_t)b * cf.cap * kRow;
  const auto key = [&](int i) { return kScoreKeyOne - __float_as_uint(sr[(int64_t)kp[i] * kRow + 4]); };
  uint32_t cutoff = kNoKey;  // rows with key <= cutoff stay
  if (cf.P > 0 && nk > cf.P) {  // (uniform)
    const auto visit = [&](auto f) {
      for (int i = t; i < nk; i += kTopkThreads) f(key(i));
    };
    const TopkCut cut = block_topk_cut(cf.P, kScoreKeyBits, hist, scr, visit);
    if (cut.r > 0) {
      cutoff = cut.kc;
    } else {  // the P keys below kc are taken: the cut-off is the largest of them
      if (t == 0) best = 0u;
      __syncthreads();
      uint32_t m = 0u;
      for (int i = t; i < nk; i += kTopkThreads) {
        const uint32_t kk = key(i);
        if (kk < cut.kc) m = max(m, kk);
      }
      atomicMax(&best, m);
      __syncthreads();
      cutoff = best;
    }
  }
  float* out = rows + (int64_t)b * cf.R * kRow;
  int base = 0;
  for (int i0 = 0; i0 < nk; i0 += kTopkThreads) {
    const int i = i0 + t;
    const bool stay = i < nk && key(i) <= cutoff;
    int tot;
    const int pos = base + block_exclusive_scan<kTopkThreads>(stay ? 1 : 0, scr, tot);
    if (stay && pos < cf.R) {
      const float* src = sr + (int64_t)kp[i] * kRow;
#pragma unroll
      for (int a = 0; a < kRow; ++a) out[(int64_t)pos * kRow + a] = src[a];
    }
    base += tot;
  }
  for (int64_t e = (int64_t)min(base, cf.R) * kRow + t; e < (int64_t)cf.R * kRow; e += kTopkThreads) out[e] = 0.0f;
  if (t == 0) counts[b] = base;
}

struct DdWorkspace {
  uint32_t* keys;
  unsigned long long *sel, *skey, *mask;
  int32_t *lcount, *total, *keep, *nkeep;
  float *cand, *srow;
  size_t bytes;
};

DdWorkspace dd_carve(void* base, const DdCfg& cf) {
  Carver c(base);
  DdWorkspace w;
  const size_t B = (size_t)cf.B, cap = (size_t)cf.cap, cb = (cap + 63) / 64;
  w.keys = c.take<uint32_t>(B * (size_t)cf.kpi);
  w.sel = c.take<unsigned long long>(B * cf.L * cf.K);
  w.lcount = c.take<int32_t>(B * cf.L);
  w.cand = c.take<float>(B * cap * kRow);
  w.skey = c.take<unsigned long long>(B * cap);
  w.srow = c.take<float>(B * cap * kRow);
  w.total = c.take<int32_t>(B);
  w.mask = c.take<unsigned long long>(B * cap * cb);
  w.keep = c.take<int32_t>(B * cap);
  w.nkeep = c.take<int32_t>(B);
  w.bytes = c.off;
  return w;
}

// PD3_OK with `cf` and the levels' shapes filled, PD3_EINVAL or PD3_EUNSUPPORTED.  channels < 0: the from-maps form.
int dd_shape(int batch, int levels, const int64_t* table, int channels, int num_classes, int box3d_classes,
             int weight_levels, int pre_nms_topk, int post_nms_topk, int nms_categories, int flags, float pre_nms_thresh,
             float nms_thresh, float min_depth, float max_depth, float factor, DdCfg& cf, DdLevels& lvs) {
  if (batch < 0 || !table || channels == 0 || levels <= 0 || num_classes <= 0 || nms_categories < 0 || flags < 0 ||
      flags >= 32 || (box3d_classes != 1 && box3d_classes != num_classes))
    return PD3_EINVAL;
  if (levels > kMaxLevels || num_classes > kMaxClasses || channels > kMaxC || pre_nms_topk < 1 ||
      pre_nms_topk > kTopkMaxK || !(nms_thresh > 0.0f) || batch > 65535)
    return PD3_EUNSUPPORTED;
  if (channels > 0 && weight_levels != 1 && weight_levels != levels) return PD3_EINVAL;
  int64_t off = 0;
  for (int l = 0; l < levels; ++l) {
    const int64_t* r = table + l * 5;
    if (r[0] <= 0 || r[1] <= 0 || r[2] <= 0) return PD3_EINVAL;
    if (r[0] > 65535 || r[1] > 65535 || r[2] > 65535 || num_classes * r[0] * r[1] >= (int64_t)1 << 30)
      return PD3_EUNSUPPORTED;
    DdLevel& lv = lvs.lv[l];
    lv = DdLevel{};
    lv.H = (int)r[0], lv.W = (int)r[1], lv.stride = (int)r[2];
    lv.pitch = lv.W;
    if (channels > 0) {
      if (r[3] < r[1] || r[4] < (int64_t)channels * r[0] * r[3]) return PD3_EINVAL;
      if (r[3] > 65535) return PD3_EUNSUPPORTED;
      lv.pitch = (int)r[3], lv.bstride = r[4];
    }
    lv.key_off = off;
    off += num_classes * r[0] * r[1];
  }
  const int cap = levels * pre_nms_topk;
  if (nms_sweep_lds(cap) > kLdsBytes || (cap + 63) / 64 > kNmsMaxWords) return PD3_EUNSUPPORTED;
  cf = DdCfg{};
  cf.B = batch, cf.L = levels, cf.nc = num_classes, cf.ncp = box3d_classes, cf.wl = weight_levels, cf.C = channels;
  cf.K = pre_nms_topk, cf.P = post_nms_topk, cf.cap = cap, cf.R = post_nms_topk > 0 ? post_nms_topk : cap;
  cf.cats = nms_categories, cf.flags = flags, cf.kpi = off;
  cf.thr = pre_nms_thresh, cf.nms_thr = nms_thresh, cf.min_depth = min_depth, cf.max_depth = max_depth;
  cf.factor = factor;
  return PD3_OK;
}

bool dd_pointers(const void* const* arr, int levels) {
  if (!arr) return false;
  for (int l = 0; l < levels; ++l)
    if (!arr[l]) return false;
  return true;
}

template <bool LAZY>
int dd_run(const DdLevels& lvs, const DdCfg& cf, const DdWeights& wt, void* rows, void* counts, void* workspace,
           size_t workspace_bytes, void* stream) {
  const DdWorkspace w = dd_carve(workspace, cf);
  if (workspace_bytes < w.bytes) return PD3_EWORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int max_hw = 0;
  for (int l = 0; l < cf.L; ++l) max_hw = std::max(max_hw, lvs.lv[l].H * lvs.lv[l].W);
  dd_keys_kernel<<<dim3((max_hw + kKeyThreads - 1) / kKeyThreads, cf.L, cf.B), kKeyThreads, 0, s>>>(lvs, cf, w.keys);
  dd_select_kernel<<<dim3(cf.L, cf.B), kTopkThreads, 0, s>>>(lvs, cf, w.keys, w.sel, w.lcount);
  constexpr int per = kDecodeThreads / kGroup;
  dd_decode_kernel<LAZY><<<dim3((cf.K + per - 1) / per, cf.L, cf.B), kDecodeThreads, 0, s>>>(lvs, cf, wt, w.sel, w.lcount,
                                                                                           w.cand, w.skey);
  dd_rank_kernel<<<dim3((cf.cap + kRankThreads - 1) / kRankThreads, cf.B), kRankThreads, 0, s>>>(cf, w.lcount, w.cand,
                                                                                               w.skey, w.srow, w.total);
  const int cb = (cf.cap + 63) / 64;
  dd_nms_mask_kernel<<<dim3(cb, cb, cf.B), 64, 0, s>>>(w.srow, w.total, cf.cap, cb, cf.nms_thr, w.mask);
  if (const int rc = launch_lds(nms_sweep_kernel, cf.B, kNmsSweepThreads, nms_sweep_lds(cf.cap), s, w.mask, w.total, 0,
                                cf.cap, cb, w.keep, w.nkeep))
    return rc;
  dd_finish_kernel<<<cf.B, kTopkThreads, 0, s>>>(cf, w.srow, w.keep, w.nkeep, static_cast<float*>(rows),
                                                static_cast<int32_t*>(counts));
  return launch_status();
}

}  // namespace

extern "C" size_t pd3_dd3d_workspace(int batch, int levels, const int64_t* level_table, int num_classes,
                                     int pre_nms_topk) {
  DdCfg cf;
  DdLevels lvs;
  if (batch <= 0 || dd_shape(batch, levels, level_table, -1, num_classes, 1, 1, pre_nms_topk, 0, 0, 0, 0.f, 1.f, 0.f,
                             0.f, 0.f, cf, lvs) != PD3_OK)
    return 0;
  return dd_carve(nullptr, cf).bytes;
}

extern "C" int pd3_dd3d_head_forward(const void* const* logits, const void* const* centerness,
                                     const void* const* box2d_feat, const void* const* box3d_feat,
                                     const int64_t* level_table, const void* box2d_weight, const void* box2d_bias,
                                     const void* box3d_weight, const void* box3d_bias, const void* scales,
                                     const void* intrinsics, const void* canon_box_sizes, int batch, int levels,
                                     int channels, int num_classes, int box3d_classes, int box3d_weight_levels,
                                     int pre_nms_topk, int post_nms_topk, int nms_categories, int flags,
                                     float pre_nms_thresh, float nms_thresh, float min_depth, float max_depth,
                                     float depth_factor, void* rows, void* counts, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  if (channels <= 0) return PD3_EINVAL;
  DdCfg cf;
  DdLevels lvs;
  const int st = dd_shape(batch, levels, level_table, channels, num_classes, box3d_classes, box3d_weight_levels,
                          pre_nms_topk, post_nms_topk, nms_categories, flags, pre_nms_thresh, nms_thresh, min_depth,
                          max_depth, depth_factor, cf, lvs);
  if (st != PD3_OK) return st;
  if (batch == 0) return PD3_OK;
  cf.has3d = box3d_feat != nullptr;
  if (!dd_pointers(logits, levels) || !dd_pointers(centerness, levels) || !dd_pointers(box2d_feat, levels) ||
      (cf.has3d && (!dd_pointers(box3d_feat, levels) || !box3d_weight || !box3d_bias || !intrinsics ||
                    !canon_box_sizes)) ||
      !box2d_weight || !box2d_bias || !scales || !rows || !counts || !workspace)
    return PD3_EINVAL;
  for (int l = 0; l < levels; ++l) {
    lvs.lv[l].logits = static_cast<const float*>(logits[l]);
    lvs.lv[l].ctr = static_cast<const float*>(centerness[l]);
    lvs.lv[l].f2d = static_cast<const float*>(box2d_feat[l]);
    lvs.lv[l].f3d = cf.has3d ? static_cast<const float*>(box3d_feat[l]) : nullptr;
  }
  const DdWeights wt{static_cast<const float*>(box2d_weight), static_cast<const float*>(box2d_bias),
                     static_cast<const float*>(box3d_weight), static_cast<const float*>(box3d_bias),
                     static_cast<const float*>(scales), static_cast<const float*>(intrinsics),
                     static_cast<const float*>(canon_box_sizes)};
  return dd_run<true>(lvs, cf, wt, rows, counts, workspace, workspace_bytes, stream);
}

extern "C" int pd3_dd3d_post_process(const void* const* logits, const void* const* centerness,
                                     const void* const* box2d_reg, const void* const* box3d_quat,
                                     const void* const* box3d_ctr, const void* const* box3d_depth,
                                     const void* const* box3d_size, const void* const* box3d_conf,
                                     const int64_t* level_table, const void* intrinsics, const void* canon_box_sizes,
                                     int batch, int levels, int num_classes, int box3d_classes, int pre_nms_topk,
                                     int post_nms_topk, int nms_categories, int flags, float pre_nms_thresh,
                                     float nms_thresh, float min_depth, float max_depth, float depth_factor, void* rows,
                                     void* counts, void* workspace, size_t workspace_bytes, void* stream) {
  DdCfg cf;
  DdLevels lvs;
  const int st = dd_shape(batch, levels, level_table, -1, num_classes, box3d_classes, 1, pre_nms_topk, post_nms_topk,
                          nms_categories, flags, pre_nms_thresh, nms_thresh, min_depth, max_depth, depth_factor, cf, lvs);
  if (st != PD3_OK) return st;
  if (batch == 0) return PD3_OK;
  const void* const* maps3d[5] = {box3d_quat, box3d_ctr, box3d_depth, box3d_size, box3d_conf};
  cf.has3d = box3d_quat != nullptr;
  for (int m = 0; m < 5; ++m)
    if ((maps3d[m] != nullptr) != (cf.has3d != 0) || (cf.has3d && !dd_pointers(maps3d[m], levels))) return PD3_EINVAL;
  if (!dd_pointers(logits, levels) || !dd_pointers(centerness, levels) || !dd_pointers(box2d_reg, levels) ||
      (cf.has3d && (!intrinsics || !canon_box_sizes)) || !rows || !counts || !workspace)
    return PD3_EINVAL;
  for (int l = 0; l < levels; ++l) {
    lvs.lv[l].logits = static_cast<const float*>(logits[l]);
    lvs.lv[l].ctr = static_cast<const float*>(centerness[l]);
    lvs.lv[l].m[0] = static_cast<const float*>(box2d_reg[l]);
    for (int m = 0; m < 5; ++m) lvs.lv[l].m[1 + m] = cf.has3d ? static_cast<const float*>(maps3d[m][l]) : nullptr;
  }
  const DdWeights wt{nullptr, nullptr, nullptr, nullptr, nullptr, static_cast<const float*>(intrinsics),
                     static_cast<const float*>(canon_box_sizes)};
  return dd_run<false>(lvs, cf, wt, rows, counts, workspace, workspace_bytes, stream);
}
