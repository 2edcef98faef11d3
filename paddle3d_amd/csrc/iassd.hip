// IA-SSD on the device: one scale of SAModuleMSG_WithSampling.forward (models/detection/iassd/iassd_modules.py:204-221)
// as one kernel, from the ball query to the max pool over nsample, with no idx and no [B, *, m, nsample] tensor in
// global memory; and IASSD_Head.generate_predicted_boxes with PointResidual_BinOri_Coder.decode_paddle
// (iassd_head.py:606-621, iassd_coder.py:76-121) as one kernel.  The conventions are csrc/pvrcnn.hip's
// (stack_sa_pool_kernel): the factorised first convolution, eval BatchNorms as scale / shift, relu and max that keep a
// NaN, the 16x16x4 fp32 MFMA as an ascending fmaf chain, padded LDS rows, 64-bit offsets, no atomics.
//
// sa_msg_pool.  The scale's mlp is three times Conv2d / BN / ReLU, (3 + C) -> c1 -> c2 -> c3.  The first convolution is
// linear in [d; f], so the caller forms features_in = features @ W1[:, 3:]^T once over the n source points and passes
// w_pos = W1[:, :3]:
//
//   h1[s, j] = relu(scale1[j] * (features_in[b, idx_s, j] + ((w_pos[j,0] * dx + w_pos[j,1] * dy) + w_pos[j,2] * dz))
//                   + shift1[j])                                                                  (no FMA)
//   h2[s, c] = relu(scale2[c] * (sum_j w2[c, j] * h1[s, j]) + shift2[c])                          (no FMA outside the sum)
//   h3[s, c] = relu(scale3[c] * (sum_j w3[c, j] * h2[s, j]) + shift3[c])
//   out[c]   = max_s h3[s, c]
//
// with idx exactly pd3_ball_query_batch's row (csrc/pointnet2.hip: d2 < r2 on the squares of (new - x), a NaN is no hit,
// the first nsample hits in index order), d = xyz[b, idx_s] - new_xyz.  Unused slots repeat the first hit, which a max
// does not see: the max runs over the hits.  A row without a hit is point 0 of the frame, a real point: its own
// features_in row and d = xyz[b, 0] - new_xyz, one slot.  Each sum over j is an ascending-j fp32 fmaf chain from 0: what
// v_mfma_f32_16x16x4_f32 computes, so a VALU fmaf loop gives the same bits and the result depends neither on the tiling
// nor on where a row sits in the launch.  relu(v) = v > 0 ? v : +0 (a NaN stays); the max keeps a NaN once it has met one.
//
// The widths are run-time values walked in 16-column tiles (one kernel, no instance per triple).  At 256 x 256 a weight
// matrix is 256 KiB: it fits neither a wave's registers nor the LDS, so its fragments come from L2 and what matters is
// how many rows each fetched fragment serves.  A workgroup of four waves therefore takes a PASS of 64 activation rows =
// four row tiles of 16 slots: four queries at nsample <= 16, two at <= 32, one above (query i of the pass owns rows
// i * 64 / Q ...).  Per pass:
//   query    the 4 / Q waves of a query each scan a contiguous share of the frame's 64-point steps as ball_query_kernel
//            does (__ballot + mbcnt place the hits) and leave idx, d and a hit count in their own LDS list; the
//            query's row is the lists in share order, cut at nsample.  A row tile none of whose slots is a hit is
//            dead: no layer computes it and the pool does not read it.
//   layer 1  16 .. 256 threads per row (c1 rounded up to a power of two), the channel fastest (features_in rows are read
//            contiguously; the row's list entry is looked up once, no division per element), into buffer A
//            as [64, c1] with row stride c1 + 4 floats (the A-fragment reads of 16 rows x 4 consecutive j then touch
//            64 different banks: (c + 4) / 4 is odd for every c that is a multiple of 16).
//   layer 2  A -> buffer B [64, c2 + 4], layer 3 B -> A [64, c3 + 4]: cin / 4 steps of
//            __builtin_amdgcn_mfma_f32_16x16x4f32 per 16 x 16 output tile (A[i = lane & 15][k = lane >> 4] =
//            h[i][4 * step + k], B[k][n = lane & 15] = w[16 * tile + n][4 * step + k]; D: column lane & 15, rows
//            4 * (lane >> 4) + reg).  With four or more column tiles a wave takes the column tiles w, w + 4, ... and
//            all four row tiles, so a weight fragment fetched from L2 serves the pass's 64 rows (four accumulators);
//            with fewer, wave w takes row tile w and every column tile (the weights are then <= 48 rows).
//   pool     a thread per (query, channel) takes the max over the query's hit slots of buffer A and stores it,
//            the channel fastest.
// Block barriers separate the phases.  LDS: 64 * (max(c1, c3) + c2 + 8) floats + 2.3 KiB, 11 KiB at 16/16/32, 133 KiB at
// 256/256/256 (one workgroup per CU there).
//
// iassd_decode.  A thread per row:
//   k = argmax of cls_preds[row] (the first maximum wins; a NaN counts as the maximum, so the first NaN wins);
//   with mean_size: (dxa, dya, dza) = mean_size[k], diagonal = sqrt(dxa * dxa + dya * dya),
//     x = xt * diagonal + xa, y = yt * diagonal + ya, z = zt * dza + za, dx = exp(dxt) * dxa, dy = exp(dyt) * dya,
//     dz = exp(dzt) * dza; without: x = xt + xa, ..., dx = exp(dxt), ...;
//   bin = argmax of box_preds[row, 6 : 6 + bins] under the same rule, res = box_preds[row, 6 + bins + bin];
//   heading = ((float(bin) * bin_inter - pi) + half) + res * half with bin_inter = float(2 pi / bins), half =
//   float(pi / bins) and pi = float(pi), each rounded from fp64 once (the reference's Python scalars).
// exp is libm_exact.hpp's expf (glibc's bits).
//
// No FMA but the MFMA chain (-ffp-contract=off).  tests/golden/iassd_numpy.py restates both in the same order and both
// equal it bit for bit.
#include "common.hpp"
#include "head_math.hpp"
#include "libm_exact.hpp"
#include "pointnet2_common.hpp"

#include <cmath>

namespace {

using pd3::pn2::ballot_rank;
using pd3::relu_keep_nan;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / pd3::kWave;
constexpr int kRows = 64;        // activation rows of a pass: four row tiles of 16 slots
constexpr int kTiles = kRows / 16;
constexpr int kMaxSample = 64;   // a row of idx is one wave's lanes
constexpr int kMaxWidth = 256;
constexpr int kMaxBlocks = 2048;  // 8 per CU: the workgroups walk the rest of the passes

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float max_keep_nan(float acc, float v) { return (v > acc || v != v) ? v : acc; }

// One Conv / BN / ReLU layer over the pass's live row tiles: in [64, cin] (row stride ins) -> out [64, cout] (row
// stride outs), both in LDS.  Every thread of the workgroup calls it; `live` has bit r set for a live row tile.
__device__ __forceinline__ void mlp_layer(const float* in, int cin, int ins, float* out, int cout, int outs,
                                          const float* __restrict__ w, const float* __restrict__ scale,
                                          const float* __restrict__ shift, unsigned live, int wave, int lane) {
  const int nt = cout >> 4, ks = cin >> 2;
  const bool wide = nt >= kWaves;
  const int col = lane & 15, kq = lane >> 4;
  const int r0 = wide ? 0 : wave;
  const unsigned mine = wide ? live : (live >> wave) & 1u;  // bit r: row tile r0 + r is this wave's and live
  if (mine == 0) return;
  const bool l0 = mine & 1u, l1 = mine & 2u, l2 = mine & 4u, l3 = mine & 8u;
  const float* a0 = in + ((r0 + 0) * 16 + col) * ins + kq;
  const float* a1 = a0 + 16 * ins;
  const float* a2 = a0 + 32 * ins;
  const float* a3 = a0 + 48 * ins;
  for (int t = wide ? wave : 0; t < nt; t += wide ? kWaves : 1) {
    const int c = 16 * t + col;
    const float* wr = w + (int64_t)c * cin + kq;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0, acc2 = acc0, acc3 = acc0;
    if (mine == 0xFu) {  // the full pass: nothing between the MFMAs but their operands
      for (int k = 0; k < ks; ++k) {
        const float b = wr[4 * k];
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[4 * k], b, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[4 * k], b, acc1, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[4 * k], b, acc2, 0, 0, 0);
        acc3 = __builtin_amdgcn_mfma_f32_16x16x4f32(a3[4 * k], b, acc3, 0, 0, 0);
      }
    } else {
      for (int k = 0; k < ks; ++k) {
        const float b = wr[4 * k];
        if (l0) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[4 * k], b, acc0, 0, 0, 0);
        if (l1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[4 * k], b, acc1, 0, 0, 0);
        if (l2) acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[4 * k], b, acc2, 0, 0, 0);
        if (l3) acc3 = __builtin_amdgcn_mfma_f32_16x16x4f32(a3[4 * k], b, acc3, 0, 0, 0);
      }
    }
    const float sc = scale[c], sh = shift[c];
    float* o = out + (r0 * 16 + 4 * kq) * outs + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (l0) o[(0 + r) * outs] = relu_keep_nan(sc * acc0[r] + sh);
      if (l1) o[(16 + r) * outs] = relu_keep_nan(sc * acc1[r] + sh);
      if (l2) o[(32 + r) * outs] = relu_keep_nan(sc * acc2[r] + sh);
      if (l3) o[(48 + r) * outs] = relu_keep_nan(sc * acc3[r] + sh);
    }
  }
}

// waves_per_eu: the scan phase hides its loads behind other waves; without the hint the allocator takes 84 + 16 registers
// (4 waves per SIMD), with it 74 and no scratch (6)
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(6, 8))) void sa_msg_pool_kernel(
    const float* __restrict__ new_xyz, const float* __restrict__ xyz, const float* __restrict__ features_in,
    const float* __restrict__ w_pos, const float* __restrict__ scale1, const float* __restrict__ shift1,
    const float* __restrict__ w2, const float* __restrict__ scale2, const float* __restrict__ shift2,
    const float* __restrict__ w3, const float* __restrict__ scale3, const float* __restrict__ shift3, int64_t total,
    int m, int n, int c1, int c2, int c3, float r2, int nsample, int qpp, float* __restrict__ out, int64_t ld_out) {
  extern __shared__ __attribute__((aligned(16))) float ia_smem[];
  __shared__ int s_idx[kWaves][kMaxSample];
  __shared__ float s_d[kWaves][3][kMaxSample];
  __shared__ int s_cnt[kWaves];  // hits in the wave's list, -1: no such query
  __shared__ int64_t s_frame[kWaves];  // the frame of the wave's query
  const int sa = (c1 > c3 ? c1 : c3) + 4, sb = c2 + 4;
  float* buf_a = ia_smem;
  float* buf_b = ia_smem + kRows * sa;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sp = kRows / qpp;  // rows of a query
  const int sp_log = qpp == 4 ? 4 : (qpp == 2 ? 5 : 6);
  const int tpr_log = c1 <= 16 ? 4 : (c1 <= 32 ? 5 : (c1 <= 64 ? 6 : (c1 <= 128 ? 7 : 8)));  // threads per row of layer 1
  const int wpq = kWaves / qpp;  // waves that scan for a query: each a contiguous share of the 64-point steps
  const int64_t passes = (total + qpp - 1) / qpp;
  const int64_t share = 64 * (((int64_t)(n + 63) / 64 + wpq - 1) / wpq);
  const int qi = wave / wpq, seg = wave - qi * wpq;
  const int first = (int)(seg * share < n ? seg * share : n), last = (int)((seg + 1) * share < n ? (seg + 1) * share : n);

  // hits of the pass's query i over its waves' lists, cut at nsample; -1: no such query
  auto hits_of = [&](int i) {
    int c = s_cnt[i * wpq];
    if (c < 0) return -1;
    for (int k = 1; k < wpq; ++k) c += s_cnt[i * wpq + k];
    return c < nsample ? c : nsample;
  };

  for (int64_t pass = blockIdx.x; pass < passes; pass += gridDim.x) {
    // ---- query: wave (qi, seg) collects the first nsample hits of its share of the frame's points, their index and
    // offset from the query, in its own list; the query's row is the lists in segment order, cut at nsample
    {
      const int64_t gq = pass * qpp + qi;
      int cnt = -1;
      if (gq < total) {
        const int64_t b = gq / m;
        const float* cq = new_xyz + gq * 3;
        const float nx = cq[0], ny = cq[1], nz = cq[2];
        const float* p = xyz + b * n * 3;
        cnt = 0;
        for (int base = first; base < last && cnt < nsample; base += 64) {
          const int k = base + lane;
          bool hit = false;
          float dx = 0.f, dy = 0.f, dz = 0.f;
          if (k < last) {
            dx = p[3 * (int64_t)k] - nx, dy = p[3 * (int64_t)k + 1] - ny, dz = p[3 * (int64_t)k + 2] - nz;
            hit = (dx * dx + dy * dy) + dz * dz < r2;  // the squares of ball_query_kernel's (new - x)
          }
          const uint64_t mask = __ballot(hit);
          if (mask == 0) continue;
          const int pos = cnt + ballot_rank(mask);
          if (hit && pos < nsample) {
            s_idx[wave][pos] = k;
            s_d[wave][0][pos] = dx;
            s_d[wave][1][pos] = dy;
            s_d[wave][2][pos] = dz;
          }
          cnt += __popcll(mask);
        }
        if (cnt > nsample) cnt = nsample;
      }
      if (lane == 0) s_cnt[wave] = cnt, s_frame[wave] = gq / m;
    }
    __syncthreads();

    unsigned live = 0;
#pragma unroll
    for (int r = 0; r < kTiles; ++r) {
      const int i = (r * 16) / sp, slot0 = r * 16 - i * sp, cnt = hits_of(i);
      if (cnt >= 0 && slot0 < (cnt < 1 ? 1 : cnt)) live |= 1u << r;
    }

    // ---- layer 1: 2^tpr_log threads per row of the live row tiles, the channel fastest; slots behind the hits are
    // slot 0 again, a row without a hit is point 0 of the frame (ball_query_kernel's fill)
    for (int row = threadIdx.x >> tpr_log; row < kRows; row += kThreads >> tpr_log) {
      if (!((live >> (row >> 4)) & 1u)) continue;
      const int i = row >> sp_log, s = row - (i << sp_log), cnt = hits_of(i);
      const int64_t gq = pass * qpp + i, b = s_frame[i * wpq];
      int64_t src = 0;
      float dx, dy, dz;
      if (cnt > 0) {
        int w = i * wpq, pos = s < cnt ? s : 0;
        for (int k = 1; k < wpq && pos >= s_cnt[w]; ++k) pos -= s_cnt[w++];
        src = s_idx[w][pos];
        dx = s_d[w][0][pos], dy = s_d[w][1][pos], dz = s_d[w][2][pos];
      } else {
        const float* p = xyz + b * n * 3;
        const float* cq = new_xyz + gq * 3;
        dx = p[0] - cq[0], dy = p[1] - cq[1], dz = p[2] - cq[2];
      }
      const float* f = features_in ? features_in + (b * n + src) * c1 : nullptr;
      for (int j = threadIdx.x & ((1 << tpr_log) - 1); j < c1; j += 1 << tpr_log) {
        const float fv = f ? f[j] : 0.f;
        const float pos = (w_pos[3 * j] * dx + w_pos[3 * j + 1] * dy) + w_pos[3 * j + 2] * dz;
        buf_a[row * sa + j] = relu_keep_nan(scale1[j] * (fv + pos) + shift1[j]);
      }
    }
    __syncthreads();
    mlp_layer(buf_a, c1, sa, buf_b, c2, sb, w2, scale2, shift2, live, wave, lane);
    __syncthreads();
    mlp_layer(buf_b, c2, sb, buf_a, c3, sa, w3, scale3, shift3, live, wave, lane);
    __syncthreads();

    // ---- pool: the max over the hit slots (one slot for a row without a hit)
    for (int e = threadIdx.x; e < qpp * c3; e += kThreads) {
      const int i = e / c3, c = e - i * c3, cnt = hits_of(i);
      if (cnt < 0) continue;
      const int lim = cnt < 1 ? 1 : cnt;
      const float* h = buf_a + (i * sp) * sa + c;
      float best = 0.f;  // every term is >= +0 (or a NaN): 0 is neutral for the max
      for (int s = 0; s < lim; ++s) best = max_keep_nan(best, h[s * sa]);
      out[(pass * qpp + i) * ld_out + c] = best;
    }
    __syncthreads();  // the pass is read before the next one is written
  }
}

// The first maximum of v[0 .. k) with a NaN counting as the maximum (torch.argmax).
__device__ __forceinline__ int argmax_first(const float* __restrict__ v, int k) {
  int best = 0;
  float bv = v[0];
  for (int i = 1; i < k; ++i) {
    const float x = v[i];
    if (bv == bv && (x > bv || x != x)) best = i, bv = x;
  }
  return best;
}

__global__ __launch_bounds__(256) void iassd_decode_kernel(const float* __restrict__ cls_preds,
                                                           const float* __restrict__ box_preds,
                                                           const float* __restrict__ centers, int64_t ld_centers,
                                                           const float* __restrict__ mean_size, int64_t m,
                                                           int num_classes, int bins, float bin_inter, float pi,
                                                           float half, float* __restrict__ boxes) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= m) return;
  const float* e = box_preds + row * (6 + 2 * bins);
  const float* c = centers + row * ld_centers;
  float* o = boxes + row * 7;
  const float ex = pd3::lm::expf(e[3]), ey = pd3::lm::expf(e[4]), ez = pd3::lm::expf(e[5]);
  if (mean_size) {
    const float* a = mean_size + 3 * argmax_first(cls_preds + row * num_classes, num_classes);
    const float dxa = a[0], dya = a[1], dza = a[2];
    const float diagonal = sqrtf(dxa * dxa + dya * dya);
    o[0] = e[0] * diagonal + c[0];
    o[1] = e[1] * diagonal + c[1];
    o[2] = e[2] * dza + c[2];
    o[3] = ex * dxa;
    o[4] = ey * dya;
    o[5] = ez * dza;
  } else {
    o[0] = e[0] + c[0];
    o[1] = e[1] + c[1];
    o[2] = e[2] + c[2];
    o[3] = ex;
    o[4] = ey;
    o[5] = ez;
  }
  const int bin = argmax_first(e + 6, bins);
  const float rg = ((float)bin * bin_inter - pi) + half;
  o[6] = rg + e[6 + bins + bin] * half;
}

bool width_ok(int c) { return c >= 16 && c <= kMaxWidth && c % 16 == 0; }

}  // namespace

extern "C" {

int pd3_sa_msg_pool(const float* new_xyz, const float* xyz, const float* features_in, const float* w_pos,
                    const float* scale1, const float* shift1, const float* w2, const float* scale2,
                    const float* shift2, const float* w3, const float* scale3, const float* shift3, int batch, int m,
                    int n, int c1, int c2, int c3, float radius, int nsample, float* out, int64_t ld_out,
                    void* stream) {
  if (batch < 0 || m < 0 || n < 0 || c1 < 1 || c2 < 1 || c3 < 1 || nsample < 1 || ld_out < c3) return PD3_EINVAL;
  if (!width_ok(c1) || !width_ok(c2) || !width_ok(c3) || nsample > kMaxSample) return PD3_EUNSUPPORTED;
  const int64_t total = (int64_t)batch * m;
  if (total == 0) return PD3_OK;
  if (n == 0 || !new_xyz || !xyz || !w_pos || !scale1 || !shift1 || !w2 || !scale2 || !shift2 || !w3 || !scale3 ||
      !shift3 || !out)
    return PD3_EINVAL;
  const int qpp = nsample <= 16 ? 4 : (nsample <= 32 ? 2 : 1);
  const int64_t passes = pd3::ceil_div(total, qpp);
  const int lds = kRows * ((c1 > c3 ? c1 : c3) + c2 + 8) * (int)sizeof(float);
  const dim3 grid((unsigned)(passes < kMaxBlocks ? passes : kMaxBlocks));
  const int rc = pd3::launch_lds(sa_msg_pool_kernel, grid, kThreads, lds, (hipStream_t)stream, new_xyz, xyz, features_in,
                                 w_pos, scale1, shift1, w2, scale2, shift2, w3, scale3, shift3, total, m, n, c1, c2, c3,
                                 radius * radius, nsample, qpp, out, ld_out);
  return rc ? rc : pd3::launch_status();
}

int pd3_iassd_decode(const float* cls_preds, const float* box_preds, const float* centers, int64_t ld_centers,
                     const float* mean_size, int64_t m, int num_classes, int bins, float* boxes, void* stream) {
  if (m < 0 || num_classes < 1 || bins < 1 || ld_centers < 3) return PD3_EINVAL;
  if (m == 0) return PD3_OK;
  if (!cls_preds || !box_preds || !centers || !boxes) return PD3_EINVAL;
  const int64_t blocks = pd3::ceil_div(m, 256);
  if (blocks > INT32_MAX) return PD3_EUNSUPPORTED;
  const double bin_inter = 2.0 * M_PI / bins;
  hipLaunchKernelGGL(iassd_decode_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, cls_preds,
                     box_preds, centers, ld_centers, mean_size, m, num_classes, bins, (float)bin_inter, (float)M_PI,
                     (float)(bin_inter / 2), boxes);
  return pd3::launch_status();
}

}  // extern "C"
