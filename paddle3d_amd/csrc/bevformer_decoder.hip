// BEVFormer's decoder, detection head and NMS-free decode (paddle3d/models/transformers/decoders.py, decoder_layers.py,
// attentions/multihead_attention.py, attentions/spatial_cross_attention.py:531-640, utils/box_coder.py:133-214,
// utils/box.py:107-138, detection/bevformer/bevformer_head.py:613-634): the three stages that are more than Linear
// layers, each as one kernel, fp32.
//
// pd3_mha_forward                    paddle.nn.MultiHeadAttention's core without masks or dropout
//   q [B, Nq, M, d], k and v [B, Nk, M, d] (the Linear outputs viewed per head), scale (host float, head_dim ** -0.5
//   rounded to fp32) -> out [B, Nq, M * d].  Per (b, m, query i), in this order:
//     qs_c = q_ic * scale
//     s_j  = fmaf(qs_{d-1}, k_{j,d-1}, ... fmaf(qs_1, k_j1, fmaf(qs_0, k_j0, +0)))         ascending c
//     mx   = s_0 when s_0 is a NaN, else the largest s_j that is no NaN (what `mx = s_0; mx = s_j > mx ? s_j : mx`
//            in index order gives, the convention of group_softmax; the sign of a zero maximum does not reach e)
//     e_j  = expf(s_j - mx)  (glibc's bits, libm_exact.hpp)
//     p_l  = ((0 + e_l) + e_{l+64}) + e_{l+128} ...  for l = 0 .. 63 (p_l = 0 for l >= Nk);
//     sum  = the halving tree over p: 32 times p_l + p_{l+32}, then 16 times + 16, ... down to one value
//            (an association that depends on Nk only)
//     a_j  = e_j / sum
//     out_c = fmaf(a_{Nk-1}, v_{Nk-1,c}, ... fmaf(a_1, v_1c, fmaf(a_0, v_0c, +0)))         ascending j
//   Both products are v_mfma_f32_16x16x4_f32, whose result is the k-ordered fp32 fmaf chain (csrc/pvrcnn.hip relies on
//   the same): queries as M, keys (then channels) as N.  Exact two-pass softmax: a workgroup (256 threads, 4 waves)
//   owns 16 queries of one (b, m) and keeps their Nk scores in LDS, so the result depends neither on the tiling nor on
//   where a frame sits in the batch.
//     phase 1  the scaled query tile [16][d + 4] goes to LDS; each wave walks pairs of 16-key tiles (two independent
//              accumulators, d / 4 steps each) and writes S [16][SN], SN = 16 * ceil(Nk / 16) + 4 floats (4 * odd: the A
//              fragment reads of 16 rows x 4 consecutive columns touch 64 different banks)
//     phase 2  wave w owns rows 4 w .. 4 w + 3: lane-strided maximum, expf (its table in LDS, four independent
//              evaluations per lane and step), partial sums, the xor butterfly (every lane ends with the same bits,
//              addition being commutative), division; the padded columns are written as +0
//     phase 3  wave w owns the channel tiles w, w + 4, ...: one accumulator, 4 * ceil(Nk / 16) dependent steps
//   In phases 1 and 3 the operands from global memory (k, v) are fetched 8 MFMA steps at a time into a ring of
//   registers, 3 (phase 1) and 6 (phase 3) such items ahead of the MFMAs that use them -- a wave that waited for each
//   fetch spent most of its time waiting; the order of the steps is untouched.
//   Padded query rows load 0 and are never stored; padded keys load 0 for k and v, their scores are never stored and
//   their weight is +0 (an accumulator that starts at +0 and adds a_j * v_j with a_j >= +0 is never -0, so the padded
//   steps fmaf(+0, +0, acc) leave every bit).  No address outside q, k, v is formed for a load.
//   Supported (mha_supported): d % 16 == 0, d <= 128 and Nk <= 2048 -- LDS 16 * (SN + d + 4) * 4 B <= 139776 B of the
//   160 KiB, and nothing in the kernel keeps more than one accumulator pair in registers whatever d is -- with q, k, v
//   and out 16-byte aligned.  Anything else: PD3_EUNSUPPORTED without a launch.
//
// pd3_bevformer_dec_ca               CustomMSDeformableAttention.forward's sampling (:600-632, reference_points of 2)
//   value [B, S, M, C] (projected), offsets [B, Q, M, L, P, 2], logits [B, Q, M, L*P], reference_points [B, Q, Lr, 2]
//   with Lr = 1 (broadcast over the levels) or Lr = L -> out [B, Q, M*C].  Per (b, q, m): the softmax of
//   csrc/bevformer.hip; col = 0; for l (outer), p (inner), i = l*P + p: loc = ref[b, q, Lr == 1 ? 0 : l] +
//   (off_x / (float)W_l, off_y / (float)H_l); the msda_point.hpp step against value row b: col = col + val * a_i;
//   out = col.  The lane map, group_softmax and AttnDims are bevformer_attn.hpp's (TSA's single-queue case).
//   Supported: C % 4 == 0 with 16-B aligned value and out, L*P <= 32.
//
// pd3_nms_free_decode                NMSFreeCoder.decode for the whole batch, one 1024-thread workgroup per frame
//   cls [B, Q, K] logits, bbox [B, Q, code] (code 8 or 10, metres), post_center_range[6] host floats, max_num <= 1024,
//   score_threshold (double; negative: None), bottom_center -> boxes [B, max_num, code-1], scores [B, max_num],
//   labels [B, max_num] int32, count [B] int32.
//     score = 1.0f / (1.0f + expf(-x)); the max_num largest of the Q*K scores ordered by (score descending, flat index
//     ascending) (block_topk.hpp on the keys bits(1.0f) - bits(score), recomputed from cls in every pass: no
//     workspace); a NaN score sorts last and is never kept.
//     label = idx % K, row = idx / K, b = bbox[row]; rot = atan2f(b6, b7); w, l, h = expf(b2), expf(b3), expf(b5);
//     box = (b0, b1, b4, w, l, h, rot[, b8, b9]).
//     threshold (box_coder.py:158-166; applied when score_threshold > 0): top = the best score.  top > (float)thr:
//     keep score > (float)thr.  Otherwise tmp = thr (double); repeat tmp = tmp * 0.9; tmp < 0.01: keep all; top >=
//     (float)tmp: keep score >= (float)tmp.
//     mask = b0 >= r0 && b1 >= r1 && b4 >= r2 && b0 <= r3 && b1 <= r4 && b4 <= r5 && threshold.
//     bottom_center: z = z - h * 0.5f (two roundings).  Kept rows are compacted in rank order; rows at and after
//     count are zeros with label -1; every output element is written on every call.
//   LDS: block_topk.hpp's 32 KiB histograms, 8 KiB list and scan scratch, and expf's 256-byte table, all static.
//
// No FMA but the MFMA chains (-ffp-contract=off), no atomics on global memory, no zeroing pass, 64-bit offsets.
#include "../../include/paddle3d_amd.h"
#include "bevformer_attn.hpp"
#include "block_topk.hpp"

#include <cmath>

namespace {

using namespace pd3;
using namespace pd3::bevattn;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMhaThreads = 256;
constexpr int kMhaWaves = kMhaThreads / kWave;
constexpr int kMhaMaxD = 128;
constexpr int kMhaMaxNk = 2048;
constexpr int kQPad = 4;
constexpr int kMhaU = 8;       // MFMA steps whose global operands are fetched together (an item)
constexpr int kMhaDepth1 = 3;  // items in flight ahead of the MFMAs in phase 1 (two tiles: 16 loads each)
constexpr int kMhaDepth3 = 6;  // and in phase 3 (8 loads each): 48 loads, about 1900 MFMA cycles of cover

__global__ void __launch_bounds__(kMhaThreads) mha_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                          const float* __restrict__ v, float* __restrict__ out, int Nq,
                                                          int Nk, int M, int d, int QB, int SN, float scale) {
  extern __shared__ float lds[];
  __shared__ uint64_t etab[32];  // expf's table: a read per call from memory is a global load the polynomial waits for
  lm::exp2f_tab_fill(etab);
  const auto tab = [&](int i) { return etab[i]; };
  float* S = lds;               // [16][SN] scores, then weights
  float* Qs = lds + 16 * SN;    // [16][d + kQPad] scaled queries
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
  const int col = lane & 15, kq = lane >> 4;
  const int qb = (int)(blockIdx.x % (unsigned)QB);
  const int64_t bm = blockIdx.x / (unsigned)QB;
  const int m = (int)(bm % M);
  const int64_t b = bm / M;
  const int q0 = qb * 16;
  const int QS = d + kQPad;
  const int64_t MD = (int64_t)M * d;
  // ---- the scaled query tile -------------------------------------------------------------------------------------
  for (int idx = tid; idx < 16 * d; idx += kMhaThreads) {
    const int i = idx / d, c = idx - i * d;
    const int qi = q0 + i;
    Qs[i * QS + c] = qi < Nq ? q[((b * Nq + qi) * M + m) * d + c] * scale : 0.0f;
  }
  __syncthreads();
  // ---- phase 1: S = Qs K^T, two key tiles per wave and step --------------------------------------------------------
  // The wave's work is a list of items (pair of key tiles, chunk of kMhaU k-steps); the k operands of item w +
  // kMhaDepth1 are fetched before the MFMAs of item w are issued, into a ring of registers.
  const int NT = (Nk + 15) >> 4;
  const float* kbase = k + (b * Nk * M + m) * d;
  {
    const int chunks = (d + 4 * kMhaU - 1) / (4 * kMhaU);
    const int pairs = NT > 2 * wave ? (NT - 2 * wave + 2 * kMhaWaves - 1) / (2 * kMhaWaves) : 0;
    const int items = pairs * chunks;
    const auto fetch = [&](int item, float (&b0)[kMhaU], float (&b1)[kMhaU]) {
      const int p = item / chunks, s0 = (item - p * chunks) * 4 * kMhaU;
      const int j0 = (2 * wave + 2 * kMhaWaves * p) * 16 + col, j1 = j0 + 16;
      const bool ok0 = item < items && j0 < Nk, ok1 = item < items && j1 < Nk;  // behind the list: zeros, no load
      const float* k0 = kbase + (ok0 ? j0 : 0) * MD + kq + s0;
      const float* k1 = kbase + (ok1 ? j1 : 0) * MD + kq + s0;
#pragma unroll
      for (int u = 0; u < kMhaU; ++u) {
        const bool in = s0 + 4 * u < d;
        b0[u] = ok0 && in ? k0[4 * u] : 0.0f;
        b1[u] = ok1 && in ? k1[4 * u] : 0.0f;
      }
    };
    float n0[kMhaDepth1][kMhaU], n1[kMhaDepth1][kMhaU];
#pragma unroll
    for (int r = 0; r < kMhaDepth1; ++r) fetch(r, n0[r], n1[r]);
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const float* qa = Qs + col * QS + kq;
    for (int base = 0; base < items; base += kMhaDepth1) {
#pragma unroll
      for (int r = 0; r < kMhaDepth1; ++r) {
        const int item = base + r;
        if (item >= items) break;  // uniform
        float b0[kMhaU], b1[kMhaU];
#pragma unroll
        for (int u = 0; u < kMhaU; ++u) b0[u] = n0[r][u], b1[u] = n1[r][u];
        fetch(item + kMhaDepth1, n0[r], n1[r]);
        const int p = item / chunks, ch = item - p * chunks, s0 = ch * 4 * kMhaU;
        if (ch == 0) acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < kMhaU; ++u) {
          if (s0 + 4 * u < d) {  // uniform
            const float a = qa[s0 + 4 * u];
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0[u], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1[u], acc1, 0, 0, 0);
          }
        }
        if (ch == chunks - 1) {
          const int j0 = (2 * wave + 2 * kMhaWaves * p) * 16 + col, j1 = j0 + 16;
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4) {
            if (j0 < Nk) S[(4 * kq + q4) * SN + j0] = acc0[q4];
            if (j1 < Nk) S[(4 * kq + q4) * SN + j1] = acc1[q4];
          }
        }
      }
    }
  }
  __syncthreads();
  // ---- phase 2: the two-pass softmax of rows 4 wave .. 4 wave + 3 --------------------------------------------------
  for (int r = 4 * wave; r < 4 * wave + 4; ++r) {
    float* row = S + r * SN;
    float mx = -INFINITY;
    for (int j = lane; j < Nk; j += kWave) {
      const float x = row[j];
      mx = x > mx ? x : mx;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float x = __shfl_xor(mx, o, kWave);
      mx = x > mx ? x : mx;
    }
    const float s0 = row[0];
    if (s0 != s0) mx = s0;
    float p = 0.0f;
    for (int j = lane; j < Nk; j += 4 * kWave) {  // four independent expf per lane and step, p in index order
      float e[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) e[u] = lm::expf_with(j + u * kWave < Nk ? row[j + u * kWave] - mx : 0.0f, tab);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (j + u * kWave < Nk) {
          row[j + u * kWave] = e[u];
          p = p + e[u];
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) p = p + __shfl_xor(p, o, kWave);
    for (int j = lane; j < NT * 16; j += kWave) row[j] = j < Nk ? row[j] / p : 0.0f;
  }
  __syncthreads();
  // ---- phase 3: out = P V, channel tiles over the waves; v is fetched kMhaDepth3 items ahead ------------------------
  const float* vbase = v + (b * Nk * M + m) * d;
  const int steps = NT * 16;  // keys, four to an MFMA
  const int items = (steps + 4 * kMhaU - 1) / (4 * kMhaU);
  for (int ct = wave; ct < (d >> 4); ct += kMhaWaves) {
    const int c = ct * 16 + col;
    const float* vp = vbase + c;
    const float* pa = S + col * SN + kq;
    const auto fetch = [&](int item, float (&bv)[kMhaU]) {
#pragma unroll
      for (int u = 0; u < kMhaU; ++u) {
        const int j = (item * kMhaU + u) * 4 + kq;
        bv[u] = j < Nk ? vp[j * MD] : 0.0f;
      }
    };
    float nv[kMhaDepth3][kMhaU];
#pragma unroll
    for (int r = 0; r < kMhaDepth3; ++r) fetch(r, nv[r]);  // an item behind the list has j >= Nk: zeros, no load
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int base = 0; base < items; base += kMhaDepth3) {
#pragma unroll
      for (int r = 0; r < kMhaDepth3; ++r) {
        const int item = base + r;
        if (item >= items) break;  // uniform
        float bv[kMhaU];
#pragma unroll
        for (int u = 0; u < kMhaU; ++u) bv[u] = nv[r][u];
        fetch(item + kMhaDepth3, nv[r]);
#pragma unroll
        for (int u = 0; u < kMhaU; ++u) {
          const int s4 = (item * kMhaU + u) * 4;
          if (s4 < steps) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[s4], bv[u], acc, 0, 0, 0);  // uniform
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qi = q0 + 4 * kq + r;
      if (qi < Nq) out[((b * Nq + qi) * M + m) * d + c] = acc[r];
    }
  }
}

bool mha_supported(const void* q, const void* k, const void* v, const void* out, int d, int Nk) {
  return d >= 16 && d % 16 == 0 && d <= kMhaMaxD && Nk <= kMhaMaxNk && aligned16(q) && aligned16(k) && aligned16(v) &&
         aligned16(out);
}

__global__ void __launch_bounds__(kThreads) dec_ca_kernel(AttnDims d, int ref_stride_l, const float* __restrict__ value,
                                                          const int64_t* __restrict__ shapes,
                                                          const int64_t* __restrict__ start,
                                                          const float* __restrict__ offsets,
                                                          const float* __restrict__ logits,
                                                          const float* __restrict__ ref, float* __restrict__ out) {
  extern __shared__ float lds[];
  const int grp = threadIdx.x / d.G, lane_g = threadIdx.x - grp * d.G;
  const int64_t bqm = (int64_t)blockIdx.x * d.groups + grp;
  const bool active = grp < d.groups && bqm < (int64_t)d.B * d.Q * d.M;
  const int LP = d.L * d.P;
  float* w = lds + grp * LP;  // only dereferenced by active lanes
  group_softmax(logits + (active ? bqm : 0) * LP, LP, lane_g, d.G, active, w);
  if (!active) return;
  const int m = (int)(bqm % d.M);
  const int64_t bq = bqm / d.M;
  const int b = (int)(bq / d.Q);
  const MsdaArgs<float> g = point_args(value, shapes, start, d);
  const float* off = offsets + bqm * LP * 2;
  const float* r = ref + bq * (ref_stride_l ? d.L : 1) * 2;
  const int64_t MC = (int64_t)d.M * d.C;
  for (int c0 = lane_g * 4; c0 < d.C; c0 += d.G * 4) {
    float col[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    sample_source(g, b, off, w, r, 1, 0, ref_stride_l, value + (int64_t)m * d.C + c0, MC, col);
    *reinterpret_cast<float4*>(out + bqm * d.C + c0) = make_float4(col[0], col[1], col[2], col[3]);
  }
}

constexpr uint32_t kKeyOne = 0x3F800000u;  // bits of 1.0f
constexpr uint32_t kKeyNan = 0x3FFFFFFFu;  // a NaN score sorts after every number
constexpr int kKeyBits = 30;

template <class Tab>
__device__ __forceinline__ uint32_t score_key(float x, Tab tab) {
  const float s = 1.0f / (1.0f + lm::expf_with(-x, tab));
  const uint32_t bits = __float_as_uint(s);
  return bits <= kKeyOne ? kKeyOne - bits : kKeyNan;  // s in [0, 1]: key in [0, bits(1.0f)]
}

struct DecodeCfg {
  int Q, K, code, max_num, bottom_center, use_thr;
  double thr;
  float r[6];
};

__global__ void __launch_bounds__(kTopkThreads) nms_free_decode_kernel(DecodeCfg c, const float* __restrict__ cls,
                                                                       const float* __restrict__ bbox,
                                                                       float* __restrict__ boxes,
                                                                       float* __restrict__ scores,
                                                                       int* __restrict__ labels,
                                                                       int* __restrict__ count) {
  __shared__ int hist[kTopkHistWords];
  __shared__ unsigned long long list[kTopkMaxK];
  __shared__ int scr[kTopkScratch];
  __shared__ uint64_t etab[32];  // expf's table (libm_exact.hpp expf_with)
  lm::exp2f_tab_fill(etab);
  __syncthreads();
  const auto tab = [&](int i) { return etab[i]; };
  const int frame = blockIdx.x, tid = threadIdx.x;
  const int n = c.Q * c.K, K = c.max_num;
  const float* x = cls + (int64_t)frame * n;
  const TopkCut cut = n > K ? block_topk_cut(K, kKeyBits, hist, scr,
                                             [&](auto f) {
                                               for (int i = tid; i < n; i += kTopkThreads) f(score_key(x[i], tab));
                                             })
                            : TopkCut{0xFFFFFFFFu, 0};  // > every key: all entries
  block_topk_compact(
      cut, n, [&](int i) { return score_key(x[i], tab); }, [](int i, int) { return (uint32_t)i; }, list, scr);
  block_topk_sort(list, K);
  // ---- the threshold the loop of box_coder.py:158-166 ends with (uniform over the workgroup) ----------------------
  int mode = 2;  // 0: score > cur, 1: score >= cur, 2: all
  float cur = 0.0f;
  if (c.use_thr) {
    const uint32_t k0 = (uint32_t)(list[0] >> 32);
    const float top = k0 == kKeyNan ? __uint_as_float(0x7FC00000u) : __uint_as_float(kKeyOne - k0);
    if (top > (float)c.thr) {
      mode = 0;
      cur = (float)c.thr;
    } else {
      double tmp = c.thr;
      for (;;) {
        tmp = tmp * 0.9;
        if (tmp < 0.01) break;
        if (top >= (float)tmp) {
          mode = 1;
          cur = (float)tmp;
          break;
        }
      }
    }
  }
  // ---- decode of the tid-th best entry (denormalize_bbox) -----------------------------------------------------------
  const int W = c.code - 1;
  bool keep = false;
  float bx[9] = {};
  float score = 0.f;
  int label = 0;
  if (tid < K) {
    const unsigned long long e = list[tid];
    const uint32_t key = (uint32_t)(e >> 32);
    const int flat = (int)(uint32_t)e;
    if (key != kKeyNan && (uint32_t)flat < (uint32_t)n) {
      score = __uint_as_float(kKeyOne - key);
      const int row = flat / c.K;
      label = flat - row * c.K;
      const float* p = bbox + ((int64_t)frame * c.Q + row) * c.code;
      bx[0] = p[0], bx[1] = p[1], bx[2] = p[4];
      bx[3] = lm::expf_with(p[2], tab), bx[4] = lm::expf_with(p[3], tab), bx[5] = lm::expf_with(p[5], tab);
      bx[6] = lm::atan2f(p[6], p[7]);
      if (c.code > 8) bx[7] = p[8], bx[8] = p[9];
      keep = bx[0] >= c.r[0] && bx[1] >= c.r[1] && bx[2] >= c.r[2] && bx[0] <= c.r[3] && bx[1] <= c.r[4] &&
             bx[2] <= c.r[5];
      if (mode == 0) keep = keep && score > cur;
      if (mode == 1) keep = keep && score >= cur;
      if (c.bottom_center) bx[2] = bx[2] - bx[5] * 0.5f;
    }
  }
  int total;
  const int pos = block_exclusive_scan<kTopkThreads>(keep ? 1 : 0, scr, total);
  if (keep) {
    const int64_t o = (int64_t)frame * K + pos;
    for (int j = 0; j < W; ++j) boxes[o * W + j] = bx[j];
    scores[o] = score;
    labels[o] = label;
  }
  if (tid >= total && tid < K) {
    const int64_t o = (int64_t)frame * K + tid;
    for (int j = 0; j < W; ++j) boxes[o * W + j] = 0.0f;
    scores[o] = 0.0f;
    labels[o] = -1;
  }
  if (tid == 0) count[frame] = total;
}

}  // namespace

extern "C" {

int pd3_mha_forward(const void* q, const void* k, const void* v, int batch, int num_query, int num_key, int num_heads,
                    int head_dim, float scale, void* out, void* stream) {
  if (batch < 0 || num_query < 0 || num_key < 1 || num_heads < 1 || head_dim < 1) return PD3_EINVAL;
  if (!mha_supported(q, k, v, out, head_dim, num_key)) return PD3_EUNSUPPORTED;
  if (batch == 0 || num_query == 0) return PD3_OK;
  if (!q || !k || !v || !out) return PD3_EINVAL;
  const int QB = (num_query + 15) / 16;
  const int64_t blocks = (int64_t)batch * num_heads * QB;
  if (blocks > 0x7fffffff) return PD3_EUNSUPPORTED;
  const int SN = (num_key + 15) / 16 * 16 + 4;
  const int lds = 16 * (SN + head_dim + kQPad) * (int)sizeof(float);
  const int rc = pd3::launch_lds(mha_kernel, (unsigned)blocks, kMhaThreads, (size_t)lds, (hipStream_t)stream,
                                 static_cast<const float*>(q), static_cast<const float*>(k), static_cast<const float*>(v),
                                 static_cast<float*>(out), num_query, num_key, num_heads, head_dim, QB, SN, scale);
  return rc ? rc : pd3::launch_status();
}

int pd3_bevformer_dec_ca(const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                         const void* sampling_offsets, const void* attention_logits, const void* reference_points,
                         int batch, int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                         int num_point, int num_ref_levels, void* out, void* stream) {
  AttnDims d;
  if (int e = attn_dims(batch, spatial_size, num_heads, channels, num_levels, num_query, num_point, &d)) return e;
  if (num_ref_levels != 1 && num_ref_levels != num_levels) return PD3_EINVAL;
  if (!(channels % 4 == 0 && aligned16(value) && aligned16(out) && (int64_t)num_levels * num_point <= kMaxLP))
    return PD3_EUNSUPPORTED;
  if (batch == 0 || num_query == 0) return PD3_OK;
  if (!value || !spatial_shapes || !level_start_index || !sampling_offsets || !attention_logits ||
      !reference_points || !out)
    return PD3_EINVAL;
  const int64_t blocks = pd3::ceil_div((int64_t)batch * num_query * num_heads, d.groups);
  if (blocks > 0x7fffffff) return PD3_EUNSUPPORTED;
  const size_t lds = (size_t)d.groups * num_levels * num_point * sizeof(float);
  hipLaunchKernelGGL(dec_ca_kernel, dim3((unsigned)blocks), dim3(kThreads), lds, (hipStream_t)stream, d,
                     num_ref_levels == 1 ? 0 : 1, static_cast<const float*>(value), spatial_shapes, level_start_index,
                     static_cast<const float*>(sampling_offsets), static_cast<const float*>(attention_logits),
                     static_cast<const float*>(reference_points), static_cast<float*>(out));
  return pd3::launch_status();
}

int pd3_nms_free_decode(const void* cls_scores, const void* bbox_preds, const float* post_center_range, int batch,
                        int num_query, int num_classes, int code_size, int max_num, double score_threshold,
                        int bottom_center, void* boxes, void* scores, void* labels, void* count, void* stream) {
  if (batch < 0 || num_query < 1 || num_classes < 1 || (code_size != 8 && code_size != 10) || max_num < 1 ||
      !post_center_range || !(score_threshold == score_threshold) || std::isinf(score_threshold))
    return PD3_EINVAL;
  if ((int64_t)num_query * num_classes > 0x7fffffff) return PD3_EUNSUPPORTED;
  if (max_num > num_query * num_classes) return PD3_EINVAL;
  if (max_num > kTopkMaxK) return PD3_EUNSUPPORTED;
  if (batch == 0) return PD3_OK;
  if (!cls_scores || !bbox_preds || !boxes || !scores || !labels || !count) return PD3_EINVAL;
  DecodeCfg c;
  c.Q = num_query;
  c.K = num_classes;
  c.code = code_size;
  c.max_num = max_num;
  c.bottom_center = bottom_center ? 1 : 0;
  c.use_thr = score_threshold > 0.0 ? 1 : 0;  // None (negative) and 0.0 (`if self.score_threshold:`) apply nothing
  c.thr = score_threshold;
  for (int i = 0; i < 6; ++i) c.r[i] = post_center_range[i];
  hipLaunchKernelGGL(nms_free_decode_kernel, dim3((unsigned)batch), dim3(kTopkThreads), 0, (hipStream_t)stream, c,
                     static_cast<const float*>(cls_scores), static_cast<const float*>(bbox_preds),
                     static_cast<float*>(boxes), static_cast<float*>(scores), static_cast<int*>(labels),
                     static_cast<int*>(count));
  return pd3::launch_status();
}

}  // extern "C"
