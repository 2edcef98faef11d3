// BEVFusion's Anchor3DHead at inference for gfx950: the head's three 1x1 convolutions, get_bboxes / get_bboxes_single,
// box3d_multiclass_nms and the direction fix of a whole batch in one launch sequence, every count on the device.
// (reference: paddle3d/models/heads/dense_heads/anchor3d_head.py:146-161, :378-520,
//  paddle3d/models/detection/bevfusion/utils.py:92-103 limit_period, :189-276 box3d_multiclass_nms,
//  paddle3d/utils/box_coder.py:270-310 DeltaXYZWLHRBBoxCoder.decode.)
//
// The reference evaluates the three convolutions densely, transposes and reshapes the maps, takes sigmoid / max / topk /
// sort, gathers and decodes <= nms_pre anchors and then loops over the classes in Python (nonzero with a host-side
// count, argsort, nms_gpu with its mask copy and host sweep, four gathers).  Here the head is LAZY: only conv_cls runs
// densely and only the per-anchor maximum leaves that kernel; conv_reg, conv_dir_cls and the per-class scores are
// evaluated at the <= nms_pre selected anchors only.  pd3_anchor3d_get_bboxes is the same sequence from existing maps.
//
// Index arithmetic: anchor i = (y * W + x) * A + a, map channel a * width + component (width = nc, code_size, 2): the
// reference's transpose([1, 2, 0]).reshape([-1, width]).  N = H * W * A, K = min(nms_pre, N), or N when nms_pre <= 0.
//
// Arithmetic order (fp32, every operation rounded on its own, -ffp-contract=off; tests/golden/anchor3d_numpy.py
// restates it):
//   logit(row, p)  = fmaf(f[C-1], w[C-1], ... fmaf(f[1], w[1], fmaf(f[0], w[0], +0))) + bias[row]      ascending channel;
//                    the chain is what a sequence of v_mfma_f32_16x16x4_f32 on one accumulator computes when step s
//                    holds channels 4 s .. 4 s + 3 (csrc/petr.hip, csrc/bevformer_decoder.hip rely on the same); the
//                    dense kernel (a) and the candidate kernel (d) both take their logits from that instruction with
//                    the weight as the A operand and the feature column as the B operand: the same bits
//   sigmoid(x)     = 1.0f / (1.0f + expf(-x)), expf with glibc's bits (libm_exact.hpp)
//   max_score(i)   = m, where m = sigmoid(logit_0) and, for c = 1 .. nc - 1 in turn, m = s_c when s_c > m
//   selection      key(i) = bits(1.0f) - bits(max_score) (a NaN: bits(1.0f) + 1, after every number); the K smallest
//                  (key, i) pairs, then in ascending i: topk + sort; ties at the cut go to the lower anchor index
//   candidate k    the nc class scores sigmoid(logit), the direction bit (d1 > d0: the first maximum wins), and
//                  DeltaXYZWLHRBBoxCoder.decode against anchor row i:
//                    za' = za + ha * 0.5f; diag = sqrtf(la * la + wa * wa); xg = xt * diag + xa; yg = yt * diag + ya;
//                    zg = zt * ha + za'; lg = expf(lt) * la; wg = expf(wt) * wa; hg = expf(ht) * ha; rg = rt + ra;
//                    zg = zg - hg * 0.5f; extra columns t + a; row (xg, yg, zg, wg, lg, hg, rg, extras)
//                  NMS box (xg, yg, zg, wg, lg, hg, -rg) and its BoxPre record (iou3d_geom.hpp)
//   class sets     per (frame, class): candidates with score > score_thr in anchor order, stably by descending score
//                  (sort of (bits(1.0f) - bits(score), k)): nonzero + argsort
//   NMS            nms_kernels.hpp over the batch * nc sets (the reference's nms_gpu bits), kept rows class-major
//   max_num        when a frame keeps more: the max_num smallest (key, concatenated position) pairs in that order
//   direction      val = r - dir_offset; rot = val - floorf(val / pi + dir_limit_offset) * pi;
//                  r = (rot + dir_offset) + pi * (float)dir_bit          pi = (float)M_PI; dir_offset, dir_limit_offset
//                  rounded to fp32 by the caller
// Nothing depends on the frame's place in the batch, on the grid or on the stream.
//
// Launches (one memset first: the NMS pool's counters):
//   a.  a3d_dense_max_kernel   grid (ceil(HW / 128), B), 256 threads: wave w owns 32 pixels (two 16-pixel tiles, so a
//       weight fragment feeds two MFMAs), all class rows of a chunk of anchors as up to 12 MFMA tiles (channel rows as M,
//       pixels as N); the fragments of the next four channel steps are fetched before the MFMAs of the current four; the logits
//       of a 16-pixel tile go through the wave's own LDS tile, one lane per (pixel, anchor) then takes the maximum.
//       Pixels past H * W load 0 and store nothing.
//       Weight packing (ops/anchor3d_head.py pack_cls_weight): anchors in chunks of APC = 192 / nc, a chunk's rows
//       (anchor-major, zero-padded to whole tiles of 16) as [tile][C / 4][64], lane (m = lane & 15, k = lane >> 4)
//       holding w[row 16 tile + m][channel 4 s + k].
//   a'. a3d_maps_max_kernel    the same maximum from an existing cls_score map, thread = (pixel, anchor)
//   c.  a3d_topk_kernel        one workgroup per frame (block_topk.hpp), then a second sort on the anchor index
//   d.  a3d_rows_kernel        one wave per candidate: three MFMA tiles (class, regression, direction rows of the
//       anchor against the cell's feature column) or a gather from the maps; sigmoid, direction bit, decode, BoxPre
//   e.  a3d_class_sets_kernel  one workgroup per (frame, class): flag, bitonic sort, the set's BoxPre / xyr / order
//   f.  nms_cand_kernel + nms_pairs_kernel + nms_sweep_kernel, a3d_concat_kernel (class-major keys and sources),
//       a3d_output_kernel (max_num cut, direction fix, fixed-size rows, zeros past the count)
// No atomics but the NMS pool's, no host synchronisation, 64-bit offsets.
#include "../../include/paddle3d_amd.h"
#include "block_topk.hpp"
#include "common.hpp"
#include "head_math.hpp"
#include "libm_exact.hpp"
#include "nms_kernels.hpp"

#include <algorithm>

namespace {

using namespace pd3;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kKeyNaN = kScoreKeyOne + 1u;  // a NaN score: after every number
constexpr int kChunkRows = 192;               // class rows of one chunk of anchors
constexpr int kChunkTiles = kChunkRows / 16;
constexpr int kLogitStride = kChunkRows + 1;
constexpr int kMaxCode = 16, kMaxClasses = 16, kMaxAnchors = 32, kMaxK = 1024;
constexpr float kPiF = 3.14159265358979323846f;

struct A3dShape {
  int B, C, H, W, HW, A, nc, cs, N, K, max_num;
  int apc, tiles_full;  // anchors per chunk, tiles of a full chunk
};

__device__ __forceinline__ uint32_t score_key(float s) { return s == s ? kScoreKeyOne - __float_as_uint(s) : kKeyNaN; }

// ---- a. dense class-score maximum ------------------------------------------------------------------------------------
constexpr int kWaveTiles = 2;                        // 16-pixel tiles of one wave: a weight fragment feeds two MFMAs
constexpr int kDensePixels = 4 * 16 * kWaveTiles;    // pixels of a workgroup

__global__ __launch_bounds__(256) void a3d_dense_max_kernel(const float* __restrict__ feat,
                                                            const float* __restrict__ wp,
                                                            const float* __restrict__ bias, A3dShape sh,
                                                            float* __restrict__ max_score) {
  __shared__ uint64_t etab[32];
  __shared__ float logits[4][16][kLogitStride];
  lm::exp2f_tab_fill(etab);
  __syncthreads();
  const auto tab = [&](int i) { return etab[i]; };
  const int lane = lane_id(), wave = wave_id();
  const int col = lane & 15, g = lane >> 4;
  const int b = blockIdx.y;
  const int pix0 = blockIdx.x * kDensePixels + wave * 16 * kWaveTiles;
  if (pix0 >= sh.HW) return;  // the whole wave: nothing below is a block barrier
  const int S = sh.C >> 2;
  bool ok[kWaveTiles];
  const float* fp[kWaveTiles];
#pragma unroll
  for (int n = 0; n < kWaveTiles; ++n) {
    const int pix = pix0 + 16 * n + col;
    ok[n] = pix < sh.HW;
    fp[n] = feat + ((int64_t)b * sh.C + g) * sh.HW + (ok[n] ? pix : pix0);
  }
  float (*lg)[kLogitStride] = logits[wave];
  for (int a0 = 0, t0 = 0; a0 < sh.A; a0 += sh.apc, t0 += sh.tiles_full) {
    const int na = min(sh.apc, sh.A - a0), rows = na * sh.nc, nt = (rows + 15) >> 4;
    f32x4 acc[kWaveTiles][kChunkTiles];
#pragma unroll
    for (int n = 0; n < kWaveTiles; ++n)
#pragma unroll
      for (int j = 0; j < kChunkTiles; ++j) acc[n][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* wq = wp + (int64_t)t0 * S * 64 + lane;
    // the fragments of the next four steps are fetched before the MFMAs of the current four (two register sets; a wave
    // is alone on its SIMD at this register count, so the fetch distance is what hides the memory latency; S % 4 == 0
    // since C % 16 == 0)
    const auto fetch = [&](int s0, float (&av)[4][kChunkTiles], float (&bv)[4][kWaveTiles]) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int n = 0; n < kWaveTiles; ++n) bv[u][n] = ok[n] ? fp[n][(int64_t)4 * (s0 + u) * sh.HW] : 0.0f;
#pragma unroll
        for (int j = 0; j < kChunkTiles; ++j) av[u][j] = j < nt ? wq[((int64_t)j * S + s0 + u) * 64] : 0.0f;
      }
    };
    const auto mma = [&](const float (&av)[4][kChunkTiles], const float (&bv)[4][kWaveTiles]) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < kChunkTiles; ++j)
          if (j < nt) {
#pragma unroll
            for (int n = 0; n < kWaveTiles; ++n)
              acc[n][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][j], bv[u][n], acc[n][j], 0, 0, 0);
          }
    };
    float a_even[4][kChunkTiles], a_odd[4][kChunkTiles], b_even[4][kWaveTiles], b_odd[4][kWaveTiles];
    fetch(0, a_even, b_even);
    for (int s = 0; s < S; s += 8) {
      if (s + 4 < S) fetch(s + 4, a_odd, b_odd);
      mma(a_even, b_even);
      if (s + 4 < S) {
        if (s + 8 < S) fetch(s + 8, a_even, b_even);
        mma(a_odd, b_odd);
      }
    }
    const float* bq = bias + (int64_t)a0 * sh.nc;
#pragma unroll
    for (int n = 0; n < kWaveTiles; ++n) {
      const int pixn = pix0 + 16 * n;
      if (pixn >= sh.HW) break;  // uniform
#pragma unroll
      for (int j = 0; j < kChunkTiles; ++j)
        if (j < nt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * j + 4 * g + r;
            if (row < rows) lg[col][row] = acc[n][j][r] + bq[row];
          }
        }
      wave_lds_order();
      for (int idx = lane; idx < 16 * na; idx += kWave) {
        const int p = idx / na, al = idx - p * na;
        if (pixn + p >= sh.HW) continue;
        const float* x = &lg[p][al * sh.nc];
        float best = sigmoid_exact(x[0], tab);
        for (int c = 1; c < sh.nc; ++c) {
          const float s = sigmoid_exact(x[c], tab);
          if (s > best) best = s;
        }
        max_score[(int64_t)b * sh.N + (int64_t)(pixn + p) * sh.A + a0 + al] = best;
      }
      wave_lds_order();
    }
  }
}

// ---- a'. the same maximum from an existing map: grid (ceil(HW / 256), A, B) -----------------------------------------
__global__ __launch_bounds__(256) void a3d_maps_max_kernel(const float* __restrict__ cls, A3dShape sh,
                                                           float* __restrict__ max_score) {
  __shared__ uint64_t etab[32];
  lm::exp2f_tab_fill(etab);
  __syncthreads();
  const auto tab = [&](int i) { return etab[i]; };
  const int pix = blockIdx.x * blockDim.x + threadIdx.x, a = blockIdx.y, b = blockIdx.z;
  if (pix >= sh.HW) return;
  const float* x = cls + ((int64_t)b * sh.A * sh.nc + (int64_t)a * sh.nc) * sh.HW + pix;
  float best = sigmoid_exact(x[0], tab);
  for (int c = 1; c < sh.nc; ++c) {
    const float s = sigmoid_exact(x[(int64_t)c * sh.HW], tab);
    if (s > best) best = s;
  }
  max_score[(int64_t)b * sh.N + (int64_t)pix * sh.A + a] = best;
}

// ---- c. selection: grid (B), kTopkThreads ----------------------------------------------------------------------------
__global__ __launch_bounds__(kTopkThreads) void a3d_topk_kernel(const float* __restrict__ max_score, int N, int K,
                                                                int* __restrict__ sel) {
  __shared__ unsigned long long list[kTopkMaxK];
  __shared__ int hist[kTopkHistWords];
  __shared__ int scr[kTopkScratch];
  const int b = blockIdx.x, t = threadIdx.x;
  const float* sc = max_score + (int64_t)b * N;
  const auto key = [&](int i) { return score_key(sc[i]); };
  const auto visit = [&](auto f) {
    if ((N & 3) == 0) {  // frames start 16-byte aligned then: four scores per load, four loads in flight
#pragma unroll 4
      for (int i = t * 4; i < N; i += kTopkThreads * 4) {
        const float4 v = *reinterpret_cast<const float4*>(sc + i);
        f(score_key(v.x));
        f(score_key(v.y));
        f(score_key(v.z));
        f(score_key(v.w));
      }
    } else {
#pragma unroll 4
      for (int i = t; i < N; i += kTopkThreads) f(key(i));
    }
  };
  const TopkCut cut = N > K ? block_topk_cut(K, kScoreKeyBits, hist, scr, visit) : TopkCut{kScoreKeyAll, 0};
  block_topk_compact(cut, N, key, [](int i, int) { return (uint32_t)i; }, list, scr);
  // topk_inds.sort(): the taken anchors in ascending index
  const unsigned long long e = list[t];
  list[t] = e == ~0ull ? ~0ull : (e & 0xffffffffull);
  __syncthreads();
  block_topk_sort(list, K);
  if (t < K) sel[(int64_t)b * K + t] = (int)(uint32_t)list[t];
}

// ---- d. candidate rows: grid (ceil(K / 4), B), 256 threads, one wave per candidate -----------------------------------
struct A3dCand {
  float* scores;   // [B][K][nc]
  float* boxes;    // [B][K][cs]
  int* dir;        // [B][K]
  BoxPre* pre;     // [B][K]
  float4* xyr;     // [B][K]
};

template <bool LAZY>
__global__ __launch_bounds__(256) void a3d_rows_kernel(const float* __restrict__ feat, const float* __restrict__ wp,
                                                       const float* __restrict__ cls_bias,
                                                       const float* __restrict__ reg_w,
                                                       const float* __restrict__ reg_b,
                                                       const float* __restrict__ dir_w,
                                                       const float* __restrict__ dir_b,
                                                       const float* __restrict__ cls_map,
                                                       const float* __restrict__ reg_map,
                                                       const float* __restrict__ dir_map,
                                                       const float* __restrict__ anchors,
                                                       const int* __restrict__ sel, A3dShape sh, A3dCand cd) {
  __shared__ uint64_t etab[32];
  __shared__ float vals[4][3][16];
  lm::exp2f_tab_fill(etab);
  __syncthreads();
  const auto tab = [&](int i) { return etab[i]; };
  const int lane = lane_id(), wave = wave_id();
  const int b = blockIdx.y, k = blockIdx.x * 4 + wave;
  if (k >= sh.K) return;  // the whole wave
  const int i = min(max(sel[(int64_t)b * sh.K + k], 0), sh.N - 1);  // (always inside: exactly K anchors are taken)
  const int pix = i / sh.A, a = i - pix * sh.A;
  float (*v)[16] = vals[wave];
  if constexpr (LAZY) {
    const int m = lane & 15, g = lane >> 4, S = sh.C >> 2;
    // the anchor's class rows inside the packed weight (see the header)
    const int q = a / sh.apc, rl = (a - q * sh.apc) * sh.nc + m;
    const bool okc = m < sh.nc, okr = m < sh.cs, okd = m < 2;
    const float* wc = wp + ((int64_t)(q * sh.tiles_full + (okc ? rl >> 4 : 0)) * S) * 64 + g * 16 + (okc ? rl & 15 : 0);
    const float* wr = reg_w + ((int64_t)a * sh.cs + (okr ? m : 0)) * sh.C + g;
    const float* wd = dir_w + ((int64_t)a * 2 + (okd ? m : 0)) * sh.C + g;
    const float* fp = feat + ((int64_t)b * sh.C + g) * sh.HW + pix;
    f32x4 ac = {0.f, 0.f, 0.f, 0.f}, ar = ac, ad = ac;
    for (int s0 = 0; s0 < S; s0 += 4) {  // four steps' fragments in flight (S % 4 == 0: C % 16 == 0)
      float bv[4], c[4], r[4], d[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int s = s0 + u;
        bv[u] = fp[(int64_t)4 * s * sh.HW];
        c[u] = okc ? wc[(int64_t)s * 64] : 0.0f;
        r[u] = okr ? wr[4 * s] : 0.0f;
        d[u] = okd ? wd[4 * s] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        ac = __builtin_amdgcn_mfma_f32_16x16x4f32(c[u], bv[u], ac, 0, 0, 0);
        ar = __builtin_amdgcn_mfma_f32_16x16x4f32(r[u], bv[u], ar, 0, 0, 0);
        ad = __builtin_amdgcn_mfma_f32_16x16x4f32(d[u], bv[u], ad, 0, 0, 0);
      }
    }
    if (m == 0) {  // column 0 (every column holds the same feature cell): rows 4 g .. 4 g + 3
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * g + r;
        v[0][row] = row < sh.nc ? ac[r] + cls_bias[a * sh.nc + row] : 0.0f;
        v[1][row] = row < sh.cs ? ar[r] + reg_b[a * sh.cs + row] : 0.0f;
        v[2][row] = row < 2 ? ad[r] + dir_b[a * 2 + row] : 0.0f;
      }
    }
  } else {
    if (lane < 16) {
      const int64_t hw = sh.HW;
      v[0][lane] = lane < sh.nc ? cls_map[((int64_t)b * sh.A * sh.nc + a * sh.nc + lane) * hw + pix] : 0.0f;
      v[1][lane] = lane < sh.cs ? reg_map[((int64_t)b * sh.A * sh.cs + a * sh.cs + lane) * hw + pix] : 0.0f;
      v[2][lane] = lane < 2 ? dir_map[((int64_t)b * sh.A * 2 + a * 2 + lane) * hw + pix] : 0.0f;
    }
  }
  wave_lds_order();
  const int64_t o = (int64_t)b * sh.K + k;
  if (lane < sh.nc) cd.scores[o * sh.nc + lane] = sigmoid_exact(v[0][lane], tab);
  if (lane >= 7 && lane < sh.cs) cd.boxes[o * sh.cs + lane] = v[1][lane] + anchors[(int64_t)i * sh.cs + lane];
  if (lane == 0) {
    const float* an = anchors + (int64_t)i * sh.cs;
    const float xa = an[0], ya = an[1], wa = an[3], la = an[4], ha = an[5], ra = an[6];
    const float za = an[2] + ha * 0.5f;
    const float diag = sqrtf(la * la + wa * wa);
    const float xg = v[1][0] * diag + xa;
    const float yg = v[1][1] * diag + ya;
    float zg = v[1][2] * ha + za;
    const float lgt = lm::expf_with(v[1][4], tab) * la;
    const float wg = lm::expf_with(v[1][3], tab) * wa;
    const float hg = lm::expf_with(v[1][5], tab) * ha;
    const float rg = v[1][6] + ra;
    zg = zg - hg * 0.5f;
    float* bx = cd.boxes + o * sh.cs;
    bx[0] = xg;
    bx[1] = yg;
    bx[2] = zg;
    bx[3] = wg;
    bx[4] = lgt;
    bx[5] = hg;
    bx[6] = rg;
    cd.dir[o] = v[2][1] > v[2][0] ? 1 : 0;
    const float nb[7] = {xg, yg, zg, wg, lgt, hg, -rg};
    const BoxPre bp = box_prepare(nb);
    cd.pre[o] = bp;
    cd.xyr[o] = make_float4(bp.cx, bp.cy, bp.rad, 0.f);
  }
}

// ---- e. per-class candidate sets: grid (nc, B), kTopkThreads ---------------------------------------------------------
__global__ __launch_bounds__(kTopkThreads) void a3d_class_sets_kernel(A3dCand cd, int K, int nc, float score_thr,
                                                                      int* __restrict__ counts,
                                                                      int* __restrict__ order,
                                                                      BoxPre* __restrict__ pre,
                                                                      float4* __restrict__ xyr) {
  __shared__ unsigned long long list[kTopkMaxK];
  const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int64_t set = (int64_t)b * nc + c;
  const float s = t < K ? cd.scores[((int64_t)b * K + t) * nc + c] : 0.0f;
  const bool in = t < K && s > score_thr;
  list[t] = in ? ((unsigned long long)score_key(s) << 32) | (unsigned)t : ~0ull;
  const int count = __syncthreads_count(in ? 1 : 0);
  block_topk_sort(list, K);
  if (t < count) {
    const int k = (int)(uint32_t)list[t];
    order[set * K + t] = k;
    pre[set * K + t] = cd.pre[(int64_t)b * K + k];
    xyr[set * K + t] = cd.xyr[(int64_t)b * K + k];
  }
  if (t == 0) counts[set] = count;
}

// ---- f. kept rows class-major: grid (nc, B), 256 threads ------------------------------------------------------------
__global__ __launch_bounds__(256) void a3d_concat_kernel(A3dCand cd, int K, int nc, const int* __restrict__ order,
                                                         const int32_t* __restrict__ keep,
                                                         const int32_t* __restrict__ nkeep,
                                                         uint32_t* __restrict__ cat_key,
                                                         uint32_t* __restrict__ cat_src) {
  const int c = blockIdx.x, b = blockIdx.y;
  const int64_t set = (int64_t)b * nc + c;
  int off = 0;
  for (int j = 0; j < c; ++j) off += nkeep[(int64_t)b * nc + j];
  const int n = nkeep[set];
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
    const int k = order[set * K + keep[set * K + j]];
    const int64_t e = (int64_t)b * nc * K + off + j;
    cat_key[e] = score_key(cd.scores[((int64_t)b * K + k) * nc + c]);
    cat_src[e] = ((uint32_t)c << 16) | (uint32_t)k;
  }
}

// grid (B), kTopkThreads: the max_num cut, the direction fix, fixed-size rows
__global__ __launch_bounds__(kTopkThreads) void a3d_output_kernel(A3dCand cd, int K, int nc, int cs, int max_num,
                                                                  float dir_offset, float dir_limit_offset,
                                                                  const int32_t* __restrict__ nkeep,
                                                                  const uint32_t* __restrict__ cat_key,
                                                                  const uint32_t* __restrict__ cat_src,
                                                                  float* __restrict__ out_boxes,
                                                                  float* __restrict__ out_scores,
                                                                  int32_t* __restrict__ out_labels,
                                                                  int32_t* __restrict__ out_counts) {
  __shared__ unsigned long long list[kTopkMaxK];
  __shared__ int hist[kTopkHistWords];
  __shared__ int scr[kTopkScratch];
  const int b = blockIdx.x, t = threadIdx.x;
  int total = 0;
  for (int j = 0; j < nc; ++j) total += nkeep[(int64_t)b * nc + j];
  const uint32_t* kg = cat_key + (int64_t)b * nc * K;
  const uint32_t* sg = cat_src + (int64_t)b * nc * K;
  const int rows = min(total, max_num);
  int e = t;
  if (total > max_num) {  // scores.argsort(descending=True)[:max_num], stable
    const auto key = [&](int i) { return kg[i]; };
    const auto visit = [&](auto f) {
      for (int i = t; i < total; i += kTopkThreads) f(kg[i]);
    };
    const TopkCut cut = block_topk_cut(max_num, kScoreKeyBits, hist, scr, visit);
    block_topk_compact(cut, total, key, [](int i, int) { return (uint32_t)i; }, list, scr);
    block_topk_sort(list, max_num);
    e = (int)(uint32_t)list[t];
  }
  if (t < max_num) {
    float* ob = out_boxes + ((int64_t)b * max_num + t) * cs;
    if (t < rows) {
      const uint32_t src = sg[e];
      const int c = (int)(src >> 16), k = (int)(src & 0xffffu);
      const int64_t o = (int64_t)b * K + k;
      const float* bx = cd.boxes + o * cs;
      for (int j = 0; j < cs; ++j) ob[j] = bx[j];
      // anchor3d_head.py:515-519 with limit_period (utils.py:103)
      const float val = bx[6] - dir_offset;
      const float rot = val - floorf(val / kPiF + dir_limit_offset) * kPiF;
      ob[6] = (rot + dir_offset) + kPiF * (float)cd.dir[o];
      out_scores[(int64_t)b * max_num + t] = cd.scores[o * nc + c];
      out_labels[(int64_t)b * max_num + t] = c;
    } else {
      for (int j = 0; j < cs; ++j) ob[j] = 0.0f;
      out_scores[(int64_t)b * max_num + t] = 0.0f;
      out_labels[(int64_t)b * max_num + t] = 0;
    }
  }
  if (t == 0) out_counts[b] = rows;
}

struct A3dWorkspace {
  float* max_score;
  int* sel;
  A3dCand cd;
  int *set_counts, *order;
  BoxPre* pre;
  NmsPool pool;
  unsigned long long* mask;
  int32_t *keep, *nkeep;
  uint32_t *cat_key, *cat_src;
  size_t bytes;
};

A3dWorkspace a3d_carve(void* base, const A3dShape& sh) {
  Carver c(base);
  A3dWorkspace w;
  const size_t B = (size_t)sh.B, K = (size_t)sh.K, sets = B * sh.nc, cb = (K + 63) / 64;
  w.pool.counts = c.take<int>(sets * 2 * kNmsCtrStride);  // first: what the set-up memset clears
  w.max_score = c.take<float>(B * sh.N);
  w.sel = c.take<int>(B * K);
  w.cd.scores = c.take<float>(B * K * sh.nc);
  w.cd.boxes = c.take<float>(B * K * sh.cs);
  w.cd.dir = c.take<int>(B * K);
  w.cd.pre = c.take<BoxPre>(B * K);
  w.cd.xyr = c.take<float4>(B * K);
  w.set_counts = c.take<int>(sets);
  w.order = c.take<int>(sets * K);
  w.pre = c.take<BoxPre>(sets * K);
  w.pool.xyr = c.take<float4>(sets * K);
  w.pool.per_set = nms_pool_per_set((int)K);
  w.pool.pairs = c.take<uint32_t>(sets * w.pool.per_set);
  w.pool.tiles = c.take<uint32_t>(sets * cb * cb);
  w.mask = c.take<unsigned long long>(sets * K * cb);
  w.keep = c.take<int32_t>(sets * K);
  w.nkeep = c.take<int32_t>(sets);
  w.cat_key = c.take<uint32_t>(sets * K);
  w.cat_src = c.take<uint32_t>(sets * K);
  w.bytes = c.off;
  return w;
}

// PD3_OK with `sh` filled, PD3_EINVAL or PD3_EUNSUPPORTED.  channels < 0: the from-maps form (no channel predicate).
int a3d_shape(int batch, int channels, int feat_h, int feat_w, int num_anchors, int num_classes, int code_size,
              int nms_pre, int max_num, A3dShape& sh) {
  if (batch < 0 || feat_h <= 0 || feat_w <= 0 || num_anchors <= 0 || num_classes <= 0 || code_size <= 0 ||
      max_num <= 0 || channels == 0)
    return PD3_EINVAL;
  if (channels > 0 && (channels % 16 != 0 || channels < 16 || channels > 512)) return PD3_EUNSUPPORTED;
  if (num_classes > kMaxClasses || num_anchors > kMaxAnchors || code_size < 7 || code_size > kMaxCode ||
      max_num > kMaxK)
    return PD3_EUNSUPPORTED;
  const int64_t hw = (int64_t)feat_h * feat_w, n = hw * num_anchors;
  if (n >= (int64_t)1 << 30 || (int64_t)std::max(batch, 1) * n >= (int64_t)1 << 31 || batch > 65535 ||
      (int64_t)batch * num_classes > 65535)
    return PD3_EUNSUPPORTED;
  const int64_t k = nms_pre > 0 ? std::min<int64_t>(nms_pre, n) : n;
  if (k > kMaxK) return PD3_EUNSUPPORTED;
  sh.B = batch;
  sh.C = channels;
  sh.H = feat_h;
  sh.W = feat_w;
  sh.HW = (int)hw;
  sh.A = num_anchors;
  sh.nc = num_classes;
  sh.cs = code_size;
  sh.N = (int)n;
  sh.K = (int)k;
  sh.max_num = max_num;
  sh.apc = kChunkRows / num_classes;
  sh.tiles_full = (sh.apc * num_classes + 15) / 16;
  return PD3_OK;
}

// stages c .. f, shared by the two entry points (max_score is in the workspace)
template <bool LAZY>
int a3d_finish(const A3dShape& sh, const A3dWorkspace& w, const float* feat, const float* wp, const float* cls_b,
               const float* reg_w, const float* reg_b, const float* dir_w, const float* dir_b, const float* cls_map,
               const float* reg_map, const float* dir_map, const float* anchors, float score_thr, float nms_thr,
               float dir_offset, float dir_limit_offset, float* boxes, float* scores, int32_t* labels, int32_t* counts,
               hipStream_t s) {
  const int sets = sh.B * sh.nc, cb = (sh.K + 63) / 64;
  a3d_topk_kernel<<<sh.B, kTopkThreads, 0, s>>>(w.max_score, sh.N, sh.K, w.sel);
  a3d_rows_kernel<LAZY><<<dim3((sh.K + 3) / 4, sh.B), 256, 0, s>>>(feat, wp, cls_b, reg_w, reg_b, dir_w, dir_b, cls_map,
                                                                   reg_map, dir_map, anchors, w.sel, sh, w.cd);
  a3d_class_sets_kernel<<<dim3(sh.nc, sh.B), kTopkThreads, 0, s>>>(w.cd, sh.K, sh.nc, score_thr, w.set_counts, w.order,
                                                                   w.pre, w.pool.xyr);
  nms_enqueue_mask_pooled(w.pre, w.set_counts, sets, sh.K, cb, nms_thr, w.mask, w.pool, s);
  if (const int rc = launch_lds(nms_sweep_kernel, sets, kNmsSweepThreads, nms_sweep_lds(sh.K), s, w.mask, w.set_counts, 0,
                                sh.K, cb, w.keep, w.nkeep))
    return rc;
  a3d_concat_kernel<<<dim3(sh.nc, sh.B), 256, 0, s>>>(w.cd, sh.K, sh.nc, w.order, w.keep, w.nkeep, w.cat_key, w.cat_src);
  a3d_output_kernel<<<sh.B, kTopkThreads, 0, s>>>(w.cd, sh.K, sh.nc, sh.cs, sh.max_num, dir_offset, dir_limit_offset,
                                                  w.nkeep, w.cat_key, w.cat_src, boxes, scores, labels, counts);
  return launch_status();
}

}  // namespace

extern "C" size_t pd3_anchor3d_head_workspace(int batch, int feat_h, int feat_w, int num_anchors, int num_classes,
                                              int code_size, int nms_pre) {
  A3dShape sh;
  if (batch <= 0 || a3d_shape(batch, -1, feat_h, feat_w, num_anchors, num_classes, code_size, nms_pre, 1, sh) != PD3_OK)
    return 0;
  return a3d_carve(nullptr, sh).bytes;
}

extern "C" int pd3_anchor3d_head_forward(const void* feat, const void* cls_weight_packed, const void* cls_bias,
                                         const void* reg_weight, const void* reg_bias, const void* dir_weight,
                                         const void* dir_bias, const void* anchors, int batch, int channels, int feat_h,
                                         int feat_w, int num_anchors, int num_classes, int code_size, int nms_pre,
                                         int max_num, float score_thr, float nms_thr, float dir_offset,
                                         float dir_limit_offset, void* boxes, void* scores, void* labels, void* counts,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  if (channels <= 0) return PD3_EINVAL;
  A3dShape sh;
  const int st = a3d_shape(batch, channels, feat_h, feat_w, num_anchors, num_classes, code_size, nms_pre, max_num, sh);
  if (st != PD3_OK) return st;
  if (batch == 0) return PD3_OK;
  if (!feat || !cls_weight_packed || !cls_bias || !reg_weight || !reg_bias || !dir_weight || !dir_bias || !anchors ||
      !boxes || !scores || !labels || !counts || !workspace)
    return PD3_EINVAL;
  const A3dWorkspace w = a3d_carve(workspace, sh);
  if (workspace_bytes < w.bytes) return PD3_EWORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const hipError_t e = hipMemsetAsync(w.pool.counts, 0, (size_t)sh.B * sh.nc * 2 * kNmsCtrStride * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  const float* f = static_cast<const float*>(feat);
  const float* wp = static_cast<const float*>(cls_weight_packed);
  const float* cb = static_cast<const float*>(cls_bias);
  a3d_dense_max_kernel<<<dim3((sh.HW + kDensePixels - 1) / kDensePixels, sh.B), 256, 0, s>>>(f, wp, cb, sh, w.max_score);
  return a3d_finish<true>(sh, w, f, wp, cb, static_cast<const float*>(reg_weight), static_cast<const float*>(reg_bias),
                          static_cast<const float*>(dir_weight), static_cast<const float*>(dir_bias), nullptr, nullptr,
                          nullptr, static_cast<const float*>(anchors), score_thr, nms_thr, dir_offset, dir_limit_offset,
                          static_cast<float*>(boxes), static_cast<float*>(scores), static_cast<int32_t*>(labels),
                          static_cast<int32_t*>(counts), s);
}

extern "C" int pd3_anchor3d_get_bboxes(const void* cls_score, const void* bbox_pred, const void* dir_cls_pred,
                                       const void* anchors, int batch, int feat_h, int feat_w, int num_anchors,
                                       int num_classes, int code_size, int nms_pre, int max_num, float score_thr,
                                       float nms_thr, float dir_offset, float dir_limit_offset, void* boxes,
                                       void* scores, void* labels, void* counts, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  A3dShape sh;
  const int st = a3d_shape(batch, -1, feat_h, feat_w, num_anchors, num_classes, code_size, nms_pre, max_num, sh);
  if (st != PD3_OK) return st;
  if (batch == 0) return PD3_OK;
  if (!cls_score || !bbox_pred || !dir_cls_pred || !anchors || !boxes || !scores || !labels || !counts || !workspace)
    return PD3_EINVAL;
  const A3dWorkspace w = a3d_carve(workspace, sh);
  if (workspace_bytes < w.bytes) return PD3_EWORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const hipError_t e = hipMemsetAsync(w.pool.counts, 0, (size_t)sh.B * sh.nc * 2 * kNmsCtrStride * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  const float* cm = static_cast<const float*>(cls_score);
  a3d_maps_max_kernel<<<dim3((sh.HW + 255) / 256, sh.A, sh.B), 256, 0, s>>>(cm, sh, w.max_score);
  return a3d_finish<false>(sh, w, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, cm,
                           static_cast<const float*>(bbox_pred), static_cast<const float*>(dir_cls_pred),
                           static_cast<const float*>(anchors), score_thr, nms_thr, dir_offset, dir_limit_offset,
                           static_cast<float*>(boxes), static_cast<float*>(scores), static_cast<int32_t*>(labels),
                           static_cast<int32_t*>(counts), s);
}
