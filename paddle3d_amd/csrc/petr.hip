// PETR / PETRv2's head (paddle3d/models/heads/dense_heads/petr_head.py, models/layers/petr_transformer.py,
// models/layers/transformer_layers.py): the two stages that are more than Linear layers and 1x1 convolutions, each as
// one kernel, fp32.
//
// pd3_mha_stream_forward             paddle.nn.MultiHeadAttention's core for any number of keys, with a key padding mask
//   q [B, Nq, M, d], k and v [B, Nk, M, d] (the Linear outputs viewed per head), key_mask uint8 [B, Nk] or NULL (non-zero:
//   padded), scale (host float, head_dim ** -0.5 rounded to fp32) -> out [B, Nq, M * d].  PETRMultiheadAttention inverts
//   the padding mask and Paddle turns the boolean attn_mask into the additive (cast(mask) - 1.0) * 1e9, so a padded key
//   keeps its place in the softmax with -1e9f added to its score; it is not skipped.  Per (b, m, query i), in this order:
//     qs_c = q_ic * scale
//     s_j  = fmaf(qs_{d-1}, k_{j,d-1}, ... fmaf(qs_1, k_j1, fmaf(qs_0, k_j0, +0)))         ascending c (pd3_mha_forward's)
//     t_j  = s_j + (-1e9f) for a padded key, s_j otherwise
//     mx   = t_0 when t_0 is a NaN, else the largest t_j that is no NaN (pd3_mha_forward's convention; the sign of a
//            zero maximum does not reach e)
//     e_j  = expf(t_j - mx)  (glibc's bits, libm_exact.hpp)
//     p_l  = ((0 + e_l) + e_{l+64}) + e_{l+128} ...  for l = 0 .. 63 (p_l = 0 for l >= Nk);
//     sum  = the halving tree over p: 32 times p_l + p_{l+32}, then 16 times + 16, ... down to one value
//            (pd3_mha_forward's association: it depends on Nk only)
//     A_w  for w = 0 .. 3, per channel c: the fmaf chain from +0 of fmaf(e_j, v_jc, .) over the keys of the 16-key tiles
//            T = w, w + 4, w + 8, ... in ascending T, and inside a tile in the order 16 T + (0, 4, 8, 12, 1, 5, 9, 13,
//            2, 6, 10, 14, 3, 7, 11, 15); keys >= Nk take part as fmaf(+0, +0, .), which changes no bit
//            (a partition of the keys that depends on Nk only; A_w = +0 when w >= ceil(Nk / 16))
//     out_c = (((A_0 + A_1) + A_2) + A_3) / sum                                  one division per output element
//   The weights e_j are not divided: the division is applied once to the accumulated row.  Nothing above depends on
//   Nq, on the query tiling, on the frame's place in the batch, on the grid or on the stream; it depends on (Nk, d).
//   Every product is v_mfma_f32_16x16x4_f32, whose result is the k-ordered fp32 fmaf chain (csrc/bevformer_decoder.hip
//   relies on the same).  A workgroup (256 threads, 4 waves) owns 16 queries of one (b, m); wave w owns the key tiles
//   w, w + 4, ...  Scores are computed transposed, S^T = K Qs^T (keys as M, queries as N; a * b commutes, so the chain
//   is s_j's): lane (query = lane & 15, g = lane >> 4) then holds the scores of keys 16 T + 4 g + r, r = 0 .. 3, of its
//   query, which is the A operand P V wants when MFMA step r of a tile takes keys 16 T + 4 g + r -- no score ever goes
//   through LDS or global memory; hence the key order above.
//     pass 1  every wave walks its tiles: d / 4 MFMAs, the mask, the running maximum; xor 16, 32 and [4][16] floats
//             of LDS combine the maxima (a maximum of numbers is exact in any order)
//     pass 2  the same scores again (the same chain, the same bits), expf (its table in LDS), p_{16 w + 4 g + r} +=
//             e, and 4 * d / 16 MFMAs into the d / 16 accumulators of the wave; then P [16][64] and A [4][16][d] go to
//             LDS, the xor butterfly gives sum (every lane the same bits, addition being commutative), and the
//             workgroup adds the four A_w, divides and stores 16 rows of d floats
//   The k fragments of the next tile are fetched before the MFMAs of the current one; v of the current tile is
//   fetched before its scores are computed.  Block index = query block * (B * M) + (b * M + m): with B * M a multiple
//   of 8 all query blocks of a head run on one XCD and share its L2.
//   LDS: 16 * 64 + 4 * 16 * (d + 4) floats and less than 1 KiB more, whatever Nk is.
//   Padded query rows load 0 and are never stored; padded keys load 0 for k and v, never count for mx and have e =
//   +0.  No address outside q, k, v, key_mask is formed for a load.
//   Supported (mha_stream_supported): d % 16 == 0, d <= 128, q, k, v and out 16-byte aligned (every access is a single
//   float today; the alignment is reserved for vector loads).  Anything else: PD3_EUNSUPPORTED without a launch.
//
// pd3_petr_coords3d                  PETRHead.position_embeding from the frustum grid through inverse_sigmoid
//   img2lidars [BN, 4, 4] (rows m_c), H, W, D, pad_h, pad_w (integers), depth_start (double), position_range r[6] host
//   floats, LID, token_mask uint8 [BN, H, W] or NULL -> coords [BN, 3 * D, H, W] (channel d * 3 + c), coords_mask uint8
//   [BN, H, W] or NULL.  Host, once: bin = (float)(((double)r3 - depth_start) / (D * (1 + D))) with LID, (float)(((double)
//   r3 - depth_start) / D) without; den_c = (float)((double)r_{c+3} - (double)r_c); ds = (float)depth_start; eps = 1e-5f.
//   Per (bn, h, w, d), plain fp32, every operation rounded on its own:
//     ch = ((float)h * (float)pad_h) / (float)H;  cw = ((float)w * (float)pad_w) / (float)W
//     i = (float)d;  cd = ((bin * i) * (i + 1)) + ds with LID, (bin * i) + ds without
//     s = cd < eps ? eps : cd;  x = cw * s;  y = ch * s
//     v_c = ((m_c0 * x + m_c1 * y) + m_c2 * cd) + m_c3                                     c = 0, 1, 2
//     n_c = (v_c - r_c) / den_c;   outside_c = n_c > 1 || n_c < 0  (a NaN is not outside)
//     n_c = n_c < 0 ? 0 : (n_c > 1 ? 1 : n_c);  x1 = n_c < eps ? eps : n_c;  u = 1 - n_c;  x2 = u < eps ? eps : u
//     ratio = x1 / x2;  coords = (float)log((double)ratio)    (a NaN stays one through every comparison)
//   coords_mask = (2 * (number of outside_c over d and c) > D) || token_mask != 0, the reference's `sum > D * 0.5`.
//   A workgroup (256 threads) owns 64 consecutive w of one (bn, h): thread (w = tid & 63, g = tid >> 6) walks d = g, g +
//   4, ...; stores are coalesced along w; the four counts of a w meet in 1 KiB of LDS (integers: exact in any order).
//   No [.., 4, 4] tile is formed.  Every shape whose BN * H * ceil(W / 64) is below 2^31 is taken (PD3_EUNSUPPORTED
//   beyond); nothing needs an alignment.
//
// No FMA but the MFMA chains (-ffp-contract=off), no atomics on global memory, no zeroing pass, 64-bit offsets.
#include "../../include/paddle3d_amd.h"
#include "bevformer_attn.hpp"

#include <cmath>

namespace {

using namespace pd3;
using namespace pd3::bevattn;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kStreamThreads = 256;
constexpr int kStreamWaves = kStreamThreads / kWave;
constexpr int kStreamMaxD = 128;
constexpr int kAPad = 4;
constexpr float kMaskAdd = -1e9f;

template <int DT>  // head_dim / 16
__global__ void __launch_bounds__(kStreamThreads) mha_stream_kernel(const float* __restrict__ q,
                                                                    const float* __restrict__ k,
                                                                    const float* __restrict__ v,
                                                                    const uint8_t* __restrict__ key_mask,
                                                                    float* __restrict__ out, int Nq, int Nk, int M,
                                                                    int BM, float scale) {
  constexpr int d = 16 * DT, S = 4 * DT, AS = d + kAPad;
  __shared__ uint64_t etab[32];  // expf's table (libm_exact.hpp expf_with)
  __shared__ float wmx[kStreamWaves][16], t0s[16], sums[16];
  __shared__ float P[16][kWave + 1];
  __shared__ float A[kStreamWaves][16][AS];
  lm::exp2f_tab_fill(etab);
  const auto tab = [&](int i) { return etab[i]; };
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
  const int col = lane & 15, g = lane >> 4;
  const int64_t bm = blockIdx.x % (unsigned)BM;
  const int q0 = (int)(blockIdx.x / (unsigned)BM) * 16;
  const int m = (int)(bm % M);
  const int64_t b = bm / M;
  const int64_t MD = (int64_t)M * d;
  const int NT = (Nk + 15) >> 4;
  // ---- the scaled queries, as the B operand: lane (query col, g) holds qs[col][4 s + g] ----------------------------
  float qs[S];
  {
    const int qi = q0 + col;
    const float* qp = q + ((b * Nq + (qi < Nq ? qi : 0)) * M + m) * d + g;
#pragma unroll
    for (int s = 0; s < S; ++s) qs[s] = qi < Nq ? qp[4 * s] * scale : 0.0f;
  }
  const float* kbase = k + (b * Nk * M + m) * d;
  const float* vbase = v + (b * Nk * M + m) * d;
  const uint8_t* mbase = key_mask ? key_mask + b * Nk : nullptr;
  const auto fetch_k = [&](int t, float (&kr)[S]) {  // behind the list or the keys: zeros, no load
    const int j = t * 16 + col;
    const bool ok = t < NT && j < Nk;
    const float* kp = kbase + (ok ? j : 0) * MD + g;
#pragma unroll
    for (int s = 0; s < S; ++s) kr[s] = ok ? kp[4 * s] : 0.0f;
  };
  const auto fetch_mask = [&](int t, bool (&pad)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = t * 16 + 4 * g + r;
      pad[r] = mbase && j < Nk ? mbase[j] != 0 : false;
    }
  };
  const auto scores = [&](const float (&kr)[S], const bool (&pad)[4]) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < S; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[s], qs[s], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (pad[r]) acc[r] = acc[r] + kMaskAdd;
    return acc;
  };
  // ---- pass 1: the maximum of the query's scores -------------------------------------------------------------------
  float mx = -INFINITY, t0 = 0.0f;
  {
    float kr[S], kn[S];
    fetch_k(wave, kr);
    for (int t = wave; t < NT; t += kStreamWaves) {
      bool pad[4];
      fetch_mask(t, pad);
      fetch_k(t + kStreamWaves, kn);
      const f32x4 acc = scores(kr, pad);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float x = acc[r];
        if (t * 16 + 4 * g + r < Nk) mx = x > mx ? x : mx;
      }
      if (t == 0) t0 = acc[0];  // key 0 in the lanes with g == 0
#pragma unroll
      for (int s = 0; s < S; ++s) kr[s] = kn[s];
    }
  }
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const float x = __shfl_xor(mx, o, kWave);
    mx = x > mx ? x : mx;
  }
  if (g == 0) {
    wmx[wave][col] = mx;
    if (wave == 0) t0s[col] = t0;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kStreamWaves; ++w) {
    const float x = wmx[w][col];
    mx = x > mx ? x : mx;
  }
  t0 = t0s[col];
  if (t0 != t0) mx = t0;
  // ---- pass 2: e, the lane sums and the wave's share of P V ---------------------------------------------------------
  float p[4] = {0.f, 0.f, 0.f, 0.f};
  f32x4 oacc[DT];
#pragma unroll
  for (int ct = 0; ct < DT; ++ct) oacc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    float kr[S], kn[S];
    fetch_k(wave, kr);
    for (int t = wave; t < NT; t += kStreamWaves) {
      bool pad[4];
      fetch_mask(t, pad);
      float vr[DT][4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = t * 16 + 4 * g + r;
        const float* vp = vbase + (j < Nk ? j : 0) * MD + col;
#pragma unroll
        for (int ct = 0; ct < DT; ++ct) vr[ct][r] = j < Nk ? vp[16 * ct] : 0.0f;
      }
      fetch_k(t + kStreamWaves, kn);
      const f32x4 acc = scores(kr, pad);
      float e[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool in = t * 16 + 4 * g + r < Nk;
        e[r] = lm::expf_with(in ? acc[r] - mx : 0.0f, tab);
        e[r] = in ? e[r] : 0.0f;
        p[r] = p[r] + e[r];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int ct = 0; ct < DT; ++ct) oacc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(e[r], vr[ct][r], oacc[ct], 0, 0, 0);
      }
#pragma unroll
      for (int s = 0; s < S; ++s) kr[s] = kn[s];
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) P[col][16 * wave + 4 * g + r] = p[r];
#pragma unroll
  for (int ct = 0; ct < DT; ++ct) {
#pragma unroll
    for (int r = 0; r < 4; ++r) A[wave][4 * g + r][16 * ct + col] = oacc[ct][r];
  }
  __syncthreads();
  for (int i = 4 * wave; i < 4 * wave + 4; ++i) {
    float x = P[i][lane];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = x + __shfl_xor(x, o, kWave);
    if (lane == 0) sums[i] = x;
  }
  __syncthreads();
  for (int idx = tid; idx < 16 * d; idx += kStreamThreads) {
    const int i = idx / d, c = idx - i * d;
    const int qi = q0 + i;
    if (qi < Nq) {
      const float a = ((A[0][i][c] + A[1][i][c]) + A[2][i][c]) + A[3][i][c];
      out[((b * Nq + qi) * M + m) * d + c] = a / sums[i];
    }
  }
}

template <int DT>
int launch_stream(const float* q, const float* k, const float* v, const uint8_t* key_mask, float* out, int Nq, int Nk,
                  int M, int BM, unsigned blocks, float scale, hipStream_t stream) {
  hipLaunchKernelGGL(mha_stream_kernel<DT>, dim3(blocks), dim3(kStreamThreads), 0, stream, q, k, v, key_mask, out, Nq, Nk,
                     M, BM, scale);
  return pd3::launch_status();
}

bool mha_stream_supported(const void* q, const void* k, const void* v, const void* out, int d) {
  return d >= 16 && d % 16 == 0 && d <= kStreamMaxD && aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out);
}

constexpr int kCoordThreads = 256;
constexpr int kCoordW = 64;                             // consecutive w of a workgroup
constexpr int kCoordG = kCoordThreads / kCoordW;        // threads that share a w and split d
constexpr float kCoordEps = 1e-5f;

struct CoordCfg {
  int H, W, D, WT, LID;
  float pad_h, pad_w, ds, bin;
  float r[3], den[3];
};

__global__ void __launch_bounds__(kCoordThreads) petr_coords3d_kernel(CoordCfg c, const float* __restrict__ img2lidars,
                                                                      const uint8_t* __restrict__ token_mask,
                                                                      float* __restrict__ coords,
                                                                      uint8_t* __restrict__ coords_mask) {
  __shared__ int cnt[kCoordG][kCoordW];
  const int wl = threadIdx.x & (kCoordW - 1), g = threadIdx.x / kCoordW;
  const int wt = (int)(blockIdx.x % (unsigned)c.WT);
  const int64_t row = blockIdx.x / (unsigned)c.WT;  // bn * H + h
  const int h = (int)(row % c.H);
  const int64_t bn = row / c.H;
  const int w = wt * kCoordW + wl;
  const bool active = w < c.W;
  float mat[3][4];
#pragma unroll
  for (int i = 0; i < 12; ++i) mat[i >> 2][i & 3] = img2lidars[bn * 16 + i];
  const float ch = ((float)h * c.pad_h) / (float)c.H;
  const float cw = ((float)w * c.pad_w) / (float)c.W;
  const int64_t HW = (int64_t)c.H * c.W;
  int outside = 0;
  if (active) {
    float* dst = coords + (bn * 3 * c.D * c.H + h) * c.W + w;
    for (int d = g; d < c.D; d += kCoordG) {
      const float i = (float)d;
      const float cd = c.LID ? ((c.bin * i) * (i + 1.0f)) + c.ds : (c.bin * i) + c.ds;
      const float s = cd < kCoordEps ? kCoordEps : cd;
      const float x = cw * s, y = ch * s;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float val = ((mat[a][0] * x + mat[a][1] * y) + mat[a][2] * cd) + mat[a][3];
        float n = (val - c.r[a]) / c.den[a];
        outside += (n > 1.0f || n < 0.0f) ? 1 : 0;
        n = n < 0.0f ? 0.0f : (n > 1.0f ? 1.0f : n);
        const float x1 = n < kCoordEps ? kCoordEps : n;
        const float u = 1.0f - n;
        const float x2 = u < kCoordEps ? kCoordEps : u;
        const float ratio = x1 / x2;
        dst[(int64_t)(d * 3 + a) * HW] = (float)log((double)ratio);
      }
    }
  }
  if (!coords_mask) return;  // uniform
  cnt[g][wl] = outside;
  __syncthreads();
  if (g == 0 && active) {
    int total = 0;
#pragma unroll
    for (int i = 0; i < kCoordG; ++i) total += cnt[i][wl];
    const int64_t o = row * c.W + w;
    const bool tm = token_mask ? token_mask[o] != 0 : false;
    coords_mask[o] = (2 * total > c.D || tm) ? 1 : 0;
  }
}

}  // namespace

extern "C" {

int pd3_mha_stream_forward(const void* q, const void* k, const void* v, const void* key_mask, int batch, int num_query,
                           int num_key, int num_heads, int head_dim, float scale, void* out, void* stream) {
  if (batch < 0 || num_query < 0 || num_key < 1 || num_heads < 1 || head_dim < 1) return PD3_EINVAL;
  if (!mha_stream_supported(q, k, v, out, head_dim)) return PD3_EUNSUPPORTED;
  if (batch == 0 || num_query == 0) return PD3_OK;
  if (!q || !k || !v || !out) return PD3_EINVAL;
  const int64_t BM = (int64_t)batch * num_heads;
  const int64_t blocks = BM * ((num_query + 15) / 16);
  if (blocks > 0x7fffffff) return PD3_EUNSUPPORTED;
  const float* qf = static_cast<const float*>(q);
  const float* kf = static_cast<const float*>(k);
  const float* vf = static_cast<const float*>(v);
  const uint8_t* mf = static_cast<const uint8_t*>(key_mask);
  float* of = static_cast<float*>(out);
  const hipStream_t st = (hipStream_t)stream;
#define PD3_STREAM_CASE(DT) \
  case DT:                  \
    return launch_stream<DT>(qf, kf, vf, mf, of, num_query, num_key, num_heads, (int)BM, (unsigned)blocks, scale, st)
  switch (head_dim / 16) {
    PD3_STREAM_CASE(1);
    PD3_STREAM_CASE(2);
    PD3_STREAM_CASE(3);
    PD3_STREAM_CASE(4);
    PD3_STREAM_CASE(5);
    PD3_STREAM_CASE(6);
    PD3_STREAM_CASE(7);
    PD3_STREAM_CASE(8);
  }
#undef PD3_STREAM_CASE
  return PD3_EUNSUPPORTED;
}

int pd3_petr_coords3d(const void* img2lidars, int num_views, int feat_h, int feat_w, int depth_num, int pad_h, int pad_w,
                      double depth_start, const float* position_range, int lid, const void* token_mask, void* coords,
                      void* coords_mask, void* stream) {
  if (num_views < 0 || feat_h < 0 || feat_w < 0 || depth_num < 0 || !position_range || !(depth_start == depth_start))
    return PD3_EINVAL;
  if (num_views == 0 || feat_h == 0 || feat_w == 0 || depth_num == 0) return PD3_OK;
  CoordCfg c;
  c.H = feat_h, c.W = feat_w, c.D = depth_num, c.LID = lid ? 1 : 0;
  c.WT = (feat_w + kCoordW - 1) / kCoordW;
  const int64_t blocks = (int64_t)num_views * feat_h * c.WT;
  if (blocks > 0x7fffffff) return PD3_EUNSUPPORTED;
  if (!img2lidars || !coords) return PD3_EINVAL;
  c.pad_h = (float)pad_h, c.pad_w = (float)pad_w, c.ds = (float)depth_start;
  const double span = (double)position_range[3] - depth_start;
  c.bin = lid ? (float)(span / ((double)depth_num * (1.0 + (double)depth_num))) : (float)(span / (double)depth_num);
  for (int i = 0; i < 3; ++i) {
    c.r[i] = position_range[i];
    c.den[i] = (float)((double)position_range[i + 3] - (double)position_range[i]);
  }
  hipLaunchKernelGGL(petr_coords3d_kernel, dim3((unsigned)blocks), dim3(kCoordThreads), 0, (hipStream_t)stream, c,
                     static_cast<const float*>(img2lidars), static_cast<const uint8_t*>(token_mask),
                     static_cast<float*>(coords), static_cast<uint8_t*>(coords_mask));
  return pd3::launch_status();
}

}  // extern "C"
