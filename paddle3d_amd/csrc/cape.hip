// CAPE / CAPE-T's head (paddle3d/models/layers/cape_transformer.py): the two stages that are more than Linear layers,
// each as one kernel, fp32.  The sibling of csrc/petr.hip: read that file's header first.
//
// pd3_cape_cva_forward               CrossAttention.forward (cape_transformer.py:200-269) from the projected rows to the
//   per-head output.  q_a [B, Q, M, d], q_g [B, N, Q, M, d], k_a, k_g and v [B, N, K, M, d] (the Linear outputs viewed per
//   head, no permuted copy), mask uint8 [B, N, K] or NULL (non-zero: masked), scale_a and scale_g device float [M] (they
//   are parameters: read here, never on the host) -> out [B, Q, M * d], what self.proj receives.  The softmax runs over
//   the N * K keys of all cameras; the geometry query differs per camera.  The keys of camera n are padded to KT =
//   ceil(K / 16) tiles of 16, so no tile straddles two cameras; tile T = n * KT + t holds the keys 16 t + (0 .. 15) of
//   camera n, those with 16 t + o >= K being padding.  Per (b, m, query i), in this order:
//     a_nj = fmaf(qa_{d-1}, ka_{nj,d-1}, ... fmaf(qa_0, ka_{nj,0}, +0))         ascending c (q_a of the query, k_a of key
//                                                                               j of camera n)
//     g_nj = fmaf(qg_{n,d-1}, kg_{nj,d-1}, ... fmaf(qg_{n,0}, kg_{nj,0}, +0))   (q_g of the query FOR CAMERA n)
//     s_nj = (a_nj * scale_a[m]) + (g_nj * scale_g[m])          three roundings, the reference's dot_a * scale_a + dot_g *
//                                                               scale_g; no FMA
//     t_nj = -inf for a masked key (replaced, not added to: masked_fill), s_nj otherwise
//     mx   = t_00 when t_00 is a NaN, else the largest t_nj that is no NaN (pd3_mha_forward's convention); -inf when
//            every key is masked
//     e_nj = expf(t_nj - mx)  (glibc's bits, libm_exact.hpp): +0 for a masked key beside an unmasked one; a row whose
//            keys are all masked has -inf - -inf = NaN everywhere, and its output is NaN -- the reference's softmax
//     The padded key list has NT = N * KT tiles; padding keys have e = +0 and never count for mx.  With l = 0 .. 63:
//     p_l  = ((0 + e_l) + e_{l+64}) + e_{l+128} ...  over the padded list (p_l = 0 for l >= 16 NT);
//     sum  = the halving tree over p: 32 times p_l + p_{l+32}, then 16 times + 16, ... down to one value
//     A_w  for w = 0 .. 3, per channel c: the fmaf chain from +0 of fmaf(e, v_c, .) over the keys of the tiles T = w,
//            w + 4, w + 8, ... in ascending T, and inside a tile in the order 16 t + (0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10,
//            14, 3, 7, 11, 15); padding keys take part as fmaf(+0, +0, .), which changes no bit
//     out_c = (((A_0 + A_1) + A_2) + A_3) / sum                                  one division per output element
//   Nothing above depends on Q, on the query tiling, on the frame's place in the batch, on the grid or on the stream;
//   the partition of the keys and the association of the sums depend on (N, K, d) only.
//   Masked keys are NOT skipped: a masked key, and a wholly masked camera, takes part as fmaf(+0, v, .).  The reference
//   multiplies the zero weight by v, so an Inf or a NaN in v under a masked key (or under an unmasked key whose weight
//   underflowed to 0) makes the row's channel NaN; so it does here.
//   Every product is v_mfma_f32_16x16x4_f32, whose result is the k-ordered fp32 fmaf chain.  A workgroup (256 threads, 4
//   waves) owns 16 queries of one (b, m); wave w owns the tiles w, w + 4, ...  Scores are computed transposed, S^T = K
//   Q^T twice (k_a with q_a, k_g with q_g of the tile's camera) -- lane (query = lane & 15, g = lane >> 4) holds the scores
//   of keys 16 t + 4 g + r, r = 0 .. 3, of its query, the A operand of P V; no score, weight or expanded q_a goes through
//   LDS or global memory.  A wave keeps q_a and the q_g of its current camera in registers (2 * d / 4 floats per lane)
//   and reloads q_g only when its next tile belongs to another camera.  Two passes, as in mha_stream_kernel: the maximum
//   first, then the same scores again (the same chains, the same bits), expf with its table in LDS, the lane sums and P V.
//   Block index = query block * (B * M) + (b * M + m): with B * M a multiple of 8 all query blocks of a head run on one
//   XCD and share its L2 (petr.hip's reasoning; CAPE-T: 2 frames * 8 heads).
//   LDS: 16 * 65 + 4 * 16 * (d + 4) floats and less than 1 KiB more, whatever N and K are.
//   Padded query rows load 0 and are never stored; padding keys load 0 for k_a, k_g and v.  No address outside the
//   operands is formed for a load.
//   Supported (cva_supported): d % 16 == 0, d <= 128 (no instance uses scratch: DESIGN.md 4.5zh), the five row tensors
//   and out 16-byte aligned (every access is a single float today; the alignment is reserved for vector loads; the mask
//   and the scales need none), N * ceil(K / 16) and B * M * ceil(Q / 16) below 2^31.  Anything else: PD3_EUNSUPPORTED
//   without a launch.
//
// pd3_cape_posemb3d                  pos2posemb3d (cape_transformer.py:76-91), optionally behind prepare_emb's world
//   transform (:540-557).  points [B, Q, 3]; bound (6 host floats lo_xyz, hi_xyz, or NULL: the points are in final
//   units); rot [B, N, 3, 3] and trans [B, N, 3], or both NULL (num_views == 0); dim_t [F] host floats (the reference's
//   temperature ** (2 * (i // 2) / F), computed by the caller in the reference's order) -> out [B, N, Q, 3 * F], or [B, Q,
//   3 * F] without views.  Host, once: span_c = hi_c - lo_c in fp32; two_pi = (float)(2 * pi).  Per (b, n, q), plain fp32,
//   every operation rounded on its own:
//     u_c = (p_c * span_c) + lo_c                                   with bound, p_c without
//     w_c = u_c + t_{n,c};  x_r = ((R_{n,r0} * w_0) + (R_{n,r1} * w_1)) + (R_{n,r2} * w_2)        with views, x = u without
//     s_c = x_c * two_pi;  y_ci = s_c / dim_t[i]
//     e_ci = sinf(y_ci) for even i, cosf(y_ci) for odd i  (glibc's bits, libm_exact.hpp)
//     row = (e_10 .. e_1,F-1, e_00 .. e_0,F-1, e_20 .. e_2,F-1)                      the reference's concat (y, x, z)
//   One thread per output element (the transform of a point is a dozen operations beside one sinf); stores are
//   coalesced along the row.  Supported (posemb3d_supported): F even, 2 <= F <= 128 (dim_t travels as a kernel
//   argument), fewer than 2^31 workgroups.  Nothing needs an alignment.
//
// No FMA but the MFMA chains (-ffp-contract=off), no atomics on global memory, no zeroing pass, 64-bit offsets.
#include "../../include/paddle3d_amd_cape.h"
#include "bevformer_attn.hpp"

#include <cmath>

namespace {

using namespace pd3;
using namespace pd3::bevattn;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kCvaThreads = 256;
constexpr int kCvaWaves = kCvaThreads / kWave;
constexpr int kCvaMaxD = 128;
constexpr int kAPad = 4;

struct CvaArgs {
  const float* q_a;
  const float* q_g;
  const float* k_a;
  const float* k_g;
  const float* v;
  const uint8_t* mask;
  const float* scale_a;
  const float* scale_g;
  float* out;
  int N, Q, K, M, BM;
};

template <int DT>  // head_dim / 16
__global__ void __launch_bounds__(kCvaThreads) cape_cva_kernel(CvaArgs a) {
  constexpr int d = 16 * DT, S = 4 * DT, AS = d + kAPad;
  __shared__ uint64_t etab[32];  // expf's table (libm_exact.hpp expf_with)
  __shared__ float wmx[kCvaWaves][16], t0s[16], sums[16];
  __shared__ float P[16][kWave + 1];
  __shared__ float A[kCvaWaves][16][AS];
  lm::exp2f_tab_fill(etab);
  const auto tab = [&](int i) { return etab[i]; };
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
  const int col = lane & 15, g = lane >> 4;
  const int N = a.N, Q = a.Q, K = a.K, M = a.M;
  const int64_t bm = blockIdx.x % (unsigned)a.BM;
  const int q0 = (int)(blockIdx.x / (unsigned)a.BM) * 16;
  const int m = (int)(bm % M);
  const int64_t b = bm / M;
  const int KT = (K + 15) >> 4;
  const int NT = N * KT;
  const float sa = a.scale_a[m], sg = a.scale_g[m];
  const int qi = q0 + col;
  const bool qok = qi < Q;
  // ---- the queries, as the B operand: lane (query col, g) holds q[col][4 s + g] --------------------------------------
  float qa[S], qg[S];
  {
    const float* qp = a.q_a + ((b * Q + (qok ? qi : 0)) * M + m) * d + g;
#pragma unroll
    for (int s = 0; s < S; ++s) qa[s] = qok ? qp[4 * s] : 0.0f;
  }
  const auto fetch_qg = [&](int n) {
    const float* qp = a.q_g + (((b * N + n) * Q + (qok ? qi : 0)) * M + m) * d + g;
#pragma unroll
    for (int s = 0; s < S; ++s) qg[s] = qok ? qp[4 * s] : 0.0f;
  };
  const auto fetch_k = [&](int T, float (&kar)[S], float (&kgr)[S]) {  // behind the list or the camera: zeros, no load
    const int n = T / KT;
    const int j = (T - n * KT) * 16 + col;
    const bool ok = T < NT && j < K;
    const int64_t off = (((b * N + (ok ? n : 0)) * K + (ok ? j : 0)) * M + m) * d + g;
    const float* kap = a.k_a + off;
    const float* kgp = a.k_g + off;
#pragma unroll
    for (int s = 0; s < S; ++s) kar[s] = ok ? kap[4 * s] : 0.0f;
#pragma unroll
    for (int s = 0; s < S; ++s) kgr[s] = ok ? kgp[4 * s] : 0.0f;
  };
  // the four keys of this lane in tile (n, t): inside the camera, and masked
  const auto fetch_mask = [&](int n, int t, bool (&in)[4], bool (&msk)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = t * 16 + 4 * g + r;
      in[r] = j < K;
      msk[r] = a.mask && in[r] ? a.mask[(b * N + n) * K + j] != 0 : false;
    }
  };
  const auto scores = [&](const float (&kar)[S], const float (&kgr)[S], const bool (&msk)[4]) {
    f32x4 da = {0.f, 0.f, 0.f, 0.f}, dg = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < S; ++s) da = __builtin_amdgcn_mfma_f32_16x16x4f32(kar[s], qa[s], da, 0, 0, 0);
#pragma unroll
    for (int s = 0; s < S; ++s) dg = __builtin_amdgcn_mfma_f32_16x16x4f32(kgr[s], qg[s], dg, 0, 0, 0);
    f32x4 t;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float x = da[r] * sa;
      const float y = dg[r] * sg;
      t[r] = msk[r] ? -INFINITY : x + y;
    }
    return t;
  };
  // ---- pass 1: the maximum of the query's scores -------------------------------------------------------------------
  float mx = -INFINITY, t0 = 0.0f;
  {
    float kar[S], kgr[S], kan[S], kgn[S];
    int cam = -1;
    fetch_k(wave, kar, kgr);
    for (int T = wave; T < NT; T += kCvaWaves) {
      const int n = T / KT, t = T - n * KT;
      if (n != cam) {  // wave-uniform
        fetch_qg(n);
        cam = n;
      }
      bool in[4], msk[4];
      fetch_mask(n, t, in, msk);
      fetch_k(T + kCvaWaves, kan, kgn);
      const f32x4 acc = scores(kar, kgr, msk);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float x = acc[r];
        if (in[r]) mx = x > mx ? x : mx;
      }
      if (T == 0) t0 = acc[0];  // key 0 of camera 0 in the lanes with g == 0
#pragma unroll
      for (int s = 0; s < S; ++s) kar[s] = kan[s], kgr[s] = kgn[s];
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
  for (int w = 0; w < kCvaWaves; ++w) {
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
    float kar[S], kgr[S], kan[S], kgn[S];
    int cam = -1;
    fetch_k(wave, kar, kgr);
    for (int T = wave; T < NT; T += kCvaWaves) {
      const int n = T / KT, t = T - n * KT;
      if (n != cam) {
        fetch_qg(n);
        cam = n;
      }
      bool in[4], msk[4];
      fetch_mask(n, t, in, msk);
      float vr[DT][4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = t * 16 + 4 * g + r;
        const float* vp = a.v + (((b * N + n) * K + (in[r] ? j : 0)) * M + m) * d + col;
#pragma unroll
        for (int ct = 0; ct < DT; ++ct) vr[ct][r] = in[r] ? vp[16 * ct] : 0.0f;
      }
      fetch_k(T + kCvaWaves, kan, kgn);
      const f32x4 acc = scores(kar, kgr, msk);
      float e[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        e[r] = lm::expf_with(in[r] ? acc[r] - mx : 0.0f, tab);
        e[r] = in[r] ? e[r] : 0.0f;
        p[r] = p[r] + e[r];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int ct = 0; ct < DT; ++ct) oacc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(e[r], vr[ct][r], oacc[ct], 0, 0, 0);
      }
#pragma unroll
      for (int s = 0; s < S; ++s) kar[s] = kan[s], kgr[s] = kgn[s];
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
  for (int idx = tid; idx < 16 * d; idx += kCvaThreads) {
    const int i = idx / d, c = idx - i * d;
    const int qo = q0 + i;
    if (qo < Q) {
      const float x = ((A[0][i][c] + A[1][i][c]) + A[2][i][c]) + A[3][i][c];
      a.out[((b * Q + qo) * M + m) * d + c] = x / sums[i];
    }
  }
}

template <int DT>
int launch_cva(const CvaArgs& a, unsigned blocks, hipStream_t stream) {
  hipLaunchKernelGGL(cape_cva_kernel<DT>, dim3(blocks), dim3(kCvaThreads), 0, stream, a);
  return pd3::launch_status();
}

bool cva_supported(const void* const (&ptrs)[6], int d) {
  for (const void* p : ptrs)
    if (!aligned16(p)) return false;
  return d >= 16 && d % 16 == 0 && d <= kCvaMaxD;
}

constexpr int kPosThreads = 256;
constexpr int kPosMaxF = 128;
constexpr float kTwoPi = (float)(2.0 * 3.14159265358979323846);

struct PosCfg {
  int N, Q, F;       // N == 0: no views
  int has_bound;
  int64_t total;     // output elements
  float lo[3], span[3];
  float dim_t[kPosMaxF];
};

__global__ void __launch_bounds__(kPosThreads) cape_posemb3d_kernel(PosCfg c, const float* __restrict__ points,
                                                                    const float* __restrict__ rot,
                                                                    const float* __restrict__ trans,
                                                                    float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * kPosThreads + threadIdx.x;
  if (idx >= c.total) return;
  const int W = 3 * c.F;
  const int64_t row = idx / W;  // (b, n, q) or (b, q)
  const int ch = (int)(idx - row * W);
  const int blk = ch / c.F, i = ch - blk * c.F;
  const int axis = blk == 0 ? 1 : (blk == 1 ? 0 : 2);  // the reference's concat (y, x, z)
  const int q = (int)(row % c.Q);
  const int64_t bn = row / c.Q;  // b * N + n with views, b without
  const int64_t b = c.N > 0 ? bn / c.N : bn;
  const float* p = points + (b * c.Q + q) * 3;
  float u[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) u[k] = c.has_bound ? (p[k] * c.span[k]) + c.lo[k] : p[k];
  float x;
  if (c.N > 0) {
    const float* t = trans + bn * 3;
    const float* r = rot + bn * 9 + axis * 3;
    const float w0 = u[0] + t[0], w1 = u[1] + t[1], w2 = u[2] + t[2];
    x = ((r[0] * w0) + (r[1] * w1)) + (r[2] * w2);
  } else {
    x = axis == 0 ? u[0] : (axis == 1 ? u[1] : u[2]);
  }
  const float s = x * kTwoPi;
  const float y = s / c.dim_t[i];
  out[idx] = (i & 1) ? lm::cosf(y) : lm::sinf(y);
}

}  // namespace

extern "C" {

int pd3_cape_cva_forward(const void* q_a, const void* q_g, const void* k_a, const void* k_g, const void* v,
                         const void* mask, const void* scale_a, const void* scale_g, int batch, int num_cams,
                         int num_query, int num_key, int num_heads, int head_dim, void* out, void* stream) {
  if (batch < 0 || num_query < 0 || num_cams < 1 || num_key < 1 || num_heads < 1 || head_dim < 1) return PD3_EINVAL;
  const void* const ptrs[6] = {q_a, q_g, k_a, k_g, v, out};  // the mask and the scales are read element by element
  if (!cva_supported(ptrs, head_dim)) return PD3_EUNSUPPORTED;
  const int64_t BM = (int64_t)batch * num_heads;
  const int64_t blocks = BM * ((num_query + 15) / 16);
  const int64_t tiles = (int64_t)num_cams * ((num_key + 15) / 16);
  if (blocks > 0x7fffffff || BM > 0x7fffffff || tiles > 0x7fffffff - kCvaWaves) return PD3_EUNSUPPORTED;
  if (batch == 0 || num_query == 0) return PD3_OK;
  if (!q_a || !q_g || !k_a || !k_g || !v || !scale_a || !scale_g || !out) return PD3_EINVAL;
  CvaArgs a;
  a.q_a = static_cast<const float*>(q_a), a.q_g = static_cast<const float*>(q_g);
  a.k_a = static_cast<const float*>(k_a), a.k_g = static_cast<const float*>(k_g);
  a.v = static_cast<const float*>(v), a.mask = static_cast<const uint8_t*>(mask);
  a.scale_a = static_cast<const float*>(scale_a), a.scale_g = static_cast<const float*>(scale_g);
  a.out = static_cast<float*>(out);
  a.N = num_cams, a.Q = num_query, a.K = num_key, a.M = num_heads, a.BM = (int)BM;
  const hipStream_t st = (hipStream_t)stream;
#define PD3_CVA_CASE(DT) \
  case DT:               \
    return launch_cva<DT>(a, (unsigned)blocks, st)
  switch (head_dim / 16) {
    PD3_CVA_CASE(1);
    PD3_CVA_CASE(2);
    PD3_CVA_CASE(3);
    PD3_CVA_CASE(4);
    PD3_CVA_CASE(5);
    PD3_CVA_CASE(6);
    PD3_CVA_CASE(7);
    PD3_CVA_CASE(8);
  }
#undef PD3_CVA_CASE
  return PD3_EUNSUPPORTED;
}

int pd3_cape_posemb3d(const void* points, const float* bound, const void* rot, const void* trans, const float* dim_t,
                      int batch, int num_views, int num_query, int num_feats, void* out, void* stream) {
  if (batch < 0 || num_views < 0 || num_query < 0 || num_feats < 1 || !dim_t) return PD3_EINVAL;
  if ((num_views > 0) != (rot != nullptr) || (rot != nullptr) != (trans != nullptr)) return PD3_EINVAL;
  if (num_feats % 2 != 0 || num_feats > kPosMaxF) return PD3_EUNSUPPORTED;
  PosCfg c;
  c.N = num_views, c.Q = num_query, c.F = num_feats, c.has_bound = bound ? 1 : 0;
  c.total = (int64_t)batch * (num_views > 0 ? num_views : 1) * num_query * 3 * num_feats;
  const int64_t blocks = (c.total + kPosThreads - 1) / kPosThreads;
  if (blocks > 0x7fffffff) return PD3_EUNSUPPORTED;
  if (c.total == 0) return PD3_OK;
  if (!points || !out) return PD3_EINVAL;
  for (int k = 0; k < 3; ++k) {
    c.lo[k] = bound ? bound[k] : 0.0f;
    c.span[k] = bound ? bound[k + 3] - bound[k] : 1.0f;
  }
  for (int i = 0; i < kPosMaxF; ++i) c.dim_t[i] = i < num_feats ? dim_t[i] : 1.0f;
  hipLaunchKernelGGL(cape_posemb3d_kernel, dim3((unsigned)blocks), dim3(kPosThreads), 0, (hipStream_t)stream, c,
                     static_cast<const float*>(points), static_cast<const float*>(rot),
                     static_cast<const float*>(trans), static_cast<float*>(out));
  return pd3::launch_status();
}

}  // extern "C"
