// PointPillarsScatter + the first (strided) convolution of SecondBackbone as ONE kernel from the inverse map to NCHW: the
// span form of the sparse first layer (pillar_conv.hip explains the layer and its three-step form, which stays the general
// path).  The three-step form writes the rulebook (nbr [rows][9], out_cell, cell_row, order), the result rows [rows, C] and
// reads all of them back only to transpose the rows into NCHW: ten launches.  Here a workgroup owns a SPAN = 256
// consecutive output cells of one output row (the tile rows_to_dense_tile_kernel writes) x 64 output channels and does
// everything for it in LDS:
//   index     a thread per cell reads its nine cells of the inverse map; per tap k the span's cells that HAVE the tap are
//             compacted (ballot + prefix, ascending cell order: no atomics) into list[k], their pillar rows into nb[k]
//   multiply  taps in ascending order, a barrier between them; per tap, 32-cell blocks of list[k] x 32-channel blocks are
//             the waves' units.  The accumulators live in the LDS tile [channel][256 + 4]: a unit reads its 32 x 32 block
//             from the tile as the MFMA's C operand, runs the tap's K = 64 (two chunks x two K-steps x six piece
//             products, the order of sp_gemm_rows_x3_kernel) and writes it back.  A cell therefore executes exactly the
//             taps it has (2.5 of nine on a nuScenes canvas; a 32-row block of the gather-GEMM executes the union of its
//             rows' taps, 4.9).
//   output    the tile leaves as 1 KB channel segments: bias + ReLU for the active cells, fill[c] for the others
// Same bytes as the three-step form: a row's accumulator sees the same chain -- +0, then for each tap the row has, in
// ascending order, chunk 0 K-steps 0, 1, chunk 1 K-steps 0, 1, each the six products lo*hi .. hi*hi -- with the same lane
// <-> K assignment (the packed weight is pd3_sparse_pack_weight_bf16x3's).  A tap a row lacks adds exact zeros to a
// non-negative-zero accumulator there and is skipped here; an fp32 value survives the LDS round trip unchanged.
// A wave's A operand (its 32 channels of the tap's weight pieces, 12 KB) goes from the L2 straight into registers, so
// that LDS holds the tile and the index only (79 KB): two workgroups per CU, one in its index or output phase while the
// other multiplies.  The first unit's gathered rows are fetched one tap ahead.  cout = 128 runs as two workgroups per
// span (64 channels each).
// Measured on the way (16 frames, 512 x 512, per launch): weights double-buffered in LDS, one workgroup per CU 378 us;
// this form 260; with sx_split's conversions in pairs 250; the units' waves apart on the SIMDs of a CU's two workgroups
// 261 (kept: no cost); rows two taps ahead 259, a second set of weight registers 276, the next span's inverse-map cells
// fetched behind the output phase 249, each wave its own half of the cells and no barrier between taps 297: a tap of a
// span is one block (29 cells) whose chain -- rows, 220 VALU instructions of cutting, 24 dependent MFMAs, 32 LDS
// accesses of accumulators -- occupies one wave of four, and only a second workgroup fills the gaps.
#include "../../include/paddle3d_amd.h"
#include "common.hpp"

namespace pd3 {

typedef __bf16 ps_b8 __attribute__((ext_vector_type(8)));
typedef float ps_f32x16 __attribute__((ext_vector_type(16)));
typedef float ps_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kPsCells = 256;                   // cells of a span = threads of a workgroup
constexpr int kPsPitch = kPsCells + 4;          // floats per channel line of the tile
constexpr int kPsCh = 64;                       // output channels of a workgroup
constexpr int kPsCin = 64, kPsKC = 32;          // input channels; chunk of the packed weight
constexpr int kPsGrid = 512;                    // workgroups of the persistent grid (two per CU)
constexpr size_t kPsLds = (size_t)kPsCh * kPsPitch * 4 + 9 * kPsCells * 4 + 9 * kPsCells + 64 * 4 + 4 * 8 + 2 * kPsCh * 4;
static_assert(2 * kPsLds <= 160 * 1024, "two workgroups per CU");

struct PcSpanArgs {
  const float* feats;    // [n_in, 64]
  const int32_t* inv;    // [batch, ny, nx]: pillar row or -1
  const __bf16* wpk;     // pd3_sparse_pack_weight_bf16x3 of [9, 64, cout]
  const float *bias, *fill;
  float* out;            // [batch, cout, ho, wo]
  int n_in, batch, ny, nx, ho, wo, cout, relu;
  int spans;             // batch * ho * (wo / 256)
};

// the gathered rows of one unit, as loaded: [chunk][K-step][low / high four of the lane's eight values]
struct PsRows {
  ps_f32x4 v[2][2][2];
  int cell;
  bool live;
};

typedef float ps_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 ps_b2 __attribute__((ext_vector_type(2)));

// x = hi + mid + lo exactly, every piece a bf16 (round to nearest even): sx_split of sparse_conv_x3.hip, two values per
// conversion (v_cvt_pk_bf16_f32 takes two), and a lane without a row zeroes its twelve piece registers, not its 32 values
__device__ __forceinline__ void ps_split(ps_f32x4 lo4, ps_f32x4 hi4, bool live, ps_b8& h, ps_b8& m, ps_b8& l) {
#pragma unroll
  for (int e = 0; e < 8; e += 2) {
    const ps_f32x2 x = e < 4 ? ps_f32x2{lo4[e & 3], lo4[(e & 3) + 1]} : ps_f32x2{hi4[e & 3], hi4[(e & 3) + 1]};
    const ps_b2 a = __builtin_convertvector(x, ps_b2);
    const ps_f32x2 r1 = x - __builtin_convertvector(a, ps_f32x2);
    const ps_b2 b = __builtin_convertvector(r1, ps_b2);
    const ps_f32x2 r2 = r1 - __builtin_convertvector(b, ps_f32x2);
    const ps_b2 c = __builtin_convertvector(r2, ps_b2);
    h[e] = a[0], h[e + 1] = a[1];
    m[e] = b[0], m[e + 1] = b[1];
    l[e] = c[0], l[e + 1] = c[1];
  }
  typedef unsigned ps_u32x4 __attribute__((ext_vector_type(4)));
  const unsigned keep = live ? ~0u : 0u;
  h = __builtin_bit_cast(ps_b8, __builtin_bit_cast(ps_u32x4, h) & keep);
  m = __builtin_bit_cast(ps_b8, __builtin_bit_cast(ps_u32x4, m) & keep);
  l = __builtin_bit_cast(ps_b8, __builtin_bit_cast(ps_u32x4, l) & keep);
}

__global__ __launch_bounds__(kPsCells, 2) void pc_span_x3_kernel(PcSpanArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ps_smem[];
  float* tile = reinterpret_cast<float*>(ps_smem);                              // [64][260]: the accumulators
  int* nb = reinterpret_cast<int*>(tile + kPsCh * kPsPitch);                          // [9][256]: pillar row of (tap, cell)
  uint8_t* list = reinterpret_cast<uint8_t*>(nb + 9 * kPsCells);                // [9][256]: the cells that have tap k
  int* cnt = reinterpret_cast<int*>(list + 9 * kPsCells);                       // [9][4] per wave, [36 + k] per tap
  unsigned long long* act = reinterpret_cast<unsigned long long*>(cnt + 64);    // [4]: the active cells, a bit each
  float* sbias = reinterpret_cast<float*>(act + 4);                             // [64]
  float* sfill = sbias + kPsCh;                                                 // [64]
  const int t = threadIdx.x, lane = lane_id(), wave = wave_id();
  const int l31 = lane & 31, kh = lane >> 5;
  // The wave's first unit (in an SGPR: the units' branches are uniform): channel block wave & 1 of cell block wave >> 1
  // -- of the other cell block in the second half of the grid.  Most taps of a span have one block: two of the four
  // waves multiply.  Two workgroups share a CU, their waves w share a SIMD, and a CU's second workgroup comes from the
  // grid's second half: so the two workgroups' busy waves sit on different SIMDs.
  const int uwave = __builtin_amdgcn_readfirstlane(wave) ^ (((int)blockIdx.x / (kPsGrid / 2)) & 1) * 2;
  const int nh = a.cout / kPsCh, half = blockIdx.x % nh;  // (the grid is a multiple of nh: a workgroup keeps its half)
  const int sp_stride = gridDim.x / nh;
  const int spr = a.wo / kPsCells;
  const int64_t plane = (int64_t)a.ho * a.wo;
  // (no pillar at all: every fetch below is still issued, from a row that exists -- the packed weight -- and zeroed)
  const float* fsrc = a.n_in > 0 ? a.feats : reinterpret_cast<const float*>(a.wpk);

  for (int i = t; i < kPsCh * kPsPitch; i += kPsCells) tile[i] = 0.f;
  if (t < kPsCh) {
    sbias[t] = a.bias ? a.bias[half * kPsCh + t] : 0.f;
    sfill[t] = a.fill[half * kPsCh + t];
  }

  // the nine cells of the inverse map of thread t's output cell of span sp, as loaded (addresses clamped), and which of
  // them lie on the canvas
  auto load_inv = [&](int sp, int (&j)[9], int& valid) {
    const int xs = sp % spr, r = sp / spr;
    const int oy = r % a.ho, b = r / a.ho;
    const int ix0 = 2 * (xs * kPsCells + t) - 1, iy0 = 2 * oy - 1;
    valid = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int iy = iy0 + k / 3, ix = ix0 + k % 3;
      const bool ok = iy >= 0 && iy < a.ny && ix >= 0 && ix < a.nx;
      valid |= ok ? 1 << k : 0;
      const int cy = min(max(iy, 0), a.ny - 1), cx = min(max(ix, 0), a.nx - 1);
      j[k] = a.inv[((int64_t)b * a.ny + cy) * a.nx + cx];
    }
  };

  // The wave's A operand of a tap, straight into registers: lane (m = l31, kh) of channel block i = wave & 1 (a wave's
  // units all have its parity), chunk c, K-step s, piece p reads the 16 bytes [p][channel][s][kh][8] of the packed weight.
  // One set: the next tap's pieces are fetched when the wave's last unit of this tap has multiplied.
  ps_b8 wa[2][2][3];
  auto load_w = [&](int k) {
    const ps_b8* w8 = reinterpret_cast<const ps_b8*>(a.wpk) + (half * kPsCh + (uwave & 1) * 32 + l31) * (kPsKC / 8) + kh;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int sx = 0; sx < 2; ++sx) wa[c][sx][p] = w8[(int64_t)(k * 6 + c * 3 + p) * a.cout * (kPsKC / 8) + sx * 2];
  };
  auto units_of = [&](int k) { return 2 * ((__builtin_amdgcn_readfirstlane(cnt[36 + k]) + 31) >> 5); };
  // the rows of block `blk` of tap k's list: always issued (a lane without a row reads row 0 and is zeroed when it is
  // cut), so that the number of loads in flight is a constant the compiler can wait against
  auto gather = [&](int k, int blk, PsRows& g) {
    const int idx = blk * 32 + l31;
    g.live = idx < cnt[36 + k];
    g.cell = g.live ? (int)list[k * kPsCells + idx] : 0;
    const int j = g.live ? nb[k * kPsCells + g.cell] : 0;
    const ps_f32x4* src = reinterpret_cast<const ps_f32x4*>(fsrc + (int64_t)j * kPsCin + kh * (kPsKC / 2));
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        g.v[c][s][0] = src[c * (kPsKC / 4) + 2 * s];
        g.v[c][s][1] = src[c * (kPsKC / 4) + 2 * s + 1];
      }
  };
  // one unit: block of 32 cells x channel block i of tap k.  D[m = (reg & 3) + 8 (reg >> 2) + 4 kh][n = l31]
  auto unit = [&](const PsRows& g) {
    float* tl = tile + ((uwave & 1) * 32 + 4 * kh) * kPsPitch + g.cell;
    ps_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float v = tl[((r & 3) + 8 * (r >> 2)) * kPsPitch];
      acc[r] = g.live ? v : 0.f;
    }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        ps_b8 b0, b1, b2;
        const ps_b8(&av)[3] = wa[c][s];
        ps_split(g.v[c][s][0], g.v[c][s][1], g.live, b0, b1, b2);
        // the small products first (sp_gemm_rows_x3_kernel's order)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[0], b2, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[2], b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[1], b1, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[0], b1, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[1], b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[0], b0, acc, 0, 0, 0);
      }
    if (g.live) {
#pragma unroll
      for (int r = 0; r < 16; ++r) tl[((r & 3) + 8 * (r >> 2)) * kPsPitch] = acc[r];
    }
  };

  // tap k: `cur` holds the rows of the wave's first unit (in flight since the tap before), `nxt` takes those of tap k + 1
  auto step = [&](int k, PsRows& cur, PsRows& nxt) {
    const int units = units_of(k);
    const bool then = k < 8 && uwave < units_of(k < 8 ? k + 1 : k);  // the wave has a unit in the next tap
    if (k < 8) gather(k + 1, uwave >> 1, nxt);
    // the wave's units uwave, uwave + 4, ...: the first one's rows are here, a tap with more than 64 cells gathers the
    // further ones as they come (into the same registers: a third set would not leave two workgroups per CU)
    if (uwave < units) unit(cur);
#pragma clang loop unroll(disable)
    for (int u = uwave + 4; u < units; u += 4) {
      gather(k, u >> 1, cur);
      unit(cur);
    }
    if (then) load_w(k + 1);
    px_lds_barrier();
  };

  // Trip i of the workgroups takes spans [i G, (i + 1) G), G = workgroups per half; workgroup g takes the one at (g +
  // i rot) % G.  Not g: spans are output rows, a lidar canvas is dense in its middle rows and all but empty at its edges,
  // and with 256 rows and 256 workgroups a workgroup would get the SAME row of every frame -- the middle rows' workgroups
  // all of the work.  Rotated by G / trips per trip a workgroup's rows are spread evenly over the canvas.
  const int g = blockIdx.x / nh, trips = (a.spans + sp_stride - 1) / sp_stride;
  const int rot = max(sp_stride / trips, 1);
  auto span_of = [&](int i) {
    const int sp = i * sp_stride + (g + i * rot) % sp_stride;
    return i < trips && sp < a.spans ? sp : -1;
  };

  for (int trip = 0; trip < trips; ++trip) {
    const int sp = span_of(trip);
    if (sp < 0) continue;  // (the last trip of some workgroups)
    int jn[9], vn;
    load_inv(sp, jn, vn);
    __syncthreads();  // the span before is out of the tile, the index and the bitmap
    int pos[9], mask = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int j = jn[k];
      const bool has = ((vn >> k) & 1) && j >= 0 && j < a.n_in;
      nb[k * kPsCells + t] = has ? j : -1;
      mask |= has ? 1 << k : 0;
      const unsigned long long bal = __ballot(has);
      pos[k] = __popcll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) cnt[k * 4 + wave] = __popcll(bal);
    }
    {
      const unsigned long long bal = __ballot(mask != 0);
      if (lane == 0) act[wave] = bal;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      int base = 0;
#pragma unroll
      for (int w = 0; w < 3; ++w) base += w < wave ? cnt[k * 4 + w] : 0;
      if ((mask >> k) & 1) list[k * kPsCells + base + pos[k]] = (uint8_t)t;
    }
    if (t < 9) cnt[36 + t] = cnt[t * 4] + cnt[t * 4 + 1] + cnt[t * 4 + 2] + cnt[t * 4 + 3];
    const bool any = (act[0] | act[1] | act[2] | act[3]) != 0ull;
    const int xs = sp % spr, r = sp / spr;
    const int oy = r % a.ho, b = r / a.ho;
    __syncthreads();
    if (any) {
      PsRows ra, rb;
      gather(0, uwave >> 1, ra);
      if (uwave < units_of(0)) load_w(0);
#pragma unroll 1
      for (int k = 0; k < 8; k += 2) {
        step(k, ra, rb);
        step(k + 1, rb, ra);
      }
      step(8, ra, rb);
    }
    // the tile leaves (a wave = one channel's 1 KB segment per trip) and is cleared for the next span
    float* o = a.out + ((int64_t)b * a.cout + half * kPsCh) * plane + (int64_t)oy * a.wo + xs * kPsCells;
#pragma unroll 4
    for (int it = 0; it < kPsCh * kPsCells / 4 / kPsCells; ++it) {
      const int e = it * kPsCells + t;
      const int c = e >> 6, p4 = e & 63;
      float* tl = tile + c * kPsPitch + p4 * 4;
      const ps_f32x4 v = *reinterpret_cast<const ps_f32x4*>(tl);
      const unsigned bits = (unsigned)(act[p4 >> 4] >> ((p4 & 15) * 4)) & 15u;
      const float bs = sbias[c], fl = sfill[c];
      ps_f32x4 ov;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float x = v[q];
        if (a.bias) x += bs;
        if (a.relu) x = fmaxf(x, 0.f);
        ov[q] = (bits >> q) & 1u ? x : fl;
      }
      *reinterpret_cast<ps_f32x4*>(o + c * plane + p4 * 4) = ov;
      if (any) *reinterpret_cast<ps_f32x4*>(tl) = ps_f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
}

}  // namespace pd3

using namespace pd3;

extern "C" int pd3_pillar_conv_span_x3(const float* feats, int n_in, const int32_t* inverse_map, int batch, int ny, int nx,
                                       int stride, int cin, int cout, const void* weight_packed, const float* bias,
                                       const float* fill, int relu, float* out, void* stream) {
  if (!inverse_map || !weight_packed || !fill || !out || n_in < 0 || (n_in > 0 && !feats) || batch <= 0 || ny <= 0 ||
      nx <= 0 || cin <= 0 || cout <= 0)
    return PD3_EINVAL;
  if (stride != 2 || cin != kPsCin || (cout != 64 && cout != 128)) return PD3_EUNSUPPORTED;
  const int ho = (ny - 1) / 2 + 1, wo = (nx - 1) / 2 + 1;
  if (wo % kPsCells != 0) return PD3_EUNSUPPORTED;
  const int64_t spans = (int64_t)batch * ho * (wo / kPsCells);
  if (spans >= ((int64_t)1 << 30)) return PD3_EUNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(feats) % 16 != 0 || reinterpret_cast<uintptr_t>(weight_packed) % 16 != 0 ||
      reinterpret_cast<uintptr_t>(out) % 16 != 0)
    return PD3_EINVAL;
  PcSpanArgs a{feats, inverse_map, static_cast<const __bf16*>(weight_packed), bias, fill, out, n_in, batch, ny, nx, ho, wo,
               cout, relu ? 1 : 0, (int)spans};
  const int nh = cout / kPsCh;
  const unsigned grid = (unsigned)(spans < kPsGrid / nh ? spans : kPsGrid / nh) * nh;
  const int rc = launch_lds(pc_span_x3_kernel, grid, kPsCells, kPsLds, static_cast<hipStream_t>(stream), a);
  return rc ? rc : launch_status();
}
