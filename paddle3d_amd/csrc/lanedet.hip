// BEV-LaneDet's lane head tail and lane post-processing at inference for gfx950: the four final 3x3 convolutions of
// InstanceEmbeddingOffsetYZ (seg densely, emb / offset / z LAZILY at the selected pixels), the ordered selection, the
// online clustering, the canvas, the per-row lane points and the cubic fit of a whole batch, every count on the device.
// (reference: paddle3d/models/detection/bev_lanedet/bev_lanedet.py:50-108, :419-430, paddle3d/datasets/apollo/
//  cluster.py:44-140, post_process.py:26-75, apollo_lane_metric.py:355-383.)
//
// The reference saves four maps per frame and makes the lanes later on the host, by nested Python loops over every BEV
// pixel.  pd3_lanedet_post_process does that work from the same maps; pd3_lanedet_head_forward starts one layer
// earlier and evaluates three of the four final convolutions at the selected pixels only.
//
// Arithmetic order (fp32 unless said, every operation rounded on its own, -ffp-contract=off;
// tests/golden/lanedet_numpy.py restates it):
//   conv3x3(row)   acc = +0; for c ascending, ky = 0..2, kx = 0..2: acc = fmaf(v, w[row][c][ky][kx], acc) with
//                  v = feat[c][y + ky - 1][x + kx - 1] inside the map and +0 outside (the dense convolution's zero
//                  padding, tap for tap); then acc + bias[row]
//   sigmoid        1 / (1 + expf(-x)), expf with glibc's bits (libm_exact.hpp): the offset only; seg stays a logit
//   selection      the pixels with seg >= conf (conf rounded to fp32; a NaN is not selected) in row-major order per frame
//   distance       nd == 1: |e - c|; nd > 1: sqrtf(((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3), d = e - c, channel order
//   clustering     per selected pixel in order: best = gap + 1 (fp32), id = none; for centre ids ascending:
//                  d < best -> (best, id) = (d, centre) (strict: the lowest id wins a tie, a NaN distance never wins);
//                  best < gap: the pixel joins, c = (c * (float)num + e) / (float)(num + 1) per channel, num += 1;
//                  else it founds centre number `centres` with c = e, num = 1.  A 129th centre sets flag bit 0.
//   canvas         id + 1 on the pixels of the centres with num >= min_cluster_size; more than 32 such centres set flag
//                  bit 1 (a DEFINITION: the cap counts canvas ids, before lanes with fewer than 2 rows are dropped)
//   rows           per (canvas id, row y with pixels of it), x ascending, in double: col = sum((double)x + (double)off)
//                  / n, zr = (float)(sum((double)z) / n) -- one rounding each
//   points         rows of a lane from the largest y down (the reference's reversal), in double:
//                  xm = (max_x / mx - ((double)y + 0.5)) * mx, ym = (col * my - (w / 2.0) * my) * -1.0;
//                  (float)xm, (float)ym, zr; lanes with fewer than 2 rows are dropped
//   fit            lanes with >= 4 rows, in double: Y = xm, X = -ym, Z = (double)zr; Ymin = Y of the first point, Ymax = Y
//                  of the last; mid = (Ymin + Ymax) / 2, half = (Ymax - Ymin) / 2; t = (Y - mid) / half; powers
//                  p1 = t, p(k+1) = p(k) * t up to p6; S[k] += p(k) (S[0] += 1), bx[k] += p(k) * X, bz[k] += p(k) * Z
//                  (k = 0..3, p0 * X = X) over the points in order; A[i][j] = S[i + j]; Cholesky A = L L^T (row by
//                  row: s = A[i][j]; s -= L[i][k] * L[j][k] for k ascending; diagonal sqrt(s), else s / L[j][j]);
//                  forward then backward substitution in the same form; samples k = 0..39: Yk = Ymin + k * ((Ymax -
//                  Ymin) / 39), Y39 = Ymax; tk = (Yk - mid) / half; Horner ((c3 * tk + c2) * tk + c1) * tk + c0; each
//                  of X, Yk, Z rounded to fp32 once.  half <= 0 or a non-positive pivot: fit_ok = 0.  Lanes with 2 or 3
//                  rows have fit_ok = 0 (the reference's polyfit is rank deficient there; the host finishes them).
// Nothing depends on the frame's place in the batch, on the grid or on the stream.
//
// Launches:
//   a. lane_seg_kernel / lane_flag_kernel   one pixel per thread: the seg convolution (lazy) or a read; flag = seg >= conf
//   b. scan.hpp's three launches            the ordered compaction: pixel list, selected-pixel count per frame
//   c. lane_gather_kernel                   thread = (selected pixel, output): emb, offset, z by convolution or by read
//   d. lane_cluster_kernel                  ONE wave64 per frame: centres in registers (2 per lane), distances by every
//                                           lane, the wave minimum by DPP and the lowest id by a ballot; 64 embeddings
//                                           are fetched at a time and handed out by readlane: no LDS, no barrier and no
//                                           memory latency in the chain
//   e. lane_lanes_kernel                    one workgroup per frame: canvas, row means (a thread per canvas id and
//                                           row), point numbers (a wave per canvas id, ballots), points, fit (a thread
//                                           per lane over its compacted operands)
// No atomics, no host synchronisation, 64-bit offsets.
#include "../../include/paddle3d_amd_lanedet.h"
#include "common.hpp"
#include "head_math.hpp"
#include "libm_exact.hpp"
#include "scan.hpp"

#include <limits.h>

namespace {

using namespace pd3;

constexpr int kMaxCentres = 128, kMaxLanes = 32, kFit = 40, kMaxNd = 4, kMaxC = 128, kMaxH = 1024;
constexpr int kPixThreads = 64, kGatherThreads = 256, kLaneThreads = 1024;
static_assert(kMaxCentres == 2 * kWave && kMaxCentres <= 255, "two centres per lane; the canvas is uint8");

struct LaneShape {
  int B, C, H, W, HW, nd, pitch, min_size, logit;
  int64_t bstride;  // floats between two frames of a branch map
  float conf, gap;
  double max_x, mx, my;
};

struct LaneFeat {  // the lazy form's inputs
  const float *seg, *emb, *off, *z;
  const float *wseg, *bseg, *wemb, *bemb, *woff, *boff, *wz, *bz;
};

struct LaneOut {
  uint8_t* labels;
  int32_t *num_lanes, *lane_id, *lane_rows, *fit_ok, *flags, *nsel;
  float *points, *fit;
};

struct LaneWorkspace {
  int *flag, *partial, *pix, *cid, *cnum, *ncen, *rcnt;
  float *ev, *ov, *zv, *rz;
  double *rcol, *cy, *cx, *cz;
  size_t bytes;
};

LaneWorkspace lane_carve(void* base, const LaneShape& sh) {
  Carver c(base);
  LaneWorkspace w;
  const size_t B = (size_t)sh.B, HW = (size_t)sh.HW;
  w.flag = c.take<int>(B * HW);
  w.partial = c.take<int>(B * scan_num_tiles(sh.HW));
  w.pix = c.take<int>(B * HW);
  w.cid = c.take<int>(B * HW);
  w.cnum = c.take<int>(B * kMaxCentres);
  w.ncen = c.take<int>(B);
  w.ev = c.take<float>(B * HW * kMaxNd);
  w.ov = c.take<float>(B * HW);
  w.zv = c.take<float>(B * HW);
  w.rcol = c.take<double>(B * kMaxLanes * sh.H);
  w.cy = c.take<double>(B * kMaxLanes * sh.H);
  w.cx = c.take<double>(B * kMaxLanes * sh.H);
  w.cz = c.take<double>(B * kMaxLanes * sh.H);
  w.rz = c.take<float>(B * kMaxLanes * sh.H);
  w.rcnt = c.take<int>(B * kMaxLanes * sh.H);
  w.bytes = c.off;
  return w;
}

// the final 3x3 convolution's output `row` at (y, x) of frame-local map `f` (weights [rows][C][3][3])
__device__ __forceinline__ float lane_conv_at(const float* __restrict__ f, const float* __restrict__ w, float bias,
                                              const LaneShape& sh, int y, int x) {
  const int64_t plane = (int64_t)sh.H * sh.pitch;
  float acc = 0.0f;
#pragma unroll 4
  for (int c = 0; c < sh.C; ++c) {  // four channels' taps in flight
    const float* fc = f + (int64_t)c * plane;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int yy = y + ky - 1, xx = x + kx - 1;
        const bool in = yy >= 0 && yy < sh.H && xx >= 0 && xx < sh.W;
        const float v = in ? fc[(int64_t)yy * sh.pitch + xx] : 0.0f;
        acc = fmaf(v, w[c * 9 + ky * 3 + kx], acc);
      }
  }
  return acc + bias;
}

// ---- a. the flags: grid (ceil(HW / 64), B) --------------------------------------------------------------------------
__global__ __launch_bounds__(kPixThreads) void lane_seg_kernel(LaneFeat in, LaneShape sh, int* __restrict__ flag) {
  __shared__ float ws[kMaxC * 9];
  for (int i = threadIdx.x; i < sh.C * 9; i += kPixThreads) ws[i] = in.wseg[i];
  __syncthreads();
  const int b = blockIdx.y, p = blockIdx.x * kPixThreads + threadIdx.x;
  if (p >= sh.HW) return;
  const int y = p / sh.W, x = p - y * sh.W;
  const float s = lane_conv_at(in.seg + (int64_t)b * sh.bstride, ws, in.bseg[0], sh, y, x);
  flag[(int64_t)b * sh.HW + p] = s >= sh.conf ? 1 : 0;
}

__global__ __launch_bounds__(kGatherThreads) void lane_flag_kernel(const float* __restrict__ seg, LaneShape sh,
                                                                   int* __restrict__ flag) {
  const int b = blockIdx.y, p = blockIdx.x * kGatherThreads + threadIdx.x;
  if (p >= sh.HW) return;
  flag[(int64_t)b * sh.HW + p] = seg[(int64_t)b * sh.HW + p] >= sh.conf ? 1 : 0;
}

struct LaneCompact {  // scan.hpp's epilogue: selected pixel number `prefix` of the frame is pixel i
  int* pix;
  int HW;
  __device__ __forceinline__ void operator()(int frame, int64_t i, int v, int prefix, int) const {
    if (v) pix[(int64_t)frame * HW + prefix] = (int)i;
  }
};

// ---- c. emb, offset and z of the selected pixels: grid (ceil(HW * (nd + 2) / 256), B) ----------------------------------
template <bool LAZY>
__global__ __launch_bounds__(kGatherThreads) void lane_gather_kernel(LaneFeat in, LaneShape sh,
                                                                     const int* __restrict__ pix,
                                                                     const int32_t* __restrict__ nsel,
                                                                     float* __restrict__ ev, float* __restrict__ ov,
                                                                     float* __restrict__ zv) {
  __shared__ uint64_t etab[32];
  lm::exp2f_tab_fill(etab);
  __syncthreads();
  const auto tab = [&](int i) { return etab[i]; };
  const int b = blockIdx.y, rows = sh.nd + 2;
  const int64_t e = (int64_t)blockIdx.x * kGatherThreads + threadIdx.x;
  const int n = min(max(nsel[b], 0), sh.HW);
  if (e >= (int64_t)n * rows) return;
  const int i = (int)(e / rows), j = (int)(e - (int64_t)i * rows);
  const int p = min(max(pix[(int64_t)b * sh.HW + i], 0), sh.HW - 1);  // (always inside: the list holds pixel numbers)
  const int y = p / sh.W, x = p - y * sh.W;
  float v;
  if constexpr (LAZY) {
    const int64_t fb = (int64_t)b * sh.bstride;
    if (j < sh.nd)
      v = lane_conv_at(in.emb + fb, in.wemb + (int64_t)j * sh.C * 9, in.bemb[j], sh, y, x);
    else if (j == sh.nd)
      v = sigmoid_exact(lane_conv_at(in.off + fb, in.woff, in.boff[0], sh, y, x), tab);
    else
      v = lane_conv_at(in.z + fb, in.wz, in.bz[0], sh, y, x);
  } else {
    if (j < sh.nd)
      v = in.emb[((int64_t)b * sh.nd + j) * sh.HW + p];
    else if (j == sh.nd) {
      v = in.off[(int64_t)b * sh.HW + p];
      if (sh.logit) v = sigmoid_exact(v, tab);
    } else
      v = in.z[(int64_t)b * sh.HW + p];
  }
  if (j < sh.nd)
    ev[((int64_t)b * sh.HW + i) * kMaxNd + j] = v;  // by selection number: the cluster kernel walks them in order
  else if (j == sh.nd)
    ov[(int64_t)b * sh.HW + p] = v;                  // by pixel: the lanes kernel reads them through the canvas
  else
    zv[(int64_t)b * sh.HW + p] = v;
}

// ---- d. the online clustering: grid (B), one wave64 ------------------------------------------------------------------
template <int ND>
__device__ __forceinline__ float lane_distance(const float* c, const float* e) {
  if constexpr (ND == 1) return fabsf(e[0] - c[0]);
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < ND; ++k) {
    const float d = e[k] - c[k];
    s = k == 0 ? d * d : s + d * d;
  }
  return sqrtf(s);
}

template <int ND>
__device__ __forceinline__ void lane_join(float* c, int& num, const float* e) {
  const float fn = (float)num, fn1 = (float)(num + 1);
#pragma unroll
  for (int k = 0; k < ND; ++k) c[k] = (c[k] * fn + e[k]) / fn1;
  num += 1;
}

// The minimum of one uint32 per lane over the wave, in every lane: four DPP steps leave a row's minimum in each of its 16
// lanes (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror), row_bcast:15 and row_bcast:31 fold the four rows
// into lane 63.  No LDS crossbar (a shuffle is a ds_bpermute) in the per-pixel chain.
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t lane_dpp_min(uint32_t x) {
  return min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, CTRL, ROWS, 0xF, false));
}

__device__ __forceinline__ uint32_t lane_wave_min(uint32_t v) {
  v = lane_dpp_min<0xB1, 0xF>(v);
  v = lane_dpp_min<0x4E, 0xF>(v);
  v = lane_dpp_min<0x141, 0xF>(v);
  v = lane_dpp_min<0x140, 0xF>(v);
  v = lane_dpp_min<0x142, 0xA>(v);  // rows 1 and 3 take lane 15 of the row before (rows 0 and 2 keep their own)
  v = lane_dpp_min<0x143, 0xC>(v);  // rows 2 and 3 take lane 31
  return (uint32_t)__builtin_amdgcn_readlane((int)v, kWave - 1);
}

template <int ND>
__global__ __launch_bounds__(kWave) void lane_cluster_kernel(const float* __restrict__ ev,
                                                             const int32_t* __restrict__ nsel, LaneShape sh,
                                                             int* __restrict__ cid, int* __restrict__ cnum,
                                                             int* __restrict__ ncen, int32_t* __restrict__ flags) {
  constexpr uint32_t kNone = 0xFFFFFFFFu;  // above the bits of every distance that can win (those are < gap + 1)
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = min(max(nsel[b], 0), sh.HW);
  const float* eb = ev + (int64_t)b * sh.HW * kMaxNd;
  int* cb = cid + (int64_t)b * sh.HW;
  float c0[ND], c1[ND], e[ND], mine[ND], ahead[ND];  // centres `lane` and `lane + 64`
#pragma unroll
  for (int k = 0; k < ND; ++k) c0[k] = c1[k] = e[k] = mine[k] = ahead[k] = 0.0f;
  int n0 = 0, n1 = 0, nc = 0;
  bool over = false;
  const float gap = sh.gap, open = sh.gap + 1.0f;
  if (lane < n) {
#pragma unroll
    for (int k = 0; k < ND; ++k) ahead[k] = eb[(int64_t)lane * kMaxNd + k];
  }
  // 64 pixels at a time: lane l holds pixel base + l's embedding, and the next 64 travel while these are placed
  for (int base = 0; base < n && !over; base += kWave) {
#pragma unroll
    for (int k = 0; k < ND; ++k) mine[k] = ahead[k];
    if (base + kWave + lane < n) {
#pragma unroll
      for (int k = 0; k < ND; ++k) ahead[k] = eb[(int64_t)(base + kWave + lane) * kMaxNd + k];
    }
    const int m = min(kWave, n - base);
    int myid = 0;
    for (int j = 0; j < m; ++j) {
#pragma unroll
      for (int k = 0; k < ND; ++k) e[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine[k]), j));
      // a distance that can win is below gap + 1, not a NaN and not negative: its bits order as it does
      const float d0 = lane_distance<ND>(c0, e);
      const uint32_t k0 = (lane < nc && d0 < open) ? __float_as_uint(d0) : kNone;
      uint32_t k1 = kNone;
      if (nc > kWave) {
        const float d1 = lane_distance<ND>(c1, e);
        if (lane + kWave < nc && d1 < open) k1 = __float_as_uint(d1);
      }
      const uint32_t best = lane_wave_min(min(k0, k1));
      int id;
      if (best != kNone && __uint_as_float(best) < gap) {
        // the lowest id among the centres at that distance: ids below 64 first
        const unsigned long long lo = __ballot(k0 == best);
        const bool low = lo != 0;
        const unsigned long long hit = low ? lo : __ballot(k1 == best);
        const int owner = __ffsll(hit) - 1;
        id = low ? owner : owner + kWave;
        if (lane == owner) {
          if (low)
            lane_join<ND>(c0, n0, e);
          else
            lane_join<ND>(c1, n1, e);
        }
      } else {
        if (nc == kMaxCentres) {
          over = true;
          break;
        }
        id = nc;
        if (lane == (nc & (kWave - 1))) {
          if (nc < kWave) {
#pragma unroll
            for (int k = 0; k < ND; ++k) c0[k] = e[k];
            n0 = 1;
          } else {
#pragma unroll
            for (int k = 0; k < ND; ++k) c1[k] = e[k];
            n1 = 1;
          }
        }
        nc += 1;
      }
      if (lane == j) myid = id;
    }
    if (!over && lane < m) cb[base + lane] = myid;
  }
  cnum[(int64_t)b * kMaxCentres + lane] = over ? 0 : n0;
  cnum[(int64_t)b * kMaxCentres + kWave + lane] = over ? 0 : n1;
  if (lane == 0) {
    ncen[b] = over ? 0 : nc;
    flags[b] = over ? 1 : 0;
  }
}

// ---- e. canvas, rows, points and fit: grid (B), 1024 threads ---------------------------------------------------------
// The cubic fits of one lane from its operands in point order (Y = x_m, X = -y_m, Z), `rows` >= 4 of them.
__device__ void lane_fit(const double* __restrict__ opy, const double* __restrict__ opx, const double* __restrict__ opz,
                         int rows, float* __restrict__ fit, int32_t* __restrict__ ok) {
  const double Ymin = opy[0], Ymax = opy[rows - 1];
  const double mid = (Ymin + Ymax) / 2.0, half = (Ymax - Ymin) / 2.0;
  if (!(half > 0.0)) return;
  double S[7], bx[4], bz[4];
  for (int i = 0; i < 7; ++i) S[i] = 0.0;
  for (int i = 0; i < 4; ++i) bx[i] = bz[i] = 0.0;
#pragma unroll 2
  for (int k = 0; k < rows; ++k) {
    const double t = (opy[k] - mid) / half, X = opx[k], Z = opz[k];
    double p[7];
    p[0] = 1.0;
    p[1] = t;
#pragma unroll
    for (int i = 2; i < 7; ++i) p[i] = p[i - 1] * t;
#pragma unroll
    for (int i = 0; i < 7; ++i) S[i] += p[i];
    bx[0] += X;
    bz[0] += Z;
#pragma unroll
    for (int i = 1; i < 4; ++i) {
      bx[i] += p[i] * X;
      bz[i] += p[i] * Z;
    }
  }
  double L[4][4];
  bool spd = true;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j > i) continue;
      double s = S[i + j];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < j) s -= L[i][q] * L[j][q];
      if (i == j) {
        if (!(s > 0.0)) spd = false;
        L[i][i] = sqrt(s);
      } else {
        L[i][j] = s / L[j][j];
      }
    }
  if (!spd) return;
  double cx[4], cz[4];
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    double* c = pass ? cz : cx;
    const double* r = pass ? bz : bx;
    double u[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double s = r[i];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < i) s -= L[i][q] * u[q];
      u[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 3; i >= 0; --i) {
      double s = u[i];
#pragma unroll
      for (int q = 3; q >= 0; --q)
        if (q > i) s -= L[q][i] * c[q];
      c[i] = s / L[i][i];
    }
  }
  const double step = (Ymax - Ymin) / 39.0;
  for (int s = 0; s < kFit; ++s) {
    const double Y = s == kFit - 1 ? Ymax : Ymin + (double)s * step;
    const double t = (Y - mid) / half;
    fit[s * 3 + 0] = (float)(((cx[3] * t + cx[2]) * t + cx[1]) * t + cx[0]);
    fit[s * 3 + 1] = (float)Y;
    fit[s * 3 + 2] = (float)(((cz[3] * t + cz[2]) * t + cz[1]) * t + cz[0]);
  }
  *ok = 1;
}

__global__ __launch_bounds__(kLaneThreads) void lane_lanes_kernel(const int* __restrict__ pix,
                                                                  const int* __restrict__ cid,
                                                                  const int* __restrict__ cnum,
                                                                  const int* __restrict__ ncen,
                                                                  const float* __restrict__ ov,
                                                                  const float* __restrict__ zv, LaneShape sh,
                                                                  double* __restrict__ rcol, double* __restrict__ cyw,
                                                                  double* __restrict__ cxw, double* __restrict__ czw,
                                                                  float* __restrict__ rz,
                                                                  int* __restrict__ rcnt, LaneOut out) {
  __shared__ int smem[kLaneThreads / kWave + 1];
  __shared__ int slot_of[kMaxCentres];
  __shared__ int centre_of[kMaxLanes], nrows[kMaxLanes], lane_of[kMaxLanes];
  const int b = blockIdx.x, t = threadIdx.x;
  int flag = out.flags[b] & 1;
  const int nc = flag ? 0 : min(max(ncen[b], 0), kMaxCentres);
  const int n = flag ? 0 : min(max(out.nsel[b], 0), sh.HW);
  const int q = (t < nc && cnum[(int64_t)b * kMaxCentres + t] >= sh.min_size) ? 1 : 0;
  int total;
  const int r = block_exclusive_scan<kLaneThreads>(q, smem, total);
  if (t < kMaxCentres) slot_of[t] = (q && r < kMaxLanes) ? r : -1;
  if (q && r < kMaxLanes) centre_of[r] = t;
  if (total > kMaxLanes) {
    flag |= 2;
    total = 0;
  }
  // every output element is written: zero first
  uint8_t* lab = out.labels + (int64_t)b * sh.HW;
  float* pts = out.points + (int64_t)b * kMaxLanes * sh.H * 3;
  float* fit = out.fit + (int64_t)b * kMaxLanes * kFit * 3;
  for (int i = t; i < sh.HW; i += kLaneThreads) lab[i] = 0;
  for (int i = t; i < kMaxLanes * sh.H * 3; i += kLaneThreads) pts[i] = 0.0f;
  for (int i = t; i < kMaxLanes * kFit * 3; i += kLaneThreads) fit[i] = 0.0f;
  if (t < kMaxLanes) {
    out.lane_id[b * kMaxLanes + t] = 0;
    out.lane_rows[b * kMaxLanes + t] = 0;
    out.fit_ok[b * kMaxLanes + t] = 0;
  }
  __syncthreads();
  if (flag || total == 0) {  // uniform over the workgroup
    if (t == 0) {
      out.num_lanes[b] = 0;
      out.flags[b] = flag;
    }
    return;
  }
  const int* pb = pix + (int64_t)b * sh.HW;
  const int* cb = cid + (int64_t)b * sh.HW;
  for (int i = t; i < n; i += kLaneThreads) {
    const int c = min(max(cb[i], 0), kMaxCentres - 1), p = min(max(pb[i], 0), sh.HW - 1);
    if (slot_of[c] >= 0) lab[p] = (uint8_t)(c + 1);
  }
  __syncthreads();  // the frame's canvas is in memory
  double* rc = rcol + (int64_t)b * kMaxLanes * sh.H;
  float* rzz = rz + (int64_t)b * kMaxLanes * sh.H;
  int* rn = rcnt + (int64_t)b * kMaxLanes * sh.H;
  const float* ob = ov + (int64_t)b * sh.HW;
  const float* zb = zv + (int64_t)b * sh.HW;
  for (int task = t; task < total * sh.H; task += kLaneThreads) {
    const int s = task / sh.H, y = task - s * sh.H;
    const uint8_t id = (uint8_t)(centre_of[s] + 1);
    double sc = 0.0, sz = 0.0;
    int cnt = 0;
    for (int x = 0; x < sh.W; ++x) {
      const int p = y * sh.W + x;
      if (lab[p] != id) continue;
      sc += (double)x + (double)ob[p];
      sz += (double)zb[p];
      ++cnt;
    }
    rn[task] = cnt;
    rc[task] = cnt ? sc / (double)cnt : 0.0;
    rzz[task] = cnt ? (float)(sz / (double)cnt) : 0.0f;
  }
  __syncthreads();  // the frame's row table is in memory
  // a wave per canvas id: the rows from the largest y down, 64 at a time; a row's place among the present ones is its
  // point number, and its operands (Y = x_m, X = -y_m, Z) go there
  double* cy = cyw + (int64_t)b * kMaxLanes * sh.H;
  double* cx = cxw + (int64_t)b * kMaxLanes * sh.H;
  double* cz = czw + (int64_t)b * kMaxLanes * sh.H;
  const int lane = t & (kWave - 1);
  const double centre = (double)sh.W / 2.0;
  for (int s = t >> 6; s < total; s += kLaneThreads / kWave) {
    int run = 0;
    for (int y0 = sh.H - 1; y0 >= 0; y0 -= kWave) {
      const int y = y0 - lane;
      const bool present = y >= 0 && rn[s * sh.H + y] > 0;
      const unsigned long long bal = __ballot(present);
      if (present) {
        const int k = run + __popcll(bal & ((1ull << lane) - 1ull));
        cy[s * sh.H + k] = (sh.max_x / sh.mx - ((double)y + 0.5)) * sh.mx;
        cx[s * sh.H + k] = -((rc[s * sh.H + y] * sh.my - centre * sh.my) * -1.0);
        cz[s * sh.H + k] = (double)rzz[s * sh.H + y];
      }
      run += __popcll(bal);
    }
    if (lane == 0) nrows[s] = run;
  }
  __syncthreads();
  if (t == 0) {
    int l = 0;
    for (int s = 0; s < total; ++s) lane_of[s] = nrows[s] >= 2 ? l++ : -1;
    out.num_lanes[b] = l;
    out.flags[b] = flag;
  }
  __syncthreads();
  for (int task = t; task < total * sh.H; task += kLaneThreads) {
    const int s = task / sh.H, k = task - s * sh.H, l = lane_of[s];
    if (l < 0 || k >= nrows[s]) continue;
    float* p = pts + ((int64_t)l * sh.H + k) * 3;
    p[0] = (float)cy[task];
    p[1] = (float)(-cx[task]);
    p[2] = (float)cz[task];
  }
  if (t < total && lane_of[t] >= 0) {
    const int l = lane_of[t];
    out.lane_id[b * kMaxLanes + l] = centre_of[t] + 1;
    out.lane_rows[b * kMaxLanes + l] = nrows[t];
    if (nrows[t] >= 4)
      lane_fit(cy + t * sh.H, cx + t * sh.H, cz + t * sh.H, nrows[t], fit + (int64_t)l * kFit * 3,
               out.fit_ok + b * kMaxLanes + l);
  }
}

// PD3_OK with `sh` filled, PD3_EINVAL or PD3_EUNSUPPORTED.  channels < 0: the from-maps form.
int lane_shape(int batch, int channels, int h, int w, int nd, int pitch, int64_t bstride, float conf, float gap,
               int min_size, double max_x, double mx, double my, int logit, LaneShape& sh) {
  if (batch < 0 || h <= 0 || w <= 0 || nd <= 0 || channels == 0 || !(mx > 0.0) || !(my > 0.0)) return PD3_EINVAL;
  if (channels > 0 && (pitch < w || bstride < (int64_t)channels * h * pitch)) return PD3_EINVAL;
  if (nd > kMaxNd || h > kMaxH || (int64_t)h * w > (int64_t)1 << 20 || batch > 65535 || channels > kMaxC ||
      (channels > 0 && (int64_t)channels * h * pitch >= (int64_t)1 << 31))
    return PD3_EUNSUPPORTED;
  sh.B = batch;
  sh.C = channels;
  sh.H = h;
  sh.W = w;
  sh.HW = h * w;
  sh.nd = nd;
  sh.pitch = pitch;
  sh.bstride = bstride;
  sh.min_size = min_size;
  sh.logit = logit;
  sh.conf = conf;
  sh.gap = gap;
  sh.max_x = max_x;
  sh.mx = mx;
  sh.my = my;
  return PD3_OK;
}

template <bool LAZY>
int lane_run(const LaneFeat& in, const LaneShape& sh, const LaneOut& out, void* workspace, size_t workspace_bytes,
             hipStream_t s) {
  const LaneWorkspace w = lane_carve(workspace, sh);
  if (workspace_bytes < w.bytes) return PD3_EWORKSPACE;
  if constexpr (LAZY)
    lane_seg_kernel<<<dim3((sh.HW + kPixThreads - 1) / kPixThreads, sh.B), kPixThreads, 0, s>>>(in, sh, w.flag);
  else
    lane_flag_kernel<<<dim3((sh.HW + kGatherThreads - 1) / kGatherThreads, sh.B), kGatherThreads, 0, s>>>(in.seg, sh,
                                                                                                       w.flag);
  enqueue_exclusive_scan(w.flag, (int64_t)sh.HW, (int64_t)sh.HW, sh.B, w.partial, out.nsel, (int*)nullptr,
                         LoadIdentity{}, LaneCompact{w.pix, sh.HW}, s);
  const int64_t entries = (int64_t)sh.HW * (sh.nd + 2);
  lane_gather_kernel<LAZY><<<dim3((unsigned)ceil_div(entries, kGatherThreads), sh.B), kGatherThreads, 0, s>>>(
      in, sh, w.pix, out.nsel, w.ev, w.ov, w.zv);
  switch (sh.nd) {
    case 1: lane_cluster_kernel<1><<<sh.B, kWave, 0, s>>>(w.ev, out.nsel, sh, w.cid, w.cnum, w.ncen, out.flags); break;
    case 2: lane_cluster_kernel<2><<<sh.B, kWave, 0, s>>>(w.ev, out.nsel, sh, w.cid, w.cnum, w.ncen, out.flags); break;
    case 3: lane_cluster_kernel<3><<<sh.B, kWave, 0, s>>>(w.ev, out.nsel, sh, w.cid, w.cnum, w.ncen, out.flags); break;
    default: lane_cluster_kernel<4><<<sh.B, kWave, 0, s>>>(w.ev, out.nsel, sh, w.cid, w.cnum, w.ncen, out.flags); break;
  }
  lane_lanes_kernel<<<sh.B, kLaneThreads, 0, s>>>(w.pix, w.cid, w.cnum, w.ncen, w.ov, w.zv, sh, w.rcol, w.cy, w.cx, w.cz, w.rz, w.rcnt,
                                                  out);
  return launch_status();
}

bool lane_out(void* labels, void* num_lanes, void* lane_id, void* lane_rows, void* fit_ok, void* points, void* fit,
              void* flags, void* num_selected, LaneOut& o) {
  if (!labels || !num_lanes || !lane_id || !lane_rows || !fit_ok || !points || !fit || !flags || !num_selected)
    return false;
  o = LaneOut{static_cast<uint8_t*>(labels),   static_cast<int32_t*>(num_lanes), static_cast<int32_t*>(lane_id),
              static_cast<int32_t*>(lane_rows), static_cast<int32_t*>(fit_ok),    static_cast<int32_t*>(flags),
              static_cast<int32_t*>(num_selected), static_cast<float*>(points),   static_cast<float*>(fit)};
  return true;
}

}  // namespace

extern "C" size_t pd3_lanedet_workspace(int batch, int h, int w, int nd) {
  LaneShape sh;
  if (batch <= 0 || lane_shape(batch, -1, h, w, nd, w, 0, 0.f, 0.f, 0, 1.0, 1.0, 1.0, 0, sh) != PD3_OK) return 0;
  return lane_carve(nullptr, sh).bytes;
}

extern "C" int pd3_lanedet_post_process(const void* seg, const void* emb, const void* offset, const void* z,
                                        int offset_is_logit, int batch, int h, int w, int nd, float conf,
                                        float emb_margin, int min_cluster_size, double max_x, double meter_per_pixel_x,
                                        double meter_per_pixel_y, void* labels, void* num_lanes, void* lane_id,
                                        void* lane_rows, void* fit_ok, void* points, void* fit, void* flags,
                                        void* num_selected, void* workspace, size_t workspace_bytes, void* stream) {
  LaneShape sh;
  const int st = lane_shape(batch, -1, h, w, nd, w, 0, conf, emb_margin, min_cluster_size, max_x, meter_per_pixel_x,
                            meter_per_pixel_y, offset_is_logit ? 1 : 0, sh);
  if (st != PD3_OK) return st;
  if (batch == 0) return PD3_OK;
  LaneOut out;
  if (!seg || !emb || !offset || !z || !workspace ||
      !lane_out(labels, num_lanes, lane_id, lane_rows, fit_ok, points, fit, flags, num_selected, out))
    return PD3_EINVAL;
  LaneFeat in{};
  in.seg = static_cast<const float*>(seg);
  in.emb = static_cast<const float*>(emb);
  in.off = static_cast<const float*>(offset);
  in.z = static_cast<const float*>(z);
  return lane_run<false>(in, sh, out, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int pd3_lanedet_head_forward(const void* seg_feat, const void* emb_feat, const void* offset_feat,
                                        const void* z_feat, int64_t batch_stride, int pitch, int channels,
                                        const void* seg_weight, const void* seg_bias, const void* emb_weight,
                                        const void* emb_bias, const void* offset_weight, const void* offset_bias,
                                        const void* z_weight, const void* z_bias, int batch, int h, int w, int nd,
                                        float conf, float emb_margin, int min_cluster_size, double max_x,
                                        double meter_per_pixel_x, double meter_per_pixel_y, void* labels,
                                        void* num_lanes, void* lane_id, void* lane_rows, void* fit_ok, void* points,
                                        void* fit, void* flags, void* num_selected, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  if (channels <= 0) return PD3_EINVAL;
  LaneShape sh;
  const int st = lane_shape(batch, channels, h, w, nd, pitch, batch_stride, conf, emb_margin, min_cluster_size, max_x,
                            meter_per_pixel_x, meter_per_pixel_y, 1, sh);
  if (st != PD3_OK) return st;
  if (batch == 0) return PD3_OK;
  LaneOut out;
  if (!seg_feat || !emb_feat || !offset_feat || !z_feat || !seg_weight || !seg_bias || !emb_weight || !emb_bias ||
      !offset_weight || !offset_bias || !z_weight || !z_bias || !workspace ||
      !lane_out(labels, num_lanes, lane_id, lane_rows, fit_ok, points, fit, flags, num_selected, out))
    return PD3_EINVAL;
  const LaneFeat in{static_cast<const float*>(seg_feat),      static_cast<const float*>(emb_feat),
                    static_cast<const float*>(offset_feat),   static_cast<const float*>(z_feat),
                    static_cast<const float*>(seg_weight),    static_cast<const float*>(seg_bias),
                    static_cast<const float*>(emb_weight),    static_cast<const float*>(emb_bias),
                    static_cast<const float*>(offset_weight), static_cast<const float*>(offset_bias),
                    static_cast<const float*>(z_weight),      static_cast<const float*>(z_bias)};
  return lane_run<true>(in, sh, out, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}
