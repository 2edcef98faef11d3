// Voxel R-CNN's RoI grid pool on the device: the inner part of NeighborVoxelSAModuleMSG.forward
// (models/common/pointnet2_stack/voxel_pool_modules.py:123-155) for one scale as one kernel, from the voxel query to
// the pool over nsample, with no [M, *, nsample] tensor in global memory.
//
//   pooled[m, c] = pool_s relu(features_in[idx[m, s], c] + (pos_scale[c] * ((w[c,0] * dx + w[c,1] * dy) + w[c,2] * dz)
//                                                             + pos_shift[c]))
//
// idx is pd3_voxel_query's row (csrc/pointnet2_stack.hip: (dz, dy, dx) order, !(d2 > r2), unused slots repeat the
// first hit), d = xyz[idx] - new_xyz, and a row without a hit has features = 0 and d = 0 in all nsample slots (the
// reference's two `[empty_ball_mask] = 0`).  relu(v) = v > 0 ? v : +0, a NaN stays a NaN.
//
// One wave per query.  Query phase: as voxel_query_kernel, 64 window cells per step, __ballot + mbcnt place the hits;
// a hit lane has the voxel's centre in registers, so it leaves the row and d in the wave's 1 KB of LDS and the
// aggregation reads xyz no more.  Aggregation phase: lanes are (sample group g = lane / C1, channel c = lane % C1),
// G = 64 / C1 groups; group g takes the slots s = g, g + G, ... in order, so at C1 = 32 a half-wave reads one 128-byte
// feature row per load and the loads of a lane are independent.  The position weights, scale and shift of the lane's
// channel stay in registers.  Max pool: slots behind the hits repeat slot 0, so the loop ends at the hit count (one
// slot for a row without a hit).  Avg pool: all nsample slots are summed (a repeated slot counts as often as it does
// in the reference), each group in slot order, the groups' sums by the tree (g0 + g1) + (g2 + g3), then one fp32
// division by nsample.  Groups meet by __shfl_xor; lanes of group 0 store the row (C1 * 4 contiguous bytes).
// The wave's LDS is written and read by that wave alone: a wavefront-scope fence and wave barrier order the phases.
//
// No FMA (-ffp-contract=off), no atomics, 64-bit offsets.
//
// The small entry points of the head, one thread per row:
//   roi_grid_points     RoIHeadBase.get_global_grid_points_of_roi + get_dense_grid_points (roi_head_base.py:324-346)
//                       and the coordinate part of VoxelRCNNHead.roi_grid_pool (voxelrcnn_head.py:165-183, 227-230).
//                       Grid point i of a RoI is nonzero()'s (ix, iy, iz) = (i / G^2, i / G % G, i % G);
//                       local = ((idx + 0.5) / G) * size - size / 2; rotate_points_along_z (box_utils.py:17-37) as the
//                       matmul's sums, x' = (x * cos + y * (-sin)) + z * 0, y' = (x * sin + y * cos) + z * 0,
//                       z' = (x * 0 + y * 0) + z * 1; + centre; coords = floor(floor((xyz - min) / voxel) / stride).
//   rcnn_decode_boxes   RoIHeadBase.generate_predicted_boxes (roi_head_base.py:293-322) with
//                       ResidualCoder.decode_paddle (box_coder.py:66-100): decode against the RoI with its centre
//                       zeroed, rotate the centre by the RoI's heading (same sums), add the RoI's centre.
// sinf / cosf / expf carry glibc's bits (libm_exact.hpp), divisions and sqrtf are correctly rounded.
//
// class_agnostic_nms (model_nms_utils.py:20-66) for a whole batch: can_score_kernel (max / argmax over the classes,
// first maximum wins, optional sigmoid per class before the comparison, the >= score_thresh filter, a descending
// sort key and the frame's count), a stable radix sort of the keys (radix_sort.hpp: ties keep index order),
// can_boxes_kernel (the first min(count, nms_pre_maxsize) rows in the NMS kernels' layout, columns as they are),
// the pooled rotated-box bit matrix and sweep of nms_kernels.hpp, can_output_kernel (the first nms_post_maxsize kept
// rows, zeros behind them, the reference's box_empty row for a frame that passes nothing under a threshold).
//
// tests/golden/roi_head_numpy.py restates all of this in the same order; the device results equal it bit for bit.
#include "common.hpp"
#include "head_math.hpp"
#include "libm_exact.hpp"
#include "nms_kernels.hpp"
#include "pointnet2_common.hpp"
#include "radix_sort.hpp"

#include <algorithm>
#include <cmath>

namespace {

using namespace pd3;
using pd3::pn2::ballot_rank;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / pd3::kWave;
constexpr int kMaxSample = 64;  // a row of idx is one wave's lanes

template <int C1>
__global__ __launch_bounds__(kThreads) void voxel_pool_kernel(
    const float* __restrict__ new_xyz, const float* __restrict__ xyz, const int* __restrict__ new_coords,
    const int* __restrict__ point_indices, const float* __restrict__ features_in, const float* __restrict__ w_pos,
    const float* __restrict__ pos_scale, const float* __restrict__ pos_shift, int m, int n, int B, int Z, int Y, int X,
    float r2, int nsample, int zr, int yr, int xr, int pool, float* __restrict__ pooled) {
  static_assert(C1 == 16 || C1 == 32 || C1 == 64, "lanes are (64 / C1 sample groups) x C1 channels");
  constexpr int G = 64 / C1;
  __shared__ int s_idx[kWaves][kMaxSample];
  __shared__ float s_d[kWaves][3][kMaxSample];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t q = (int64_t)blockIdx.x * kWaves + wave;
  if (q >= m) return;  // whole waves leave; no block barrier below
  const float* cq = new_xyz + q * 3;
  const float nx = cq[0], ny = cq[1], nz = cq[2];
  const int* co = new_coords + q * 4;
  const int b = co[0], cz = co[1], cy = co[2], cx = co[3];
  const int c = lane % C1, g = lane / C1;
  const float w0 = w_pos[3 * c], w1 = w_pos[3 * c + 1], w2 = w_pos[3 * c + 2];
  const float sc = pos_scale[c], sh = pos_shift[c];

  // ---- query: the first nsample hits of the window, rows of xyz and their offsets from the query, into LDS
  const int wx = 2 * xr + 1, wyx = (2 * yr + 1) * wx, win = zr < 0 ? 0 : (2 * zr + 1) * wyx;
  int cnt = 0;
  if (b >= 0 && b < B) {
    const int* grid = point_indices + (int64_t)b * Z * Y * X;
    for (int base = 0; base < win && cnt < nsample; base += 64) {
      const int w = base + lane;
      bool hit = false;
      int ni = -1;
      float dx = 0.f, dy = 0.f, dz = 0.f;
      if (w < win) {
        const int64_t z = (int64_t)cz + w / wyx - zr, y = (int64_t)cy + (w % wyx) / wx - yr,
                      x = (int64_t)cx + w % wx - xr;
        if (z >= 0 && z < Z && y >= 0 && y < Y && x >= 0 && x < X) {
          ni = grid[(z * Y + y) * X + x];
          if (ni >= 0 && ni < n) {
            const float* p = xyz + 3 * (int64_t)ni;
            dx = p[0] - nx, dy = p[1] - ny, dz = p[2] - nz;
            hit = !((dx * dx + dy * dy) + dz * dz > r2);  // as voxel_query_kernel
          }
        }
      }
      const uint64_t mask = __ballot(hit);
      if (mask == 0) continue;
      const int pos = cnt + ballot_rank(mask);
      if (hit && pos < nsample) {
        s_idx[wave][pos] = ni;
        s_d[wave][0][pos] = dx;
        s_d[wave][1][pos] = dy;
        s_d[wave][2][pos] = dz;
      }
      cnt += __popcll(mask);
    }
  }
  if (cnt > nsample) cnt = nsample;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  // ---- aggregation: group g over the slots g, g + G, ...; slots behind the hits are slot 0 again
  const int lim = pool == 0 ? (cnt < 1 ? 1 : cnt) : nsample;
  float acc = 0.f;  // every term is >= +0 (or a NaN): 0 is neutral for the max and for the sum
  for (int s = g; s < lim; s += G) {
    float f = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
    if (cnt > 0) {
      const int ss = s < cnt ? s : 0;
      f = features_in[(int64_t)s_idx[wave][ss] * C1 + c];
      dx = s_d[wave][0][ss], dy = s_d[wave][1][ss], dz = s_d[wave][2][ss];
    }
    const float v = relu_keep_nan(f + (sc * ((w0 * dx + w1 * dy) + w2 * dz) + sh));
    if (pool == 0)
      acc = (v > acc || v != v) ? v : acc;
    else
      acc = acc + v;
  }
#pragma unroll
  for (int o = C1; o < 64; o <<= 1) {
    const float other = __shfl_xor(acc, o);
    if (pool == 0)
      acc = (other > acc || other != other) ? other : acc;
    else
      acc = acc + other;
  }
  if (pool != 0) acc = acc / (float)nsample;
  if (g == 0) pooled[q * C1 + c] = acc;
}

// ---- roi_grid_points ------------------------------------------------------------------------------------------------
constexpr int kMaxStrides = 4;

struct GridCfg {
  float lo[3], voxel[3];
  int stride[kMaxStrides];
  int nstrides;
};

// float -> int32 as astype('int32') of an in-range value; out of range saturates, a NaN is 0
__device__ __forceinline__ int to_i32(float f) {
  if (f != f) return 0;
  if (f >= 2147483648.f) return INT32_MAX;
  if (f <= -2147483648.f) return INT32_MIN;
  return (int)f;
}

__global__ __launch_bounds__(256) void roi_grid_points_kernel(const float* __restrict__ rois, int64_t total,
                                                              int rois_per_frame, int G, GridCfg cfg,
                                                              float* __restrict__ grid_xyz, int* __restrict__ coords) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int g3 = G * G * G;
  const int64_t roi = t / g3;
  const int i = (int)(t - roi * g3);
  const float* r = rois + roi * 7;
  const float idx[3] = {(float)(i / (G * G)), (float)(i / G % G), (float)(i % G)};
  float l[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) l[k] = ((idx[k] + 0.5f) / (float)G) * r[3 + k] - r[3 + k] / 2.f;
  const float ca = lm::cosf(r[6]), sa = lm::sinf(r[6]);
  float p[3];
  p[0] = ((l[0] * ca + l[1] * (-sa)) + l[2] * 0.f) + r[0];
  p[1] = ((l[0] * sa + l[1] * ca) + l[2] * 0.f) + r[1];
  p[2] = ((l[0] * 0.f + l[1] * 0.f) + l[2] * 1.f) + r[2];
  float* o = grid_xyz + t * 3;
  o[0] = p[0], o[1] = p[1], o[2] = p[2];
  float c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = floorf((p[k] - cfg.lo[k]) / cfg.voxel[k]);
  const int b = (int)(roi / rois_per_frame);
  for (int s = 0; s < cfg.nstrides; ++s) {
    int* oc = coords + ((int64_t)s * total + t) * 4;
    const float st = (float)cfg.stride[s];
    oc[0] = b;
#pragma unroll
    for (int k = 0; k < 3; ++k) oc[1 + k] = to_i32(floorf(c[k] / st));
  }
}

// ---- rcnn_decode_boxes ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rcnn_decode_kernel(const float* __restrict__ rois,
                                                          const float* __restrict__ box_preds, int64_t n,
                                                          float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const float* a = rois + t * 7;
  const float* e = box_preds + t * 7;
  const float dxa = a[3], dya = a[4], dza = a[5], ra = a[6];
  const float diag = sqrtf(dxa * dxa + dya * dya);
  const float xg = e[0] * diag + 0.f, yg = e[1] * diag + 0.f, zg = e[2] * dza + 0.f;  // the anchor's centre is zeroed
  const float ca = lm::cosf(ra), sa = lm::sinf(ra);
  float* o = out + t * 7;
  o[0] = ((xg * ca + yg * (-sa)) + zg * 0.f) + a[0];
  o[1] = ((xg * sa + yg * ca) + zg * 0.f) + a[1];
  o[2] = ((xg * 0.f + yg * 0.f) + zg * 1.f) + a[2];
  o[3] = lm::expf(e[3]) * dxa;
  o[4] = lm::expf(e[4]) * dya;
  o[5] = lm::expf(e[5]) * dza;
  o[6] = e[6] + ra;
}

// ---- class_agnostic_nms ---------------------------------------------------------------------------------------------
constexpr uint32_t kCanKeyOut = 0xFFFFFFFFu;  // sorts after every kept row (a kept key never has all bits set)

// Descending order as an ascending uint32: -0 and +0 tie, every NaN sorts as the largest value (argsort.hip's key).
__device__ __forceinline__ uint32_t can_key(float score) {
  uint32_t b = __float_as_uint(score);
  if ((b & 0x7FFFFFFFu) == 0u) b = 0u;
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) b = 0x7FC00000u;
  const uint32_t asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ~asc;
}

// grid (ceil(A / 256), B)
__global__ __launch_bounds__(256) void can_score_kernel(const float* __restrict__ cls_preds, int A, int K,
                                                        int apply_sigmoid, float score_thresh,
                                                        float* __restrict__ scores, int* __restrict__ labels,
                                                        uint32_t* __restrict__ keys, int* __restrict__ counts) {
  const int frame = blockIdx.y;
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  int selected = 0;
  if (a < A) {
    const int64_t o = (int64_t)frame * A + a;
    const float* c = cls_preds + o * K;
    float best = 0.f;
    int arg = 0;
    for (int k = 0; k < K; ++k) {
      const float s = apply_sigmoid ? 1.0f / (1.0f + lm::expf(-c[k])) : c[k];
      if (k == 0 || s > best) {
        best = s;
        arg = k;
      }
    }
    scores[o] = best;
    labels[o] = arg;
    selected = score_thresh != score_thresh || best >= score_thresh;  // a NaN threshold is "no threshold"
    keys[o] = selected ? can_key(best) : kCanKeyOut;
  }
  const unsigned long long ball = __ballot(selected);
  __shared__ int wsum[4];
  if (lane_id() == 0) wsum[wave_id()] = __popcll(ball);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int s = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (s) atomicAdd(&counts[frame], s);
  }
}

// grid (ceil(cap / 256), B): the first min(count, cap) rows of the order, columns as they are
__global__ __launch_bounds__(256) void can_boxes_kernel(const float* __restrict__ boxes,
                                                        const uint32_t* __restrict__ sidx,
                                                        const int* __restrict__ counts, int A, int cap,
                                                        BoxPre* __restrict__ pre, float4* __restrict__ xyr) {
  const int frame = blockIdx.y;
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= min(counts[frame], cap)) return;
  const uint32_t a = sidx[(int64_t)frame * A + r];
  const float* bx = boxes + ((int64_t)frame * A + a) * 7;
  const float nb[7] = {bx[0], bx[1], bx[2], bx[3], bx[4], bx[5], bx[6]};
  const BoxPre bp = box_prepare(nb);
  pre[(int64_t)frame * cap + r] = bp;
  xyr[(int64_t)frame * cap + r] = make_float4(bp.cx, bp.cy, bp.rad, 0.f);
}

// grid (B): rows [0, count) in kept order, zeros in [count, post); under a threshold a frame that passed nothing gets
// the reference's box_empty row (zero box, score -1, label -1) in row 0 and count 0
__global__ __launch_bounds__(256) void can_output_kernel(const float* __restrict__ boxes,
                                                         const float* __restrict__ scores,
                                                         const int* __restrict__ labels,
                                                         const int64_t* __restrict__ labels_in,
                                                         const uint32_t* __restrict__ sidx,
                                                         const int* __restrict__ counts,
                                                         const int32_t* __restrict__ keep,
                                                         const int32_t* __restrict__ nkeep, int A, int cap, int post,
                                                         int has_thresh, float* __restrict__ out_boxes,
                                                         float* __restrict__ out_scores,
                                                         int64_t* __restrict__ out_labels,
                                                         int32_t* __restrict__ out_count) {
  const int frame = blockIdx.x;
  out_boxes += (int64_t)frame * post * 7;
  out_scores += (int64_t)frame * post;
  out_labels += (int64_t)frame * post;
  const int passed = counts[frame];
  const int rows = passed > 0 ? min(nkeep[frame], post) : 0;
  for (int r = threadIdx.x; r < post; r += blockDim.x) {
    float* o = out_boxes + (int64_t)r * 7;
    if (r < rows) {
      const uint32_t a = sidx[(int64_t)frame * A + keep[(int64_t)frame * cap + r]];
      const int64_t src = (int64_t)frame * A + a;
#pragma unroll
      for (int k = 0; k < 7; ++k) o[k] = boxes[src * 7 + k];
      out_scores[r] = scores[src];
      out_labels[r] = labels_in ? labels_in[src] : (int64_t)labels[src];
    } else {
      const bool fake = r == 0 && has_thresh && passed == 0;
#pragma unroll
      for (int k = 0; k < 7; ++k) o[k] = 0.f;
      out_scores[r] = fake ? -1.f : 0.f;
      out_labels[r] = fake ? -1 : 0;
    }
  }
  if (threadIdx.x == 0) out_count[frame] = rows;
}

struct CanWorkspace {
  int *counts, *labels, *hist, *partial;
  float* scores;
  uint32_t *keys_a, *vals_a, *keys_b, *vals_b;
  unsigned long long* mask;
  BoxPre* pre;
  NmsPool pool;
  int32_t *keep, *nkeep;
  size_t zero_bytes, bytes;
};

CanWorkspace can_carve(void* base, int batch, int64_t A, int cap, const RadixPlan& plan) {
  Carver c(base);
  CanWorkspace w;
  const size_t ba = (size_t)batch * A, cb = ((size_t)cap + 63) / 64;
  w.counts = c.take<int>((size_t)batch);
  w.pool.counts = c.take<int>((size_t)batch * 2 * kNmsCtrStride);
  w.zero_bytes = c.off;  // counts and the pool's counters: one memset
  w.scores = c.take<float>(ba);
  w.labels = c.take<int>(ba);
  w.keys_a = c.take<uint32_t>(ba);
  w.vals_a = c.take<uint32_t>(ba);
  w.keys_b = c.take<uint32_t>(ba);
  w.vals_b = c.take<uint32_t>(ba);
  w.hist = c.take<int>((size_t)batch * radix_hist_ints(plan));
  w.partial = c.take<int>((size_t)batch * scan_num_tiles((int64_t)radix_hist_ints(plan)));
  w.mask = c.take<unsigned long long>((size_t)batch * cap * cb);
  w.pre = c.take<BoxPre>((size_t)batch * cap);
  w.pool.xyr = c.take<float4>((size_t)batch * cap);
  w.pool.per_set = nms_pool_per_set(cap);
  w.pool.pairs = c.take<uint32_t>((size_t)batch * w.pool.per_set);
  w.pool.tiles = c.take<uint32_t>((size_t)batch * cb * cb);
  w.keep = c.take<int32_t>((size_t)batch * cap);
  w.nkeep = c.take<int32_t>((size_t)batch);
  w.bytes = c.off;
  return w;
}

// 0 when the shape is one the entry point takes
int can_check(int batch, int64_t A, int K, int pre, int post) {
  if (batch < 0 || A < 0 || K < 1 || pre < 1 || post < 1) return PD3_EINVAL;
  if (A >= (int64_t)1 << 30 || (int64_t)batch * A >= (int64_t)1 << 31) return PD3_EUNSUPPORTED;
  if (((int64_t)pre + 63) / 64 > kNmsMaxWords || batch > 65535) return PD3_EUNSUPPORTED;
  return PD3_OK;
}

}  // namespace

extern "C" {

int pd3_roi_grid_points(const float* rois, int64_t num_rois, int rois_per_frame, int grid_size, const float* range_min,
                        const float* voxel_size, const int* strides, int num_strides, float* roi_grid_xyz, int* coords,
                        void* stream) {
  if (num_rois < 0 || rois_per_frame < 1 || grid_size < 1 || num_strides < 0 || !range_min || !voxel_size ||
      (num_strides > 0 && !strides))
    return PD3_EINVAL;
  if (num_strides > kMaxStrides || grid_size > 1024) return PD3_EUNSUPPORTED;
  const int64_t total = num_rois * grid_size * grid_size * grid_size;
  if (total == 0) return PD3_OK;
  if (!rois || !roi_grid_xyz || (num_strides > 0 && !coords)) return PD3_EINVAL;
  const int64_t blocks = pd3::ceil_div(total, 256);
  if (blocks > INT32_MAX) return PD3_EUNSUPPORTED;
  GridCfg cfg;
  for (int k = 0; k < 3; ++k) cfg.lo[k] = range_min[k], cfg.voxel[k] = voxel_size[k];
  cfg.nstrides = num_strides;
  for (int k = 0; k < kMaxStrides; ++k) cfg.stride[k] = k < num_strides ? strides[k] : 1;
  hipLaunchKernelGGL(roi_grid_points_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rois, total,
                     rois_per_frame, grid_size, cfg, roi_grid_xyz, coords);
  return pd3::launch_status();
}

int pd3_rcnn_decode_boxes(const float* rois, const float* box_preds, int64_t n, float* out, void* stream) {
  if (n < 0) return PD3_EINVAL;
  if (n == 0) return PD3_OK;
  if (!rois || !box_preds || !out) return PD3_EINVAL;
  const int64_t blocks = pd3::ceil_div(n, 256);
  if (blocks > INT32_MAX) return PD3_EUNSUPPORTED;
  hipLaunchKernelGGL(rcnn_decode_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rois, box_preds,
                     n, out);
  return pd3::launch_status();
}

size_t pd3_class_agnostic_nms_workspace(int batch, int64_t num_boxes, int nms_pre_maxsize) {
  if (can_check(batch, num_boxes, 1, nms_pre_maxsize, 1) != PD3_OK) return 0;
  return can_carve(nullptr, batch, num_boxes, nms_pre_maxsize, radix_plan(kCanKeyOut, num_boxes)).bytes;
}

int pd3_class_agnostic_nms(const float* box_preds, const float* cls_preds, int batch, int64_t num_boxes,
                           int num_classes, int apply_sigmoid, float score_thresh, const int64_t* labels,
                           int nms_pre_maxsize, float nms_thresh, int nms_post_maxsize, float* out_boxes,
                           float* out_scores, int64_t* out_labels, int32_t* out_count, void* workspace,
                           size_t workspace_bytes, void* stream) {
  const int bad = can_check(batch, num_boxes, num_classes, nms_pre_maxsize, nms_post_maxsize);
  if (bad != PD3_OK) return bad;
  if (batch == 0) return PD3_OK;
  if (!out_boxes || !out_scores || !out_labels || !out_count || !workspace ||
      (num_boxes > 0 && (!box_preds || !cls_preds)))
    return PD3_EINVAL;
  const int64_t a = num_boxes;
  const int cap = nms_pre_maxsize, cb = (cap + 63) / 64;
  const RadixPlan plan = radix_plan(kCanKeyOut, a);
  CanWorkspace w = can_carve(workspace, batch, a, cap, plan);
  if (workspace_bytes < w.bytes) return PD3_EWORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(w.counts, 0, w.zero_bytes, s);
  if (e != hipSuccess) return (int)e;
  const uint32_t* sidx = w.vals_a;
  if (a > 0) {
    can_score_kernel<<<dim3((unsigned)ceil_div(a, 256), batch), 256, 0, s>>>(
        cls_preds, (int)a, num_classes, apply_sigmoid, score_thresh, w.scores, w.labels, w.keys_a, w.counts);
    const int where = enqueue_radix_sort(w.keys_a, w.vals_a, w.keys_b, w.vals_b, a, a, batch, plan,
                                         /*identity_vals=*/true, w.hist, w.partial, s);
    sidx = where ? w.vals_b : w.vals_a;
    can_boxes_kernel<<<dim3((cap + 255) / 256, batch), 256, 0, s>>>(box_preds, sidx, w.counts, (int)a, cap, w.pre,
                                                                    w.pool.xyr);
    nms_enqueue_mask_pooled(w.pre, w.counts, batch, cap, cb, nms_thresh, w.mask, w.pool, s);
    if (const int rc = launch_lds(nms_sweep_kernel, batch, kNmsSweepThreads, nms_sweep_lds(cap), s, w.mask, w.counts, 0, cap,
                                  cb, w.keep, w.nkeep))
      return rc;
  }
  can_output_kernel<<<batch, 256, 0, s>>>(box_preds, w.scores, w.labels, labels, sidx, w.counts, w.keep, w.nkeep,
                                          (int)a, cap, nms_post_maxsize, score_thresh == score_thresh ? 1 : 0,
                                          out_boxes, out_scores, out_labels, out_count);
  return launch_status();
}

int pd3_voxel_pool(const float* new_xyz, const float* xyz, const int* new_coords, const int* point_indices,
                   const float* features_in, const float* w_pos, const float* pos_scale, const float* pos_shift, int m,
                   int n, int batch, int z, int y, int x, int c1, float radius, int nsample, int z_range, int y_range,
                   int x_range, int pool, float* pooled, void* stream) {
  if (m < 0 || n < 0 || batch < 0 || z < 0 || y < 0 || x < 0 || c1 < 1 || nsample < 1 || (pool != 0 && pool != 1))
    return PD3_EINVAL;
  if ((c1 != 16 && c1 != 32 && c1 != 64) || nsample > kMaxSample) return PD3_EUNSUPPORTED;
  if (m == 0) return PD3_OK;
  if (batch == 0 || !new_xyz || !new_coords || !w_pos || !pos_scale || !pos_shift || !pooled ||
      (n > 0 && (!xyz || !features_in)))
    return PD3_EINVAL;
  if ((int64_t)batch * z * y * x > 0 && !point_indices) return PD3_EINVAL;
  const bool empty = z_range < 0 || y_range < 0 || x_range < 0;  // an empty window: every row without a hit
  if (!empty && (2 * (int64_t)z_range + 1) * (2 * (int64_t)y_range + 1) * (2 * (int64_t)x_range + 1) > INT32_MAX - 64)
    return PD3_EUNSUPPORTED;
  if (empty) z_range = y_range = x_range = -1;
  const float r2 = radius * radius;
  const dim3 grid((unsigned)pd3::ceil_div(m, kWaves)), block(kThreads);
  hipStream_t s = (hipStream_t)stream;
#define PD3_VOXEL_POOL(C)                                                                                             \
  hipLaunchKernelGGL(voxel_pool_kernel<C>, grid, block, 0, s, new_xyz, xyz, new_coords, point_indices, features_in,   \
                     w_pos, pos_scale, pos_shift, m, n, batch, z, y, x, r2, nsample, z_range, y_range, x_range, pool, \
                     pooled)
  if (c1 == 16)
    PD3_VOXEL_POOL(16);
  else if (c1 == 32)
    PD3_VOXEL_POOL(32);
  else
    PD3_VOXEL_POOL(64);
#undef PD3_VOXEL_POOL
  return pd3::launch_status();
}

}  // extern "C"
