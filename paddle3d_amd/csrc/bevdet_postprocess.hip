// BEVDet4D CenterHead post-processing for gfx950: decode, Scale-NMS / circle NMS and the merge of all tasks of a
// batch in one launch sequence, every count on the device.
// (reference: CenterHeadMatch.get_bboxes, paddle3d/models/heads/dense_heads/bevdet_centerhead.py:669-783;
//  CenterPointBBoxCoder.decode / _topk :1083-1214; get_task_detections :785-906; _circle_nms :912-921;
//  nms_bev :939-968; rotate_nms_pcdet, paddle3d/models/layers/layer_libs.py:210-249; circle_nms,
//  paddle3d/geometries/bbox.py:450-474.)
//
// A "set" is one (frame, task): set = frame * num_tasks + task.  Launches for the whole batch:
//   1. bd_select_decode_kernel  one 1024-thread workgroup per set: sigmoid keys of all ncls * H * W (class, cell)
//      entries, exact top-max_num selection (block_topk.hpp), decode of the
//      selected entries only, score / centre masks, order-keeping compaction; lays out the NMS input of the set
//   2. nms_cand_kernel + nms_pairs_kernel (nms_kernels.hpp): rotated-IoU bit matrix of the 'rotate' sets, with
//      the set's own nms_thr
//   3. bd_circle_mask_kernel    centre-distance bit matrix of the 'circle' sets, same [set][cap][cb] layout
//   4. nms_sweep_kernel (nms_kernels.hpp): greedy sweep of every set, whichever kernel built its matrix
//   5. bd_merge_kernel          one workgroup per frame: post_max_size cap, post-NMS range mask, dims scaled back,
//      z to the box bottom, label offsets, tasks concatenated in order
//
// Selection.  With the tie rule (equal scores: ascending flat index class * H * W + cell) the coder's two top-K
// passes (per class over H * W, then over ncls * K) are ONE selection over the keys ordered by (score desc, class
// asc, cell asc): entry = (bits(1.0f) - bits(score)) << 32 | flat.  The keys of a set live in a global workspace
// (128 KiB for a 2-class 128 x 128 task, L2-resident), not in LDS, so the map size is bounded only by the flat index
// (H * W <= 2^24, the bound under which the reference's float `ind / W` equals integer division).
// LDS budget of bd_select_decode_kernel (static, no dynamic-LDS attribute, hence no fall-back path to need):
//   histograms 8 replicas x 1024 bins x 4 B = 32 KiB, sorted list 1024 x 8 B = 8 KiB, scan scratch 192 B: ~40.2 KiB
//   of gfx950's 160 KiB per CU.  max_num <= 1024 (the list); larger is PD3_EUNSUPPORTED.
//
// Arithmetic (build flags: -ffp-contract=off, correctly rounded fp32 divide): every decode operation is one
// rounded fp32 operation in the reference's order; sigmoid = 1 / (1 + expf(-x)) and exp / atan2 with glibc's
// bits (libm_exact.hpp), as cp_best_class does; heading of the NMS box -(-rot - P) - P with P = fp32(pi / 2),
// the conversion nms_bev and rotate_nms_pcdet each apply once; Scale-NMS dims d * f for the IoU and (d * f) / f in
// the output; circle distance fp32 with each square rounded, compared with min_radius in double.
#include "../../include/paddle3d_amd.h"
#include "block_topk.hpp"
#include "common.hpp"
#include "nms_kernels.hpp"
#include "radix_sort.hpp"

#include <algorithm>
#include <cstring>

namespace pd3 {

constexpr int kBdMaxTasks = 16;
constexpr int kBdMaxClasses = 64;   // classes of all tasks together (rescale factors)
constexpr uint32_t kBdKeyOne = 0x3F800000u;  // bits of 1.0f
constexpr uint32_t kBdKeyNan = 0x3FFFFFFFu;  // a NaN score sorts after every number
constexpr int kBdKeyBits = 30;
constexpr float kBdHalfPi = 1.57079637050628662109375f;  // fp32(pi / 2)

struct BdHeads {
  const float* hm[kBdMaxTasks];
  const float* reg[kBdMaxTasks];
  const float* height[kBdMaxTasks];
  const float* dim[kBdMaxTasks];
  const float* rot[kBdMaxTasks];
  const float* vel[kBdMaxTasks];
  int ncls[kBdMaxTasks];
  int cls_off[kBdMaxTasks];   // running class count: label offset and first rescale factor of the task
  int circle[kBdMaxTasks];    // nms_type: 0 rotate, 1 circle
  float nms_thr[kBdMaxTasks];
  double min_radius[kBdMaxTasks];
  float factor[kBdMaxClasses];
};

struct BdCfg {
  int hw, feat_w, num_tasks, batch, cap, pre_max, post_max, norm_bbox;
  int64_t key_stride;
  float osf, vx, vy, pcx, pcy, score_threshold;
  float r[6];      // coder post_center_range
  float lim[6];    // test_cfg post_center_limit_range
  int use_lim;
};

struct BdWork {
  uint32_t* keys;          // [sets][key_stride]
  float* boxes;            // [sets][cap][9] decoded, in score order
  float* scores;           // [sets][cap]
  int* labels;             // [sets][cap] task-local class
  int* count;              // [sets] decoded boxes that passed the masks
  int* rot_n;              // [sets] boxes the rotated NMS sees (0 for circle sets)
  int* circ_n;             // [sets] boxes the circle NMS sees (0 for rotate sets)
  int* nms_n;              // [sets] boxes of the sweep
  float* set_thr;          // [sets] nms_thr of the set's task
  double* set_rad;         // [sets] min_radius of the set's task
  float* nms_boxes;        // [sets][cap][7]
  BoxPre* pre;             // [sets][cap]
  NmsPool pool;
  unsigned long long* mask;  // [sets][cap][cb]
  int32_t* keep;           // [sets][cap]
  int32_t* nkeep;          // [sets]
};

__device__ __forceinline__ uint32_t bd_key(float s) {
  const uint32_t bits = __float_as_uint(s);
  return bits <= kBdKeyOne ? kBdKeyOne - bits : kBdKeyNan;  // s in [0, 1]: key in [0, bits(1.0f)]
}

static __global__ __launch_bounds__(kTopkThreads) void bd_select_decode_kernel(BdHeads h, BdCfg c, BdWork w, int sets) {
  __shared__ int hist[kTopkHistWords];
  __shared__ unsigned long long list[kTopkMaxK];
  __shared__ int scr[kTopkScratch];
  const int set = blockIdx.x, t = set % c.num_tasks, frame = set / c.num_tasks;
  const int hw = c.hw, ncls = h.ncls[t], n = ncls * hw;
  const int tid = threadIdx.x;
  uint32_t* keys = w.keys + (int64_t)set * c.key_stride;
  // ---- keys of every (class, cell) entry: the same sigmoid expression as cp_best_class ----------------------------
  {
    const float* hm = h.hm[t] + (int64_t)frame * n;
    for (int i = tid; i < n; i += kTopkThreads) keys[i] = bd_key(1.0f / (1.0f + lm::expf(-hm[i])));
  }
  if (tid == 0) {  // the pool counters of nms_kernels.hpp: no set-up memset
    w.pool.counts[set * kNmsCtrStride] = 0;
    w.pool.counts[(sets + set) * kNmsCtrStride] = 0;
  }
  __syncthreads();
  const int K = min(c.cap, n);
  // ---- selection (block_topk.hpp); the keys are read back by other threads, hence the full barrier above ---------
  const TopkCut cut = n > K ? block_topk_cut(K, kBdKeyBits, hist, scr,
                                             [&](auto f) {
                                               for (int i = tid; i < n; i += kTopkThreads) f(keys[i]);
                                             })
                            : TopkCut{0xFFFFFFFFu, 0};  // > every key: all entries
  block_topk_compact(
      cut, n, [&](int i) { return keys[i]; }, [](int i, int) { return (uint32_t)i; }, list, scr);
  block_topk_sort(list, K);
  // ---- decode of the r-th best entry (decode :1125-1214) ----------------------------------------------------------
  bool keep = false;
  float bx[9] = {};
  float score = 0.f;
  int cls = 0;
  if (tid < K) {
    const unsigned long long e = list[tid];
    const int flat = (int)(uint32_t)e;
    score = __uint_as_float(kBdKeyOne - (uint32_t)(e >> 32));
    if ((uint32_t)(e >> 32) == kBdKeyNan) score = __uint_as_float(0x7FC00000u);
    cls = flat / hw;
    const int cell = flat - cls * hw;
    const int xs = cell % c.feat_w, ys = cell / c.feat_w;
    const float* regp = h.reg[t] + (int64_t)frame * 2 * hw;
    const float* heip = h.height[t] + (int64_t)frame * hw;
    const float* dimp = h.dim[t] + (int64_t)frame * 3 * hw;
    const float* rotp = h.rot[t] + (int64_t)frame * 2 * hw;
    const float* velp = h.vel[t] + (int64_t)frame * 2 * hw;
    const float x = (((float)xs + regp[cell]) * c.osf) * c.vx + c.pcx;
    const float y = (((float)ys + regp[cell + hw]) * c.osf) * c.vy + c.pcy;
    const float z = heip[cell];
    float d[3] = {dimp[cell], dimp[cell + hw], dimp[cell + 2 * hw]};
    if (c.norm_bbox) {
#pragma unroll
      for (int k = 0; k < 3; ++k) d[k] = lm::expf(d[k]);
    }
    const float ang = atan2_rn(rotp[cell], rotp[cell + hw]);
    bx[0] = x, bx[1] = y, bx[2] = z, bx[3] = d[0], bx[4] = d[1], bx[5] = d[2], bx[6] = ang;
    bx[7] = velp[cell], bx[8] = velp[cell + hw];
    keep = x >= c.r[0] && y >= c.r[1] && z >= c.r[2] && x <= c.r[3] && y <= c.r[4] && z <= c.r[5];
    if (c.score_threshold != 0.f) keep = keep && score > c.score_threshold;  // `if self.score_threshold:`
  }
  int total;
  const int pos = block_exclusive_scan<kTopkThreads>(keep ? 1 : 0, scr, total);
  const int64_t row = (int64_t)set * c.cap + pos;
  const bool circle = h.circle[t] != 0;
  if (keep) {
#pragma unroll
    for (int k = 0; k < 9; ++k) w.boxes[row * 9 + k] = bx[k];
    w.scores[row] = score;
    w.labels[row] = cls;
    if (!circle && pos < c.pre_max) {
      // get_task_detections :799-813 (dims * factor), nms_bev :958-961 + rotate_nms_pcdet :222-228 (3 <-> 4 twice,
      // heading converted twice)
      const float f = h.factor[h.cls_off[t] + cls];
      const float th1 = -bx[6] - kBdHalfPi;
      const float nb[7] = {bx[0], bx[1], bx[2], bx[3] * f, bx[4] * f, bx[5] * f, -th1 - kBdHalfPi};
      float* q = w.nms_boxes + row * 7;
#pragma unroll
      for (int k = 0; k < 7; ++k) q[k] = nb[k];
      const BoxPre bp = box_prepare(nb);
      w.pre[row] = bp;
      w.pool.xyr[row] = make_float4(bp.cx, bp.cy, bp.rad, 0.f);
    }
  }
  if (tid == 0) {
    const int nn = circle ? total : min(total, c.pre_max);
    w.count[set] = total;
    w.nms_n[set] = nn;
    w.rot_n[set] = circle ? 0 : nn;
    w.circ_n[set] = circle ? nn : 0;
    w.set_thr[set] = h.nms_thr[t];
    w.set_rad[set] = h.min_radius[t];
  }
}

// Centre-distance suppression bits (circle_nms, bbox.py:463-472): bit (i, j), j > i, when
// (x_i - x_j)^2 + (y_i - y_j)^2 <= thresh, the sum in fp32 with each term rounded, the comparison in double.  Points
// are rows of `pts` (x at +0, y at +1, `row_stride` floats apart), set s at pts + s * cap * row_stride.
// grid (cb, cb, sets), one wave: tile (row block, column block) of the [set][cap][cb] matrix of nms_kernels.hpp.
static __global__ __launch_bounds__(64) void bd_circle_mask_kernel(const float* __restrict__ pts, int row_stride,
                                                                   const int* __restrict__ counts, int n_fixed,
                                                                   int cap, int cb,
                                                                   const double* __restrict__ set_rad, double rad_fixed,
                                                                   unsigned long long* __restrict__ mask) {
  const int set = blockIdx.z;
  const int n = counts ? min(counts[set], cap) : n_fixed;
  const int row_blk = blockIdx.y, col_blk = blockIdx.x;
  if (col_blk < row_blk || row_blk * 64 >= n || col_blk * 64 >= n) return;
  const double thr = set_rad ? set_rad[set] : rad_fixed;
  __shared__ float cx[64], cy[64];
  const int lane = threadIdx.x;
  const float* p = pts + (int64_t)set * cap * row_stride;
  const int col_size = min(n - col_blk * 64, 64), row_size = min(n - row_blk * 64, 64);
  if (lane < col_size) {
    cx[lane] = p[(int64_t)(col_blk * 64 + lane) * row_stride];
    cy[lane] = p[(int64_t)(col_blk * 64 + lane) * row_stride + 1];
  }
  __syncthreads();
  if (lane >= row_size) return;
  const float mx = p[(int64_t)(row_blk * 64 + lane) * row_stride], my = p[(int64_t)(row_blk * 64 + lane) * row_stride + 1];
  unsigned long long bits = 0ull;
  for (int i = row_blk == col_blk ? lane + 1 : 0; i < col_size; ++i) {
    const float dx = mx - cx[i], dy = my - cy[i];
    const float dist = dx * dx + dy * dy;
    if ((double)dist <= thr) bits |= 1ull << i;
  }
  mask[((int64_t)set * cap + row_blk * 64 + lane) * cb + col_blk] = bits;
}

// get_task_detections :871-901 / the circle branch :712-739, then get_bboxes' merge :745-782.  One workgroup per
// frame walks the tasks in order: kept rows up to post_max_size, for rotate tasks the dims scaled back and the
// post_center_limit_range mask, z moved to the box bottom, labels offset by the running class count.  Rows behind
// the frame's count read zero.
static __global__ __launch_bounds__(256) void bd_merge_kernel(BdHeads h, BdCfg c, BdWork w, float* __restrict__ out_b,
                                                              float* __restrict__ out_s, int32_t* __restrict__ out_l,
                                                              int32_t* __restrict__ out_n) {
  __shared__ int scr[8];
  const int frame = blockIdx.x, tid = threadIdx.x;
  const int rows_cap = c.num_tasks * c.post_max;
  out_b += (int64_t)frame * rows_cap * 9;
  out_s += (int64_t)frame * rows_cap;
  out_l += (int64_t)frame * rows_cap;
  int off = 0;
  for (int t = 0; t < c.num_tasks; ++t) {
    const int set = frame * c.num_tasks + t;
    const int nk = min(w.nkeep[set], c.post_max);
    const bool circle = h.circle[t] != 0;
    for (int r0 = 0; r0 < nk; r0 += 256) {
      const int r = r0 + tid;
      bool ok = false;
      float bx[9];
      float sc = 0.f;
      int lb = 0;
      if (r < nk) {
        const int64_t row = (int64_t)set * c.cap + w.keep[(int64_t)set * c.cap + r];
#pragma unroll
        for (int k = 0; k < 9; ++k) bx[k] = w.boxes[row * 9 + k];
        sc = w.scores[row];
        lb = w.labels[row];
        ok = true;
        if (!circle) {
          const float f = h.factor[h.cls_off[t] + lb];
          bx[3] = (bx[3] * f) / f;
          bx[4] = (bx[4] * f) / f;
          bx[5] = (bx[5] * f) / f;
          if (c.use_lim)
            ok = bx[0] >= c.lim[0] && bx[1] >= c.lim[1] && bx[2] >= c.lim[2] && bx[0] <= c.lim[3] &&
                 bx[1] <= c.lim[4] && bx[2] <= c.lim[5];
        }
      }
      int total;
      const int pos = off + block_exclusive_scan<256>(ok ? 1 : 0, scr, total);
      if (ok) {
        bx[2] = bx[2] - bx[5] * 0.5f;
        float* q = out_b + (int64_t)pos * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) q[k] = bx[k];
        out_s[pos] = sc;
        out_l[pos] = lb + h.cls_off[t];
      }
      off += total;
    }
  }
  for (int r = off + tid; r < rows_cap; r += 256) {
#pragma unroll
    for (int k = 0; k < 9; ++k) out_b[(int64_t)r * 9 + k] = 0.f;
    out_s[r] = 0.f;
    out_l[r] = 0;
  }
  if (tid == 0) out_n[frame] = off;
}

static BdWork bd_carve(void* base, int sets, int64_t key_stride, int cap, size_t* bytes) {
  Carver cv(base);
  BdWork w;
  const size_t cb = ((size_t)cap + 63) / 64;
  w.keys = cv.take<uint32_t>((size_t)sets * key_stride);
  w.boxes = cv.take<float>((size_t)sets * cap * 9);
  w.scores = cv.take<float>((size_t)sets * cap);
  w.labels = cv.take<int>((size_t)sets * cap);
  w.count = cv.take<int>((size_t)sets);
  w.rot_n = cv.take<int>((size_t)sets);
  w.circ_n = cv.take<int>((size_t)sets);
  w.nms_n = cv.take<int>((size_t)sets);
  w.set_thr = cv.take<float>((size_t)sets);
  w.set_rad = cv.take<double>((size_t)sets);
  w.nms_boxes = cv.take<float>((size_t)sets * cap * 7);
  w.pre = cv.take<BoxPre>((size_t)sets * cap);
  w.pool.xyr = cv.take<float4>((size_t)sets * cap);
  w.pool.per_set = nms_pool_per_set(cap);
  w.pool.pairs = cv.take<uint32_t>((size_t)sets * w.pool.per_set);
  w.pool.counts = cv.take<int>((size_t)sets * 2 * kNmsCtrStride);
  w.pool.tiles = cv.take<uint32_t>((size_t)sets * cb * cb);
  w.mask = cv.take<unsigned long long>((size_t)sets * cap * cb);
  w.keep = cv.take<int32_t>((size_t)sets * cap);
  w.nkeep = cv.take<int32_t>((size_t)sets);
  *bytes = cv.off;
  return w;
}

// ---------------------------------------------------------------------------------------------------------------------
// standalone circle_nms: descending stable score order by a radix sort, the distance matrix, the sweep, indices back
static __global__ __launch_bounds__(256) void bd_circle_keys_kernel(const float* __restrict__ dets, int n,
                                                                    uint32_t* __restrict__ keys) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t u = __float_as_uint(dets[(int64_t)i * 3 + 2]);
  const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending order of the float
  keys[i] = ~asc;                                                    // ascending key = descending score
}

static __global__ __launch_bounds__(256) void bd_circle_gather_kernel(const float* __restrict__ dets, int n,
                                                                      const uint32_t* __restrict__ order,
                                                                      float* __restrict__ xy) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t j = order[i];
  xy[2 * i] = dets[j * 3];
  xy[2 * i + 1] = dets[j * 3 + 1];
}

static __global__ __launch_bounds__(256) void bd_circle_map_kernel(const int32_t* __restrict__ keep_sorted,
                                                                   const int32_t* __restrict__ num,
                                                                   const uint32_t* __restrict__ order,
                                                                   int32_t* __restrict__ keep) {
  const int nk = num[0];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nk; i += gridDim.x * 256) keep[i] = (int32_t)order[keep_sorted[i]];
}

struct CnWork {
  uint32_t *keys_a, *vals_a, *keys_b, *vals_b;
  int *hist, *partial;
  float* xy;
  unsigned long long* mask;
  int32_t* keep_sorted;
  size_t bytes;
};

static CnWork cn_carve(void* base, int n) {
  const RadixPlan plan = radix_plan(0xFFFFFFFFu, n);
  const size_t cb = ((size_t)n + 63) / 64;
  Carver cv(base);
  CnWork w;
  w.keys_a = cv.take<uint32_t>(n);
  w.vals_a = cv.take<uint32_t>(n);
  w.keys_b = cv.take<uint32_t>(n);
  w.vals_b = cv.take<uint32_t>(n);
  w.hist = cv.take<int>(radix_hist_ints(plan));
  w.partial = cv.take<int>(scan_num_tiles((int64_t)radix_hist_ints(plan)));
  w.xy = cv.take<float>((size_t)n * 2);
  w.mask = cv.take<unsigned long long>((size_t)n * cb);
  w.keep_sorted = cv.take<int32_t>(n);
  w.bytes = cv.off;
  return w;
}

static hipError_t bd_sweep(const unsigned long long* mask, const int* counts, int n_fixed, int sets, int cap, int cb,
                           int32_t* keep, int32_t* nkeep, hipStream_t s) {
  return (hipError_t)launch_lds(nms_sweep_kernel, sets, kNmsSweepThreads, nms_sweep_lds(cap), s, mask, counts, n_fixed, cap,
                                cb, keep, nkeep);
}

}  // namespace pd3

using namespace pd3;

static bool bd_shape_ok(int batch, int num_tasks, const int* task_classes, int feat_h, int feat_w, int64_t* key_stride,
                        int* total_classes) {
  if (batch <= 0 || num_tasks <= 0 || num_tasks > kBdMaxTasks || feat_h <= 0 || feat_w <= 0 || !task_classes)
    return false;
  const int64_t hw = (int64_t)feat_h * feat_w;
  if (hw > (1 << 24)) return false;
  int64_t ks = 0;
  int tc = 0;
  for (int t = 0; t < num_tasks; ++t) {
    if (task_classes[t] <= 0) return false;
    ks = std::max<int64_t>(ks, hw * task_classes[t]);
    tc += task_classes[t];
  }
  if (ks >= ((int64_t)1 << 31) || tc > kBdMaxClasses) return false;
  *key_stride = ks;
  *total_classes = tc;
  return true;
}

extern "C" size_t pd3_bevdet_postprocess_workspace(int batch, int num_tasks, const int* task_classes, int feat_h,
                                                   int feat_w, int max_num) {
  int64_t ks;
  int tc;
  if (!bd_shape_ok(batch, num_tasks, task_classes, feat_h, feat_w, &ks, &tc) || max_num <= 0 || max_num > kTopkMaxK)
    return 0;
  size_t bytes;
  bd_carve(nullptr, batch * num_tasks, ks, max_num, &bytes);
  return bytes;
}

extern "C" int pd3_bevdet_postprocess(
    const float* const* heatmap, const float* const* reg, const float* const* height, const float* const* dim,
    const float* const* rot, const float* const* vel, int batch, int num_tasks, const int* task_classes, int feat_h,
    int feat_w, const int* nms_type, const float* nms_thr, const double* min_radius, const float* rescale_factors,
    int max_num, int pre_max_size, int post_max_size, float score_threshold, int norm_bbox,
    const float* post_center_range, const float* post_center_limit_range, const float* pc_range,
    const float* voxel_size, float out_size_factor, float* out_bboxes, float* out_scores, int32_t* out_labels,
    int32_t* out_count, void* workspace, size_t workspace_bytes, void* stream) {
  if (!heatmap || !reg || !height || !dim || !rot || !vel || !nms_type || !nms_thr || !min_radius ||
      !rescale_factors || !post_center_range || !pc_range || !voxel_size || !out_bboxes || !out_scores ||
      !out_labels || !out_count || !workspace)
    return PD3_EINVAL;
  int64_t ks;
  int tc;
  if (!bd_shape_ok(batch, num_tasks, task_classes, feat_h, feat_w, &ks, &tc)) {
    // maps beyond 2^24 cells (the float `ind / W` of _topk stops being integer division) and more tasks or classes
    // than the kernels hold are not supported; everything else is a bad argument
    if (batch > 0 && num_tasks > 0 && feat_h > 0 && feat_w > 0 && task_classes &&
        ((int64_t)feat_h * feat_w > (1 << 24) || num_tasks > kBdMaxTasks))
      return PD3_EUNSUPPORTED;
    return PD3_EINVAL;
  }
  if (max_num <= 0 || pre_max_size <= 0 || post_max_size <= 0) return PD3_EINVAL;
  if (max_num > feat_h * feat_w) return PD3_EINVAL;  // paddle.topk(k > H * W) raises in the reference
  if (max_num > kTopkMaxK) return PD3_EUNSUPPORTED;
  const int sets = batch * num_tasks, cap = max_num, cb = (cap + 63) / 64;
  size_t need;
  BdWork w = bd_carve(workspace, sets, ks, cap, &need);
  if (workspace_bytes < need) return PD3_EWORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);

  BdHeads h{};
  int off = 0;
  for (int t = 0; t < num_tasks; ++t) {
    if (!heatmap[t] || !reg[t] || !height[t] || !dim[t] || !rot[t] || !vel[t]) return PD3_EINVAL;
    if (nms_type[t] != 0 && nms_type[t] != 1) return PD3_EINVAL;
    h.hm[t] = heatmap[t];
    h.reg[t] = reg[t];
    h.height[t] = height[t];
    h.dim[t] = dim[t];
    h.rot[t] = rot[t];
    h.vel[t] = vel[t];
    h.ncls[t] = task_classes[t];
    h.cls_off[t] = off;
    h.circle[t] = nms_type[t];
    h.nms_thr[t] = nms_thr[t];
    h.min_radius[t] = min_radius[t];
    for (int k = 0; k < task_classes[t]; ++k) {
      h.factor[off + k] = rescale_factors[off + k];
      if (nms_type[t] == 0 && !(rescale_factors[off + k] != 0.f)) return PD3_EINVAL;  // the scale back divides
    }
    off += task_classes[t];
  }
  BdCfg c{};
  c.hw = feat_h * feat_w;
  c.feat_w = feat_w;
  c.num_tasks = num_tasks;
  c.batch = batch;
  c.cap = cap;
  c.pre_max = pre_max_size;
  c.post_max = post_max_size;
  c.norm_bbox = norm_bbox ? 1 : 0;
  c.key_stride = ks;
  c.osf = out_size_factor;
  c.vx = voxel_size[0];
  c.vy = voxel_size[1];
  c.pcx = pc_range[0];
  c.pcy = pc_range[1];
  c.score_threshold = score_threshold;
  for (int k = 0; k < 6; ++k) c.r[k] = post_center_range[k];
  c.use_lim = post_center_limit_range ? 1 : 0;
  for (int k = 0; k < 6 && post_center_limit_range; ++k) c.lim[k] = post_center_limit_range[k];

  bd_select_decode_kernel<<<sets, kTopkThreads, 0, s>>>(h, c, w, sets);
  nms_enqueue_mask_pooled(w.pre, w.rot_n, sets, cap, cb, 0.f, w.mask, w.pool, s, w.set_thr);
  bd_circle_mask_kernel<<<dim3(cb, cb, sets), 64, 0, s>>>(w.boxes, 9, w.circ_n, 0, cap, cb, w.set_rad, 0.0, w.mask);
  const hipError_t e = bd_sweep(w.mask, w.nms_n, 0, sets, cap, cb, w.keep, w.nkeep, s);
  if (e != hipSuccess) return (int)e;
  bd_merge_kernel<<<batch, 256, 0, s>>>(h, c, w, out_bboxes, out_scores, out_labels, out_count);
  return launch_status();
}

extern "C" size_t pd3_circle_nms_workspace(int n) {
  if (n <= 0 || n > kNmsMaxWords * 64) return 0;
  return cn_carve(nullptr, n).bytes;
}

extern "C" int pd3_circle_nms(const float* dets, int n, double thresh, int32_t* keep, int32_t* num_to_keep,
                              void* workspace, size_t workspace_bytes, void* stream) {
  if (!keep || !num_to_keep || n < 0 || (n > 0 && (!dets || !workspace))) return PD3_EINVAL;
  if (n > kNmsMaxWords * 64) return PD3_EUNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n == 0) {
    const hipError_t e = hipMemsetAsync(num_to_keep, 0, sizeof(int32_t), s);
    return e == hipSuccess ? 0 : (int)e;
  }
  CnWork w = cn_carve(workspace, n);
  if (workspace_bytes < w.bytes) return PD3_EWORKSPACE;
  const int cb = (n + 63) / 64;
  const int blocks = (n + 255) / 256;
  bd_circle_keys_kernel<<<blocks, 256, 0, s>>>(dets, n, w.keys_a);
  const int where = enqueue_radix_sort(w.keys_a, w.vals_a, w.keys_b, w.vals_b, n, n, 1, radix_plan(0xFFFFFFFFu, n),
                                       /*identity_vals=*/true, w.hist, w.partial, s);
  const uint32_t* order = where ? w.vals_b : w.vals_a;
  bd_circle_gather_kernel<<<blocks, 256, 0, s>>>(dets, n, order, w.xy);
  bd_circle_mask_kernel<<<dim3(cb, cb, 1), 64, 0, s>>>(w.xy, 2, nullptr, n, n, cb, nullptr, thresh, w.mask);
  const hipError_t e = bd_sweep(w.mask, nullptr, n, 1, n, cb, w.keep_sorted, num_to_keep, s);
  if (e != hipSuccess) return (int)e;
  bd_circle_map_kernel<<<std::min(blocks, 64), 256, 0, s>>>(w.keep_sorted, num_to_keep, order, keep);
  return launch_status();
}
