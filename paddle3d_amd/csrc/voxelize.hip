// hard_voxelize for gfx950 -- deterministic, bit-exact with the reference CPU operator
// (reference: paddle3d/ops/voxel/voxelize_op.cc:19-82).
//
// The reference CPU kernel is a sequential scan: voxel ids are handed out in order of each cell's
// FIRST point, every voxel keeps its FIRST max_num_points_in_voxel points in input order, and once
// max_voxels voxels exist, points that would open a new voxel are dropped (:60-64).  Restated as
// order-independent facts:
//   voxel id of a cell  = rank of the cell's minimum point index among all occupied cells,
//                         dropped when rank >= max_voxels;
//   slot of a point     = number of earlier points in the same cell, dropped when >= max points.
// Both follow from ONE stable sort of the points by cell id (radix_sort.hpp): cells become contiguous
// segments whose elements stay in input order.  Pipeline per launch sequence (grid.y = frame):
//   1. cell_key_kernel     point -> uint32 cell key (INVALID = ncells for out-of-range points)
//   2. stable radix sort   (key, point index)
//   3. seg_head_kernel     mark[point] = sorted position if the point is its cell's first, else -1
//   4. exclusive scan of (mark >= 0) in ORIGINAL point order = voxel id; fused epilogue records the
//      segment start of every voxel id < max_voxels
//   5. gather_kernel       voxel-parallel: writes the complete fixed-shape outputs (data AND zero
//                          padding) exactly once, fully coalesced -- no separate memset of `voxels`.
// HBM traffic per frame ~= the algorithmic bytes (points read once, outputs written once); the sort
// scratch (a few MB per frame) lives in L2 / Infinity Cache.
#include "../../include/paddle3d_amd.h"
#include "common.hpp"

#include <mutex>
#include <type_traits>
#include "radix_sort.hpp"
#include "scan.hpp"
#include "voxelize_wave3d.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace pd3 {

struct VoxGrid {
  float min_x, min_y, min_z;
  float size_x, size_y, size_z;
  int gx, gy, gz;
  uint32_t ncells;
};

// floor((p - min) / size) exactly as voxelize_op.cc:37-45 (fp32 subtract, correctly rounded fp32
// divide, floor), then the int conversion.  On the reference's x86 host a NaN / out-of-int-range
// value converts to INT_MIN (cvttss2si "integer indefinite") and is therefore rejected by the
// `coord < 0` test; v_cvt_i32_f32 would saturate / return 0 instead, so reject those explicitly.
__device__ __forceinline__ bool axis_cell(float p, float lo, float size, int extent, int& c) {
  const float q = floorf((p - lo) / size);
  if (!(q >= 0.0f && q < (float)extent)) return false;  // also false for NaN
  c = (int)q;
  return c < extent;
}

// The same for double points (PD_DISPATCH_FLOATING_TYPES, voxelize_op.cc:128, instantiates the CPU kernel for double
// too): `points[i] - range_min` and the division promote the float attributes to double (:37-45 with T = double).
__device__ __forceinline__ bool axis_cell(double p, float lo, float size, int extent, int& c) {
  const double q = floor((p - (double)lo) / (double)size);
  if (!(q >= 0.0 && q < (double)extent)) return false;  // also false for NaN
  c = (int)q;
  return c < extent;
}

template <typename T>
__global__ __launch_bounds__(256) void cell_key_kernel(const T* __restrict__ points,
                                                       const int32_t* __restrict__ num_points,
                                                       int64_t max_points, int dim, VoxGrid g,
                                                       uint32_t* __restrict__ keys) {
  const int frame = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= max_points) return;
  const int64_t n = num_points ? (int64_t)num_points[frame] : max_points;
  uint32_t key = g.ncells;
  if (i < n) {
    const T* p = points + ((int64_t)frame * max_points + i) * dim;
    int cx, cy, cz;
    if (axis_cell(p[0], g.min_x, g.size_x, g.gx, cx) && axis_cell(p[1], g.min_y, g.size_y, g.gy, cy) &&
        axis_cell(p[2], g.min_z, g.size_z, g.gz, cz)) {
      key = ((uint32_t)cz * (uint32_t)g.gy + (uint32_t)cy) * (uint32_t)g.gx + (uint32_t)cx;
    }
  }
  keys[(int64_t)frame * max_points + i] = key;
}

// dynamic_voxelize: the per-point half of voxelization (no per-voxel cap): coors[i] = (z, y, x) cell of point i by
// the same rule as hard_voxelize (voxelize_op.cc:37-45), (-1, -1, -1) if the point falls outside the range.
__global__ __launch_bounds__(256) void dynamic_voxelize_kernel(const float* __restrict__ points, int64_t n,
                                                               int dim, VoxGrid g, int32_t* __restrict__ coors) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* p = points + i * dim;
  int cx = 0, cy = 0, cz = 0;
  const bool in = axis_cell(p[0], g.min_x, g.size_x, g.gx, cx) && axis_cell(p[1], g.min_y, g.size_y, g.gy, cy) &&
                  axis_cell(p[2], g.min_z, g.size_z, g.gz, cz);
  coors[i * 3 + 0] = in ? cz : -1;
  coors[i * 3 + 1] = in ? cy : -1;
  coors[i * 3 + 2] = in ? cx : -1;
}

__global__ __launch_bounds__(256) void seg_head_kernel(const uint32_t* __restrict__ skey,
                                                       const uint32_t* __restrict__ sidx,
                                                       int64_t n, uint32_t ncells,
                                                       int* __restrict__ mark) {
  const int frame = blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t* k = skey + (int64_t)frame * n;
  const uint32_t key = k[j];
  const bool head = key < ncells && (j == 0 || k[j - 1] != key);
  mark[(int64_t)frame * n + sidx[(int64_t)frame * n + j]] = head ? (int)j : -1;
}

// Epilogue of the flag scan: element i (original point order) is a cell's first point iff
// mark[i] >= 0; its exclusive prefix is the voxel id the sequential reference would hand out.
struct EpiVoxelStart {
  const int* mark;
  int* vox_start;
  int64_t n;
  int max_voxels;
  __device__ __forceinline__ void operator()(int frame, int64_t i, int flag, int prefix, int) const {
    if (flag && prefix < max_voxels)
      vox_start[(int64_t)frame * max_voxels + prefix] = mark[(int64_t)frame * n + i];
  }
};

// One thread per output float of `voxels` (coalesced 4-byte lanes over the contiguous [V,P,D] block).
template <typename T>
__global__ __launch_bounds__(256) void gather_voxels_kernel(
    const T* __restrict__ points, const uint32_t* __restrict__ skey,
    const uint32_t* __restrict__ sidx, const int* __restrict__ vox_start,
    const int* __restrict__ totals, int64_t n, int dim, int max_pts, int max_voxels,
    T* __restrict__ voxels) {
  const int frame = blockIdx.y;
  const int64_t per_frame = (int64_t)max_voxels * max_pts * dim;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= per_frame) return;
  const int row = max_pts * dim;
  const int v = (int)(e / row);
  const int r = (int)(e - (int64_t)v * row);
  const int k = r / dim, c = r - k * dim;
  const int nv = min(totals[frame], max_voxels);
  T out = (T)0;
  if (v < nv) {
    const int64_t s = vox_start[(int64_t)frame * max_voxels + v];
    const uint32_t* keyp = skey + (int64_t)frame * n;
    if (s + k < n && keyp[s + k] == keyp[s]) {
      const uint32_t pi = sidx[(int64_t)frame * n + s + k];
      out = points[((int64_t)frame * n + pi) * dim + c];
    }
  }
  voxels[(int64_t)frame * per_frame + e] = out;
}

// One thread per voxel slot: coords (z, y, x), num_points_per_voxel, and num_voxels.
__global__ __launch_bounds__(256) void voxel_meta_kernel(
    const uint32_t* __restrict__ skey, const int* __restrict__ vox_start,
    const int* __restrict__ totals, int64_t n, int max_pts, int max_voxels, VoxGrid g,
    int32_t* __restrict__ coords, int32_t* __restrict__ num_pts, int32_t* __restrict__ num_voxels,
    int32_t* __restrict__ coors4, uint2* __restrict__ vinfo) {
  const int frame = blockIdx.y;
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const int nv = min(totals[frame], max_voxels);
  if (v == 0) num_voxels[frame] = nv;
  if (v >= max_voxels) return;
  int cz = 0, cy = 0, cx = 0, cnt = 0;
  int64_t s = 0;
  if (v < nv) {
    s = vox_start[(int64_t)frame * max_voxels + v];
    const uint32_t* keyp = skey + (int64_t)frame * n;
    const uint32_t key = keyp[s];
    cx = (int)(key % (uint32_t)g.gx);
    const uint32_t t = key / (uint32_t)g.gx;
    cy = (int)(t % (uint32_t)g.gy);
    cz = (int)(t / (uint32_t)g.gy);
    for (int k = 0; k < max_pts; ++k) {
      if (s + k < n && keyp[s + k] == key) ++cnt; else break;
    }
  }
  int32_t* co = coords + ((int64_t)frame * max_voxels + v) * 3;
  co[0] = cz;
  co[1] = cy;
  co[2] = cx;
  num_pts[(int64_t)frame * max_voxels + v] = cnt;
  // (place of the voxel's points in the sorted index list, points kept): what the slot-per-lane row writer of the
  // wave form (vw_rows_kernel) reads -- the sorted index list is its `clist`
  if (vinfo) vinfo[(int64_t)frame * max_voxels + v] = make_uint2((uint32_t)s, (uint32_t)cnt);
  if (coors4) {
    int32_t* c4 = coors4 + ((int64_t)frame * max_voxels + v) * 4;
    c4[0] = v < nv ? frame : -1;
    c4[1] = cz;
    c4[2] = cy;
    c4[3] = cx;
  }
}

static bool make_grid(const float* voxel_size, const float* range, VoxGrid& g) {
  // voxelize_op.cc:97-102: static_cast<int>(round((max - min) / size)) with fp32 operands
  g.min_x = range[0];
  g.min_y = range[1];
  g.min_z = range[2];
  g.size_x = voxel_size[0];
  g.size_y = voxel_size[1];
  g.size_z = voxel_size[2];
  g.gx = (int)std::round((double)((range[3] - range[0]) / voxel_size[0]));
  g.gy = (int)std::round((double)((range[4] - range[1]) / voxel_size[1]));
  g.gz = (int)std::round((double)((range[5] - range[2]) / voxel_size[2]));
  if (g.gx <= 0 || g.gy <= 0 || g.gz <= 0) return false;
  const int64_t cells = (int64_t)g.gx * g.gy * g.gz;
  if (cells >= (int64_t)1 << 31) return false;
  g.ncells = (uint32_t)cells;
  return true;
}

struct VoxWorkspace {
  uint32_t *keys_a, *vals_a, *keys_b, *vals_b;
  int *mark, *vox_start, *hist, *partial, *totals;
  uint2* vinfo;
  size_t bytes;
};

static VoxWorkspace carve(void* base, int batch, int64_t n, int max_voxels, const RadixPlan& plan) {
  Carver c(base);
  VoxWorkspace w;
  const size_t bn = (size_t)batch * n;
  w.keys_a = c.take<uint32_t>(bn);
  w.vals_a = c.take<uint32_t>(bn);
  w.keys_b = c.take<uint32_t>(bn);
  w.vals_b = c.take<uint32_t>(bn);
  w.mark = c.take<int>(bn);
  w.vox_start = c.take<int>((size_t)batch * max_voxels);
  w.hist = c.take<int>((size_t)batch * radix_hist_ints(plan));
  const size_t scan_tiles =
      (size_t)std::max(scan_num_tiles((int64_t)radix_hist_ints(plan)), scan_num_tiles(n));
  w.partial = c.take<int>((size_t)batch * scan_tiles);
  w.totals = c.take<int>((size_t)batch);
  w.vinfo = c.take<uint2>((size_t)batch * max_voxels);
  w.bytes = c.off;
  return w;
}


// ---------------------------------------------------------------------------------------------------
// tiled fast path (voxelize_tiled.hpp)
// ---------------------------------------------------------------------------------------------------
struct VtWorkspace {
  uint32_t *recs, *dir, *cposr, *tilecnt;
  unsigned short* pos16;
  uint32_t* gstart;
  uint2* vinfo;
  float* compact;
  int* totals;
  int64_t stride;  // tiles * kVtTile: per-frame length of the per-point arrays
  int64_t cap;     // per-frame capacity of the compact payload array, in points
  size_t bytes;
};

static VtWorkspace vt_carve(void* base, int batch, int64_t n, int dim, int max_pts, int max_voxels,
                            uint32_t ncells, const VtPlan& p) {
  (void)max_pts;
  (void)ncells;
  Carver c(base);
  VtWorkspace w;
  w.stride = (int64_t)p.tiles * kVtTile;
  w.cap = n;  // every in-range point of a frame at most once
  w.recs = c.take<uint32_t>((size_t)batch * w.stride);
  w.cposr = c.take<uint32_t>((size_t)batch * w.stride);
  w.pos16 = c.take<unsigned short>((size_t)batch * w.stride);
  w.dir = c.take<uint32_t>((size_t)batch * p.tiles * p.groups);
  w.gstart = c.take<uint32_t>((size_t)batch * p.groups * p.cpg);
  w.vinfo = c.take<uint2>((size_t)batch * max_voxels);
  w.tilecnt = c.take<uint32_t>((size_t)batch * p.tiles);
  w.compact = c.take<float>((size_t)batch * w.cap * dim + 4);
  w.totals = c.take<int>((size_t)batch);
  w.bytes = c.off;
  return w;
}

// ---------------------------------------------------------------------------------------------------
// one call of hard_voxelize: what every form works on (validated and completed by vox_check, below the forms)
// ---------------------------------------------------------------------------------------------------
template <typename T>
struct VoxCall {
  const T* points;
  const int32_t* num_points;
  int batch;
  int64_t n;
  int dim;
  VoxGrid g;
  int max_pts, max_voxels;
  T* voxels;  // nullptr: pd3_hard_voxelize_index (no rows are written)
  int32_t *coords, *num_pts, *num_voxels, *coors4;
  void* workspace;
  hipStream_t s;
};

static VtGrid vt_grid(const VoxGrid& g) {
  return VtGrid{g.min_x, g.min_y, g.min_z, g.size_x, g.size_y, g.size_z,
                (float)(1.0 / (double)g.size_x), (float)(1.0 / (double)g.size_y), (float)(1.0 / (double)g.size_z),
                g.gx, g.gy, g.gz, g.ncells};
}

// Units of one [P, D] row for the gather row writers: float4s where the row is a multiple of four floats and `vec4` (the
// voxels tensor lies at a multiple of 16 bytes), else floats -- four times as many, and it is THAT count vt_div's
// x < 2^24 must hold for
static int64_t vox_rowq(int max_pts, int dim, bool vec4) {
  const int64_t row = (int64_t)max_pts * dim;
  return (row % 4 == 0 && vec4) ? row / 4 : row;
}
static bool vox_rows_fit(int max_voxels, int64_t rowq) { return (int64_t)max_voxels * rowq < ((int64_t)1 << 24) - 4096; }
static bool vox_aligned16(const float* voxels) { return reinterpret_cast<uintptr_t>(voxels) % 16 == 0; }

static bool tiled_applicable(const VoxCall<float>& c, VtPlan& plan) {
  plan = vt_plan(c.g.ncells, c.n, c.max_pts);
  return plan.ok && vox_rows_fit(c.max_voxels, vox_rowq(c.max_pts, c.dim, vox_aligned16(c.voxels)));
}

// Launch shape of vt_rows_kernel / vt_rows_gather_kernel<VEC> (VEC = 4 where vec4, else 1)
struct VtRows {
  bool vec4;
  int rowq, units, step_v, step_j;
  unsigned grid;
};
static VtRows vt_rows(const VoxCall<float>& c) {
  VtRows r;
  r.rowq = (int)vox_rowq(c.max_pts, c.dim, vox_aligned16(c.voxels));
  r.vec4 = r.rowq < c.max_pts * c.dim;
  r.units = (int)ceil_div((int64_t)c.max_voxels * r.rowq, kVtRowsThreads * kVtRowsIlp);
  r.step_v = kVtRowsThreads / r.rowq;
  r.step_j = kVtRowsThreads % r.rowq;
  r.grid = (unsigned)(r.units * c.batch);
  return r;
}

// The gather row writer: every row of `voxels` from the points through an index list (any D)
static void write_rows_gather(const VoxCall<float>& c, const uint32_t* clist, int64_t cap, const uint2* vinfo,
                              const int* totals) {
  const VtRows r = vt_rows(c);
  auto* kernel = r.vec4 ? vt_rows_gather_kernel<4> : vt_rows_gather_kernel<1>;
  kernel<<<r.grid, kVtRowsThreads, 0, c.s>>>(c.points, c.n, clist, cap, vinfo, totals, c.batch, r.units, c.max_voxels,
                                             r.rowq, r.step_v, r.step_j, c.dim, c.voxels, c.coords, c.num_pts,
                                             c.num_voxels, c.coors4);
}

// The slot-per-lane row writer (D = 4 / 5, voxel * slot below 2^24): one index load, the point's 16 + 4 bytes, the same
// two streaming stores; a wave writes 64 * D * 4 contiguous bytes
static bool slot_rows_applicable(int dim, int max_pts, int max_voxels) {
  return (dim == 4 || dim == 5) && vox_rows_fit(max_voxels, max_pts);
}
static void write_rows_slots(const VoxCall<float>& c, const uint32_t* clist, int64_t cap, const uint2* vinfo,
                             const int* totals) {
  const int sunits = (int)ceil_div((int64_t)c.max_voxels * c.max_pts, kVwRowsThreads * kVwRowsIlp);
  auto* kernel = c.dim == 4 ? vw_rows_kernel<4> : vw_rows_kernel<5>;
  kernel<<<(unsigned)(sunits * c.batch), kVwRowsThreads, 0, c.s>>>(c.points, c.n, clist, cap, vinfo, totals, c.batch, sunits,
                                                                   c.max_voxels, c.max_pts, c.voxels, c.coords, c.num_pts,
                                                                   c.num_voxels, c.coors4);
}

static int run_tiled(const VoxCall<float>& c, const VtPlan& plan, bool gather) {
  VtWorkspace w = vt_carve(c.workspace, c.batch, c.n, c.dim, c.max_pts, c.max_voxels, c.g.ncells, plan);
  const VtGrid vg = vt_grid(c.g);
  const size_t lds_a = ((size_t)kVtTile + (size_t)kVtRouteWaves * plan.groups + kVtRouteWaves + 2) * 4;
  const size_t lds_b = vt_group_lds(plan.cpg, plan.tiles);
  // the gather form keeps a list of point indices where the default form keeps the payload itself (same places)
  uint32_t* clist = reinterpret_cast<uint32_t*>(w.compact);
  const unsigned tile_grid = (unsigned)(plan.tiles * c.batch);
  vt_route_kernel<<<tile_grid, kVtRouteThreads, lds_a, c.s>>>(c.points, c.num_points, c.n, c.dim, vg, plan.low,
                                                              plan.gbits, plan.tiles, c.batch, c.max_voxels, w.recs,
                                                              w.dir, w.pos16, w.tilecnt, w.vinfo);
  vt_group_kernel<<<(unsigned)(plan.groups * c.batch), kVgThreads, lds_b, c.s>>>(
      w.recs, w.dir, plan.low, plan.gbits, plan.tiles, c.batch, c.max_pts, w.cposr, w.gstart, w.tilecnt,
      gather ? clist : nullptr, w.cap);
  // gather form: only the assign job of the C + D launch runs (the emit job's workgroups are not launched)
  auto* emit = c.dim == 4 ? vt_assign_emit_kernel<4> : (c.dim == 5 ? vt_assign_emit_kernel<5> : vt_assign_emit_kernel<0>);
  emit<<<(gather ? 1 : 2) * tile_grid, kVtRouteThreads, 0, c.s>>>(
      c.points, c.n, c.dim, plan.tiles, c.batch, w.cposr, w.pos16, w.recs, w.dir, plan.low, plan.gbits, w.tilecnt,
      c.max_voxels, vg, w.vinfo, w.totals, c.coords, c.num_pts, c.coors4, w.cap, w.compact);
  if (gather) {
    write_rows_gather(c, clist, w.cap, w.vinfo, w.totals);
    return launch_status();
  }
  const VtRows r = vt_rows(c);
  auto* rows = r.vec4 ? vt_rows_kernel<4> : vt_rows_kernel<1>;
  rows<<<r.grid, kVtRowsThreads, 0, c.s>>>(w.compact, w.cap, w.vinfo, w.totals, c.batch, r.units, c.max_voxels, r.rowq,
                                           r.step_v, r.step_j, c.dim, c.voxels, c.coords, c.num_pts, c.num_voxels,
                                           c.coors4);
  return launch_status();
}

// ---------------------------------------------------------------------------------------------------
// wave form of the tiled path (voxelize_wave.hpp)
// ---------------------------------------------------------------------------------------------------
struct VwWorkspace {
  uint32_t *recs, *dir, *clist;
  uint2 *vinfo, *flist, *fcnt;
  int* totals;
  uint32_t *gregion, *aux;  // 3-D form only
  int64_t cap;
  size_t bytes;
};

// three_d (voxelize_wave3d.hpp): first-point lists sized by the points ([frame][N], in the groups' regions) instead
// of [group][cells per group], + the region starts and the per-record word of the multi-pass groups
static VwWorkspace vw_carve(void* base, int batch, int64_t n, int max_voxels, const VwPlan& p, bool three_d = false) {
  Carver c(base);
  VwWorkspace w;
  w.cap = n;
  w.recs = c.take<uint32_t>((size_t)batch * p.tiles * p.tile);
  w.dir = c.take<uint32_t>((size_t)batch * p.tiles * p.groups);
  w.clist = c.take<uint32_t>((size_t)batch * w.cap + 4);
  w.vinfo = c.take<uint2>((size_t)batch * max_voxels);
  w.totals = c.take<int>((size_t)batch);
  w.flist = c.take<uint2>(three_d ? (size_t)batch * w.cap + 4 : (size_t)batch * p.groups * p.cpg);
  w.fcnt = c.take<uint2>((size_t)batch * vw_pow2_above(p.tiles) * p.groups);
  w.gregion = three_d ? c.take<uint32_t>((size_t)batch * p.groups) : nullptr;
  w.aux = three_d ? c.take<uint32_t>((size_t)batch * w.cap + 4) : nullptr;
  w.bytes = c.off;
  return w;
}

static bool wave3d_applicable(const VoxCall<float>& c, int shape, VwPlan& plan) {
  plan = v3_plan(c.g.ncells, c.n, c.max_pts, c.batch, shape);
  return plan.ok && slot_rows_applicable(c.dim, c.max_pts, c.max_voxels);
}

constexpr int kVwShapes = 5;

static bool wave_applicable(const VoxCall<float>& c, int shape, VwPlan& plan) {
  plan = vw_plan(c.g.ncells, c.n, c.max_pts, c.batch, shape);
  // (D = 4 / 5 rows leave through the slot-per-lane writer whatever the alignment: voxel * slot is what counts there)
  const bool vec4 = vox_aligned16(c.voxels) || c.dim == 4 || c.dim == 5;
  return plan.ok && vox_rows_fit(c.max_voxels, vox_rowq(c.max_pts, c.dim, vec4));
}

// variants of the wave form (bits)
enum : int {
  kVwPriority = 1,    // heavy waves of the group kernel raise their issue priority
  kVwTwoStreams = 2,  // run_wave_split: two half batches on two streams
  kVwCarry = 4,       // measurement: the points' payload carried through the route kernel's LDS slice
};

// index_span / index_list (pd3_hard_voxelize_index): the per-voxel (start, count) words and the index list are left in
// the CALLER's arrays instead of the workspace, and the row writer does not run (voxels == nullptr): what remains of it
// is vw_finish_index_kernel (num_voxels, the padding rows of coords / counts / coors_batched).
__global__ __launch_bounds__(256) void vw_finish_index_kernel(const int* __restrict__ totals, int batch, int max_voxels,
                                                              int32_t* __restrict__ coords, int32_t* __restrict__ num_pts,
                                                              int32_t* __restrict__ num_voxels,
                                                              int32_t* __restrict__ coors4) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)batch * max_voxels) return;
  const int frame = (int)(t / max_voxels), v = (int)(t - (int64_t)frame * max_voxels);
  const int nv = min(totals[frame], max_voxels);
  if (v == 0) num_voxels[frame] = nv;
  if (v >= nv) {
    const VtInt3 z3{0, 0, 0};
    __builtin_memcpy(coords + t * 3, &z3, sizeof(z3));
    num_pts[t] = 0;
    if (coors4) *reinterpret_cast<int4*>(coors4 + t * 4) = make_int4(-1, 0, 0, 0);
  }
}

static int run_wave(const VoxCall<float>& c, const VwPlan& plan, int variant = 0, int frame0 = 0, bool three_d = false,
                    int32_t* index_span = nullptr, int32_t* index_list = nullptr) {
  VwWorkspace w = vw_carve(c.workspace, c.batch, c.n, c.max_voxels, plan, three_d);
  if (index_span) {
    w.vinfo = reinterpret_cast<uint2*>(index_span);
    w.clist = reinterpret_cast<uint32_t*>(index_list);
  }
  VtGrid vg = vt_grid(c.g);
  if (c.g.gz == 1 && !vt_single_cell_bounds(c.g.size_z, vg.z1_lo, vg.z1_hi)) vg.z1_lo = 0.f, vg.z1_hi = -1.f;
  const int waves = plan.threads / kWave;
  const bool pay = (variant & kVwCarry) != 0 && c.voxels != nullptr;
  // up to ~104 KB of dynamic LDS (1024 x 10 tile)
  const size_t lds_a = ((size_t)plan.tile + (size_t)waves * plan.groups + waves + 2) * 4 +
                       (pay ? (size_t)plan.tile * c.dim * 4 : 0);
  const unsigned tile_grid = (unsigned)(plan.tiles * c.batch);
  // (measurement form) the carried payload goes to the head of the `voxels` buffer, which the row writer overwrites
  if (pay && (plan.threads != 512 || plan.rounds != 8 || lds_a > 160 * 1024 ||
              (int64_t)c.batch * plan.tiles * plan.tile * c.dim > (int64_t)c.batch * c.max_voxels * c.max_pts * c.dim))
    return PD3_EUNSUPPORTED;
  auto route = [&](auto kernel) {
    return launch_lds(kernel, tile_grid, plan.threads, lds_a, c.s, c.points, c.num_points, c.n, c.dim, vg, plan.low,
                      plan.gbits, plan.tiles, c.batch, c.max_voxels, w.recs, w.dir, w.vinfo, three_d ? 1 : 0,
                      pay ? c.voxels : nullptr);
  };
  int rc;
  if (pay) rc = route(vw_route_kernel<512, 8, true>);
  else if (plan.threads == 512 && plan.rounds == 8) rc = route(vw_route_kernel<512, 8>);
  else if (plan.threads == 1024 && plan.rounds == 8) rc = route(vw_route_kernel<1024, 8>);
  else if (plan.threads == 1024 && plan.rounds == 10) rc = route(vw_route_kernel<1024, 10>);
  else if (plan.threads == 512 && plan.rounds == 10) rc = route(vw_route_kernel<512, 10>);
  else if (plan.threads == 1024 && plan.rounds == 5) rc = route(vw_route_kernel<1024, 5>);
  else return PD3_EINVAL;
  if (rc != 0) return rc;
  const int tp = vw_pow2_above(plan.tiles);
  if (three_d)
    v3_group_kernel<<<(unsigned)(plan.groups * c.batch), kWave, v3_group_lds(plan.tiles), c.s>>>(
        w.recs, w.dir, plan.gbits, plan.tiles, plan.tile, tp, c.batch, c.max_pts, w.clist, w.cap, w.flist, w.fcnt,
        w.gregion, w.aux);
  else
    vw_group_kernel<<<(unsigned)(plan.groups * c.batch), kWave, vw_group_lds(plan.cpg, plan.tiles), c.s>>>(
        w.recs, w.dir, plan.low, plan.gbits, plan.tiles, plan.tile, tp, c.batch, c.max_pts, w.clist, w.cap, w.flist,
        w.fcnt, (variant & kVwPriority) ? (uint32_t)std::max<int64_t>(c.n / plan.groups, 1) : 0u);
  const size_t lds_c = (size_t)2 * (((size_t)plan.tile + 31) / 32) * 4 + (size_t)kVwAssignCap * 8;
  vw_assign_kernel<<<(unsigned)(plan.tiles * c.batch), kVwAssignThreads, lds_c, c.s>>>(
      w.flist, w.fcnt, plan.low, plan.gbits, plan.tiles, plan.tile, tp, c.batch, c.max_voxels, vg, w.vinfo, w.totals,
      c.coords, c.num_pts, c.coors4, frame0, three_d ? w.gregion : nullptr, w.cap);
  if (index_span)
    vw_finish_index_kernel<<<(unsigned)ceil_div((int64_t)c.batch * c.max_voxels, 256), 256, 0, c.s>>>(
        w.totals, c.batch, c.max_voxels, c.coords, c.num_pts, c.num_voxels, c.coors4);
  else if (c.dim == 4 || c.dim == 5)
    write_rows_slots(c, w.clist, w.cap, w.vinfo, w.totals);
  else
    write_rows_gather(c, w.clist, w.cap, w.vinfo, w.totals);
  return launch_status();
}

// Two half batches on two streams (measurement form, path 12 / 13): the four kernels of a half are a chain of
// differently bound launches (route: instruction + read stream, group / assign: latency, rows: write stream) with an
// idle tail at every boundary; two independent chains let the hardware run one half's latency-bound kernels beside
// the other half's streaming ones.  Fork / join by events on the caller's stream, so the op stays one unit of work
// on that stream (and stays capturable).  Same bytes out: every frame is processed by the same kernels.
static int run_wave_split(const VoxCall<float>& c, const VwPlan& plan, int variant) {
  constexpr int kMaxDev = 16;
  static hipStream_t side[kMaxDev] = {};
  static hipEvent_t fork_ev[kMaxDev] = {}, join_ev[kMaxDev] = {};
  static std::mutex mu;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev || c.batch < 2) return run_wave(c, plan, variant);
  // One side stream and one fork / join event pair per device, shared by every caller: the lock is held from the fork
  // to the join so that two host threads on different streams of one device cannot interleave their records and waits
  // (this is a measurement form; the library's own choice never takes it).
  std::lock_guard<std::mutex> lock(mu);
  if (!side[dev]) {  // the slot counts as initialised only when all three objects exist
    hipStream_t st = nullptr;
    hipEvent_t ef = nullptr, ej = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ef, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ej, hipEventDisableTiming) != hipSuccess) {
      if (ej) (void)hipEventDestroy(ej);
      if (ef) (void)hipEventDestroy(ef);
      if (st) (void)hipStreamDestroy(st);
      return PD3_EINVAL;
    }
    fork_ev[dev] = ef;
    join_ev[dev] = ej;
    side[dev] = st;
  }
  // frames [0, b0) stay on the caller's stream; frames [b0, batch) go to the side stream with a workspace region of
  // their own behind the first half's
  const int b0 = c.batch / 2;
  VoxCall<float> lo = c, hi = c;
  lo.batch = b0;
  hi.batch = c.batch - b0;
  hi.points += (int64_t)b0 * c.n * c.dim;
  if (hi.num_points) hi.num_points += b0;
  hi.voxels += (int64_t)b0 * c.max_voxels * c.max_pts * c.dim;
  hi.coords += (int64_t)b0 * c.max_voxels * 3;
  hi.num_pts += (int64_t)b0 * c.max_voxels;
  hi.num_voxels += b0;
  if (hi.coors4) hi.coors4 += (int64_t)b0 * c.max_voxels * 4;
  hi.workspace = static_cast<char*>(c.workspace) + align_up(vw_carve(nullptr, b0, c.n, c.max_voxels, plan).bytes, 256);
  hi.s = side[dev];
  hipError_t e = hipEventRecord(fork_ev[dev], c.s);
  if (e == hipSuccess) e = hipStreamWaitEvent(side[dev], fork_ev[dev], 0);
  if (e != hipSuccess) return (int)e;
  int rc = run_wave(lo, plan, variant);
  if (rc != 0) return rc;
  rc = run_wave(hi, plan, variant, b0);
  if (rc != 0) return rc;
  e = hipEventRecord(join_ev[dev], side[dev]);
  if (e == hipSuccess) e = hipStreamWaitEvent(c.s, join_ev[dev], 0);
  return e == hipSuccess ? 0 : (int)e;
}

// generic path: stable radix sort of (cell, index), segment heads, flag scan in point order, voxel-parallel gather
template <typename T>
static int run_sort_path(const VoxCall<T>& c) {
  const int64_t n = c.n;
  const RadixPlan plan = radix_plan(c.g.ncells, n);
  VoxWorkspace w = carve(c.workspace, c.batch, n, c.max_voxels, plan);
  hipStream_t s = c.s;

  dim3 pgrid((unsigned)ceil_div(n, 256), c.batch);
  cell_key_kernel<T><<<pgrid, 256, 0, s>>>(c.points, c.num_points, n, c.dim, c.g, w.keys_a);
  const int where = enqueue_radix_sort(w.keys_a, w.vals_a, w.keys_b, w.vals_b, n, n, c.batch, plan,
                                       /*identity_vals=*/true, w.hist, w.partial, s);
  const uint32_t* skey = where ? w.keys_b : w.keys_a;
  const uint32_t* sidx = where ? w.vals_b : w.vals_a;
  seg_head_kernel<<<pgrid, 256, 0, s>>>(skey, sidx, n, c.g.ncells, w.mark);
  EpiVoxelStart epi{w.mark, w.vox_start, n, c.max_voxels};
  enqueue_exclusive_scan(w.mark, n, n, c.batch, w.partial, w.totals, (int*)nullptr, LoadNonNegative{},
                         epi, s);
  dim3 mgrid((unsigned)ceil_div(c.max_voxels, 256), c.batch);
  // fp32 points of 4 / 5 floats: the fixed-shape rows are written by the wave form's slot-per-lane row writer, with the
  // sorted index list as its `clist`.  The float-per-thread gather it replaces here spent 205 us per 8 frames of
  // config 4 (1.25 TB/s) on three divisions and three dependent loads per output float.
  if constexpr (std::is_same<T, float>::value) {
    if (slot_rows_applicable(c.dim, c.max_pts, c.max_voxels)) {
      voxel_meta_kernel<<<mgrid, 256, 0, s>>>(skey, w.vox_start, w.totals, n, c.max_pts, c.max_voxels, c.g, c.coords,
                                              c.num_pts, c.num_voxels, c.coors4, w.vinfo);
      write_rows_slots(c, sidx, n, w.vinfo, w.totals);
      return launch_status();
    }
  }
  const int64_t per_frame = (int64_t)c.max_voxels * c.max_pts * c.dim;
  dim3 ggrid((unsigned)ceil_div(per_frame, 256), c.batch);
  gather_voxels_kernel<T><<<ggrid, 256, 0, s>>>(c.points, skey, sidx, w.vox_start, w.totals, n, c.dim, c.max_pts,
                                                c.max_voxels, c.voxels);
  voxel_meta_kernel<<<mgrid, 256, 0, s>>>(skey, w.vox_start, w.totals, n, c.max_pts, c.max_voxels, c.g, c.coords,
                                          c.num_pts, c.num_voxels, c.coors4, nullptr);
  return launch_status();
}

// The path selector of pd3_hard_voxelize_path, decoded: the form, the route-tile shape forced on it (-1: chosen from
// the sizes) and the variant bits of the wave form.
enum VoxForm {
  kFormAuto,         // the library's choice: wave form (2-D, else 3-D), else the tiled gather form, else the sort path
  kFormSort,         // stable radix sort of (cell, index), segment heads, flag scan in point order, voxel-parallel gather
  kFormTiled,        // voxelize_tiled.hpp, the payload kept in the workspace
  kFormTiledGather,  // the same with a list of point indices instead
  kFormWave,         // voxelize_wave.hpp
  kFormWave3d,       // voxelize_wave3d.hpp: the wave form for 3-D grids
};
struct VoxPath {
  VoxForm form;
  int shape, variant;
};
constexpr VoxPath kVoxPaths[] = {
    // 0: (heavy group waves at raised issue priority: 112.8-116.2 against 113.1-122.1 us per 16 frames in four A/B pairs
    //  on two boxes, profiles/r04_vox_paths.txt; path 5 is the same without it)
    {kFormAuto, -1, kVwPriority},
    {kFormSort, -1, 0},         // 1
    {kFormTiled, -1, 0},        // 2
    {kFormTiledGather, -1, 0},  // 3
    {kFormTiledGather, -1, 0},  // 4 (no form of its own)
    {kFormWave, -1, 0},         // 5
    {kFormWave, 0, 0},          // 6 .. 5 + kVwShapes: the route-tile shape forced (measurement)
    {kFormWave, 1, 0},
    {kFormWave, 2, 0},
    {kFormWave, 3, 0},
    {kFormWave, 4, 0},
    {kFormWave, -1, kVwPriority},  // 11 .. 13: measurement variants of the wave form
    {kFormWave, -1, kVwTwoStreams},
    {kFormWave, -1, kVwPriority | kVwTwoStreams},
    {kFormWave3d, -1, 0},  // 14; 15 / 16: its route tile forced to 8192 / 10240 points
    {kFormWave3d, 1, 0},
    {kFormWave3d, 2, 0},
    {kFormWave, 0, kVwPriority | kVwCarry},  // 17 measurement: path 6 (4096-point route tiles) + the carried payload
};
constexpr int kVoxPathCount = (int)(sizeof(kVoxPaths) / sizeof(kVoxPaths[0]));
static_assert(kVoxPathCount == 18 && kVwShapes == 5, "the selector values 0 .. 17 are part of the ABI");

// What the three entry points check before anything runs, in this order (it decides which status wins when two things are
// wrong): null pointers, numeric ranges, the grid and the path selector, the workspace size.  Fills c.g.
// rows_out: the entry's own row output is there (voxels; or the span and list arrays of pd3_hard_voxelize_index).
template <typename T>
static int vox_check(VoxCall<T>& c, bool rows_out, const float* voxel_size, const float* range, int path,
                     size_t workspace_bytes) {
  if (!c.points || !rows_out || !c.coords || !c.num_pts || !c.num_voxels || !c.workspace) return PD3_EINVAL;
  if (c.batch <= 0 || c.n <= 0 || c.n >= ((int64_t)1 << 31) || c.dim < 3 || c.max_pts <= 0 || c.max_voxels <= 0)
    return PD3_EINVAL;
  if (!make_grid(voxel_size, range, c.g) || path < 0 || path >= kVoxPathCount) return PD3_EINVAL;
  if (workspace_bytes < pd3_hard_voxelize_workspace(c.batch, c.n, c.dim, voxel_size, range, c.max_pts, c.max_voxels))
    return PD3_EWORKSPACE;
  return 0;
}

}  // namespace pd3

using namespace pd3;

extern "C" size_t pd3_hard_voxelize_workspace(int batch, int64_t max_points, int num_point_dim,
                                              const float* voxel_size,
                                              const float* point_cloud_range,
                                              int max_num_points_in_voxel, int max_voxels) {
  VoxCall<float> c{};  // the sizes only (no voxels tensor: the aligned row writers)
  c.batch = batch;
  c.n = max_points;
  c.dim = num_point_dim;
  c.max_pts = max_num_points_in_voxel;
  c.max_voxels = max_voxels;
  if (batch <= 0 || max_points <= 0 || max_voxels <= 0 || !make_grid(voxel_size, point_cloud_range, c.g))
    return 0;
  const RadixPlan plan = radix_plan(c.g.ncells, max_points);
  size_t bytes = carve(nullptr, batch, max_points, max_voxels, plan).bytes;
  VtPlan vp;
  if (tiled_applicable(c, vp))
    bytes = std::max(bytes, vt_carve(nullptr, batch, max_points, num_point_dim, max_num_points_in_voxel, max_voxels,
                                     c.g.ncells, vp).bytes);
  for (int shape = -1; shape < kVwShapes; ++shape) {
    VwPlan wp;
    if (wave_applicable(c, shape, wp)) {
      bytes = std::max(bytes, vw_carve(nullptr, batch, max_points, max_voxels, wp).bytes);
      if (batch >= 2)  // the two-stream form carves one region per half batch
        bytes = std::max(bytes, align_up(vw_carve(nullptr, batch / 2, max_points, max_voxels, wp).bytes, 256) +
                                    vw_carve(nullptr, batch - batch / 2, max_points, max_voxels, wp).bytes);
    }
  }
  for (int shape = -1; shape < 3; ++shape) {
    VwPlan wp;
    if (wave3d_applicable(c, shape, wp))
      bytes = std::max(bytes, vw_carve(nullptr, batch, max_points, max_voxels, wp, true).bytes);
  }
  return bytes;
}

extern "C" int pd3_hard_voxelize_path(const float* points, const int32_t* num_points, int batch,
                                      int64_t max_points, int num_point_dim, const float* voxel_size,
                                      const float* point_cloud_range, int max_num_points_in_voxel,
                                      int max_voxels, float* voxels, int32_t* coords,
                                      int32_t* num_points_per_voxel, int32_t* num_voxels,
                                      int32_t* coors_batched, void* workspace, size_t workspace_bytes,
                                      void* stream, int path) {
  VoxCall<float> c{points, num_points, batch, max_points, num_point_dim, {}, max_num_points_in_voxel, max_voxels,
                   voxels, coords, num_points_per_voxel, num_voxels, coors_batched, workspace,
                   static_cast<hipStream_t>(stream)};
  if (const int rc = vox_check(c, voxels != nullptr, voxel_size, point_cloud_range, path, workspace_bytes))
    return rc;
  const VoxPath p = kVoxPaths[path];
  VwPlan wp;
  VtPlan vp;
  switch (p.form) {
    case kFormWave:
      if (!wave_applicable(c, p.shape, wp)) return PD3_EUNSUPPORTED;
      return (p.variant & kVwTwoStreams) ? run_wave_split(c, wp, p.variant) : run_wave(c, wp, p.variant);
    case kFormWave3d:
      if (!wave3d_applicable(c, p.shape, wp)) return PD3_EUNSUPPORTED;
      return run_wave(c, wp, 0, 0, true);
    case kFormTiled:
    case kFormTiledGather:
      if (!tiled_applicable(c, vp)) return PD3_EUNSUPPORTED;
      return run_tiled(c, vp, p.form == kFormTiledGather);
    case kFormSort:
      return run_sort_path(c);
    case kFormAuto:
      break;
  }
  if (wave_applicable(c, -1, wp)) return run_wave(c, wp, p.variant);
  if (wave3d_applicable(c, -1, wp)) return run_wave(c, wp, 0, 0, true);
  if (tiled_applicable(c, vp)) return run_tiled(c, vp, true);
  return run_sort_path(c);
}

extern "C" int64_t pd3_hard_voxelize_index_list_entries(int batch, int64_t max_points) {
  if (batch <= 0 || max_points <= 0) return 0;
  return (int64_t)batch * max_points + 4;
}

extern "C" int pd3_hard_voxelize_index(const float* points, const int32_t* num_points, int batch, int64_t max_points,
                                       int num_point_dim, const float* voxel_size, const float* point_cloud_range,
                                       int max_num_points_in_voxel, int max_voxels, int32_t* vox_span,
                                       int32_t* point_list, int32_t* coords, int32_t* num_points_per_voxel,
                                       int32_t* num_voxels, int32_t* coors_batched, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  VoxCall<float> c{points, num_points, batch, max_points, num_point_dim, {}, max_num_points_in_voxel, max_voxels,
                   nullptr, coords, num_points_per_voxel, num_voxels, coors_batched, workspace,
                   static_cast<hipStream_t>(stream)};
  if (const int rc = vox_check(c, vox_span && point_list, voxel_size, point_cloud_range, 0, workspace_bytes))
    return rc;
  VwPlan wp;
  if (wave_applicable(c, -1, wp)) return run_wave(c, wp, kVwPriority, 0, false, vox_span, point_list);
  if (wave3d_applicable(c, -1, wp)) return run_wave(c, wp, 0, 0, true, vox_span, point_list);
  return PD3_EUNSUPPORTED;  // (the tiled and sort forms keep no per-voxel index list: run pd3_hard_voxelize)
}

extern "C" int pd3_hard_voxelize(const float* points, const int32_t* num_points, int batch,
                                 int64_t max_points, int num_point_dim, const float* voxel_size,
                                 const float* point_cloud_range, int max_num_points_in_voxel,
                                 int max_voxels, float* voxels, int32_t* coords,
                                 int32_t* num_points_per_voxel, int32_t* num_voxels,
                                 int32_t* coors_batched, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  return pd3_hard_voxelize_path(points, num_points, batch, max_points, num_point_dim, voxel_size,
                                point_cloud_range, max_num_points_in_voxel, max_voxels, voxels, coords,
                                num_points_per_voxel, num_voxels, coors_batched, workspace, workspace_bytes,
                                stream, 0);
}

// double points (the reference's CPU kernel instantiated for double): always the generic sort path
extern "C" int pd3_hard_voxelize_f64(const double* points, const int32_t* num_points, int batch,
                                     int64_t max_points, int num_point_dim, const float* voxel_size,
                                     const float* point_cloud_range, int max_num_points_in_voxel,
                                     int max_voxels, double* voxels, int32_t* coords,
                                     int32_t* num_points_per_voxel, int32_t* num_voxels,
                                     int32_t* coors_batched, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  VoxCall<double> c{points, num_points, batch, max_points, num_point_dim, {}, max_num_points_in_voxel, max_voxels,
                    voxels, coords, num_points_per_voxel, num_voxels, coors_batched, workspace,
                    static_cast<hipStream_t>(stream)};
  if (const int rc = vox_check(c, voxels != nullptr, voxel_size, point_cloud_range, 0, workspace_bytes))
    return rc;
  return run_sort_path(c);
}

extern "C" int pd3_version(void) { return 200; }
extern "C" const char* pd3_target_arch(void) { return "gfx950"; }

extern "C" int pd3_dynamic_voxelize(const float* points, int64_t num_points, int num_point_dim,
                                    const float* voxel_size, const float* point_cloud_range, int32_t* coors,
                                    void* stream) {
  if (num_points < 0 || num_point_dim < 3 || !voxel_size || !point_cloud_range) return PD3_EINVAL;
  if (num_points == 0) return 0;
  if (!points || !coors) return PD3_EINVAL;
  VoxGrid g;
  if (!make_grid(voxel_size, point_cloud_range, g)) return PD3_EINVAL;
  dynamic_voxelize_kernel<<<(unsigned)ceil_div(num_points, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(
      points, num_points, num_point_dim, g, coors);
  return launch_status();
}
