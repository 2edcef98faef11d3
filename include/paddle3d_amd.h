/* paddle3d_amd.h -- C ABI of libpaddle3d_amd.so, the MI355X (gfx950) LiDAR-detection op library.
 *
 * Drop-in boundary: every entry point replaces one custom operator (or one layer built on Paddle-core
 * scatter) of the reference's `paddle3d.ops` plugin API for the LiDAR hot path.  The reference
 * registers its operators with PD_BUILD_OP(name).Inputs/.Outputs/.Attrs (file:line cited per
 * function below); a maintainer binds these symbols from a Paddle custom-op shim or via ctypes --
 * see INTEGRATION.md.  the modules under paddle3d_amd/ops/ are the ctypes binding used by this repository.
 *
 * Conventions
 *   - All pointers are DEVICE pointers unless a parameter is documented "host".
 *   - Plain C types only; `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - The library never allocates or frees device memory: outputs and `workspace` are caller-owned.
 *     Query the workspace size with the matching *_workspace() function (bytes; 256-B aligned base).
 *   - Every call is asynchronous on `stream` unless documented otherwise, re-entrant and thread-safe
 *     given disjoint buffers.
 *   - Return value: 0 ok; <0 argument error (PD3_E*); >0 a hipError_t from the launch.
 *   - fp32 only, like the reference ops (voxelize_op.cc:104-106 hard-codes FLOAT32 outputs).
 */
#ifndef PADDLE3D_AMD_H
#define PADDLE3D_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PD3_OK 0
#define PD3_EINVAL (-1)
#define PD3_EWORKSPACE (-2)
#define PD3_EUNSUPPORTED (-3)

/* Library/ABI version (major*10000 + minor*100 + patch) and the gfx target it was compiled for. */
int pd3_version(void);
const char *pd3_target_arch(void);

/* Self-check of the one undocumented hardware property the default hard_voxelize path relies on: lanes of one
 * wave-wide returning LDS add on the same word are served in ascending lane order, a wave's LDS instructions in
 * program order (csrc/selfcheck.hip).  Every wave (blocks * waves_per_block of them) walks `rounds` x 64 addresses
 * (addr [waves][rounds][64] uint32 < table, 0xFFFFFFFF = lane skips) through its own LDS table and writes what each
 * add returned (old, same shape; 0xFFFFFFFF for skipped lanes); the caller compares with a sequential count per
 * wave.  No reference counterpart (the reference's GPU path uses global atomics and is not order-exact). */
int pd3_selfcheck_lds_atomic_order(const uint32_t *addr, uint32_t *old, int blocks, int waves_per_block, int rounds,
                                   int table, void *stream);

/* Self-check of the block top-K selection the post-processing kernels share (csrc/block_topk.hpp: radix cut,
 * compaction, bitonic sort) on raw keys.  One 1024-thread workgroup per set selects the K smallest counted keys of
 * keys [sets][n] uint32 in ascending (key, index) order -- what a stable sort gives -- with the header's own functions.
 *   counted   a key below 2^key_bits (1 <= key_bits <= 30) that is not `leave_out` (a key value the caller's visit
 *             skips, the SSD head's convention; < 0: none).  A key not counted must sort after every key taken.
 *   form      0: keys read from global memory, block_topk_compact; 1: keys staged into LDS, block_topk_compact_chunks
 *             (n <= 16384), as CenterPoint's selection does
 *   skip_cut  nonzero: no radix cut, the callers' take-all TopkCut{0xFFFFFFFF, 0} (every key below 0xFFFFFFFF)
 *   idx, key  [sets][K] uint32: low and high word of the sorted list (index, key); 0xFFFFFFFF past the taken entries
 *   cut       [sets][2] uint32: kc, r as block_topk_cut returned them
 * A set that breaks the selection's precondition (skip_cut == 0: more than K keys counted; always: no more than K
 * entries taken) is not selected from: all of its idx, key and cut words are 0xFFFFFFFF.
 * PD3_EINVAL for a NULL pointer, K outside [1, 1024], key_bits outside [1, 30], n < 1, sets < 0, a form other than
 * 0 / 1, form 1 with n > 16384; nothing is launched for sets == 0.  No reference counterpart. */
int pd3_selfcheck_block_topk(const uint32_t *keys, int sets, int n, int K, int key_bits, int form, int64_t leave_out,
                             int skip_cut, uint32_t *idx, uint32_t *key, uint32_t *cut, void *stream);

/* ---------------------------------------------------------------------------------------------
 * hard_voxelize -- replaces PD_BUILD_OP(hard_voxelize), paddle3d/ops/voxel/voxelize_op.cc:183-191
 * (kernel fn hard_voxelize :149-166; CPU semantics hard_voxelize_cpu_kernel :19-82, which this
 * implementation reproduces bit-exactly, unlike the reference's own CUDA path voxelize_op.cu:208-346
 * whose atomics make voxel order and in-voxel point choice nondeterministic).
 *
 *   points            [batch, max_points, num_point_dim] fp32, row-major; frame b uses its first
 *                     num_points[b] rows (num_points == NULL: all max_points rows).
 *   voxel_size        host float[3] (x, y, z);  point_cloud_range host float[6] (xmin..zmin, xmax..zmax)
 *   voxels            [batch, max_voxels, max_num_points_in_voxel, num_point_dim] fp32, zero padded
 *   coords            [batch, max_voxels, 3] int32 (z, y, x), zero padded
 *   num_points_per_voxel [batch, max_voxels] int32, zero padded
 *   num_voxels        [batch] int32
 *   coors_batched     optional (NULL to skip) [batch, max_voxels, 4] int32 (batch, z, y, x) with batch = -1 on
 *                     padding rows: the `coors_pad` HardVoxelizer.single_forward builds with cast + F.pad
 *                     (voxelize.py:51-57), written by the same pass
 * batch = 1 is exactly the reference op; batch > 1 is the reference's HardVoxelizer python loop
 * (paddle3d/models/voxelizers/voxelize.py:60-82) in one launch sequence.
 */
size_t pd3_hard_voxelize_workspace(int batch, int64_t max_points, int num_point_dim,
                                   const float *voxel_size, const float *point_cloud_range,
                                   int max_num_points_in_voxel, int max_voxels);
int pd3_hard_voxelize(const float *points, const int32_t *num_points, int batch, int64_t max_points,
                      int num_point_dim, const float *voxel_size, const float *point_cloud_range,
                      int max_num_points_in_voxel, int max_voxels, float *voxels, int32_t *coords,
                      int32_t *num_points_per_voxel, int32_t *num_voxels, int32_t *coors_batched,
                      void *workspace, size_t workspace_bytes, void *stream);
/* Same operator with the implementation chosen by the caller (diagnostics and the parity tests, which run
 * every case on all of them): path 0 = automatic (what pd3_hard_voxelize does: 5 where the grid qualifies, else 3,
 * else 1), 1 = generic radix-sort path (any grid below 2^31 cells), 2 = tiled path, payload copied once into a
 * cell-ordered compact array, 3 = tiled path, rows gathered from the points through a cell-ordered index list (2 and
 * 3: BEV-sized grids up to 2^22 cells), 5 = wave form of the tiled path (one wave per group of 1024 cells, grids up to
 * 2^20 cells; 6 .. 10 = the same with the route kernel's tile shape forced: 4096 / 8192 / 10240 / 5120 / 5120 points;
 * 11 = 5 with heavy group waves at raised issue priority (the automatic choice), 12 / 13 = two half batches on two
 * streams), 14 = the wave form for 3-D grids of 2^20 .. 2^28 cells (15 / 16: its route tile forced), 17 = a measurement
 * form: path 6 with the points' payload carried through the route kernel's LDS slice.
 * PD3_EUNSUPPORTED when the shape does not qualify for a forced path.  Identical bytes out on every path. */
int pd3_hard_voxelize_path(const float *points, const int32_t *num_points, int batch, int64_t max_points,
                           int num_point_dim, const float *voxel_size, const float *point_cloud_range,
                           int max_num_points_in_voxel, int max_voxels, float *voxels, int32_t *coords,
                           int32_t *num_points_per_voxel, int32_t *num_voxels, int32_t *coors_batched,
                           void *workspace, size_t workspace_bytes, void *stream, int path);

/* hard_voxelize WITHOUT the padded [V, P, D] tensor (the model path; reference chain paddle3d/models/voxelizers/
 * voxelize.py:39-58 -> voxel_encoders/pillar_encoder.py:156-210): the same voxel ids, coords, counts and batched
 * coors as pd3_hard_voxelize, and in place of copies of the points an INDEX of them:
 *   vox_span   [batch, max_voxels, 2] int32: (start, count) -- voxel v of frame b holds the points
 *              point_list[b * max_points + start + 0 .. count - 1] (indices into frame b's rows of `points`,
 *              ascending = the reference's order inside a voxel); count == num_points_per_voxel
 *   point_list [pd3_hard_voxelize_index_list_entries(batch, max_points)] int32
 *   Padding rows (v >= num_voxels[b]) of vox_span read (0, 0), those of coords / num_points_per_voxel / coors_batched
 *   as in pd3_hard_voxelize; entries of point_list that no span names are scratch (unspecified).
 * A consumer reads a voxel's points from `points` itself (pd3_pillar_feature_net_indexed): the 78 %-zeros tensor is
 * neither written nor read.  Grids the wave forms do not serve (see pd3_hard_voxelize_path) return -3: run
 * pd3_hard_voxelize there.  Workspace: pd3_hard_voxelize_workspace. */
int64_t pd3_hard_voxelize_index_list_entries(int batch, int64_t max_points);
int pd3_hard_voxelize_index(const float *points, const int32_t *num_points, int batch, int64_t max_points,
                            int num_point_dim, const float *voxel_size, const float *point_cloud_range,
                            int max_num_points_in_voxel, int max_voxels, int32_t *vox_span, int32_t *point_list,
                            int32_t *coords, int32_t *num_points_per_voxel, int32_t *num_voxels,
                            int32_t *coors_batched, void *workspace, size_t workspace_bytes, void *stream);

/* hard_voxelize for double points: PD_DISPATCH_FLOATING_TYPES (voxelize_op.cc:128) instantiates the reference's CPU
 * kernel for float and double; with T = double the cell index is floor((p - (double)range_min) / (double)voxel_size)
 * (:37-45) and `voxels` is double.  Generic sort path (any grid below 2^31 cells); the workspace of
 * pd3_hard_voxelize_workspace suffices.  points / voxels fp64 device, everything else as pd3_hard_voxelize. */
int pd3_hard_voxelize_f64(const double *points, const int32_t *num_points, int batch, int64_t max_points,
                          int num_point_dim, const float *voxel_size, const float *point_cloud_range,
                          int max_num_points_in_voxel, int max_voxels, double *voxels, int32_t *coords,
                          int32_t *num_points_per_voxel, int32_t *num_voxels, int32_t *coors_batched,
                          void *workspace, size_t workspace_bytes, void *stream);

/* dynamic_voxelize -- per-point voxel coordinates without the per-voxel cap.  The reference has no such
 * operator (only a "dynamic voxelization" comment at transforms/ for num_points == -1);
 * BASELINE.json's north star names it, so it is provided with hard_voxelize's own cell rule
 * (voxelize_op.cc:37-45): coors[i] = (z, y, x) of point i, (-1, -1, -1) outside point_cloud_range.
 *   points [num_points, num_point_dim] fp32 device;  coors [num_points, 3] int32 device */
int pd3_dynamic_voxelize(const float *points, int64_t num_points, int num_point_dim, const float *voxel_size,
                         const float *point_cloud_range, int32_t *coors, void *stream);

/* ---------------------------------------------------------------------------------------------
 * pointpillars_scatter -- replaces PointPillarsScatter.forward_batch,
 * paddle3d/models/middle_encoders/pillar_scatter.py:57-93 (zeros canvas + paddle.scatter(overwrite) +
 * transpose + concat), fused into one canvas-parallel pass.
 *
 *   voxel_features [num_pillars, channels] fp32;  coords [num_pillars, 4] int32 (batch, z, y, x)
 *   canvas         [batch, channels, ny, nx] fp32 -- fully written (zero where no pillar)
 * Pillars with batch index outside [0, batch) are ignored.  Duplicate (batch, y, x): last index wins,
 * as paddle.scatter(overwrite=True) documents; the hot path never produces duplicates.
 */
size_t pd3_pointpillars_scatter_workspace(int batch, int ny, int nx);
int pd3_pointpillars_scatter(const float *voxel_features, const int32_t *coords,
                             int64_t num_pillars, int channels, int batch, int ny, int nx,
                             float *canvas, void *workspace, size_t workspace_bytes, void *stream);

/* PointPillarsScatter fused into the convolution that consumes it (round 3): the canvas is never written.
 *   pd3_pointpillars_inverse_map: inv [batch, ny*nx] int32 = the pillar row (index into voxel_features) whose coords
 *     name the cell, -1 for an empty cell; on duplicates the highest row wins (paddle.scatter(overwrite=True),
 *     pillar_scatter.py:83-90).
 *   pd3_scatter_conv3x3_bias_relu: conv3x3 / pad 1 / stride 2 + bias + ReLU (a SECOND block's first convolution,
 *     second_backbone.py:84-98, BatchNorm folded) over the canvas those two arguments describe; the kernel stages the
 *     occupied cells' channels straight from voxel_features [pillars, cin].  w_packed as pd3_conv3x3_bias_relu;
 *     out [batch, cout, ny/2, out_w] (out_w % 4 == 0, columns >= nx/2 written as zeros).  Results are bit-identical to
 *     pd3_pointpillars_scatter followed by pd3_conv3x3_bias_relu.  cin % 8 == 0, cout % 64 == 0, ny, nx even. */
int pd3_pointpillars_inverse_map(const int32_t *coords, int64_t num_pillars, int batch, int ny, int nx,
                                 int32_t *inv, void *stream);
int pd3_scatter_conv3x3_bias_relu(const float *voxel_features, const int32_t *inv, const float *w_packed,
                                  const float *bias, int batch, int cin, int cout, int ny, int nx, int stride,
                                  int relu, float *out, int out_w, void *stream);

/* The same pair -- PointPillarsScatter (pillar_scatter.py:57-93) + the strided 3x3 / pad 1 convolution that opens
 * SecondBackbone (second_backbone.py:84-98) -- as a SPARSE convolution over the occupied pillars (round 6): a nuScenes
 * canvas is 11 % occupied, an output pixel sees 2.5 of its nine cells on average and 60 % of the pixels see none.
 *   pd3_pillar_conv_rulebook: from the inverse map [batch, ny * nx] (pd3_pointpillars_inverse_map) the rulebook of the
 *     active output pixels in raster order: nbr [capacity, 9] int32 (pillar row of tap ky * 3 + kx or -1), out_cell
 *     [capacity] (pixel b * ho * wo + oy * wo + ox of a row), cell_row [batch, ho * wo] (row of a pixel or -1), n_out [1]
 *     (device: the row count; rows beyond `capacity` are dropped -- batch * ho * wo can never overflow), ho = (ny - 1) /
 *     stride + 1.  The rulebook feeds pd3_sparse_tile_order + pd3_sparse_conv3d_features_bf16x3 / _f16 (kernel_volume 9,
 *     in_feats = the pillar features, n_out as the device row count).  order (optional, [pd3_sparse_tile_order_entries(
 *     capacity)] int32): the rulebook's tile order by a counting sort over the 512 possible tap masks -- the same
 *     scheduling hint pd3_sparse_tile_order computes with its general sorting network.
 *   pd3_rows_to_dense_fill: rows [n, channels] fp32 -> out [batch, channels, h, w] NCHW through cell_row; a pixel without
 *     a row holds fill[c] (= relu(bias[c]): what the dense convolution computes from nine zeros); h * w % 4 == 0,
 *     channels % 4 == 0. */
size_t pd3_pillar_conv_rulebook_workspace(int batch, int ny, int nx, int stride);
int pd3_pillar_conv_rulebook(const int32_t *inverse_map, int batch, int ny, int nx, int stride, int32_t *nbr,
                             int32_t *out_cell, int32_t *cell_row, int32_t *n_out, int capacity, int32_t *order,
                             void *workspace, size_t workspace_bytes, void *stream);
int pd3_rows_to_dense_fill(const float *rows, const int32_t *cell_row, const float *fill, int batch, int channels, int h,
                           int w, float *out, void *stream);

/* The three steps above as ONE launch from the inverse map to NCHW, for the shapes its tile takes (the span form,
 * csrc/pillar_conv_span.hip): a workgroup owns 256 consecutive cells of an output row x 64 channels, builds the cells'
 * taps in LDS, accumulates tap by tap in an LDS tile and writes the tile as 1 KB channel segments.  No rulebook, no rows,
 * no workspace.  The same bytes as pd3_pillar_conv_rulebook -> pd3_sparse_conv3d_features_bf16x3 (bias, relu) ->
 * pd3_rows_to_dense_fill.
 *   feats [n_in, cin] fp32 pillar features (an inverse-map entry outside [0, n_in) counts as empty); inverse_map
 *   [batch, ny * nx]; weight_packed = pd3_sparse_pack_weight_bf16x3 of [9, cin, cout] (tap ky * 3 + kx); bias [cout] or
 *   NULL; fill [cout] = the value of a cell without a pillar under its nine taps (relu(bias)); out [batch, cout, ho, wo],
 *   ho = (ny - 1) / 2 + 1.  PD3_EUNSUPPORTED unless stride == 2, cin == 64, cout is 64 or 128 and wo % 256 == 0. */
int pd3_pillar_conv_span_x3(const float *feats, int n_in, const int32_t *inverse_map, int batch, int ny, int nx, int stride,
                            int cin, int cout, const void *weight_packed, const float *bias, const float *fill, int relu,
                            float *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * pillar feature net (PFN) -- replaces PillarFeatureNet.forward / PFNLayer.forward in eval mode,
 * paddle3d/models/voxel_encoders/pillar_encoder.py:156-210 / :81-105 (decorate with cluster and
 * pillar-centre offsets, mask padded slots, Linear(no bias) -> BatchNorm1D(eps 1e-3) -> ReLU -> max
 * over the points of a pillar; the non-last layer concatenates the max back).  BatchNorm is folded by
 * the caller: scale = gamma / sqrt(var + eps), shift = beta - mean * scale.
 *
 * The same entry point covers HardVFE.forward with with_cluster_center = with_voxel_center = True
 * (voxel_encoders/voxel_encoder.py:142-283, the BEVFusion LiDAR stream): voxel_center_dims = 3 adds the z
 * offset z - (coor_z * vz + z_offset) and layer 1 keeps all its C1 units (w2 is [2*C1, C2] either way).
 *
 *   voxels [M, P, D], num_points [M] int32, coors [M, 4] int32 (b, z, y, x)
 *   voxel_center_dims 2 (PillarFeatureNet: x, y) or 3 (HardVFE: x, y, z)
 *   w1 [D+3+voxel_center_dims, C1] (Paddle Linear layout [in, out]), scale1/shift1 [C1]
 *   w2 [2*C1, C2], scale2/shift2 [C2]   (w2 == NULL: single-layer PFN, output [M, C1])
 *   out [M, C2]
 * legacy == 0 only (the nuScenes configs); with_distance unsupported (no config on the path uses it).
 * Rows with num_points <= 0 (padding of a fixed-shape batch) produce zeros.
 */
int pd3_pillar_feature_net(const float *voxels, const int32_t *num_points, const int32_t *coors,
                           int64_t num_pillars, int max_points, int num_point_dim,
                           int voxel_center_dims, float vx, float vy, float vz, float x_offset,
                           float y_offset, float z_offset, const float *w1, const float *scale1,
                           const float *shift1, int c1, const float *w2, const float *scale2,
                           const float *shift2, int c2, float *out, void *stream);

/* Same operator with the kernel form named by the caller (diagnostics and the parity tests, which run every form on
 * one input; there is no environment switch): path 0 = what pd3_pillar_feature_net picks, 1 = the per-pillar forms
 * (one wave per pillar), 2 = the packed form (a wave packs the rows of 8 consecutive pillars into 16-row MFMA blocks;
 * two-layer C1 = 32, C2 = 64 nets with P <= 32 only, PD3_EUNSUPPORTED otherwise). */
int pd3_pillar_feature_net_path(const float *voxels, const int32_t *num_points, const int32_t *coors,
                                int64_t num_pillars, int max_points, int num_point_dim,
                                int voxel_center_dims, float vx, float vy, float vz, float x_offset,
                                float y_offset, float z_offset, const float *w1, const float *scale1,
                                const float *shift1, int c1, const float *w2, const float *scale2,
                                const float *shift2, int c2, float *out, int path, void *stream);

/* pd3_pillar_feature_net reading the pillars' points through pd3_hard_voxelize_index's (vox_span, point_list) from
 * the point cloud itself: points [frames, points_per_frame, D], list_stride = rows of point_list per frame
 * (= max_points of the voxelizer call), coors [num_pillars, 4], pillars_per_frame = max_voxels.  Bit-identical to
 * pd3_hard_voxelize + pd3_pillar_feature_net.  Serves the two-layer 32 / 64 net with up to 32 points of 4 / 5
 * floats per pillar and pillars_per_frame a multiple of 8; other shapes return -3 (run the pair), and so do
 * list_stride at or above 2^24 (a span's start, a position in a frame's row of the list, travels in 24 bits) and
 * points_per_frame at or above 2^24 (a conservative bound: point indices are read from the list at their full 32 bits,
 * but a list that names every point of such a frame once would not fit the row).
 * The entry reads no device memory, so two bounds are the caller's to keep (pd3_hard_voxelize_index keeps both):
 *   - coors' x and y cells lie in [0, 65536): the kernel carries them in 16 + 16 bits.  A grid with more than
 *     65 536 cells along x or y gets wrong pillar centres -- run the pair there;
 *   - a span's count is already capped at max_points: the kernel reads min(count, max_points) points and the cluster
 *     mean divides by that, where pd3_pillar_feature_net divides by the num_points it is given. */
int pd3_pillar_feature_net_indexed(const float *points, int64_t points_per_frame, const int32_t *vox_span,
                                   const int32_t *point_list, int64_t list_stride, const int32_t *coors,
                                   int64_t num_pillars, int pillars_per_frame, int max_points, int num_point_dim,
                                   int voxel_center_dims, float vx, float vy, float vz, float x_offset,
                                   float y_offset, float z_offset, const float *w1, const float *scale1,
                                   const float *shift1, int c1, const float *w2, const float *scale2,
                                   const float *shift2, int c2, float *out, void *stream);

/* VoxelMean.forward, paddle3d/models/voxel_encoders/voxel_encoder.py:44-57: sum over P / count. */
int pd3_voxel_mean(const float *voxels, const int32_t *num_points, int64_t num_voxels,
                   int max_points, int num_point_dim, float *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * iou3d_nms -- replaces the five ops of paddle3d/ops/iou3d_nms/iou3d_nms_api.cpp:73-108.
 * Boxes are [N, 7] fp32 (x, y, z, dx, dy, dz, heading).
 *
 * pd3_nms_bev / pd3_nms_normal: nms_gpu / nms_normal_gpu (iou3d_nms.cpp:86-141 / :143-204).
 * The suppression bit-matrix AND the greedy sweep run on the device (the reference copies the mask to
 * the host and sweeps there).  keep [N] int32 (first *num_to_keep entries valid) and num_to_keep [1]
 * int32 are DEVICE buffers; the Python shim returns them as CPU int32 tensors like the reference.
 */
size_t pd3_nms_workspace(int num_boxes);
int pd3_nms_bev(const float *boxes, int num_boxes, float nms_overlap_thresh, int32_t *keep,
                int32_t *num_to_keep, void *workspace, size_t workspace_bytes, void *stream);
int pd3_nms_normal(const float *boxes, int num_boxes, float nms_overlap_thresh, int32_t *keep,
                   int32_t *num_to_keep, void *workspace, size_t workspace_bytes, void *stream);
/* boxes_iou_bev_gpu / boxes_overlap_bev_gpu (iou3d_nms.cpp:44-84): dense [N, M] matrices. */
int pd3_boxes_iou_bev(const float *boxes_a, int num_a, const float *boxes_b, int num_b,
                      float *ans_iou, void *stream);
int pd3_boxes_overlap_bev(const float *boxes_a, int num_a, const float *boxes_b, int num_b,
                          float *ans_overlap, void *stream);
/* Diagnostic: the float math routines the geometry / decode kernels use, over an array -- glibc's sinf / cosf / expf /
 * atanf / atan2f bit for bit (csrc/libm_exact.hpp; what the reference's cos / sin / atan2 on floats call,
 * iou3d_cpu.cpp:77-79,128-129).  op: 0 sinf(x), 1 cosf(x), 2 expf(x), 3 atanf(x), 4 atan2f(x, y).  x, y, out device. */
int pd3_libm_eval(int op, const float *x, const float *y, float *out, int64_t n, void *stream);

/* ---------------------------------------------------------------------------------------------
 * centerpoint_postprocess -- replaces PD_BUILD_OP(centerpoint_postprocess),
 * paddle3d/ops/centerpoint_postprocess/postprocess.cc:91-104 (postprocess_gpu, postprocess.cu:104-280).
 * All tasks of one frame in one launch sequence on one stream, no host round trip inside.
 *
 *   hm/reg/height/dim/vel/rot: host arrays of `num_tasks` device pointers to contiguous fp32 NCHW
 *     maps: hm[t] [batch, hm_channels[t], H, W], reg [batch,2,H,W], height [batch,1,H,W],
 *     dim [batch,3,H,W], vel [batch,2,H,W], rot [batch,2,H,W].  batch = 1 is exactly the reference op
 *     (it rejects anything else, postprocess.cu:19-20,138); batch > 1 runs the per-frame op for every
 *     frame in the same launch sequence.
 *   hm_channels: host int[num_tasks];  label_offsets: host int[num_tasks] (the op's `num_classes` attr)
 *   out_bboxes  [batch, num_tasks * max(nms_post_max_size,1), 9 or 7] fp32
 *   out_scores  [batch, same rows] fp32;  out_labels [batch, same rows] int64
 *   out_count   [batch] int32: number of valid leading rows per frame (tasks concatenated in order;
 *               a task with no candidate contributes the reference's fake row: zeros box, score -1,
 *               label 0).  In all three forms below the rows behind it read zero in out_bboxes, out_scores
 *               and out_labels: no output needs clearing by the caller.
 */
size_t pd3_centerpoint_postprocess_workspace(int batch, int num_tasks, int feat_h, int feat_w,
                                             int nms_pre_max_size, int nms_post_max_size);
int pd3_centerpoint_postprocess(const float *const *hm, const float *const *reg,
                                const float *const *height, const float *const *dim,
                                const float *const *vel, const float *const *rot, int batch,
                                int num_tasks, const int *hm_channels, int feat_h, int feat_w,
                                const float *voxel_size, const float *point_cloud_range,
                                const float *post_center_range, const int *label_offsets,
                                int down_ratio, float score_threshold, float nms_iou_threshold,
                                int nms_pre_max_size, int nms_post_max_size, int with_velocity,
                                float *out_bboxes, float *out_scores, int64_t *out_labels,
                                int32_t *out_count, void *workspace, size_t workspace_bytes,
                                void *stream);

/* Same, for head tensors that are channel slices (views) of one wider [batch, C, H, W] map: every head pointer
 * addresses frame 0 of its slice and `head_batch_stride` (> 0, in elements, the same for all heads) leads to the
 * next frame -- what a fused CenterHead produces; saves the per-head contiguous copies. */
int pd3_centerpoint_postprocess_strided(const float *const *hm, const float *const *reg,
                                const float *const *height, const float *const *dim,
                                const float *const *vel, const float *const *rot, int64_t head_batch_stride, int batch,
                                int num_tasks, const int *hm_channels, int feat_h, int feat_w,
                                const float *voxel_size, const float *point_cloud_range,
                                const float *post_center_range, const int *label_offsets,
                                int down_ratio, float score_threshold, float nms_iou_threshold,
                                int nms_pre_max_size, int nms_post_max_size, int with_velocity,
                                float *out_bboxes, float *out_scores, int64_t *out_labels,
                                int32_t *out_count, void *workspace, size_t workspace_bytes,
                                void *stream, int selection);
/* Same as the strided form (automatic selection), plus `out_records` [batch, max_per_img, 11] fp32: the rows once
 * more in the fixed shape of the multi-GPU result hand-off -- box (7 or 9 values, zero padded to 9), score, label as
 * float, rows >= count zero -- so that the RCCL all-gather of a batch's detections (paddle3d_amd/dist.py; no
 * counterpart in the reference, whose evaluation is single device, apis/trainer.py:47-51) starts from the operator's
 * own output.  All four outputs read zero behind the last row; none needs clearing by the caller. */
int pd3_centerpoint_postprocess_records(const float *const *hm, const float *const *reg,
                                        const float *const *height, const float *const *dim,
                                        const float *const *vel, const float *const *rot,
                                        int64_t head_batch_stride, int batch, int num_tasks,
                                        const int *hm_channels, int feat_h, int feat_w, const float *voxel_size,
                                        const float *point_cloud_range, const float *post_center_range,
                                        const int *label_offsets, int down_ratio, float score_threshold,
                                        float nms_iou_threshold, int nms_pre_max_size, int nms_post_max_size,
                                        int with_velocity, float *out_bboxes, float *out_scores,
                                        int64_t *out_labels, int32_t *out_count, float *out_records,
                                        int max_per_img, void *workspace, size_t workspace_bytes, void *stream);
/* selection: how the nms_pre_max_size best cells of a task are found -- 0 automatic (an exact in-LDS top-K
 * selection where the map allows, else a full sort), 1 always the full stable radix sort of all cells (what the
 * reference does; the tests run both and require identical output). */

/* ---------------------------------------------------------------------------------------------
 * bevdet_postprocess -- BEVDet4D CenterHead post-processing on the device: CenterHeadMatch.get_bboxes
 * (paddle3d/models/heads/dense_heads/bevdet_centerhead.py:669-783) with CenterPointBBoxCoder.decode (:1119-1214),
 * Scale-NMS (get_task_detections :785-906, nms_bev :939-968) and circle NMS (:712-739).  All frames and tasks in
 * one launch sequence (6 launches), no host round trip inside.
 *
 *   heatmap/reg/height/dim/rot/vel: host arrays of `num_tasks` device pointers to contiguous fp32 NCHW maps:
 *     heatmap[t] [batch, task_classes[t], H, W], reg [batch,2,H,W], height [batch,1,H,W], dim [batch,3,H,W],
 *     rot [batch,2,H,W] (sine, cosine), vel [batch,2,H,W].  H * W <= 2^24, num_tasks <= 16, at most 64 classes.
 *   nms_type host int[num_tasks] (0 'rotate', 1 'circle'); nms_thr host float[num_tasks] (rotate tasks);
 *   min_radius host double[num_tasks] (circle tasks: compared with the SQUARED centre distance, as the reference);
 *   rescale_factors host float[sum(task_classes)]: nms_rescale_factor per class in label order (a scalar factor
 *     repeated over the task's classes; 1.0 where the reference's list is shorter; rotate tasks only, nonzero).
 *   max_num: coder top-K, 1..min(1024, H * W) (k > H * W raises in the reference's paddle.topk: PD3_EINVAL;
 *     1024 < k <= H * W: PD3_EUNSUPPORTED).  pre_max_size / post_max_size >= 1.
 *   score_threshold: 0 = none (the coder tests `if self.score_threshold:`), else score > threshold.
 *   post_center_range float[6] (coder), post_center_limit_range float[6] (test_cfg; NULL = no post-NMS mask),
 *   pc_range float[2], voxel_size float[2], out_size_factor.
 *   out_bboxes [batch, num_tasks * post_max_size, 9] fp32 (x, y, z of the box bottom, dims, rot, vx, vy)
 *   out_scores [batch, same rows] fp32; out_labels [batch, same rows] int32 (offset by the earlier tasks' classes)
 *   out_count  [batch] int32: valid leading rows per frame, tasks in order; rows behind it read zero.
 */
size_t pd3_bevdet_postprocess_workspace(int batch, int num_tasks, const int *task_classes, int feat_h, int feat_w,
                                        int max_num);
int pd3_bevdet_postprocess(const float *const *heatmap, const float *const *reg, const float *const *height,
                           const float *const *dim, const float *const *rot, const float *const *vel, int batch,
                           int num_tasks, const int *task_classes, int feat_h, int feat_w, const int *nms_type,
                           const float *nms_thr, const double *min_radius, const float *rescale_factors,
                           int max_num, int pre_max_size, int post_max_size, float score_threshold, int norm_bbox,
                           const float *post_center_range, const float *post_center_limit_range,
                           const float *pc_range, const float *voxel_size, float out_size_factor,
                           float *out_bboxes, float *out_scores, int32_t *out_labels, int32_t *out_count,
                           void *workspace, size_t workspace_bytes, void *stream);

/* circle_nms (paddle3d/geometries/bbox.py:450-474) on the device.  dets [n, 3] fp32 (x, y, score), device.
 * Greedy over descending score (equal scores: ascending index); j is suppressed by a kept i when
 * (x_i - x_j)^2 + (y_i - y_j)^2 (fp32) <= thresh (double).  keep [n] int32 receives the kept indices in order,
 * num_to_keep [1] int32 their number (both device).  n <= 65536. */
size_t pd3_circle_nms_workspace(int n);
int pd3_circle_nms(const float *dets, int n, double thresh, int32_t *keep, int32_t *num_to_keep, void *workspace,
                   size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * bevdet4d_align -- BEVDet4D temporal alignment: BEVDet4D.shift_feature for every adjacent frame and the channel
 * concat of its callers (paddle3d/models/detection/bevdet/bevdet4d.py:90-159, extract_img_feat_sequential
 * :194-216, extract_img_feat :291-298) in one launch, no host round trip.  fp32 only.
 *
 *   feats: host array of `num_frame` device pointers; feats[0] is the current frame (copied bit for bit), feats[1..]
 *     the adjacent frames.  Each is [batch, channels, feat_h, feat_w] with the element strides
 *     strides[4*f .. 4*f+3] = (n, c, h, w): contiguous NCHW and the channels-last view voxel_pooling_v2 returns are
 *     both read in place.  num_frame <= 16.  with_current 0: feats[0] is not read and the output holds the adjacent
 *     frames only (shift_feature itself).
 *   rots_cur / trans_cur / rots_adj / trans_adj / bda / bda_adj: host arrays of `num_frame - 1` device pointers, one
 *     per adjacent frame, each at camera 0 of batch entry 0: a [3, 3] rotation, a [3] translation, a [3, 3] bda,
 *     row-major and contiguous; entry b lies `pose_strides[6*(f-1) + k]` elements further (k = 0..5 in the order of
 *     the six arrays).  bda_adj NULL (or an entry NULL): bda for both poses.
 *   grid_interval / grid_lower_bound: host float[2] (x, y) of the view transformer (feat2bev); feat_h, feat_w >= 2.
 *   out [batch, (num_frame - 1 + with_current) * channels, feat_h, feat_w] contiguous; out_grid
 *     [(num_frame - 1) * batch, feat_h, feat_w, 2] (adjacent frame major) receives the normalised sampling grid,
 *     or NULL.
 *   tf is composed in double (closed-form inverse) and rounded to fp32 once; the per-pixel grid and the bilinear
 *   sum run in fp32 in the order documented in csrc/bev_shift.hip.  All offsets are 64-bit.
 */
int pd3_bevdet4d_align(const float *const *feats, const int64_t *strides, int num_frame, int with_current,
                       int batch, int channels, int feat_h, int feat_w, const float *const *rots_cur,
                       const float *const *trans_cur, const float *const *rots_adj, const float *const *trans_adj,
                       const float *const *bda, const float *const *bda_adj, const int64_t *pose_strides,
                       const float *grid_interval, const float *grid_lower_bound, float *out, float *out_grid,
                       void *stream);

/* ---------------------------------------------------------------------------------------------
 * ms_deform_attn / its gradient -- replace PD_BUILD_OP(ms_deform_attn) and PD_BUILD_GRAD_OP(ms_deform_attn)
 * (ms_deform_attn/ms_deform_attn.cc:85-101; kernels ms_deform_attn_cuda_kernel.h:37-84 bilinear sample, :86-151 its
 * gradient, :220-274 the forward loop).  BEVFormer's TemporalSelfAttention, MSDeformableAttention3D and
 * CustomMSDeformableAttention call it.
 *
 *   dtype: 0 float32, 1 float64 (every floating-point tensor of the call).
 *   value [batch, spatial_size, num_heads, channels]; spatial_shapes [num_levels, 2] int64 (H, W) and
 *     level_start_index [num_levels] int64, device memory, read by the kernels (no host round trip);
 *     sampling_loc [batch, num_query, num_heads, num_levels, num_point, 2] (x, y) in [0, 1];
 *     attn_weight [batch, num_query, num_heads, num_levels, num_point]; all contiguous.
 *   out [batch, num_query, num_heads * channels].
 *   The reference's im2col_step only slices the batch into launches; it does not change a result and is not a
 *   parameter here (one launch).  Value rows outside [0, spatial_size) (spatial_shapes / level_start_index that
 *   disagree with spatial_size) count as 0 and are never read; a level with H or W outside [1, 2^31 - 1] or
 *   |level_start_index| > 2^62 contributes nothing.  Arithmetic order: csrc/ms_deform_attn.hip.
 *   Backward: grad_out like out; writes grad_value (zeroed first, in stream order; float atomics: may differ in the
 *   last bits from run to run), grad_sampling_loc and grad_attn_weight (like their inputs; bitwise reproducible).
 *   PD3_EINVAL on dims < 1 (batch and num_query may be 0: nothing is launched, except the backward's zeroing of
 *   grad_value when num_query is 0) or a dtype other than 0 / 1.
 */
int pd3_ms_deform_attn_forward(int dtype, const void *value, const int64_t *spatial_shapes,
                               const int64_t *level_start_index, const void *sampling_loc, const void *attn_weight,
                               int batch, int spatial_size, int num_heads, int channels, int num_levels,
                               int num_query, int num_point, void *out, void *stream);
int pd3_ms_deform_attn_backward(int dtype, const void *value, const int64_t *spatial_shapes,
                                const int64_t *level_start_index, const void *sampling_loc, const void *attn_weight,
                                const void *grad_out, int batch, int spatial_size, int num_heads, int channels,
                                int num_levels, int num_query, int num_point, void *grad_value,
                                void *grad_sampling_loc, void *grad_attn_weight, void *stream);

/* ---------------------------------------------------------------------------------------------
 * pointnet2 batch ops and points_in_boxes -- what IA-SSD calls (csrc/pointnet2.hip).  fp32 only, int32 indices,
 * contiguous tensors; 64-bit offsets inside the kernels.  PD3_EINVAL on negative dims.
 *
 * farthest_point_sample -- replaces PD_BUILD_OP(farthest_point_sample) (pointnet2/sampling.cc:62, kernel
 * sampling_gpu.cu:37-149).  xyz [batch, n, 3] -> idxs [batch, m].
 *   Values: every minimum starts at 1e10 and is updated with fminf (a NaN distance never replaces it, a distance
 *   above 1e10 is clamped to 1e10, so far points tie at 1e10); distance ((dx*dx + dy*dy) + dz*dz), dx = x2 - x1.
 *   idxs[0] = 0.  m <= 0 writes nothing; m > n is legal and repeats indices under the same rule.  n = 0 with m > 0
 *   is PD3_EINVAL; n > 2^24 is PD3_EUNSUPPORTED.
 *   Ties: with bs = min(2^floor(log2 n), 1024) (the reference's opt_n_threads, sampling_gpu.cu:13-16), the winner
 *   among equal maximum distances is the point with the smallest (bitreverse_{log2 bs}(k mod bs), k) -- what the
 *   reference's per-thread strict > scan and its left-biased tree select; neither the smallest k nor the smallest
 *   k mod bs.  (bs = 4: 1 vs 2 goes to 2; bs = 1024: 3 vs 1025 goes to 1025, 1 vs 512 to 512.)
 *   tier: 0 auto, 1 register tier (n <= 16384, else PD3_EUNSUPPORTED: coordinates and minima in VGPRs, no spills),
 *   2 general tier (n <= 2^24: minima of the first 65536 points of a frame in VGPRs, the rest in the workspace;
 *   coordinates re-read from L2).  Auto picks the register tier for n <= 16384.  The workspace query returns the
 *   bytes the call needs (0 for the register tier and for n <= 65536); PD3_EWORKSPACE if it is short.
 */
size_t pd3_farthest_point_sample_workspace(int batch, int n, int tier);
int pd3_farthest_point_sample(const float *xyz, int batch, int n, int m, int tier, void *workspace,
                              size_t workspace_bytes, int *idxs, void *stream);

/* gather_operation / its gradient -- replace PD_BUILD_OP and PD_BUILD_GRAD_OP(gather_operation)
 * (pointnet2/gather_points.cc:100-110, kernels gather_points_gpu.cu:25, 69).
 *   points [batch, channels, n], idx [batch, npoints] -> out [batch, channels, npoints].
 *   An index outside [0, n) reads as 0 (the reference reads arbitrary memory) and adds nothing to the gradient.
 *   grad: grad_out [batch, channels, npoints] -> grad_points [batch, channels, n], zeroed first in stream order, then
 *   float atomic adds: the last bits may vary from run to run, as the reference's do.
 */
int pd3_gather_points(const float *points, const int *idx, int batch, int channels, int n, int npoints, float *out,
                      void *stream);
int pd3_gather_points_grad(const float *grad_out, const int *idx, int batch, int channels, int n, int npoints,
                           float *grad_points, void *stream);

/* ball_query_batch -- replaces PD_BUILD_OP(ball_query_batch) (pointnet2_batch/ball_query_batch.cc:61, kernel
 * ball_query_gpu_batch.cu:20-61).  new_xyz [batch, m, 3], xyz [batch, n, 3] -> idx [batch, m, nsample]: the first
 * nsample points in index order with ((new_x - x)^2 + (new_y - y)^2) + (new_z - z)^2 < radius * radius (fp32), the
 * unused slots filled with the first hit.  A row with no hit is 0 (the reference leaves paddle::empty memory there;
 * 0 is what OpenPCDet's batch op returns and keeps grouping in bounds).
 */
int pd3_ball_query_batch(const float *new_xyz, const float *xyz, int batch, int n, int m, float radius, int nsample,
                         int *idx, void *stream);

/* grouping_operation_batch / its gradient -- replace PD_BUILD_OP and PD_BUILD_GRAD_OP(grouping_operation_batch)
 * (pointnet2_batch/group_points_batch.cc:95-106, kernels group_points_gpu_batch.cu:25, 74).
 *   points [batch, channels, n], idx [batch, npoints, nsample] -> out [batch, channels, npoints, nsample].
 *   Indices outside [0, n) read as 0 and add nothing to the gradient.  grad: grad_out like out -> grad_points
 *   [batch, channels, n], zeroed first in stream order, then float atomic adds (last bits may vary run to run).
 */
int pd3_group_points_batch(const float *points, const int *idx, int batch, int channels, int n, int npoints,
                           int nsample, float *out, void *stream);
int pd3_group_points_batch_grad(const float *grad_out, const int *idx, int batch, int channels, int n, int npoints,
                                int nsample, float *grad_points, void *stream);

/* points_in_boxes_gpu -- replaces PD_BUILD_OP(points_in_boxes_gpu) (roiaware_pool3d/box_utils.cc:65, kernel
 * box_utils_gpu.cu:28-78).  pts [batch, npts, 3]; boxes rows (x, y, z, dx, dy, dz, heading), z at the centre, row k
 * of frame b at boxes + b * box_batch_stride + k * box_row_stride floats (box_row_stride >= 7: the [:, :, 0:7] slice
 * of an [B, M, 8] tensor is read in place) -> box_idx_of_points [batch, npts] int32: the first box in index order
 * that holds the point, -1 if none.  cosf / sinf(-heading) carry glibc's bits; |z - cz| > dz / 2.0 and
 * |local| < d / 2.0 + 1e-5f are evaluated in double, local_x / local_y in fp32 without FMA.  Boxes are staged in
 * LDS 256 at a time (any nboxes).
 */
int pd3_points_in_boxes(const float *pts, const float *boxes, int batch, int npts, int nboxes, int64_t box_row_stride,
                        int64_t box_batch_stride, int *box_idx_of_points, void *stream);

/* ---------------------------------------------------------------------------------------------
 * pointnet2 stack ops -- what PV-RCNN's StackSAModuleMSG and Voxel R-CNN's NeighborVoxelSAModuleMSG call
 * (csrc/pointnet2_stack.hip).  fp32 data, int32 indices and counts, contiguous tensors, 64-bit offsets inside the
 * kernels.  The batch counts stay on the device: nothing here synchronises with the host.  PD3_EINVAL on negative
 * dims, nsample < 1, or batch == 0 with rows to compute; m == 0 launches nothing.  batch > 256 is PD3_EUNSUPPORTED
 * (every workgroup holds the counts' prefix in LDS, one per thread).
 *   Frame of a row (ball query, grouping): the reference's scan (ball_query_gpu_stack.cu:37-42) -- the first
 *   k < batch - 1 with row < cnt[0] + ... + cnt[k], else batch - 1.  A frame with count 0 is never picked; rows past
 *   the total belong to frame batch - 1.  Sums are 64-bit (the reference's are int).
 *   Query rows: the first nsample hits in the op's order, unused slots repeat the first hit, a row with no hit is
 *   [-1, 0, 0, ...] (the reference fills paddle::full(0) and writes idx[0] = -1).  r2 = radius * radius in fp32.
 *
 * ball_query_stack -- replaces PD_BUILD_OP(ball_query_stack) (pointnet2_stack/ball_query_stack.cc:73, kernel
 * ball_query_gpu_stack.cu:26-81).  new_xyz [m, 3], new_xyz_batch_cnt [batch], xyz [n, 3], xyz_batch_cnt [batch] ->
 * idx [m, nsample], frame-local indices of the row's frame's points in index order with
 * ((new_x - x)^2 + (new_y - y)^2) + (new_z - z)^2 < r2 (a NaN distance is no hit).  Departure: the frame's point range
 * is computed with negative counts read as 0 and clamped into [0, n) (the reference reads outside xyz there);
 * consistent counts are unaffected.
 */
int pd3_ball_query_stack(const float *new_xyz, const int *new_xyz_batch_cnt, const float *xyz,
                         const int *xyz_batch_cnt, int batch, int m, int n, float radius, int nsample, int *idx,
                         void *stream);

/* voxel_query_wrapper -- replaces PD_BUILD_OP(voxel_query_wrapper) (pointnet2/voxel_query.cc:78, kernel
 * voxel_query_gpu.cu:11-93).  new_xyz [m, 3], xyz [n, 3], new_coords [m, 4] as (b, z, y, x), point_indices
 * [batch, z, y, x] -> idx [m, nsample]: rows of xyz, cells visited dz, then dy, then dx, each from -range to +range;
 * cells outside the grid and point_indices < 0 are skipped.  Hit: !(((x - new_x)^2 + (y - new_y)^2) + (z - new_z)^2
 * > r2) -- unlike the ball query, a point on the sphere and a NaN distance are hits.  The reference's cnt2 is unused
 * and its curand_init has no effect, so the scan stops at nsample hits with the same result.  Departures: a batch
 * index outside [0, batch) gives no hit and a point index >= n is skipped (both read out of bounds in the
 * reference).  A negative range is an empty window, as the reference's loops are.  A window over 2^31 - 65 cells is
 * PD3_EUNSUPPORTED.
 */
int pd3_voxel_query(const float *new_xyz, const float *xyz, const int *new_coords, const int *point_indices, int m,
                    int n, int batch, int z, int y, int x, float radius, int nsample, int z_range, int y_range,
                    int x_range, int *idx, void *stream);

/* grouping_operation_stack / its gradient -- replace PD_BUILD_OP and PD_BUILD_GRAD_OP(grouping_operation_stack)
 * (pointnet2_stack/group_points_stack.cc:117-130, kernels group_points_gpu_stack.cu:26-131).
 *   features [n, channels], features_batch_cnt [batch], idx [m, nsample] (frame-local), idx_batch_cnt [batch] ->
 *   out [m, channels, nsample], out[r, c, s] = features[start(frame(r)) + idx[r, s], c], start = the sum of the
 *   earlier frames' features_batch_cnt.  A global row outside [0, n) reads as 0 (the reference reads arbitrary
 *   memory) and adds nothing to the gradient.  grad: grad_out like out -> grad_features [n, channels], zeroed first in
 *   stream order, then float atomic adds (the last bits may vary from run to run, as the reference's do).
 */
int pd3_group_points_stack(const float *features, const int *features_batch_cnt, const int *idx,
                           const int *idx_batch_cnt, int batch, int n, int channels, int m, int nsample, float *out,
                           void *stream);
int pd3_group_points_stack_grad(const float *grad_out, const int *idx, const int *idx_batch_cnt,
                                const int *features_batch_cnt, int batch, int n, int channels, int m, int nsample,
                                float *grad_features, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Voxel R-CNN's RoI head (csrc/roi_head.hip): the fused voxel pool of NeighborVoxelSAModuleMSG, the RoI grid points,
 * class-agnostic NMS for a whole batch and the box decode of the second stage.  Inference only.  fp32 data, int32
 * indices, contiguous tensors, 64-bit offsets inside the kernels, no FMA, no float atomics; nothing here
 * synchronises with the host.
 *
 * voxel_pool -- the inner part of NeighborVoxelSAModuleMSG.forward (pointnet2_stack/voxel_pool_modules.py:123-155) for
 * one scale, from the voxel query to the pool, with no [m, *, nsample] tensor in global memory.  new_xyz [m, 3],
 * new_coords [m, 4] as (b, z, y, x), xyz [n, 3], point_indices [batch, z, y, x], features_in [n, c1] (the output of
 * mlps_in), w_pos [c1, 3], pos_scale / pos_shift [c1] (mlps_pos: the 1x1 conv weight and its BatchNorm in eval form,
 * scale = gamma / sqrt(var + eps), shift = beta - mean * scale), pool 0 max / 1 avg ->
 *   pooled [m, c1] = pool_s relu(features_in[idx[m, s]] + (pos_scale * ((w0 * dx + w1 * dy) + w2 * dz) + pos_shift))
 * with idx exactly pd3_voxel_query's row for the same arguments (unused slots repeat the first hit, so a repeated
 * slot takes part in an avg pool), d = xyz[idx] - new_xyz, and a row without a hit taking features = 0, d = 0 in all
 * nsample slots.  relu(v) = v > 0 ? v : +0 (a NaN stays).  avg: with G = 64 / c1, the slots s = g, g + G, ... are
 * summed in order for each g, the G sums by the tree (g0 + g1) + (g2 + g3), then divided by nsample.
 * Departure from the reference: idx is used as rows of xyz directly (the reference subtracts and re-adds the frame's
 * start; the same for consistent counts).  c1 not in {16, 32, 64} or nsample > 64: PD3_EUNSUPPORTED.
 */
int pd3_voxel_pool(const float *new_xyz, const float *xyz, const int *new_coords, const int *point_indices,
                   const float *features_in, const float *w_pos, const float *pos_scale, const float *pos_shift, int m,
                   int n, int batch, int z, int y, int x, int c1, float radius, int nsample, int z_range, int y_range,
                   int x_range, int pool, float *pooled, void *stream);

/* roi_grid_points -- RoIHeadBase.get_global_grid_points_of_roi + get_dense_grid_points (heads/roi_heads/
 * roi_head_base.py:324-346) and the coordinates of VoxelRCNNHead.roi_grid_pool (voxelrcnn_head.py:165-183, 227-230).
 * rois [num_rois, 7] (num_rois = frames * rois_per_frame) -> roi_grid_xyz [num_rois * G^3, 3] and, for each of
 * num_strides <= 4 strides, coords [num_strides][num_rois * G^3, 4] as (b, x, y, z) =
 * floor(floor((xyz - range_min) / voxel_size) / stride), b = roi / rois_per_frame; out of int32 range saturates, a
 * NaN is 0.  Grid point i of a RoI is (ix, iy, iz) = (i / G^2, i / G % G, i % G) (nonzero()'s order);
 * local = ((idx + 0.5) / G) * size - size / 2; rotation as the matmul's sums x' = (x * cos + y * (-sin)) + z * 0,
 * y' = (x * sin + y * cos) + z * 0, z' = (x * 0 + y * 0) + z * 1 with glibc's cosf / sinf; then + centre.
 * range_min, voxel_size [3] and strides are host arrays.
 */
int pd3_roi_grid_points(const float *rois, int64_t num_rois, int rois_per_frame, int grid_size, const float *range_min,
                        const float *voxel_size, const int *strides, int num_strides, float *roi_grid_xyz, int *coords,
                        void *stream);

/* rcnn_decode_boxes -- RoIHeadBase.generate_predicted_boxes (roi_head_base.py:293-322) with
 * ResidualCoder.decode_paddle (utils/box_coder.py:66-100, no sin / cos angle code, code size 7).  rois, box_preds
 * [n, 7] -> out [n, 7]: diag = sqrtf(dxa * dxa + dya * dya); (xg, yg, zg) = (xt * diag + 0, yt * diag + 0,
 * zt * dza + 0) rotated by the RoI's heading (the sums of roi_grid_points) + the RoI's centre; sizes expf(t) * a;
 * heading rt + ra.  expf / sinf / cosf carry glibc's bits.
 */
int pd3_rcnn_decode_boxes(const float *rois, const float *box_preds, int64_t n, float *out, void *stream);

/* class_agnostic_nms -- class_agnostic_nms (models/common/model_nms_utils.py:20-66) for a whole batch, as
 * RoIHeadBase.proposal_layer (roi_head_base.py:70-131) and VoxelRCNN.post_processing (detection/voxel_rcnn/
 * voxel_rcnn.py:145-220) call it.  box_preds [batch, num_boxes, 7], cls_preds [batch, num_boxes, num_classes],
 * labels [batch, num_boxes] int64 or NULL.  Per frame: score = max over the classes (first maximum wins) of cls or,
 * with apply_sigmoid, of 1 / (1 + expf(-cls)); rows with score >= score_thresh pass (a NaN score_thresh: all pass);
 * stable descending order (ties by index, -0 == +0, a NaN score first); the first nms_pre_maxsize; rotated NMS on the
 * 7 columns as they are (pd3_nms_bev's overlap, IoU > nms_thresh suppresses); the first nms_post_maxsize kept ->
 * boxes [batch, post, 7], scores [batch, post], labels [batch, post] int64 (the 0-based argmax, or labels' entry),
 * count [batch].  Rows behind count are zeros; under a score_thresh a frame that passes nothing gets the reference's
 * box_empty row (zero box, score -1, label -1) in row 0 and count 0.  nms_pre_maxsize, nms_post_maxsize >= 1;
 * nms_pre_maxsize > 65536 is PD3_EUNSUPPORTED.  The workspace query needs no GPU (0: shape not taken).
 */
size_t pd3_class_agnostic_nms_workspace(int batch, int64_t num_boxes, int nms_pre_maxsize);
int pd3_class_agnostic_nms(const float *box_preds, const float *cls_preds, int batch, int64_t num_boxes,
                           int num_classes, int apply_sigmoid, float score_thresh, const int64_t *labels,
                           int nms_pre_maxsize, float nms_thresh, int nms_post_maxsize, float *out_boxes,
                           float *out_scores, int64_t *out_labels, int32_t *out_count, void *workspace,
                           size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * PV-RCNN's keypoint branch and RoI head (csrc/pvrcnn.hip).  Inference only.  fp32 data, int32 counts, contiguous
 * tensors, 64-bit offsets inside the kernels, no float atomics; nothing here synchronises with the host.
 *
 * stack_sa_pool -- one scale of StackSAModuleMSG.forward (pointnet2_stack/pointnet2_modules.py:31-120) from the ball
 * query to the max pool, with no [m, *, nsample] tensor and no idx in global memory.  The scale's mlp is
 * Conv2d(3 + C -> c1) / BN / ReLU, Conv2d(c1 -> c2) / BN / ReLU; the first convolution is linear in [d; f], so the
 * caller passes features_in = features @ W1[:, 3:]^T ([n, c1], NULL reads as zeros) and w_pos = W1[:, :3].
 * new_xyz [m, 3], new_xyz_batch_cnt [batch], xyz [n, 3], xyz_batch_cnt [batch], w_pos [c1, 3], scale1 / shift1 [c1],
 * w2 [c2, c1], scale2 / shift2 [c2] (each BatchNorm in eval form, scale = gamma / sqrt(var + eps), shift = beta -
 * mean * scale, formed by the caller in fp32) -> pooled [m, c2]:
 *   h[s, j]      = relu(scale1[j] * (features_in[row_s, j] + ((w_pos[j,0] * dx + w_pos[j,1] * dy) + w_pos[j,2] * dz))
 *                       + shift1[j])                                                       (no FMA)
 *   pooled[m, c] = max_s relu(scale2[c] * (sum_j w2[c, j] * h[s, j]) + shift2[c])          (no FMA outside the sum)
 * with idx exactly pd3_ball_query_stack's row for the same arguments (the frame of a row, frame-local indices, the
 * first nsample hits in index order, d2 < r2, a NaN is no hit), row_s = start(frame) + idx[s], d = xyz[row_s] -
 * new_xyz.  A row without a hit takes features 0 and d 0: h[j] = relu(shift1[j]) (the reference's zeroed grouped
 * tensor).  The sum over j is an ascending-j fp32 fmaf chain from 0 (what v_mfma_f32_16x16x4_f32 computes), so the
 * result depends neither on the tiling nor on where a row sits in the launch.  The max runs over the hits only (unused
 * slots repeat slot 0).  relu(v) = v > 0 ? v : +0 (a NaN stays) and the max keeps a NaN, as in pd3_voxel_pool.
 * c1, c2 not in {16, 32, 64} or nsample > 64: PD3_EUNSUPPORTED; batch > 256 too.  PD3_EINVAL on negative dims,
 * nsample < 1, or batch == 0 with rows to compute; m == 0 launches nothing.
 */
int pd3_stack_sa_pool(const float *new_xyz, const int *new_xyz_batch_cnt, const float *xyz, const int *xyz_batch_cnt,
                      const float *features_in, const float *w_pos, const float *scale1, const float *shift1,
                      const float *w2, const float *scale2, const float *shift2, int batch, int m, int n, int c1,
                      int c2, float radius, int nsample, float *pooled, void *stream);

/* bev_interpolate -- VoxelSetAbstraction.interpolate_from_bev_features with bilinear_interpolate_paddle
 * (point_encoders/voxel_set_abstraction.py:32-67, 180-213) for all frames in one launch, reading the NCHW map in
 * place.  keypoints [m, 4] as (b, x, y, z), bev [batch, channels, h, w] -> out [m, channels]:
 *   xs = ((x - range_min_x) / voxel_x) / stride, ys likewise (true divisions, the reference's order);
 *   x0 = floor(xs), x1 = x0 + 1, both clipped to [0, w - 1] (y to [0, h - 1]) BEFORE the weights are formed;
 *   wa = (x1 - xs) * (y1 - ys), wb = (x1 - xs) * (ys - y0), wc = (xs - x0) * (y1 - ys), wd = (xs - x0) * (ys - y0);
 *   out = ((Ia * wa + Ib * wb) + Ic * wc) + Id * wd, Ia = bev[b, :, y0, x0], Ib = [y1, x0], Ic = [y0, x1],
 *   Id = [y1, x1].  No FMA.
 * Departures: a frame index that is no integer of [0, batch) gives a zero row (the reference drops the row); a floor
 * outside int32 saturates and a NaN is 0, as in pd3_roi_grid_points.  m * channels == 0 launches nothing.
 */
int pd3_bev_interpolate(const float *keypoints, const float *bev, int64_t m, int batch, int channels, int h, int w,
                        float range_min_x, float range_min_y, float voxel_x, float voxel_y, float stride, float *out,
                        void *stream);

/* ---------------------------------------------------------------------------------------------
 * assign_score_withk / its gradient -- replace PD_BUILD_OP and PD_BUILD_GRAD_OP(assign_score_withk)
 * (assign_score_withk/assign_score_withk_cuda.cc:265-274, CPU kernels :32-158): PAConv's weight-bank assembly
 * (csrc/assign_score_withk.hip).  fp32 data, int64 knn_idx, contiguous tensors, 64-bit offsets.
 *   scores [batch, n, k, m], points [batch, n, m, o], centers [batch, n, m, o], knn_idx [batch, n, k] ->
 *   output [batch, o, n]: for k, for m: acc = acc + points[b, kn, m, o] * s; acc = acc - centers[b, n, m, o] * s
 *   (kn = knn_idx[b, n, k], s = scores[b, n, k, m], the reference CPU kernel's order, no fma).
 *   Backward: grad_out like output -> grad_scores, grad_points, grad_centers like their inputs (each may be NULL to
 *   skip it); orders in csrc/assign_score_withk.hip.  No float atomics: every output is bitwise reproducible.
 *   Departures: kn outside [0, n) is range-tested as int64 and reads points as 0 (the forward still subtracts
 *   c * s; grad_points gets nothing) where the reference truncates it to int and reads out of bounds; offsets are
 *   64-bit; only fp32 (the reference's outputs are FLOAT32 whatever the input type); aggregate is SUM.
 *   k == 0 or m == 0 gives an all-zero output.  PD3_EINVAL on negative dims; batch * n * k >= 2^31 is
 *   PD3_EUNSUPPORTED, and so is a backward with batch > 65535.  Nothing synchronises with the host.
 *   The backward's workspace (pd3_assign_score_withk_backward_workspace; needs no GPU) holds grad_out transposed
 *   to [batch, n, o] and the inverse index of knn_idx (a stable radix sort per frame and segment starts).
 */
int pd3_assign_score_withk_forward(const float *scores, const float *points, const float *centers,
                                   const int64_t *knn_idx, int batch, int n, int k, int m, int o, float *output,
                                   void *stream);
size_t pd3_assign_score_withk_backward_workspace(int batch, int n, int k, int o);
int pd3_assign_score_withk_backward(const float *grad_out, const float *scores, const float *points,
                                    const float *centers, const int64_t *knn_idx, int batch, int n, int k, int m,
                                    int o, float *grad_scores, float *grad_points, float *grad_centers,
                                    void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * bev_pool_v2 / bev_pool_v2_bkwd -- replace PD_BUILD_OP(bev_pool_v2) (bev_pool_v2/bev_pool.cc:111-118,
 * kernel bev_pool_cuda.cu:18-44) and PD_BUILD_OP(bev_pool_v2_bkwd)
 * (bev_pool_v2_backward/bev_pool_bkwd.cc:75-80, kernel bev_pool_cuda_bkwd.cu:44-94).
 * `out` / grads are fully written (zero where no interval lands), fp32 accumulation in interval order.
 * n_points = length of the ranks_* arrays; the intervals tile [0, n_points).
 */
int pd3_bev_pool_v2(const float *depth, const float *feat, const int32_t *ranks_depth,
                    const int32_t *ranks_feat, const int32_t *ranks_bev,
                    const int32_t *interval_lengths, const int32_t *interval_starts,
                    int n_intervals, int channels, int64_t out_elems, float *out, void *stream);
int pd3_bev_pool_v2_bkwd(const float *out_grad, const float *depth, const float *feat,
                         const int32_t *ranks_depth, const int32_t *ranks_feat,
                         const int32_t *ranks_bev, const int32_t *interval_lengths,
                         const int32_t *interval_starts, int n_intervals, int64_t n_points,
                         int channels, int64_t depth_elems, int64_t feat_elems, float *depth_grad,
                         float *feat_grad, void *stream);

/* ---------------------------------------------------------------------------------------------
 * frustum_to_lidar -- LSSViewTransformer.get_lidar_coor (paddle3d/models/transformers/bevdet_transformer.py:
 * 142-192): ego-frame coordinates of every point of the camera frustums.
 *   frustum        [points_per_camera, 3] fp32 device: (u, v, depth) template of create_frustum (:126-140)
 *   inv_post_rots  [batch*num_cams, 3, 3]  inverse of the image-space augmentation rotation
 *   post_trans     [batch*num_cams, 3];  cam_to_ego [batch*num_cams, 3, 3] = rots @ inverse(cam2imgs)
 *   trans          [batch*num_cams, 3];  bda [batch, 3, 3]                (all fp32, device)
 *   coor           [batch*num_cams*points_per_camera, 3] fp32
 */
int pd3_frustum_to_lidar(const float *frustum, int64_t points_per_camera, int batch, int num_cams,
                         const float *inv_post_rots, const float *post_trans, const float *cam_to_ego,
                         const float *trans, const float *bda, float *coor, void *stream);

/* ---------------------------------------------------------------------------------------------
 * voxel_pooling_prepare -- the index build in front of bev_pool_v2, on the device: replaces
 * LSSViewTransformer.voxel_pooling_prepare_v2 (paddle3d/models/transformers/bevdet_transformer.py:230-274: quantise
 * every frustum point, keep the ones inside the grid, argsort by BEV rank, run-length encode into intervals) and
 * the same steps of LiftSplatShoot.voxel_pooling (models/detection/bevfusion/cam_stream_lss.py:318-346).
 *   coor           [num_points, 3] fp32 frustum points in the ego frame, num_points = B * N * D * H * W
 *   depth_bins, feat_hw   D and H * W (ranks_feat of mode 0 drops the depth axis)
 *   grid_lower / grid_interval / grid_size   host float[3] each, as the reference's float tensors
 *   mode 0 (BEVDet)  rank = b * (Z*Y*X) + z * (Y*X) + y * X + x;  ranks_feat = camera-pixel index
 *   mode 1 (LSS)     rank = ((b * Z + z) * X + x) * Y + y  (the cell of the reference's [B, Z, X, Y] output);
 *                    ranks_feat = point index
 *   mode 2 (LSS, split operands)  rank as mode 1, ranks_depth = point index, ranks_feat = camera-pixel index as
 *                    mode 0: pools depth [B*N, D, H, W] and feat [B*N, H, W, C] directly -- the lifted
 *                    depth (x) feat tensor of CamEncode.get_depth_feat (cam_stream_lss.py:166) is never formed
 *   ranks_bev / ranks_depth / ranks_feat [num_points] int32 (first counts[0] valid, sorted by rank, points of
 *   a cell in index order = a stable argsort), interval_starts / interval_lengths [num_points] int32 (first
 *   counts[1] valid), counts [2] int32 (device): kept points, intervals.
 * PD3_EUNSUPPORTED when batch * X * Y * Z exceeds 2^31: every cell id must fit the int32 ranks_bev (a larger grid
 * would come back with negative ranks).  A grid of exactly 2^31 cells is served.
 */
size_t pd3_voxel_pooling_prepare_workspace(int64_t num_points);
int pd3_voxel_pooling_prepare(const float *coor, int64_t num_points, int batch, int depth_bins, int feat_hw,
                              const float *grid_lower, const float *grid_interval, const float *grid_size, int mode,
                              int32_t *ranks_bev, int32_t *ranks_depth, int32_t *ranks_feat,
                              int32_t *interval_starts, int32_t *interval_lengths, int32_t *counts, void *workspace,
                              size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * sparse_conv3d -- replaces the Paddle-core sparse ops the CenterPoint-Voxel middle encoder is built
 * from: paddle.sparse.nn.SubmConv3D / Conv3D (+ BatchNorm, ReLU, sparse.add fused into the epilogue) and
 * SparseCooTensor.to_dense (call sites paddle3d/models/middle_encoders/sparse_resnet.py:31-59, :115-206;
 * sparsenet.py:31-64).  The reference arithmetic is in the paddlepaddle wheel (>= 2.4.0, not vendored):
 * parity is pinned on the public definition against a dense conv3d oracle.
 *
 * A convolution = pd3_sparse_conv3d_indices (output coordinate set + neighbour table; reusable by every
 * conv that shares the same input set, kernel, stride and padding -- the reference's `key=` hint) followed
 * by pd3_sparse_conv3d_features (gather-GEMM with fused epilogue).
 *   in_coords  [n_in, 4] int32 (batch, z, y, x); rows with batch < 0 are padding and ignored
 *   spatial_shape host int[3] (D, H, W);  kernel_size / stride / padding host int[3]
 *   subm != 0: output set = input set (same rows, same order); requires stride 1, padding = k/2
 *   subm == 0: output set = every position reached by an active input, rows sorted by (b, z, y, x)
 *   out_coords [out_cap, 4], nbr [out_cap, kd*kh*kw] int32 (input row or -1), n_out [1] int32 (device);
 *   rows at or past *n_out of out_coords / nbr -- and of every feature matrix computed through them with that n_out --
 *   are unspecified (a caller slices by the count).  subm != 0: *n_out = n_in and every row is written; the row of a
 *   padding input holds out_coords = the input row, nbr = -1 throughout, and its features are the epilogue of an empty
 *   sum.
 *   weight [kd, kh, kw, Cin, Cout] (Paddle layout); bias / scale+shift / residual may be NULL
 *   out = relu?( (sum_k W[k].in[nbr[.,k]] + bias) * scale + shift + residual ),  Cout <= 128
 */
size_t pd3_sparse_conv3d_workspace(int n_in, const int *kernel_size, int subm, int out_cap);
int pd3_sparse_conv3d_indices(const int32_t *in_coords, int n_in, int batch, const int *spatial_shape,
                              const int *kernel_size, const int *stride, const int *padding, int subm,
                              int32_t *out_coords, int32_t *nbr, int32_t *n_out, int out_cap,
                              void *workspace, size_t workspace_bytes, void *stream);
int pd3_sparse_conv3d_features(const float *in_feats, const int32_t *nbr, const int32_t *n_out,
                               int n_out_cap, int kernel_volume, int cin, int cout,
                               const float *weight, const float *bias, const float *scale,
                               const float *shift, const float *residual, int relu, float *out,
                               void *stream);
/* Tile order (a scheduling hint, never a change of results): the rows of every window of 8192 consecutive output
 * rows sorted by their neighbour mask, so that the 16-row blocks of the gather-GEMM hold rows that need the same
 * kernel offsets (a block runs an offset if ANY of its rows has that neighbour: 1.3x - 7x more steps than pairs
 * exist with rows in raster order, 1.2x - 2x in tile order).
 *   order [pd3_sparse_tile_order_entries(n_out_cap)] int32: slot -> output row, -1 past the row count
 *   n_out may be NULL (= n_out_cap); kernel_volume <= 31
 * pd3_sparse_conv3d_features_ordered = pd3_sparse_conv3d_features taking `order` (NULL: raster order); same bytes
 * out for any order. */
int64_t pd3_sparse_tile_order_entries(int n_out_cap);
int pd3_sparse_tile_order(const int32_t *nbr, const int32_t *n_out, int n_out_cap, int kernel_volume,
                          int32_t *order, void *stream);
int pd3_sparse_conv3d_features_ordered(const float *in_feats, const int32_t *nbr, const int32_t *n_out,
                                       int n_out_cap, int kernel_volume, int cin, int cout,
                                       const float *weight, const float *bias, const float *scale,
                                       const float *shift, const float *residual, int relu,
                                       const int32_t *order, float *out, void *stream);
/* The fp32 gather-GEMM on the bf16 matrix cores (round 5; the default of the fp32 encoder from 16 -> 32 channels on): every
 * fp32 operand is cut into three bf16 pieces (hi + mid + lo = the fp32 value exactly: 3 x 8 significand bits) and six of
 * the nine piece products are accumulated in fp32 (the three dropped ones: <= 2^-23 of a product, 2^-28 on average) -- the error against exact arithmetic is that of the fp32 matrix-core kernel
 * (tests/test_sparse_conv_gpu.py::test_features_bf16x3_is_fp32_arithmetic), the rate 2.7 x the fp32 pipe's.
 *   pd3_sparse_pack_weight_bf16x3       weight [K, Cin, Cout] fp32 (Paddle layout) -> 3 * K * Cin * Cout bf16 in the
 *                                       kernel's operand order; Cin % 16 == 0, Cout in {32, 64, 128}
 *   pd3_sparse_conv3d_features_bf16x3   as pd3_sparse_conv3d_features_ordered (all fp32 rows in and out) with that
 *                                       packed weight.  Other shapes return -3 (run the fp32 entry). */
int pd3_sparse_pack_weight_bf16x3(const float *weight, int kernel_volume, int cin, int cout, void *packed, void *stream);
int pd3_sparse_conv3d_features_bf16x3(const float *in_feats, const int32_t *nbr, const int32_t *n_out, int n_out_cap,
                                      int kernel_volume, int cin, int cout, const void *weight_packed,
                                      const float *bias, const float *scale, const float *shift, const float *residual,
                                      int relu, const int32_t *order, float *out, void *stream);
/* Mixed precision (the reference's amp_cfg level O2 for the CenterPoint-Voxel encoder): fp16 feature rows and weights
 * on the fp16 matrix cores, fp32 accumulation; index sets, rulebooks and tile order are the fp32 path's.
 *   pd3_sparse_pack_weight_f16   weight [K, Cin, Cout] fp32 (Paddle layout) -> packed fp16 (K * Cin * Cout halfs) in the
 *                                operand order of the kernel; Cin % 16 == 0, Cout in {32, 64, 128}
 *   pd3_sparse_conv3d_features_f16   as pd3_sparse_conv3d_features_ordered with in_feats / residual / out fp16
 *                                (out fp32 when out_f32 != 0: the encoder's last layer feeds pd3_sparse_to_dense);
 *                                bias / scale / shift stay fp32.  Other shapes return -3 (run the fp32 entry). */
int pd3_sparse_pack_weight_f16(const float *weight, int kernel_volume, int cin, int cout, void *packed, void *stream);
int pd3_sparse_conv3d_features_f16(const void *in_feats_f16, const int32_t *nbr, const int32_t *n_out, int n_out_cap,
                                   int kernel_volume, int cin, int cout, const void *weight_packed_f16,
                                   const float *bias, const float *scale, const float *shift,
                                   const void *residual_f16, int relu, const int32_t *order, void *out, int out_f32,
                                   void *stream);
/* The same kernel as a general gather-GEMM: out[row, out_off + co] = epilogue(sum_k W[k] . in[nbr[row, k]]) into a
 * channel slice of a wider row-major matrix (row stride out_ld).  Under AMP the FPN levels of SecondFPN
 * (paddle3d/models/necks/second_fpn.py:99-157: kernel = stride convolutions / transposed convolutions) are this with a
 * static neighbour table over the pixels of an fp16 NHWC map, each level writing its slice of the concatenated map. */
int pd3_gather_gemm_f16(const void *in_feats_f16, const int32_t *nbr, const int32_t *n_out, int n_out_cap,
                        int kernel_volume, int cin, int cout, const void *weight_packed_f16, const float *bias,
                        const float *scale, const float *shift, const void *residual_f16, int relu,
                        const int32_t *order, void *out, int out_f32, int out_ld, int out_off, void *stream);
/* Plan path: the index sets of a whole encoder without a host round trip between the convolutions (the
 * reference's layers read nnz on the host after every sparse op).  An index set is a SORTED array of keys
 * ((b*D + z)*H + y)*W + x (raster order; 0xFFFFFFFF = padding, at the end) with its length in device memory.
 *   pd3_sparse_sort_coords   coords [n, 4] (rows with batch < 0 are padding) -> keys_sorted [n], order [n]
 *                            (keys_sorted[i] belongs to input row order[i]), n_valid [1]
 *   pd3_sparse_conv_outputs  the output set of a regular convolution: every position an active input reaches
 *                            (paddle.sparse.nn.Conv3D), sorted; n_in / n_out are device counts, out_cap >= the
 *                            number of outputs (min(n_in_cap * prod(ceil(k/s)), batch * D' * H' * W') always is)
 *   pd3_sparse_rulebook      nbr [n_out_cap, kd*kh*kw] (input row or -1) and, if out_coords != NULL, the (b, z,
 *                            y, x) rows of the output set; in_keys / out_keys as produced above (subm != 0: pass
 *                            the same array twice); n_in / n_out may be NULL (= the caps).  A neighbour is looked
 *                            up by a binary search inside its (b, z, y) line of the sorted input array.
 * Workspaces: pd3_sparse_plan_workspace(n) for the sort, pd3_sparse_conv_outputs_workspace (a byte map of the
 * output grid) and pd3_sparse_rulebook_workspace (first row of every (b, z, y) line of the input set). */
size_t pd3_sparse_plan_workspace(int n_cap);
size_t pd3_sparse_conv_outputs_workspace(int batch, const int *spatial_shape, const int *kernel_size,
                                         const int *stride, const int *padding);
int pd3_sparse_sort_coords(const int32_t *coords, int n, int batch, const int *spatial_shape,
                           uint32_t *keys_sorted, int32_t *order, int32_t *n_valid, void *workspace,
                           size_t workspace_bytes, void *stream);
int pd3_sparse_conv_outputs(const uint32_t *in_keys, const int32_t *n_in, int n_in_cap, int batch,
                            const int *spatial_shape, const int *kernel_size, const int *stride,
                            const int *padding, uint32_t *out_keys, int32_t *n_out, int out_cap,
                            void *workspace, size_t workspace_bytes, void *stream);
size_t pd3_sparse_rulebook_workspace(int batch, const int *spatial_shape);  /* spatial_shape of the INPUT set */
int pd3_sparse_rulebook(const uint32_t *in_keys, const int32_t *n_in, int n_in_cap, const uint32_t *out_keys,
                        const int32_t *n_out, int n_out_cap, int batch, const int *spatial_shape,
                        const int *kernel_size, const int *stride, const int *padding, int subm, int32_t *nbr,
                        int32_t *out_coords, void *workspace, size_t workspace_bytes, void *stream);
/* values [n, C] at coords -> dense [batch, C*D, H, W] fp32 (to_dense + transpose + reshape of
 * sparse_resnet.py:202-205); `dense` is fully written (zero where inactive). n may be NULL (= n_cap). */
int pd3_sparse_to_dense(const float *feats, const int32_t *coords, const int32_t *n, int n_cap,
                        int channels, int batch, const int *spatial_shape, float *dense, void *stream);

/* ---------------------------------------------------------------------------------------------
 * merge_sweeps -- the caller-side step right before hard_voxelize on the nuScenes path:
 * LoadPointCloud.__call__'s multi-sweep merge, paddle3d/transforms/reader.py:118-164.
 *   points         [sweep_offsets[num_sweeps], dim_in] fp32: key frame first, then the sweeps (device)
 *   sweep_offsets  host int64[num_sweeps + 1]; sweep 0 is the key frame (kept untouched)
 *   ref_from_curr  host double[num_sweeps][16] row-major 4x4 (NULL: no transform); has_transform host
 *                  int32[num_sweeps] (NULL: every sweep has one; 0 = this sweep's `ref_from_curr` is None,
 *                  reader.py:150, e.g. the key frame repeated as padding at a scene start); time_lag host
 *                  float[num_sweeps] (NULL: zeros); remove_radius = sweep_remove_radius
 *   out            [<= total points, use_dim (+1 if use_time_lag)] fp32, rows in the reference's
 *                  concatenation order (given the sweep order); num_out [1] int32 (device); allocate
 *                  total points rows, rows at or past *num_out are unspecified
 */
size_t pd3_merge_sweeps_workspace(int64_t num_points);
int pd3_merge_sweeps(const float *points, const int64_t *sweep_offsets, int num_sweeps, int dim_in,
                     int use_dim, const double *ref_from_curr, const int32_t *has_transform,
                     const float *time_lag, int use_time_lag,
                     float remove_radius, float *out, int32_t *num_out, void *workspace,
                     size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * conv3x3_bias_relu -- dense 3x3 / pad 1 convolution, stride 1 or 2, with fused bias and ReLU on the fp32
 * matrix cores: the convolutions of SecondBackbone (paddle3d/models/backbones/second_backbone.py:72-120)
 * and CenterHead / SeparateHead (detection/centerpoint/center_head.py:43-220) with BatchNorm folded into
 * weight and bias (cuDNN convolutions in the reference).
 *   x [batch, cin, h, w] fp32 NCHW (16-byte aligned);  out [batch, cout, h/stride, out_w];  bias [cout] or NULL
 *   w_packed: the [cout, cin, 3, 3] weight re-ordered to [cout/64][cin/8][4 channel pairs][9 taps][2][64]
 *             (row = (pair*9 + ky*3 + kx)*2 + channel-of-pair; see paddle3d_amd/ops/conv.py)
 *   w / w_valid / out_w: maps whose width is not a multiple of 4 (CenterPoint-Voxel's 90 x 90 stage) live in rows
 *             padded with zeros to a multiple of 4: w is the row pitch of x, w_valid <= w its real width (columns
 *             >= w_valid hold zeros), out_w >= w_valid / stride the row pitch of out, whose columns >=
 *             w_valid / stride are written as zeros -- the next layer reads them as its own zero padding.
 *             Ordinary maps: w_valid = w, out_w = w / stride.
 *   requires cin % 8 == 0, cout % 64 == 0, h and w_valid multiples of stride, w % 4 == 0, out_w % 4 == 0 (rows
 *   are staged as aligned float4); otherwise PD3_EUNSUPPORTED.  Outputs that are not a multiple of the 4 x 32
 *   pixel tile get partial border tiles (masked stores).
 */
int pd3_conv3x3_bias_relu(const float *x, const float *w_packed, const float *bias, int batch, int cin,
                          int cout, int h, int w, int w_valid, int stride, int relu, float *out, int out_w,
                          void *stream);

/* ---------------------------------------------------------------------------------------------
 * conv3x3_winograd43_bias_relu -- the same stride-1 convolution by Winograd F(4x4, 3x3) (4x fewer multiplies;
 * all fp32; ~1e-5 absolute from the direct form for |y| ~ 1).  One fused kernel.
 *   x [batch, cin, h, w] fp32 NCHW (16-byte aligned);  out [batch, cout, h, w] (16-byte aligned);  bias or NULL
 *   channels_per_tile: 32 or 64 output channels per workgroup (64: one 512-thread workgroup per CU, half the
 *             patch-transform work per MFMA; 32: two 256-thread workgroups per CU, for cout % 64 != 0)
 *   u_packed: U = G g G^T (6x6) of the [cout, cin, 3, 3] weight, packed [cout/T][cin/4][T/16][4][16][36] for
 *             T = channels_per_tile (16-channel block, input channel, channel, component xi*6+nu;
 *             paddle3d_amd/ops/conv.py:pack_winograd43_weight)
 *   w / w_valid: row pitch of x and out, and the real width (see conv3x3_bias_relu); w_valid = w for ordinary maps
 *   requires cin % 4 == 0, cout % T == 0, w % 4 == 0 (any h; partial 8 x 64 tiles at the border are masked)
 */
int pd3_conv3x3_winograd43_bias_relu(const float *x, const float *u_packed, const float *bias, int batch,
                                     int cin, int cout, int h, int w, int w_valid, int relu, float *out,
                                     int channels_per_tile, void *stream);

/* conv3x3_winograd43_pp_bias_relu -- the same convolution, same F(4x4, 3x3) arithmetic, as a two-group ping-pong kernel
 * whose multiply waves issue only MFMAs and LDS reads; U and the raw input rows reach LDS by buffer_load ... lds.
 *   u_lane: U = G g G^T of the [cout, cin, 3, 3] weight in lane order, [cout/64][cin/8][2 trips][4 blocks][9][64 lanes][4]:
 *           lane l of block cb holds channel 64 ct + 16 cb + (l & 15), input channel 8 slot + 4 trip + (l >> 4), float4 q =
 *           components 4q .. 4q+3 of xi*6+nu (paddle3d_amd/ops/conv.py:pack_winograd43_lane_weight); 16-byte aligned
 *   requires cin % 8 == 0, cout % 64 == 0, w % 4 == 0; the same U values as the packed form give the same sums up to the
 *   order of accumulation over input channels (identical here: ascending) */
int pd3_conv3x3_winograd43_pp_bias_relu(const float *x, const float *u_lane, const float *bias, int batch, int cin,
                                        int cout, int h, int w, int w_valid, int relu, float *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * conv3x3_winograd43_ppv_bias_relu -- conv3x3_winograd43_pp_bias_relu for a layer with many output-channel blocks over
 * one input (CenterHead's 36 first-stage convolutions as one 64 -> 2304 layer, center_head.py:99-118): the input transform
 * V = B^T d B is computed ONCE by pd3_winograd43_input_transform and fetched by the convolution instead of being redone
 * by each of its cout / 64 channel blocks (csrc/conv_winograd43_ppv.hip).  Same u_lane, same arguments otherwise, the
 * same bytes out as the pp form.
 *   v_pre: pd3_winograd43_input_transform_floats(batch, cin, h, w) floats (16-byte aligned), [pixel tile][cin / 8][tile
 *          row 2][ci 8][tile 16][36]; cin % 8 == 0 (0 floats / PD3_EUNSUPPORTED otherwise)
 */
size_t pd3_winograd43_input_transform_floats(int batch, int cin, int h, int w);
int pd3_winograd43_input_transform(const float *x, int batch, int cin, int h, int w, int w_valid, float *v_pre,
                                   void *stream);
int pd3_conv3x3_winograd43_ppv_bias_relu(const float *v_pre, const float *u_lane, const float *bias, int batch, int cin,
                                         int cout, int h, int w, int w_valid, int relu, float *out, void *stream);
/* measurement hook: + cycle counters of one workgroup (blockIdx 8), dbg int64 [8 waves][4] (device): transform /
 * multiply / barrier-wait / kernel cycles (the last with the SIMD id in bits 56+; tools/prof/prof_wino_trace.py) */
int pd3_conv3x3_winograd43_pp_trace(const float *x, const float *u_lane, const float *bias, int batch, int cin, int cout,
                                    int h, int w, int relu, float *out, long long *dbg, void *stream);

/* ---------------------------------------------------------------------------------------------
 * stable_argsort -- the index order the host glue of two reference functions needs, on the library's radix sort:
 * rotate_nms_pcdet's `paddle.argsort(scores, descending=True)` (models/layers/layer_libs.py:230-236) and the re-sort
 * by ranks_feat in front of bev_pool_v2_bkwd (models/transformers/bevdet_transformer.py:60-68).  Stable: equal keys
 * keep their input order.
 *   mode 0: keys int32 >= 0 (max_key bounds them: fewer passes), ascending;  mode 1: keys fp32, descending
 *   order [n] int32 (device);  workspace: pd3_stable_argsort_workspace(n, max_key) bytes
 */
size_t pd3_stable_argsort_workspace(int64_t n, uint32_t max_key);
int pd3_stable_argsort(const void *keys, int64_t n, int mode, uint32_t max_key, int32_t *order, void *workspace,
                       size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * conv3x3_f16_bias_relu -- the stride-1 3x3 / pad 1 convolutions of SecondBackbone and CenterHead in MIXED PRECISION:
 * fp16 activations and weights on the fp16 matrix cores, fp32 accumulation, bias + ReLU fused.  The reference's AMP
 * configuration of the model (configs/centerpoint/centerpoint_pillars_02voxel_nuscenes_10sweep_ampO2_ultra.yml:5-9,
 * `amp_cfg: level O2`, cuDNN fp16 convolutions there); an option of the host classes (`model.set_amp(True)`), never the
 * fp32 default.
 *   x            [batch, h, w, cin] fp16 NHWC (16-byte aligned; pd3_f32_nchw_to_f16_nhwc makes it from an fp32 map)
 *   w_packed_f16 [cout / T][cin / 16][9 taps (dy * 3 + dx)][2 halves][T][8] fp16, T = channels_per_tile: element
 *                (ct, c, t, kh, co, e) = W[ct T + co][16 c + 8 kh + e][dy][dx] -- a 16-channel sub-chunk of a channel tile
 *                is one contiguous piece in exactly its LDS order (round 6; paddle3d_amd/ops/conv.py:
 *                pack_conv3x3_f16_weight), bias [cout] fp32 or NULL
 *   out          out_mode 0: [batch, h, w, cout] fp16 NHWC (the next fp16 layer's input);
 *                out_mode 1: [batch, cout, h, w] fp32 NCHW (what the fp32 kernels of the graph read)
 *                out_mode 3: [batch, cout / 64, h, w, 64] fp16 "group-major" (round 6): the 64 channels of each branch of
 *                            the head pixel after pixel -- what pd3_grouped_conv3x3_small_f16_gm reads
 *   channels_per_tile 128 or 64 (workgroup = T channels x 16 rows x 32 columns, walking several (pixel tile, channel
 *                tile) items)
 *   requires cin % 16 == 0, cout % T == 0; else PD3_EUNSUPPORTED (the caller runs fp32).  Maps that are not whole
 *   tiles (config 4's 180 x 180) run with masked border tiles.
 */
int pd3_conv3x3_f16_bias_relu(const void *x_f16_nhwc, const void *w_packed_f16, const float *bias, int batch, int cin,
                              int cout, int h, int w, int relu, void *out, int out_mode, int channels_per_tile,
                              void *stream);
/* out_mode "both": a block's last stride-1 layer under AMP leaves fp16 NHWC (the next block's stride-2 convolution reads
 * it) AND fp32 NCHW (the FPN level reads it) in one pass.  Arguments as pd3_conv3x3_f16_bias_relu. */
int pd3_conv3x3_f16_bias_relu_dual(const void *x_f16_nhwc, const void *w_packed_f16, const float *bias, int batch,
                                   int cin, int cout, int h, int w, int relu, void *out_f16_nhwc, float *out_f32_nchw,
                                   int channels_per_tile, void *stream);
/* The stride-2 3x3 / pad 1 convolutions that open SecondBackbone's blocks (second_backbone.py:84-113) under AMP:
 * x [batch, h, w, cin] fp16 NHWC -> out [batch, (h - 1) / 2 + 1, (w - 1) / 2 + 1, cout] fp16 NHWC; weights packed as for
 * pd3_conv3x3_f16_bias_relu with T = 128; cin % 16 == 0, cout % 128 == 0 (else -3: the caller runs the fp32 kernel). */
int pd3_conv3x3_s2_f16_bias_relu(const void *x_f16_nhwc, const void *w_packed_f16, const float *bias, int batch, int cin,
                                 int cout, int h, int w, int relu, void *out_f16_nhwc, void *stream);
/* PointPillarsScatter fused into that stride-2 convolution (the layer that opens SecondBackbone's block 0 under AMP, the
 * fp16 sibling of pd3_scatter_conv3x3_bias_relu): features_f16 [M, cin] fp16 pillar features, inverse_map [batch, ny * nx]
 * int32 (pd3_pointpillars_inverse_map: pillar row of a cell or -1) -> out [batch, ny / 2, nx / 2, cout] fp16 NHWC; the
 * canvas is never written.  channels_per_tile 64 or 128 (weights packed with that T), cin % 16 == 0. */
int pd3_scatter_conv3x3_s2_f16_bias_relu(const void *features_f16, const int32_t *inverse_map, const void *w_packed_f16,
                                         const float *bias, int batch, int cin, int cout, int ny, int nx, int relu,
                                         void *out_f16_nhwc, int channels_per_tile, void *stream);
/* The final SeparateHead convolutions under AMP (center_head.py:99-118): grouped 3x3 / pad 1 convolution + bias reading
 * the first stage's fp16 NHWC output.
 *   x_f16_nhwc [batch, h, w, groups * 64] fp16; w_f16 [groups][9 taps][out_per_group][64] fp16; bias [groups *
 *   out_per_group] fp32 or NULL; out [batch, out_groups * out_per_group, h, w] fp32 NCHW, the slice's maps at groups
 *   [out_group0, out_group0 + groups); out_per_group 1 .. 4, 64 channels per group (else -3) */
int pd3_grouped_conv3x3_small_f16(const void *x_f16_nhwc, const void *w_f16, const float *bias, int batch, int groups,
                                  int channels_per_group, int out_per_group, int h, int w, float *out, int out_groups,
                                  int out_group0, void *stream);
/* The same convolution on the group-major form of the first stage's output (out_mode 3 of pd3_conv3x3_f16_bias_relu):
 * x [batch, groups, h, w, 64] fp16.  A group's patch rows are contiguous there -- in NHWC its pixels lie groups * 128 bytes
 * apart and the fetch of a tile runs at a third of the rate of contiguous lines.  Persistent kernel, patches by LDS-DMA
 * with the XOR swizzle done by the fetch (csrc/conv_f16.hip).  Same arguments, same results bit for bit; the input below
 * 2 GB (else -3). */
int pd3_grouped_conv3x3_small_f16_gm(const void *x_f16_group_major, const void *w_f16, const float *bias, int batch,
                                     int groups, int channels_per_group, int out_per_group, int h, int w, float *out,
                                     int out_groups, int out_group0, void *stream);
/* x [batch, channels, h, w] fp32 NCHW -> out [batch, h, w, channels] fp16 NHWC (round to nearest even) */
int pd3_f32_nchw_to_f16_nhwc(const float *x, int batch, int channels, int h, int w, void *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * grouped_conv3x3_small -- grouped 3x3 / stride 1 / pad 1 convolution with 1..4 output channels per group and
 * bias, no activation: the final convolutions of all SeparateHead branches (center_head.py:99-118) as one
 * launch over the concatenated first-stage maps.
 *   x [batch, groups*cin_per_group, h, w];  out [batch, groups*cout_per_group, h, w];  bias [groups*cout_per_group] or NULL
 *   w_grouped: [groups][cin_per_group][cout_per_group][9] (the [groups*cout, cin, 3, 3] weight with the two
 *              channel axes swapped inside each group)
 *   requires cin_per_group % 4 == 0, w % 4 == 0 (any h; partial 8 x 128 tiles at the border are masked)
 */
int pd3_grouped_conv3x3_small(const float *x, const float *w_grouped, const float *bias, int batch, int groups,
                              int cin_per_group, int cout_per_group, int h, int w, float *out, void *stream);
/* The same over a SLICE of the groups: x, w_grouped and bias describe `groups` consecutive groups, whose outputs land
 * at groups [out_group0, out_group0 + groups) of out [batch, out_groups*cout_per_group, h, w].  CenterHead runs its
 * 36 branches a few at a time this way, so that a slice's first-stage map (67 MB per branch and 16 frames) is read
 * back while it is still in the last-level cache instead of after 2.4 GB have gone by. */
int pd3_grouped_conv3x3_small_slice(const float *x, const float *w_grouped, const float *bias, int batch, int groups,
                                    int cin_per_group, int cout_per_group, int h, int w, float *out, int out_groups,
                                    int out_group0, void *stream);
/* The slice form for groups whose real output-channel counts differ: group g has group_couts[g] real channels (1 ..
 * cout_per_group; a HOST array of `groups` ints, at most 64, copied into the kernel's arguments -- no device memory, the
 * launch can be captured in a graph).  Weights, bias and out keep the padded layout of the slice form (cout_per_group
 * channels per group); a workgroup multiplies its group's real channels only and stores +0.0 to the padded ones, so every
 * byte of the slice is written and equals what pd3_grouped_conv3x3_small_slice writes for zero padded weights and bias
 * (finite inputs).  The input tile reaches LDS by buffer_load ... lds, double-buffered.
 *   requires also groups <= 64 and 4 * h * w < 2^29 (else -3) */
int pd3_grouped_conv3x3_small_counts_slice(const float *x, const float *w_grouped, const float *bias, int batch, int groups,
                                           int cin_per_group, int cout_per_group, const int *group_couts, int h, int w,
                                           float *out, int out_groups, int out_group0, void *stream);

/* ---------------------------------------------------------------------------------------------
 * conv3x3_winograd_bias_relu -- the same stride-1 convolution as conv3x3_bias_relu computed by Winograd
 * F(2x2, 3x3) on the fp32 matrix cores (2.25x fewer multiplies, all fp32; results differ from the direct
 * form by fp32 rounding only, ~1e-6 relative).  One fused kernel: input transform, 16 GEMMs, output transform.
 *   x [batch, cin, h, w] fp32 NCHW (16-byte aligned);  out [batch, cout, h, w];  bias [cout] or NULL
 *   u_packed: U = G g G^T of the [cout, cin, 3, 3] weight, packed [cout/32][cin/8][2][8][16][16]
 *             (16-channel block, input channel, channel, component xi*4+nu; see paddle3d_amd/ops/conv.py)
 *   requires cin % 8 == 0, cout % 32 == 0, w % 4 == 0 (any h; partial 8 x 32 tiles at the border are masked)
 */
int pd3_conv3x3_winograd_bias_relu(const float *x, const float *u_packed, const float *bias, int batch,
                                   int cin, int cout, int h, int w, int relu, float *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * patch_conv_bias_relu -- the non-overlapping-patch convolutions of SecondFPN (paddle3d/models/necks/
 * second_fpn.py:99-157; Conv2D / Conv2DTranspose with kernel = stride, BatchNorm folded) as one fp32-MFMA
 * GEMM with bias + ReLU, written at a channel offset of a wider output tensor (the concat of the FPN levels).
 *   mode 0: Conv2D kernel 2 stride 2      x [batch, cin, h, w] -> out[:, off:off+cout] of [batch, ctot, h/2, w/2]
 *           w_packed = A[co][ci*4 + py*2 + px] from the [cout, cin, 2, 2] weight; needs h % 4 == 0, w % 4 == 0
 *   mode 1: 1x1 convolution               -> [batch, ctot, h, w];  A[co][ci]; needs (h*w) % 4 == 0
 *   mode 2: Conv2DTranspose kernel 2 stride 2 -> [batch, ctot, 2h, 2 w_valid];  A[co*4 + dy*2 + dx][ci] from the
 *           [cin, cout, 2, 2] weight; needs (h*w) % 4 == 0; w is the row pitch of x, w_valid <= w its real width
 *           (see conv3x3_bias_relu); modes 0 and 1 need w_valid == w
 *   mode 3: Conv2DTranspose kernel 4 stride 4 -> [batch, ctot, 4h, 4 w_valid];  A[co*16 + dy*4 + dx][ci] from the
 *           [cin, cout, 4, 4] weight (PointPillars' third FPN level, upsample_strides [1, 2, 4]); out 16-byte aligned
 *   A is packed [M/64][K/16][16][64] (paddle3d_amd/ops/conv.py:pack_patch_weight); K % 16 == 0, M % 64 == 0 --
 *   except mode 1, which takes any cout >= 1 with A zero-padded to ceil(cout / 64) * 64 rows (SSDHead's 1x1
 *   convolutions, pointpillars_head.py:62-69; rows >= cout are never stored)
 */
int pd3_patch_conv_bias_relu(const float *x, const float *w_packed, const float *bias, int mode, int batch,
                             int cin, int cout, int h, int w, int w_valid, int relu, float *out,
                             int out_channels_total, int out_channel_offset, void *stream);

/* ---------------------------------------------------------------------------------------------
 * patch_conv_x3_bias_relu -- modes 0, 1, 2 of patch_conv_bias_relu (same reference layers, second_fpn.py:99-157, same
 * tensors and output placement) in fp32 arithmetic on the bf16 matrix cores: every fp32 operand as three bf16 pieces whose
 * sum IS the value, six piece products accumulated in fp32 (csrc/sparse_conv_x3.hip; error vs fp64 = that of the fp32
 * kernel, tested).  One persistent kernel, 128 GEMM rows x 256 pixels per work item.
 *   w_packed: bf16 [row tile][step][16384]: a step's A pieces as the LDS image the kernel fetches, [piece 3][row 128][40]
 *   (32 values of K, 8 of padding) + 1024 of padding (paddle3d_amd/ops/conv.py:pack_patch_weight_x3):
 *     mode 0: row tile = 128 output channels, step = (dy, 16 input channels), k = (ci, dx); needs cin % 16 == 0,
 *             cout % 128 == 0, h % 2 == 0, w % 64 == 0
 *     mode 1: row tile = 128 output channels, step = 32 input channels; needs cin % 32 == 0, cout % 128 == 0
 *     mode 2: row tile = (dy, 64 output channels), rows (dx, co), step = 32 input channels; needs cin % 32 == 0,
 *             cout % 64 == 0; w = row pitch of x, w_valid its real width
 *   bias [cout] or NULL; x 16-byte aligned; out 8-byte aligned; every tensor below 2 GB; PD3_EUNSUPPORTED otherwise
 */
int pd3_patch_conv_x3_bias_relu(const float *x, const void *w_packed, const float *bias, int mode, int batch, int cin,
                                int cout, int h, int w, int w_valid, int relu, float *out, int out_channels_total,
                                int out_channel_offset, void *stream);

/* ---------------------------------------------------------------------------------------------
 * conv3x3_s2_x3_bias_relu -- the stride-2 3x3 / pad 1 convolution + bias + ReLU that opens a SECOND block
 * (second_backbone.py:72-120) in fp32 arithmetic on the bf16 matrix cores (three bf16 pieces per operand, six products,
 * fp32 accumulation: csrc/conv_s2_x3.hip; same tensors as conv3x3_bias_relu with stride 2).
 *   x [batch, cin, h, w] fp32 NCHW (16-byte aligned; w = row pitch, w_valid <= w the real width, pad columns zero: the
 *   convention of conv3x3_bias_relu) -> out [batch, cout, h/2, out_w], w_valid/2 real columns, the rest of the pitch zero
 *   w_packed: bf16 [cout/128][step = (16-channel chunk, ky)][24576]: a step's A pieces as the LDS image the kernel fetches,
 *             [piece 3][row 128][56] (k = kx * 16 + channel: 48 values, 8 of padding) + 3072 of padding
 *             (paddle3d_amd/ops/conv.py:pack_conv3x3_s2_x3_weight)
 *   needs cin % 16 == 0, cout % 128 == 0 (<= 1024), h % 2 == 0, w_valid % 2 == 0, w % 4 == 0, every tensor below 2 GB;
 *   PD3_EUNSUPPORTED otherwise (the caller runs conv3x3_bias_relu)
 */
int pd3_conv3x3_s2_x3_bias_relu(const float *x, const void *w_packed, const float *bias, int batch, int cin, int cout,
                                int h, int w, int w_valid, int relu, float *out, int out_w, void *stream);

/*
 * ssd_postprocess -- SSDHead.post_process of PointPillars for a whole batch (paddle3d/models/detection/
 * pointpillars/pointpillars_head.py:86-196: PointPillarsCoder.decode (pointpillars_coder.py:126-148), the
 * anchors_mask selection, sigmoid -> max / argmax, direction argmax, score (>=) and centre-range filter, heading
 * flip, rotate_nms_pcdet (models/layers/layer_libs.py:210-249), index_select) together with
 * AnchorGenerator.generate_anchors_mask (anchors_generator.py:103-121, :191-210) that test_forward runs per frame
 * in front of it (pointpillars.py:120-127).
 *   head_map     [batch, C, feat_h, feat_w] fp32, the 1x1 head convolutions' output as they write it (NCHW);
 *                batch_stride = elements between frames; class logits of anchor j at channels
 *                cls_channel0 + j*(num_classes + !encode_background_as_zeros) + k, box code at box_channel0 + j*7 + k,
 *                direction logits at dir_channel0 + j*2 + k (dir_channel0 < 0: use_direction_classifier=False)
 *   anchors      [A, 7] fp32 (x, y, z, w, l, h, r), A = feat_h*feat_w*anchors_per_loc, index (y*feat_w + x)*apl + j
 *   anchors_bv   [A, 4] int32 pillar-index boxes (xmin, ymin, xmax, ymax) (AnchorGenerator.anchors_bv)
 *   coors        [num_coors, 4] int32 (batch, z, y, x) of the batch's pillars; rows with batch outside [0, batch) skipped
 *   center_limit_range  6 host floats or NULL (prediction_center_limit_range=None)
 * Outputs (device): out_boxes [batch, max(post,1), 7], out_scores [batch, max(post,1)], out_labels int64, out_count
 * [batch] int32.  A frame without detections (no anchor passes the area test, or none the score / range test) has
 * count 0 and the reference's `_box_empty` row (zeros, -1, -1) in row 0.  Rows behind out_count (behind row 0 of such a
 * frame) are left to the caller: the Python shim clears the outputs first, and they then read zero.  No host
 * synchronisation.
 * selection: how the top nms_pre_max_size anchors by score are found -- 0 = radix select + ordered compaction
 * (nms_pre_max_size <= 1024; larger caps take the sort), 1 = a full stable sort of every anchor's key (the
 * reference's argsort); identical results, the argument exists so that tests run both.
 */
size_t pd3_ssd_postprocess_workspace(int batch, int feat_h, int feat_w, int anchors_per_loc, int grid_x, int grid_y,
                                     int nms_pre_max_size);
int pd3_ssd_postprocess(const float *head_map, int64_t batch_stride, int cls_channel0, int box_channel0,
                        int dir_channel0, int batch, int feat_h, int feat_w, int anchors_per_loc, int num_classes,
                        int encode_background_as_zeros, const float *anchors, const int32_t *anchors_bv,
                        const int32_t *coors, int64_t num_coors, int grid_x, int grid_y,
                        float anchor_area_threshold, float score_threshold, const float *center_limit_range,
                        float nms_iou_threshold, int nms_pre_max_size, int nms_post_max_size, float *out_boxes,
                        float *out_scores, int64_t *out_labels, int32_t *out_count, void *workspace,
                        size_t workspace_bytes, void *stream, int selection);

/* ---------------------------------------------------------------------------------------------
 * IA-SSD at inference (csrc/iassd.hip).  fp32 data, contiguous tensors unless a stride is named, 64-bit offsets inside
 * the kernels, no float atomics; nothing here synchronises with the host.
 *
 * sa_msg_pool -- one scale of SAModuleMSG_WithSampling.forward (models/detection/iassd/iassd_modules.py:204-221) from
 * the ball query to the max pool, with no idx and no [batch, *, m, nsample] tensor in global memory.  The scale's mlp
 * is three times Conv2d / BN / ReLU, (3 + C) -> c1 -> c2 -> c3; the first convolution is linear in [d; f], so the
 * caller passes features_in = features @ W1[:, 3:]^T ([batch, n, c1], NULL reads as zeros) and w_pos = W1[:, :3].
 * new_xyz [batch, m, 3], xyz [batch, n, 3], w_pos [c1, 3], scale1 / shift1 [c1], w2 [c2, c1], scale2 / shift2 [c2],
 * w3 [c3, c2], scale3 / shift3 [c3] (each BatchNorm in eval form, scale = gamma / sqrt(var + eps), shift = beta -
 * mean * scale, formed by the caller in fp32) -> the row of query (b, q) at out + (b * m + q) * ld_out, c3 floats
 * (ld_out >= c3: the columns beside it are not touched, so the scales of a layer write side by side into one buffer):
 *   h1[s, j] = relu(scale1[j] * (features_in[b, idx_s, j] + ((w_pos[j,0] * dx + w_pos[j,1] * dy) + w_pos[j,2] * dz))
 *                   + shift1[j])                                                             (no FMA)
 *   h2[s, c] = relu(scale2[c] * (sum_j w2[c, j] * h1[s, j]) + shift2[c])                     (no FMA outside the sum)
 *   h3[s, c] = relu(scale3[c] * (sum_j w3[c, j] * h2[s, j]) + shift3[c])
 *   out[c]   = max_s h3[s, c]
 * with idx exactly pd3_ball_query_batch's row for the same arguments (the first nsample points in index order with
 * ((nx - x)^2 + (ny - y)^2) + (nz - z)^2 < radius * radius, a NaN is no hit), d = xyz[b, idx_s] - new_xyz.  The max
 * runs over the hits only (unused slots repeat the first hit); a row without a hit takes its one slot, point 0 of the
 * frame, a real point with its own features_in row and d.  Each sum over j is an ascending-j fp32 fmaf chain from 0
 * (what v_mfma_f32_16x16x4_f32 computes), so the result depends neither on the tiling nor on where a row sits in the
 * launch.  relu(v) = v > 0 ? v : +0 (a NaN stays) and the max keeps a NaN, as in pd3_stack_sa_pool.
 * c1, c2, c3 each a multiple of 16 in 16 .. 256 and nsample <= 64, else PD3_EUNSUPPORTED.  PD3_EINVAL on negative
 * dims, nsample < 1, ld_out < c3, or n == 0 with rows to compute; batch * m == 0 launches nothing.
 */
int pd3_sa_msg_pool(const float *new_xyz, const float *xyz, const float *features_in, const float *w_pos,
                    const float *scale1, const float *shift1, const float *w2, const float *scale2,
                    const float *shift2, const float *w3, const float *scale3, const float *shift3, int batch, int m,
                    int n, int c1, int c2, int c3, float radius, int nsample, float *out, int64_t ld_out,
                    void *stream);

/* iassd_decode -- IASSD_Head.generate_predicted_boxes with PointResidual_BinOri_Coder.decode_paddle
 * (iassd_head.py:606-621, iassd_coder.py:76-121) in one launch.  cls_preds [m, num_classes], box_preds
 * [m, 6 + 2 * bins], the centre of row i at centers + i * ld_centers (3 floats, ld_centers >= 3: columns 1:4 of a
 * [m, 4] tensor are read in place), mean_size [num_classes, 3] or NULL (use_mean_size=False) -> boxes [m, 7]:
 *   k = argmax of the raw logits of the row (the first maximum wins, a NaN counts as the maximum);
 *   with mean_size: (dxa, dya, dza) = mean_size[k], diagonal = sqrt(dxa * dxa + dya * dya),
 *     x = xt * diagonal + xa, y = yt * diagonal + ya, z = zt * dza + za, dx = exp(dxt) * dxa, dy, dz likewise;
 *   without: x = xt + xa, y, z likewise, dx = exp(dxt), dy, dz likewise;
 *   bin = argmax of box_preds[6 : 6 + bins] under the same rule, res = box_preds[6 + bins + bin];
 *   heading = ((float(bin) * bin_inter - pi) + half) + res * half, bin_inter = float(2 pi / bins), half =
 *   float(pi / bins), pi = float(pi).
 * exp is glibc's expf (csrc/libm_exact.hpp); no FMA.  PD3_EINVAL on m < 0, num_classes < 1, bins < 1 or
 * ld_centers < 3; m == 0 launches nothing.
 */
int pd3_iassd_decode(const float *cls_preds, const float *box_preds, const float *centers, int64_t ld_centers,
                     const float *mean_size, int64_t m, int num_classes, int bins, float *boxes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * BEVFusion's Anchor3DHead at inference (csrc/anchor3d_head.hip; models/heads/dense_heads/anchor3d_head.py:146-161,
 * :378-520, models/detection/bevfusion/utils.py:92-103, :189-276, utils/box_coder.py:270-310), fp32, on `stream`, no
 * host synchronisation, every count on the device, every output element written on every call.  The arithmetic order
 * of every output is in the header of csrc/anchor3d_head.hip; tests/golden/anchor3d_numpy.py restates it.  Statuses:
 * 0, PD3_EINVAL (-1), PD3_EWORKSPACE (-2), PD3_EUNSUPPORTED (-3, nothing is launched), or a positive hipError_t.
 *
 * Common to both entry points: anchors [feat_h * feat_w * num_anchors, code_size] (anchor (y * feat_w + x) *
 * num_anchors + a, map channel a * width + component), K = min(nms_pre, anchors) or all anchors when nms_pre <= 0,
 * sigmoid class scores, a direction classifier; score_thr, nms_thr, dir_offset and dir_limit_offset as fp32 ->
 * boxes [batch, max_num, code_size], scores [batch, max_num], labels int32 [batch, max_num], counts int32 [batch];
 * rows past counts[b] are zero.  PD3_EUNSUPPORTED unless 1 <= num_classes <= 16, 1 <= num_anchors <= 32, 7 <=
 * code_size <= 16, 1 <= K <= 1024, 1 <= max_num <= 1024 (and feat_h * feat_w * num_anchors < 2^30, batch *
 * num_classes <= 65535); batch == 0 is success without a launch; nothing needs an alignment.
 * pd3_anchor3d_head_workspace: bytes of workspace for either entry point (0 for a shape they refuse); needs no GPU.
 * pd3_anchor3d_head_forward: the LAZY head.  feat [batch, channels, feat_h, feat_w]; cls_weight_packed: conv_cls's
 *   [num_anchors * num_classes, channels] weight in the MFMA lane order of the kernel file's header
 *   (ops/anchor3d_head.py pack_cls_weight); reg_weight [num_anchors * code_size, channels] and dir_weight
 *   [num_anchors * 2, channels] as the convolutions hold them; the three biases.  Only conv_cls runs densely and only
 *   the per-anchor maximum score (4 * anchors bytes per frame) is written; conv_reg, conv_dir_cls and the class
 *   scores are evaluated at the K selected anchors.  Also PD3_EUNSUPPORTED unless channels % 16 == 0 and 16 <=
 *   channels <= 512.
 * pd3_anchor3d_get_bboxes: the same sequence from existing maps cls_score [batch, num_anchors * num_classes, feat_h,
 *   feat_w], bbox_pred [batch, num_anchors * code_size, ..], dir_cls_pred [batch, num_anchors * 2, ..].
 * ------------------------------------------------------------------------------------------- */
size_t pd3_anchor3d_head_workspace(int batch, int feat_h, int feat_w, int num_anchors, int num_classes, int code_size,
                                   int nms_pre);
int pd3_anchor3d_head_forward(const void *feat, const void *cls_weight_packed, const void *cls_bias,
                              const void *reg_weight, const void *reg_bias, const void *dir_weight,
                              const void *dir_bias, const void *anchors, int batch, int channels, int feat_h,
                              int feat_w, int num_anchors, int num_classes, int code_size, int nms_pre, int max_num,
                              float score_thr, float nms_thr, float dir_offset, float dir_limit_offset, void *boxes,
                              void *scores, void *labels, void *counts, void *workspace, size_t workspace_bytes,
                              void *stream);
int pd3_anchor3d_get_bboxes(const void *cls_score, const void *bbox_pred, const void *dir_cls_pred,
                            const void *anchors, int batch, int feat_h, int feat_w, int num_anchors, int num_classes,
                            int code_size, int nms_pre, int max_num, float score_thr, float nms_thr, float dir_offset,
                            float dir_limit_offset, void *boxes, void *scores, void *labels, void *counts,
                            void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * SqueezeSegV3 (csrc/squeezeseg.hip; models/backbones/sac.py:186-197, transforms/reader.py:287-366,
 * transforms/normalize.py NormalizeRangeImage), fp32, inference only, on `stream`, no host synchronisation, every
 * output element written on every call.  The arithmetic order of every output is in the header of
 * csrc/squeezeseg.hip; tests/golden/squeezeseg_numpy.py restates it.  Statuses: 0, PD3_EINVAL (-1), PD3_EWORKSPACE
 * (-2), PD3_EUNSUPPORTED (-3, nothing is launched), or a positive hipError_t.
 *
 * pd3_sac_isk_forward: SACISKBlock.forward from xyz and feature to its first MLP layer, in one launch:
 *   Y = relu(BN(conv1x1(unfold3x3(feature) * sigmoid(BN(conv7x7(xyz)))))).  xyz [batch, 3, height, width], feature and
 *   out [batch, channels, height, width], NCHW.  attn_weight_packed holds the [9 * channels, 3, 7, 7] weight as floats
 *   [9 * channels / 16][37][64] and mlp_weight_packed the [channels, 9 * channels] weight as [9 * channels / 16][4]
 *   [channels / 16][64] (the lane orders are in the kernel file's header; ops/squeezeseg.py packs them); attn_scale,
 *   attn_shift [9 * channels] and mlp_scale, mlp_shift [channels] are the folded BatchNorms (scale = gamma / sqrt(var +
 *   eps), shift = (bias - mean) * scale + beta; the attention convolution has a bias).  None of the three [batch, 9 *
 *   channels, height, width] intermediates is written anywhere.  The bits of a pixel depend on `channels` only: not on
 *   batch, height, width, the pixel's place, the grid or the stream.  No atomics.  PD3_EUNSUPPORTED unless channels %
 *   16 == 0, 16 <= channels <= 256, height >= 1, width >= 1 and batch * height * ceil(width / 16) < 2^30; batch
 *   == 0 is success without a launch; nothing needs an alignment.
 * pd3_range_project: the reader's spherical projection and the image normalisation for `batch` frames in one call.
 *   points [num_points, 4] (x, y, z, remission; the frames concatenated), offsets int32 [batch + 1] on the device,
 *   fov_up_deg / fov_down_deg the two inclinations in degrees (3, -25), mean[5], std[5] host doubles, workspace uint64
 *   [batch, height, width] (workspace_bytes >= 8 * batch * height * width, 8-byte aligned; filled by the call) ->
 *   image [batch, 5, height, width] (range, x, y, z, remission; an empty pixel is -1 before the normalisation
 *   (float)((double)(float)((double)v - mean) / std)), proj_idx int32 [batch, height, width] (index inside the frame,
 *   -1 when empty), proj_mask uint8 = proj_idx > 0 (the reference's form: point 0's pixel is masked out too), proj_y,
 *   proj_x int32 [num_points] (-1 for a point with a non-finite coordinate, zero depth or outside every frame; such a
 *   point takes no pixel).  Pixel coordinates are computed in fp64 from the fp32 inputs; a pixel takes its nearest
 *   point, the smaller index on equal depths, through a 64-bit atomicMin (exact in any order).  Three launches.
 *   num_points up to 2^31 - 1.
 * ------------------------------------------------------------------------------------------- */
int pd3_sac_isk_forward(const void *xyz, const void *feature, const void *attn_weight_packed, const void *attn_scale,
                        const void *attn_shift, const void *mlp_weight_packed, const void *mlp_scale,
                        const void *mlp_shift, int batch, int channels, int height, int width, void *out,
                        void *stream);
int pd3_range_project(const void *points, int64_t num_points, const void *offsets, int batch, int height, int width,
                      double fov_up_deg, double fov_down_deg, const double *mean, const double *std, void *image,
                      void *proj_idx, void *proj_mask, void *proj_y, void *proj_x, void *workspace,
                      size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * PETR / PETRv2's head (csrc/petr.hip; models/heads/dense_heads/petr_head.py:364-450, models/layers/petr_transformer.py:
 * 277-360), fp32, inference only, on `stream`, no host synchronisation, no atomics on global memory, every output
 * element written on every call.  The arithmetic order of every output is in the header of csrc/petr.hip;
 * tests/golden/petr_numpy.py restates it.  Statuses: 0, PD3_EINVAL (-1), PD3_EUNSUPPORTED (-3, nothing is launched), or
 * a positive hipError_t.
 *
 * pd3_mha_stream_forward: paddle.nn.MultiHeadAttention's core for any number of keys, with an optional key padding
 *   mask.  q [batch, num_query, num_heads, head_dim], k and v [batch, num_key, num_heads, head_dim] (the Linear outputs
 *   viewed per head), key_mask uint8 [batch, num_key] or NULL (non-zero: padded; the fp32 value -1e9f is added to the
 *   key's score, as Paddle's converted boolean attn_mask does -- the key is not skipped), scale = head_dim ** -0.5 ->
 *   out [batch, num_query, num_heads * head_dim] = softmax((q * scale) k^T + mask) v per head: an exact two-pass
 *   softmax that keeps no score row anywhere (LDS use does not depend on num_key) and whose bits depend on (num_key,
 *   head_dim) only, not on num_query, the tiling, the frame's place in the batch or the stream.  The bits are not those
 *   of pd3_mha_forward.  PD3_EUNSUPPORTED unless head_dim % 16 == 0, head_dim <= 128 and q, k, v, out are 16-byte
 *   aligned (the kernel loads and stores single floats today: the alignment is reserved for vector loads); num_key < 1
 *   is PD3_EINVAL; batch == 0 or num_query == 0 is success without a launch.
 * pd3_petr_coords3d: PETRHead.position_embeding from the frustum grid through inverse_sigmoid in one launch.
 *   img2lidars [num_views, 4, 4] (num_views = batch * cameras), the feature map's feat_h x feat_w, depth_num bins from
 *   depth_start (lid != 0: linear-increasing, else uniform) up to position_range[3], pad_h x pad_w the padded image,
 *   position_range[6] host floats, token_mask uint8 [num_views, feat_h, feat_w] or NULL -> coords [num_views, 3 *
 *   depth_num, feat_h, feat_w] (channel d * 3 + c; the logarithm is (float)log((double)ratio)) and, unless NULL,
 *   coords_mask uint8 [num_views, feat_h, feat_w]: more than depth_num * 0.5 of the token's 3 * depth_num normalised
 *   coordinates outside [0, 1], OR-ed with token_mask.  A zero num_views, feat_h, feat_w or depth_num is success
 *   without a launch; no alignment is needed; PD3_EUNSUPPORTED only when num_views * feat_h * ceil(feat_w / 64)
 *   exceeds 2^31 - 1.
 * ------------------------------------------------------------------------------------------- */
int pd3_mha_stream_forward(const void *q, const void *k, const void *v, const void *key_mask, int batch, int num_query,
                           int num_key, int num_heads, int head_dim, float scale, void *out, void *stream);
int pd3_petr_coords3d(const void *img2lidars, int num_views, int feat_h, int feat_w, int depth_num, int pad_h, int pad_w,
                      double depth_start, const float *position_range, int lid, const void *token_mask, void *coords,
                      void *coords_mask, void *stream);

/* ---------------------------------------------------------------------------------------------
 * BEVFormer's decoder, head and NMS-free decode (csrc/bevformer_decoder.hip; models/transformers/decoders.py,
 * decoder_layers.py, attentions/multihead_attention.py, attentions/spatial_cross_attention.py:531-640,
 * utils/box_coder.py:133-214, utils/box.py:107-138), fp32, inference only, on `stream`, no host synchronisation, no
 * atomics on global memory, every output element written on every call.  The arithmetic order of every output is in
 * the header of csrc/bevformer_decoder.hip; tests/golden/bevformer_decoder_numpy.py restates it.  Statuses: 0,
 * PD3_EINVAL (-1), PD3_EUNSUPPORTED (-3, nothing is launched), or a positive hipError_t.
 *
 * pd3_mha_forward: paddle.nn.MultiHeadAttention's core without masks or dropout.  q [batch, num_query, num_heads,
 *   head_dim], k and v [batch, num_key, num_heads, head_dim] (the Linear outputs viewed per head), scale = head_dim **
 *   -0.5 -> out [batch, num_query, num_heads * head_dim] = softmax((q * scale) k^T) v per head, an exact two-pass
 *   softmax whose bits depend neither on the tiling nor on the frame's place in the batch.  PD3_EUNSUPPORTED unless
 *   head_dim % 16 == 0, head_dim <= 128, num_key <= 2048 and q, k, v, out are 16-byte aligned; num_key < 1 is
 *   PD3_EINVAL; batch == 0 or num_query == 0 is success without a launch.
 * pd3_bevformer_dec_ca: CustomMSDeformableAttention's sampling.  value [batch, spatial_size, num_heads, channels]
 *   (projected), sampling_offsets [batch, num_query, num_heads, num_levels, num_point, 2] and attention_logits [batch,
 *   num_query, num_heads, num_levels * num_point] as the two Linear layers give them, reference_points [batch,
 *   num_query, num_ref_levels, 2] with num_ref_levels 1 (broadcast over the levels) or num_levels, spatial_shapes
 *   [num_levels, 2] (H, W) and level_start_index [num_levels] int64 on the device -> out [batch, num_query, num_heads *
 *   channels].  PD3_EUNSUPPORTED unless channels % 4 == 0 with value and out 16-byte aligned and num_levels * num_point
 *   <= 32.
 * pd3_nms_free_decode: NMSFreeCoder.decode for the whole batch.  cls_scores [batch, num_query, num_classes] logits,
 *   bbox_preds [batch, num_query, code_size] (code_size 8 or 10; centres in metres), post_center_range[6] host floats,
 *   score_threshold (negative: None), bottom_center != 0: z = z - h * 0.5f on the kept rows -> boxes [batch, max_num,
 *   code_size - 1] (cx, cy, cz, w, l, h, rot[, vx, vy]), scores [batch, max_num], labels [batch, max_num] int32 and
 *   count [batch] int32: the kept rows of the max_num best (score descending, flat index ascending; a NaN score is
 *   never kept) in rank order, rows at and after count zeros with label -1.  max_num > num_query * num_classes or a
 *   score_threshold that is no finite number is PD3_EINVAL, max_num > 1024 PD3_EUNSUPPORTED.
 * ------------------------------------------------------------------------------------------- */
int pd3_mha_forward(const void *q, const void *k, const void *v, int batch, int num_query, int num_key, int num_heads,
                    int head_dim, float scale, void *out, void *stream);
int pd3_bevformer_dec_ca(const void *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                         const void *sampling_offsets, const void *attention_logits, const void *reference_points,
                         int batch, int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                         int num_point, int num_ref_levels, void *out, void *stream);
int pd3_nms_free_decode(const void *cls_scores, const void *bbox_preds, const float *post_center_range, int batch,
                        int num_query, int num_classes, int code_size, int max_num, double score_threshold,
                        int bottom_center, void *boxes, void *scores, void *labels, void *count, void *stream);

/* ---------------------------------------------------------------------------------------------
 * BEVFormer's encoder attention (csrc/bevformer.hip; models/transformers/encoders.py:120-176 point_sampling,
 * attentions/spatial_cross_attention.py:81-212 and :310-428, attentions/temporal_self_attention.py:207-272), fp32.  The
 * arithmetic order of every output is in the header of csrc/bevformer.hip; tests/golden/bevformer_numpy.py restates it.
 * value is the projected value [rows, spatial_size, num_heads, channels]; spatial_shapes [num_levels, 2] (H, W) and
 * level_start_index [num_levels] are int64 on the device.  Statuses: 0, PD3_EINVAL (-1), PD3_EUNSUPPORTED (-3) for a
 * shape outside: channels % 4 == 0 with value and out 16-byte aligned, num_levels * num_point <= 32, num_cams <= 8,
 * num_point % num_anchors == 0 (nothing is launched then), or a positive hipError_t.
 *
 * pd3_bevformer_point_sampling: ref_3d [num_anchors, num_query, 3] in [0, 1], lidar2img [batch, num_cams, 4, 4],
 *   pc_range[6] host floats, the image size all frames are normalised by -> reference_points_cam [num_cams, batch,
 *   num_query, num_anchors, 2], bev_mask [num_cams, batch, num_query, num_anchors] uint8, hit_bits [batch, num_query]
 *   uint8 (bit c: camera c sees an anchor of the query) and hit_count [batch, num_query] uint8.
 * pd3_bevformer_sca: value rows batch * num_cams (row b * num_cams + c), sampling_offsets [batch, num_query, num_heads,
 *   num_levels, num_point, 2] and attention_logits [batch, num_query, num_heads, num_levels * num_point] as the two
 *   Linear layers give them on the BEV queries -> out [batch, num_query, num_heads * channels]: the softmax, the
 *   sampling of every camera whose hit bit is set (summed in camera order) and the division by max(hit count, 1).
 * pd3_bevformer_tsa: value rows batch * 2 (row 2 b + j for queue entry j), sampling_offsets [batch, num_query,
 *   num_heads, 2, num_levels, num_point, 2], attention_logits [batch, num_query, num_heads, 2, num_levels * num_point],
 *   reference_points [batch * 2, num_query, num_levels, 2] -> out [batch, num_query, num_heads * channels], the mean of
 *   the two queue entries' samples.
 * ------------------------------------------------------------------------------------------- */
int pd3_bevformer_point_sampling(const void *ref_3d, const void *lidar2img, const float *pc_range, int img_h, int img_w,
                                 int batch, int num_cams, int num_query, int num_anchors, void *reference_points_cam,
                                 void *bev_mask, void *hit_bits, void *hit_count, void *stream);
int pd3_bevformer_sca(const void *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                      const void *sampling_offsets, const void *attention_logits, const void *reference_points_cam,
                      const void *hit_bits, int batch, int num_cams, int spatial_size, int num_heads, int channels,
                      int num_levels, int num_query, int num_point, int num_anchors, void *out, void *stream);
int pd3_bevformer_tsa(const void *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                      const void *sampling_offsets, const void *attention_logits, const void *reference_points,
                      int batch, int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                      int num_point, void *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * CaDDN's frustum-to-voxel and map-to-BEV stage (csrc/caddn.hip; models/detection/caddn: ffe/ffe.py:75-97,
 * f2v/frustum_grid_generator.py:87-154, f2v/sampler.py, f2v/frustum_to_voxel.py, caddn.py:113-122).  Common arguments:
 *   image_features [batch, channels, h, w] fp32 (after channel_reduce), depth_logits [batch, num_bins + 1, h, w] fp32,
 *   lidar_to_cam [batch, 4, 4], cam_to_img [batch, 3, 4] fp32 and image_shape [batch, 2] int32 (H, W of the full-resolution
 *   image; the grid is normalised by the maximum over the batch), all on the device; pc_min[3], voxel_size[3] host floats;
 *   the voxel grid (grid_x, grid_y, grid_z); mode 0 UD / 1 LID / 2 SID with depth_min, depth_max (utils/depth.py:38-47).
 * The arithmetic order of every step is stated at the top of csrc/caddn.hip and restated in tests/golden/caddn_numpy.py.
 * No atomics, no host synchronisation.  PD3_EINVAL for a size below 1 or an unknown mode, PD3_EWORKSPACE, PD3_EUNSUPPORTED
 * for batch > 65535, grid_x * grid_y or h * w * max(channels, num_bins + 1) above 2^31 - 1.
 *
 * frustum_grid: grid [batch, grid_x, grid_y, grid_z, 3] fp32, FrustumGridGenerator.forward's normalised sampling grid (voxel
 *   centres index + 0.5; scale = |w| > 1e-8 ? 1 / (w + 1e-8) : 1 after the 4x4 product and after the projection; a
 *   non-finite component is -2).
 * frustum_to_voxel: voxel_features [batch, channels, grid_z, grid_y, grid_x] fp32, FrustumToVoxel.forward over
 *   FFE.create_frustum_features without the frustum volume or the grid in memory (any channels >= 1): a pack step writes
 *   softmax(depth_logits)[:, :-1] and the features pixel-major into the workspace, then a thread per voxel writes
 *   sum_{4 (y, x) corners} w_xy * f[c, y, x] * (sum_{2 z corners} w_z * p[z, y, x]), zero padding per corner, zeros included.
 * frustum_to_bev: bev [batch, c_out, grid_y, grid_x] = relu(scale[o] * sum_k weight[o, k] * voxel[k] + shift[o]) with
 *   k = c * grid_z + z (the reference's flatten(1, 2)), weight [c_out, channels * grid_z], scale / shift [c_out] the folded
 *   BatchNorm: map_to_bev on the fp32 matrix cores in the same kernel, the voxel volume never in memory.  The sum is one
 *   fp32 fmaf chain from 0, z ascending and within a z the channels in the order stated in csrc/caddn.hip; a column's result depends neither on its tile, the
 *   launch nor its frame's place in the batch; a column without a sample is relu(shift).  channels and c_out multiples of
 *   16 up to 64 and grid_z <= 32, PD3_EUNSUPPORTED otherwise (the caller composes frustum_to_voxel with a convolution).
 */
int pd3_frustum_grid(const float *lidar_to_cam, const float *cam_to_img, const int32_t *image_shape, int batch,
                     int grid_x, int grid_y, int grid_z, const float *pc_min, const float *voxel_size, int mode,
                     double depth_min, double depth_max, int num_bins, float *grid, void *stream);
size_t pd3_frustum_to_voxel_workspace(int batch, int channels, int num_bins, int h, int w);
int pd3_frustum_to_voxel(const float *image_features, const float *depth_logits, const float *lidar_to_cam,
                         const float *cam_to_img, const int32_t *image_shape, int batch, int channels, int num_bins,
                         int h, int w, int grid_x, int grid_y, int grid_z, const float *pc_min,
                         const float *voxel_size, int mode, double depth_min, double depth_max, float *voxel_features,
                         void *workspace, size_t workspace_bytes, void *stream);
size_t pd3_frustum_to_bev_workspace(int batch, int channels, int num_bins, int h, int w, int grid_z, int c_out);
int pd3_frustum_to_bev(const float *image_features, const float *depth_logits, const float *lidar_to_cam,
                       const float *cam_to_img, const int32_t *image_shape, int batch, int channels, int num_bins,
                       int h, int w, int grid_x, int grid_y, int grid_z, const float *pc_min, const float *voxel_size,
                       int mode, double depth_min, double depth_max, const float *weight, const float *scale,
                       const float *shift, int c_out, float *bev, void *workspace, size_t workspace_bytes,
                       void *stream);

/* ---------------------------------------------------------------------------------------------
 * SMOKE's head and post-processing at inference (csrc/smoke.hip; models/detection/smoke/smoke_predictor.py:78-97,
 * processor.py:45-194, smoke_coder.py:103-383, models/layers/layer_libs.py:36-116, :181-207, layer_norm.py:20-33),
 * fp32, on `stream`, no host synchronisation, every count on the device, every output element written on every call.
 * The arithmetic order of every output is in the header of csrc/smoke.hip; tests/golden/smoke_numpy.py restates it.
 * Statuses: 0, PD3_EINVAL (-1), PD3_EWORKSPACE (-2), PD3_EUNSUPPORTED (-3, nothing is launched), or a positive
 * hipError_t.
 *
 * Common: Ks [batch, 3, 3]; mode 0 (PostProcessor.forward): trans = trans_mat [batch, 3, 3], image_size [2], rows
 * with score <= det_threshold dropped; mode 1 (export_forward): trans = down_ratios [2], image_size unused, all rows;
 * depth_ref [2], dim_ref [num_classes, 3] (all device pointers); reg_channels: five ints on the host -> rows
 * [batch, max_detection, 14] in the reference's column order and descending score, rows past counts[b] zero, counts
 * int32 [batch].  Selection: one exact top-K over the num_classes * feat_h * feat_w peak-tested scores, ties to the
 * lower flat index; a NaN heat has score 0.  PD3_EUNSUPPORTED unless 1 <= max_detection <= min(1024, feat_h * feat_w),
 * 1 <= num_classes <= 16, reg_channels == (1, 2, 3, 2, 2), num_classes * feat_h * feat_w < 2^30 and pred_2d != 0;
 * batch == 0 is success without a launch; nothing needs an alignment.
 * pd3_smoke_head_workspace: bytes of workspace for either entry point (0 for a shape they refuse); needs no GPU.
 * pd3_smoke_head_forward: the LAZY head.  cls_feat / reg_feat: the two branches' 3x3 convolution outputs
 *   [batch, channels, feat_h, pitch] (pitch >= feat_w floats per row, batch_stride floats between frames: the two
 *   pointers may address one stacked map); gamma / beta [channels] of the two norms; cls_tables / reg_tables: NULL
 *   (GroupNorm with `groups` groups: the statistics are computed here, biased variance, epsilon 1e-5, accumulated in
 *   double in a fixed order) or filled [batch, 2, groups] tables (mean, rstd), e.g. BatchNorm's running statistics with
 *   groups == channels; cls_weight [num_classes, channels], reg_weight [10, channels] and the biases.  Only the class
 *   branch runs densely; the regression branch is evaluated at the max_detection selected pixels.  Also
 *   PD3_EUNSUPPORTED unless channels % groups == 0 and channels <= 512.
 * pd3_smoke_post_process: the same selection and decode from SMOKEPredictor's outputs heat [batch, num_classes,
 *   feat_h, feat_w] and regression [batch, 10, feat_h, feat_w].
 * ------------------------------------------------------------------------------------------- */
size_t pd3_smoke_head_workspace(int batch, int feat_h, int feat_w, int num_classes, int max_detection);
int pd3_smoke_head_forward(const void *cls_feat, const void *reg_feat, int64_t batch_stride, int pitch,
                           const void *cls_gamma, const void *cls_beta, const void *reg_gamma, const void *reg_beta,
                           const void *cls_tables, const void *reg_tables, const void *cls_weight,
                           const void *cls_bias, const void *reg_weight, const void *reg_bias, const void *Ks,
                           const void *trans, const void *image_size, const void *depth_ref, const void *dim_ref,
                           int batch, int channels, int groups, int feat_h, int feat_w, int num_classes,
                           const int *reg_channels, int max_detection, float det_threshold, int mode, int pred_2d,
                           void *rows, void *counts, void *workspace, size_t workspace_bytes, void *stream);
int pd3_smoke_post_process(const void *heat, const void *regression, const void *Ks, const void *trans,
                           const void *image_size, const void *depth_ref, const void *dim_ref, int batch, int feat_h,
                           int feat_w, int num_classes, const int *reg_channels, int max_detection,
                           float det_threshold, int mode, int pred_2d, void *rows, void *counts, void *workspace,
                           size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * DD3D's FCOS heads and post-processing at inference (csrc/dd3d.hip; models/heads/fcos_heads/fcos2d_head.py:160-186,
 * :334-503, fcos3d_head.py:33-108, :268-296, :519-639, models/detection/dd3d/dd3d.py:144-176, :183-212,
 * utils/transform.py:167-246), fp32, on `stream`, no host synchronisation, every count on the device, every output
 * element written on every call.  The arithmetic order of every output and the three definitions (tie order of the
 * selection, no renormalisation of the egocentric quaternion, the NMS semantics) are in the header of csrc/dd3d.hip;
 * tests/golden/dd3d_numpy.py restates them.  Statuses: 0, PD3_EINVAL (-1), PD3_EWORKSPACE (-2), PD3_EUNSUPPORTED
 * (-3, nothing is launched), or a positive hipError_t.
 *
 * Common: per-level arguments are HOST arrays of `levels` device pointers; level_table: `levels` rows of five int64 on
 * the host (H, W, stride, pitch, batch_stride; the last two describe the tower outputs of pd3_dd3d_head_forward and are
 * ignored elsewhere); logits [batch, num_classes, H, W] and centerness [batch, 1, H, W] per level, dense; intrinsics
 * [batch, 3, 3] (inverted here, in double); canon_box_sizes [num_classes, 3]; box3d_classes: num_classes, or 1 for
 * class_agnostic_box3d (the 3D predictors then have one row per quantity); flags: 1 thresh_with_ctr, 2 locations
 * offset "half", 4 scale_depth_by_focal_lengths, 8 predict_allocentric_rot, 16 predict_distance; nms_categories: classes
 * at or above it never survive (the reference's fixed categories = [0 .. 4]).
 * -> rows [batch, R, 20] (pred_boxes 4, scores, scores_3d, pred_classes, fpn_levels, locations 2, pred_boxes3d 10), in
 * NMS order, zero past min(counts[b], R); counts int32 [batch]: the rows the reference keeps (a tie at the post-NMS cut
 * can make it exceed R); R = post_nms_topk, or levels * pre_nms_topk when post_nms_topk <= 0.
 * PD3_EUNSUPPORTED unless 1 <= pre_nms_topk <= 1024, 1 <= levels <= 8, 1 <= num_classes <= 16, num_classes * H * W <
 * 2^30 per level, channels <= 512, nms_thresh > 0 and the NMS sweep's LDS fits; batch == 0 is success without a launch;
 * nothing needs an alignment.
 * pd3_dd3d_workspace: bytes of workspace for either entry point (0 for a shape they refuse); needs no GPU.
 * pd3_dd3d_head_forward: the LAZY form.  box2d_feat / box3d_feat: the box2d and box3d towers' outputs per level
 *   [batch, channels, H, pitch] (pitch >= W floats per row, batch_stride floats between frames, both of a level);
 *   box3d_feat NULL: only_box2d (scores_3d and pred_boxes3d are zero, the order is by scores).  box2d_weight
 *   [4, channels, 3, 3], box2d_bias [4]; box3d_weight [box3d_weight_levels, 11 * box3d_classes, channels, 3, 3] with
 *   the rows quat (4 * box3d_classes), ctr (2 *), depth, size (3 *), conf, each in the reference's channel order
 *   k * box3d_classes + class, and box3d_bias likewise (zeros where a predictor has no bias); box3d_weight_levels: 1, or
 *   `levels` for use_per_level_predictors; scales [levels, 6]: the Scale / Offset values of a level (box2d_reg, proj_ctr,
 *   size, conf, depth scale, depth offset; 1 1 1 1 1 0 without use_scale).  The predictors are evaluated at the selected
 *   entries only.
 * pd3_dd3d_post_process: the same selection, decode and tail from the reference's dense head outputs (scales and ReLU
 *   applied): box2d_reg [batch, 4, H, W] and the five 3D maps per level; the five NULL: only_box2d.
 * ------------------------------------------------------------------------------------------- */
size_t pd3_dd3d_workspace(int batch, int levels, const int64_t *level_table, int num_classes, int pre_nms_topk);
int pd3_dd3d_head_forward(const void *const *logits, const void *const *centerness, const void *const *box2d_feat,
                          const void *const *box3d_feat, const int64_t *level_table, const void *box2d_weight,
                          const void *box2d_bias, const void *box3d_weight, const void *box3d_bias,
                          const void *scales, const void *intrinsics, const void *canon_box_sizes, int batch,
                          int levels, int channels, int num_classes, int box3d_classes, int box3d_weight_levels,
                          int pre_nms_topk, int post_nms_topk, int nms_categories, int flags, float pre_nms_thresh,
                          float nms_thresh, float min_depth, float max_depth, float depth_factor, void *rows,
                          void *counts, void *workspace, size_t workspace_bytes, void *stream);
int pd3_dd3d_post_process(const void *const *logits, const void *const *centerness, const void *const *box2d_reg,
                          const void *const *box3d_quat, const void *const *box3d_ctr,
                          const void *const *box3d_depth, const void *const *box3d_size,
                          const void *const *box3d_conf, const int64_t *level_table, const void *intrinsics,
                          const void *canon_box_sizes, int batch, int levels, int num_classes, int box3d_classes,
                          int pre_nms_topk, int post_nms_topk, int nms_categories, int flags, float pre_nms_thresh,
                          float nms_thresh, float min_depth, float max_depth, float depth_factor, void *rows,
                          void *counts, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PADDLE3D_AMD_H */
