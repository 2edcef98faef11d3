// CaDDN's frustum-to-voxel and map-to-BEV stage on the device (models/detection/caddn: ffe/ffe.py:75-97,
// f2v/frustum_grid_generator.py:87-154, f2v/sampler.py, f2v/frustum_to_voxel.py, caddn.py:113-122).  The reference forms
// softmax(depth_logits)[:, :-1] (x) image_features as [B, C, D, h, w], a [B, X, Y, Z, 3] sampling grid, a 5-D grid_sample
// into [B, C, X, Y, Z], a transpose and a 1x1 ConvBNReLU over the flattened (C, Z).  Here neither the frustum volume nor
// the grid is formed (all eight corners of a voxel share four (y, x) pixels and the volume is an outer product), and in
// frustum_to_bev the voxel volume is not formed either.
//
// Coordinates of voxel (ix, iy, iz) of frame b -- frustum_grid writes them, the other two entry points compute the same
// values in registers.  fp32, no FMA, every sum left to right as written:
//   trans[i][j] = l2c[i][j] * voxel[j] (j < 3);  trans[i][3] = ((l2c[i][0] * min_x + l2c[i][1] * min_y) + l2c[i][2] * min_z)
//                 + l2c[i][3]                                                       (lidar_to_cam @ grid_to_lidar)
//   p = (ix + 0.5, iy + 0.5, iz + 0.5);  ch[i] = ((p.x * trans[i][0] + p.y * trans[i][1]) + p.z * trans[i][2]) + trans[i][3]
//   s1 = |ch[3]| > 1e-8 ? 1 / (ch[3] + 1e-8) : 1;  cam = s1 * ch[0..2]
//   im[i] = ((c2i[i][0] * cam.x + c2i[i][1] * cam.y) + c2i[i][2] * cam.z) + c2i[i][3]
//   s2 = |im[2]| > 1e-8 ? 1 / (im[2] + 1e-8) : 1;  u = s2 * im[0], v = s2 * im[1];  depth = im[2] - c2i[2][3]
//   bin (utils/depth.py:38-47, its constants formed in double on the host and rounded to fp32 once):
//     UD   (depth - depth_min) / bin_size,                      bin_size = (depth_max - depth_min) / D
//     LID  -0.5 + 0.5 * sqrt(1 + (8 * (depth - depth_min)) / bin_size),  bin_size = 2 (depth_max - depth_min) / (D (1 + D))
//     SID  (D * (log(1 + depth) - log(1 + depth_min))) / (log(1 + depth_max) - log(1 + depth_min)); the log of 1 + depth
//          is the fp64 log rounded to fp32
//   g = ((u / (W_img - 1)) * 2 + -1, (v / (H_img - 1)) * 2 + -1, (bin / (D - 1)) * 2 + -1) with (H_img, W_img) the
//   maximum over the batch of image_shape; a component that is not finite is -2.
//
// Sampling (grid_sample, bilinear, zeros, align_corners=False) of component g over a size n: f = ((g + 1) * n - 1) * 0.5,
// f0 = floor(f), weights w0 = (f0 + 1) - f and w1 = f - f0 for f0 and f0 + 1; a corner outside [0, n - 1] does not count.
// With the four (y, x) corners in the order j = (y0,x0), (y0,x1), (y1,x0), (y1,x1):
//   pz_j      = wz0 * p[y_j, x_j, z0] + wz1 * p[y_j, x_j, z0 + 1]      (a z corner out of range contributes the term 0)
//   g_j       = (wx_j * wy_j) * pz_j;  an (y, x) corner out of range has g_j = 0 and feature row 0
//   sample[c] = ((g_0 * f_0[c] + g_1 * f_1[c]) + g_2 * f_2[c]) + g_3 * f_3[c]
// p = softmax over the D + 1 logits of a pixel without its last bin: m = max, e_i = expf(x_i - m) (libm_exact.hpp),
// s = e_0 + e_1 + ... in ascending i, p_i = e_i / s.  The pack step writes p as [B, h, w, D] and the features as
// [B, h, w, C] into the workspace, so a corner's D bins and C channels are contiguous.
//
// frustum_to_voxel: a thread per voxel, x fastest (the stores of a wave are contiguous for every channel), writes
// voxel_features[b, c, z, y, x] = sample[c], zeros included.
//
// frustum_to_bev: bev[b, o, y, x] = relu(scale[o] * acc + shift[o]) (no FMA; relu(v) = v > 0 ? v : +0, a NaN stays), with
// acc ONE fp32 fmaf chain from 0 over the C * Z inputs in the order z = 0 .. Z - 1 outermost and, within a z, the channels
// c = 16 q + 4 k + j for q = 0 .. C / 16 - 1, then j = 0 .. 3, then k = 0 .. 3 innermost (0, 4, 8, 12, 1, 5, 9, 13, 2, ...):
//   acc = fmaf(sample_z[c], weight[o, c * Z + z], acc)
// which is what a sequence of v_mfma_f32_16x16x4_f32 on one accumulator computes when the MFMA's k-th lane group holds
// channels 16 q + 4 k + (0 .. 3): its four floats of a corner's row are ONE 16-byte load, and step j multiplies the j-th.  A wave owns 64 consecutive columns
// n = y * X + x of a frame (4 M-tiles of 16) and all C_out channels (C_out / 16 N-tiles): 4 * C_out / 16 accumulators that
// live in registers across all z.  Per z: lane L computes the geometry (four g_j, four pixel offsets) of column n0 + L
// once; the lanes of M-tile t fetch theirs with __shfl (A[i = lane & 15][k = lane >> 4] is column 16 t + i, channel
// 16 q + 4 k + j in step 4 q + j); the A operand is formed in registers from the four gathered rows' values, the B operand
// comes from the weight repacked per call as [z][step][lane][N-tile] (contiguous per lane).  No LDS, no barrier; a column's chain depends
// neither on its tile nor on the launch nor on its frame's place in the batch.  Columns behind Y * X in the last tile
// repeat the last column and are not stored.
//
// No atomics, no host synchronisation, 64-bit offsets into every tensor.  tests/golden/caddn_numpy.py restates all of
// this in the same order.
#include "common.hpp"
#include "head_math.hpp"
#include "libm_exact.hpp"

#include <cmath>

namespace {

using pd3::relu_keep_nan;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;

struct GridArgs {
  int B, X, Y, Z, D, h, w, mode;
  float min[3], vox[3];
  float c0, c1, bins;  // the discretisation's constants
};

// What a frame's voxels share.
struct Frame {
  float t[4][4], p[3][4];
  float nx, ny, nz;
};

__device__ __forceinline__ Frame load_frame(const float* __restrict__ l2c, const float* __restrict__ c2i,
                                            const int* __restrict__ image_shape, const GridArgs& a, int b) {
  Frame f;
  const float* m = l2c + (int64_t)b * 16;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) f.t[i][j] = m[4 * i + j] * a.vox[j];
    f.t[i][3] = ((m[4 * i] * a.min[0] + m[4 * i + 1] * a.min[1]) + m[4 * i + 2] * a.min[2]) + m[4 * i + 3];
  }
  const float* q = c2i + (int64_t)b * 12;
#pragma unroll
  for (int i = 0; i < 12; ++i) f.p[i / 4][i % 4] = q[i];
  int H = image_shape[0], W = image_shape[1];
  for (int k = 1; k < a.B; ++k) {
    const int hk = image_shape[2 * k], wk = image_shape[2 * k + 1];
    H = hk > H ? hk : H;
    W = wk > W ? wk : W;
  }
  f.nx = (float)(W - 1), f.ny = (float)(H - 1), f.nz = (float)(a.D - 1);
  return f;
}

__device__ __forceinline__ float finite_or_out(float v) { return fabsf(v) <= 3.402823466e38f ? v : -2.f; }

__device__ __forceinline__ void frustum_coords(const Frame& f, const GridArgs& a, int ix, int iy, int iz, float& gx,
                                               float& gy, float& gz) {
  const float px = (float)ix + 0.5f, py = (float)iy + 0.5f, pz = (float)iz + 0.5f;
  float ch[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) ch[i] = ((px * f.t[i][0] + py * f.t[i][1]) + pz * f.t[i][2]) + f.t[i][3];
  const float s1 = fabsf(ch[3]) > 1e-8f ? 1.f / (ch[3] + 1e-8f) : 1.f;
  const float cx = s1 * ch[0], cy = s1 * ch[1], cz = s1 * ch[2];
  float im[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) im[i] = ((f.p[i][0] * cx + f.p[i][1] * cy) + f.p[i][2] * cz) + f.p[i][3];
  const float s2 = fabsf(im[2]) > 1e-8f ? 1.f / (im[2] + 1e-8f) : 1.f;
  const float u = s2 * im[0], v = s2 * im[1];
  const float depth = im[2] - f.p[2][3];
  float bin;
  if (a.mode == 0)
    bin = (depth - a.c0) / a.c1;
  else if (a.mode == 1)
    bin = -0.5f + 0.5f * sqrtf(1.f + (8.f * (depth - a.c0)) / a.c1);
  else
    bin = (a.bins * ((float)log((double)(1.f + depth)) - a.c0)) / a.c1;
  gx = finite_or_out((u / f.nx) * 2.f + -1.f);
  gy = finite_or_out((v / f.ny) * 2.f + -1.f);
  gz = finite_or_out((bin / f.nz) * 2.f + -1.f);
}

// One axis of the sampling: i0 = floor(f) as an int when a corner can be in range (ok), the weights of i0 and i0 + 1.
struct Axis {
  int i0;
  float w0, w1;
  bool ok;
};

__device__ __forceinline__ Axis axis_of(float g, int n) {
  const float f = ((g + 1.f) * (float)n - 1.f) * 0.5f;
  const float f0 = floorf(f);
  Axis a;
  a.ok = f0 >= -1.f && f0 <= (float)(n - 1);
  a.i0 = a.ok ? (int)f0 : 0;
  a.w0 = (f0 + 1.f) - f, a.w1 = f - f0;
  return a;
}

// g_j and the pixel index y * w + x (or -1: out of range, g_j = 0) of the four (y, x) corners.
struct Geo {
  float g[4];
  int o[4];
};

__device__ __forceinline__ Geo sample_geo(float gx, float gy, float gz, const GridArgs& a,
                                          const float* __restrict__ prob_b) {
  const Axis ax = axis_of(gx, a.w), ay = axis_of(gy, a.h), az = axis_of(gz, a.D);
  Geo r;
  const bool any = ax.ok && ay.ok && az.ok;
  const bool vz0 = az.i0 >= 0, vz1 = az.i0 + 1 <= a.D - 1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = ax.i0 + (j & 1), y = ay.i0 + (j >> 1);
    const bool v = any && x >= 0 && x <= a.w - 1 && y >= 0 && y <= a.h - 1;
    r.o[j] = -1, r.g[j] = 0.f;
    if (v) {
      const int pix = y * a.w + x;
      const float* p = prob_b + (int64_t)pix * a.D + az.i0;
      const float t0 = vz0 ? az.w0 * p[0] : 0.f, t1 = vz1 ? az.w1 * p[1] : 0.f;
      r.o[j] = pix;
      r.g[j] = (((j & 1) ? ax.w1 : ax.w0) * ((j >> 1) ? ay.w1 : ay.w0)) * (t0 + t1);
    }
  }
  return r;
}

// ---- frustum_grid ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void frustum_grid_kernel(const float* __restrict__ l2c,
                                                                const float* __restrict__ c2i,
                                                                const int* __restrict__ image_shape, GridArgs a,
                                                                float* __restrict__ grid) {
  const int b = blockIdx.y;
  const int64_t total = (int64_t)a.X * a.Y * a.Z;
  const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;  // (ix, iy, iz), iz fastest: the grid's own order
  if (v >= total) return;
  const Frame f = load_frame(l2c, c2i, image_shape, a, b);
  const int iz = (int)(v % a.Z), iy = (int)((v / a.Z) % a.Y), ix = (int)(v / ((int64_t)a.Z * a.Y));
  float gx, gy, gz;
  frustum_coords(f, a, ix, iy, iz, gx, gy, gz);
  float* o = grid + ((int64_t)b * total + v) * 3;
  o[0] = gx, o[1] = gy, o[2] = gz;
}

// ---- the pack step --------------------------------------------------------------------------------------------------
// [B, C, h, w] -> [B, h, w, C]; a thread per output element
__global__ __launch_bounds__(kThreads) void pack_features_kernel(const float* __restrict__ in, int64_t total, int C,
                                                                 int64_t hw, float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  const int c = (int)(t % C);
  const int64_t pix = t / C, b = pix / hw, p = pix - b * hw;
  out[t] = in[(b * C + c) * hw + p];
}

// softmax over the D + 1 logits of a pixel, the last bin dropped: [B, D + 1, h, w] -> [B, h, w, D]; a thread per pixel
// (the loads of a wave are contiguous for every bin), three passes over the logits
__global__ __launch_bounds__(kThreads) void pack_probs_kernel(const float* __restrict__ logits, int64_t pixels, int D,
                                                              int64_t hw, float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= pixels) return;
  const int64_t b = t / hw, p = t - b * hw;
  const float* x = logits + b * (D + 1) * hw + p;
  float m = x[0];
  for (int i = 1; i <= D; ++i) {
    const float v = x[(int64_t)i * hw];
    m = (v > m || v != v) ? v : m;
  }
  float s = 0.f;
  for (int i = 0; i <= D; ++i) s = s + pd3::lm::expf(x[(int64_t)i * hw] - m);
  float* o = out + t * D;
  for (int i = 0; i < D; ++i) o[i] = pd3::lm::expf(x[(int64_t)i * hw] - m) / s;
}

// weight [C_out, C * Z] -> [z][step][lane][N-tile]: the B fragments of a wave, contiguous per lane
__global__ __launch_bounds__(kThreads) void pack_weight_kernel(const float* __restrict__ w, int C, int Z, int NT,
                                                               float* __restrict__ out) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= Z * C * NT * 16) return;
  const int nt = t % NT, lane = (t / NT) % 64, step = (t / (NT * 64)) % (C / 4), z = t / (NT * 16 * C);
  const int o = 16 * nt + (lane & 15), c = 16 * (step >> 2) + 4 * (lane >> 4) + (step & 3);
  out[t] = w[(int64_t)o * C * Z + (int64_t)c * Z + z];
}

// ---- frustum_to_voxel -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void frustum_to_voxel_kernel(const float* __restrict__ feat,
                                                                    const float* __restrict__ prob,
                                                                    const float* __restrict__ l2c,
                                                                    const float* __restrict__ c2i,
                                                                    const int* __restrict__ image_shape, GridArgs a,
                                                                    int C, float* __restrict__ out) {
  const int b = blockIdx.y;
  const int64_t yx = (int64_t)a.X * a.Y, total = yx * a.Z;
  const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;  // (iz, iy, ix), ix fastest: the output's order
  if (v >= total) return;
  const Frame f = load_frame(l2c, c2i, image_shape, a, b);
  const int ix = (int)(v % a.X), iy = (int)((v / a.X) % a.Y), iz = (int)(v / yx);
  float gx, gy, gz;
  frustum_coords(f, a, ix, iy, iz, gx, gy, gz);
  const int64_t hw = (int64_t)a.h * a.w;
  const Geo q = sample_geo(gx, gy, gz, a, prob + (int64_t)b * hw * a.D);
  const float* fb = feat + (int64_t)b * hw * C;
  const float* r[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = q.o[j] >= 0 ? fb + (int64_t)q.o[j] * C : nullptr;
  float* o = out + (int64_t)b * C * total + v;
  for (int c = 0; c < C; ++c) {
    float fv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) fv[j] = r[j] ? r[j][c] : 0.f;
    o[(int64_t)c * total] = ((q.g[0] * fv[0] + q.g[1] * fv[1]) + q.g[2] * fv[2]) + q.g[3] * fv[3];
  }
}

// ---- frustum_to_bev -------------------------------------------------------------------------------------------------

template <int NT>
__global__ __launch_bounds__(kThreads) void frustum_to_bev_kernel(
    const float* __restrict__ feat, const float* __restrict__ prob, const float* __restrict__ wp,
    const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ l2c,
    const float* __restrict__ c2i, const int* __restrict__ image_shape, GridArgs a, int C, float* __restrict__ out) {
  constexpr int MT = 4;
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int64_t yx = (int64_t)a.X * a.Y;
  const int64_t n0 = ((int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6)) * 64;
  if (n0 >= yx) return;  // whole waves leave; nothing below needs the block
  const Frame f = load_frame(l2c, c2i, image_shape, a, b);
  const int64_t n = n0 + lane < yx ? n0 + lane : yx - 1;
  const int ix = (int)(n % a.X), iy = (int)(n / a.X);
  const int64_t hw = (int64_t)a.h * a.w;
  const float* pb = prob + (int64_t)b * hw * a.D;
  const float* fb = feat + (int64_t)b * hw * C;
  const int col = lane & 15, kq = lane >> 4, KS = C / 4;  // KS MFMA steps per z

  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int z = 0; z < a.Z; ++z) {
    float gx, gy, gz;
    frustum_coords(f, a, ix, iy, z, gx, gy, gz);
    const Geo geo = sample_geo(gx, gy, gz, a, pb);
    float g[MT][4];
    int o[MT][4];  // the lane's four floats of the corner's row start at pixel * C + 4 kq; -1: out of range
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        g[m][j] = __shfl(geo.g[j], 16 * m + col);
        const int pix = __shfl(geo.o[j], 16 * m + col);
        o[m][j] = pix >= 0 ? pix * C + 4 * kq : -1;
      }
    const float* wz = wp + ((int64_t)z * KS * 64 + lane) * NT;
    for (int q = 0; q < C / 16; ++q) {
      float bw[4][NT];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int t = 0; t < NT; ++t) bw[jj][t] = wz[(int64_t)(4 * q + jj) * 64 * NT + t];
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        f32x4 fv[4];  // channels 16 q + 4 kq + (0 .. 3) of the four corners' rows: 16 bytes per lane and corner
#pragma unroll
        for (int j = 0; j < 4; ++j)
          fv[j] = o[m][j] >= 0 ? *reinterpret_cast<const f32x4*>(fb + o[m][j] + 16 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const float av = ((g[m][0] * fv[0][jj] + g[m][1] * fv[1][jj]) + g[m][2] * fv[2][jj]) + g[m][3] * fv[3][jj];
#pragma unroll
          for (int t = 0; t < NT; ++t)
            acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bw[jj][t], acc[m][t], 0, 0, 0);
        }
      }
    }
  }

  // D: column lane & 15 is the output channel, rows 4 * (lane >> 4) + r are the BEV columns of the M-tile
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int oc = 16 * t + col;
    const float sc = scale[oc], sh = shift[oc];
    float* plane = out + ((int64_t)b * (16 * NT) + oc) * yx;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t nn = n0 + 16 * m + 4 * kq + r;
        if (nn < yx) plane[nn] = relu_keep_nan(sc * acc[m][t][r] + sh);
      }
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------
int make_args(int B, int D, int h, int w, int X, int Y, int Z, const float* pc_min, const float* voxel_size, int mode,
              double depth_min, double depth_max, GridArgs& a) {
  if (B < 0 || D < 1 || h < 1 || w < 1 || X < 1 || Y < 1 || Z < 1 || !pc_min || !voxel_size || mode < 0 || mode > 2)
    return PD3_EINVAL;
  if (B > 65535 || (int64_t)X * Y > INT32_MAX) return PD3_EUNSUPPORTED;
  a.B = B, a.X = X, a.Y = Y, a.Z = Z, a.D = D, a.h = h, a.w = w, a.mode = mode;
  for (int i = 0; i < 3; ++i) a.min[i] = pc_min[i], a.vox[i] = voxel_size[i];
  a.bins = (float)D;
  if (mode == 0) {
    a.c0 = (float)depth_min, a.c1 = (float)((depth_max - depth_min) / D);
  } else if (mode == 1) {
    a.c0 = (float)depth_min, a.c1 = (float)(2.0 * (depth_max - depth_min) / ((double)D * (1.0 + D)));
  } else {
    a.c0 = (float)std::log(1.0 + depth_min);
    a.c1 = (float)(std::log(1.0 + depth_max) - std::log(1.0 + depth_min));
  }
  return PD3_OK;
}

size_t packed_bytes(int B, int C, int D, int h, int w, int Z, int c_out) {
  const size_t pix = (size_t)B * h * w;
  return pd3::align_up(pix * D * sizeof(float), 256) + pd3::align_up(pix * C * sizeof(float), 256) +
         pd3::align_up((size_t)Z * C * c_out * sizeof(float), 256);
}

// prob and feat into the workspace
int pack(const float* image_features, const float* depth_logits, int B, int C, int D, int h, int w, float* prob,
         float* feat, hipStream_t s) {
  const int64_t hw = (int64_t)h * w, pixels = hw * B;
  hipLaunchKernelGGL(pack_probs_kernel, dim3((unsigned)pd3::ceil_div(pixels, kThreads)), dim3(kThreads), 0, s,
                     depth_logits, pixels, D, hw, prob);
  hipLaunchKernelGGL(pack_features_kernel, dim3((unsigned)pd3::ceil_div(pixels * C, kThreads)), dim3(kThreads), 0, s,
                     image_features, pixels * C, C, hw, feat);
  return pd3::launch_status();
}

bool maps_fit(int B, int C, int D, int h, int w) {
  const int64_t per = (int64_t)h * w * (C > D + 1 ? C : D + 1);
  return per <= INT32_MAX && pd3::ceil_div(per * B, kThreads) <= INT32_MAX;
}

}  // namespace

extern "C" {

int pd3_frustum_grid(const float* lidar_to_cam, const float* cam_to_img, const int32_t* image_shape, int batch,
                     int grid_x, int grid_y, int grid_z, const float* pc_min, const float* voxel_size, int mode,
                     double depth_min, double depth_max, int num_bins, float* grid, void* stream) {
  GridArgs a;
  const int st = make_args(batch, num_bins, 1, 1, grid_x, grid_y, grid_z, pc_min, voxel_size, mode, depth_min, depth_max, a);
  if (st != PD3_OK) return st;
  if (batch == 0) return PD3_OK;
  if (!lidar_to_cam || !cam_to_img || !image_shape || !grid) return PD3_EINVAL;
  const int64_t blocks = pd3::ceil_div((int64_t)grid_x * grid_y * grid_z, kThreads);
  if (blocks > INT32_MAX) return PD3_EUNSUPPORTED;
  hipLaunchKernelGGL(frustum_grid_kernel, dim3((unsigned)blocks, (unsigned)batch), dim3(kThreads), 0,
                     (hipStream_t)stream, lidar_to_cam, cam_to_img, image_shape, a, grid);
  return pd3::launch_status();
}

size_t pd3_frustum_to_voxel_workspace(int batch, int channels, int num_bins, int h, int w) {
  if (batch < 0 || channels < 1 || num_bins < 1 || h < 1 || w < 1) return 0;
  return packed_bytes(batch, channels, num_bins, h, w, 0, 0);
}

int pd3_frustum_to_voxel(const float* image_features, const float* depth_logits, const float* lidar_to_cam,
                         const float* cam_to_img, const int32_t* image_shape, int batch, int channels, int num_bins,
                         int h, int w, int grid_x, int grid_y, int grid_z, const float* pc_min,
                         const float* voxel_size, int mode, double depth_min, double depth_max, float* voxel_features,
                         void* workspace, size_t workspace_bytes, void* stream) {
  GridArgs a;
  const int st = make_args(batch, num_bins, h, w, grid_x, grid_y, grid_z, pc_min, voxel_size, mode, depth_min, depth_max, a);
  if (st != PD3_OK) return st;
  if (channels < 1) return PD3_EINVAL;
  if (batch == 0) return PD3_OK;
  if (!image_features || !depth_logits || !lidar_to_cam || !cam_to_img || !image_shape || !voxel_features || !workspace)
    return PD3_EINVAL;
  if (!maps_fit(batch, channels, num_bins, h, w)) return PD3_EUNSUPPORTED;
  if (workspace_bytes < packed_bytes(batch, channels, num_bins, h, w, 0, 0)) return PD3_EWORKSPACE;
  const int64_t blocks = pd3::ceil_div((int64_t)grid_x * grid_y * grid_z, kThreads);
  if (blocks > INT32_MAX) return PD3_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  pd3::Carver cv(workspace);
  const size_t pix = (size_t)batch * h * w;
  float* prob = cv.take<float>(pix * num_bins);
  float* feat = cv.take<float>(pix * channels);
  const int ps = pack(image_features, depth_logits, batch, channels, num_bins, h, w, prob, feat, s);
  if (ps != PD3_OK) return ps;
  hipLaunchKernelGGL(frustum_to_voxel_kernel, dim3((unsigned)blocks, (unsigned)batch), dim3(kThreads), 0, s, feat, prob,
                     lidar_to_cam, cam_to_img, image_shape, a, channels, voxel_features);
  return pd3::launch_status();
}

size_t pd3_frustum_to_bev_workspace(int batch, int channels, int num_bins, int h, int w, int grid_z, int c_out) {
  if (batch < 0 || channels < 1 || num_bins < 1 || h < 1 || w < 1 || grid_z < 1 || c_out < 1) return 0;
  return packed_bytes(batch, channels, num_bins, h, w, grid_z, c_out);
}

int pd3_frustum_to_bev(const float* image_features, const float* depth_logits, const float* lidar_to_cam,
                       const float* cam_to_img, const int32_t* image_shape, int batch, int channels, int num_bins,
                       int h, int w, int grid_x, int grid_y, int grid_z, const float* pc_min, const float* voxel_size,
                       int mode, double depth_min, double depth_max, const float* weight, const float* scale,
                       const float* shift, int c_out, float* bev, void* workspace, size_t workspace_bytes,
                       void* stream) {
  GridArgs a;
  const int st = make_args(batch, num_bins, h, w, grid_x, grid_y, grid_z, pc_min, voxel_size, mode, depth_min, depth_max, a);
  if (st != PD3_OK) return st;
  if (channels < 1 || c_out < 1) return PD3_EINVAL;
  if (channels % 16 || channels > 64 || c_out % 16 || c_out > 64 || grid_z > 32) return PD3_EUNSUPPORTED;
  if (batch == 0) return PD3_OK;
  if (!image_features || !depth_logits || !lidar_to_cam || !cam_to_img || !image_shape || !weight || !scale ||
      !shift || !bev || !workspace)
    return PD3_EINVAL;
  if (!maps_fit(batch, channels, num_bins, h, w)) return PD3_EUNSUPPORTED;
  if (workspace_bytes < packed_bytes(batch, channels, num_bins, h, w, grid_z, c_out)) return PD3_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  pd3::Carver cv(workspace);
  const size_t pix = (size_t)batch * h * w;
  float* prob = cv.take<float>(pix * num_bins);
  float* feat = cv.take<float>(pix * channels);
  float* wp = cv.take<float>((size_t)grid_z * channels * c_out);
  const int ps = pack(image_features, depth_logits, batch, channels, num_bins, h, w, prob, feat, s);
  if (ps != PD3_OK) return ps;
  const int nt = c_out / 16;
  hipLaunchKernelGGL(pack_weight_kernel, dim3((unsigned)pd3::ceil_div((int64_t)grid_z * channels * c_out, kThreads)),
                     dim3(kThreads), 0, s, weight, channels, grid_z, nt, wp);
  const int64_t tiles = pd3::ceil_div((int64_t)grid_x * grid_y, 64);
  const dim3 grid((unsigned)pd3::ceil_div(tiles, kThreads / 64), (unsigned)batch);
#define PD3_F2B(NT)                                                                                                   \
  hipLaunchKernelGGL((frustum_to_bev_kernel<NT>), grid, dim3(kThreads), 0, s, feat, prob, wp, scale, shift,          \
                     lidar_to_cam, cam_to_img, image_shape, a, channels, bev)
  if (nt == 1)
    PD3_F2B(1);
  else if (nt == 2)
    PD3_F2B(2);
  else if (nt == 3)
    PD3_F2B(3);
  else
    PD3_F2B(4);
#undef PD3_F2B
  return pd3::launch_status();
}

}  // extern "C"
