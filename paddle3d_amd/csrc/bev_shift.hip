// BEVDet4D temporal BEV alignment: BEVDet4D.shift_feature + the channel concat of its two callers
// (paddle3d/models/detection/bevdet/bevdet4d.py:90-159, :194-216, :291-298) in one launch.
//
// out [B, F*C, H, W] (contiguous NCHW): channels [0, C) are the current frame copied bit for bit, channels
// [f*C, (f+1)*C) the adjacent frame f warped into the current ego frame by grid_sample(bilinear, zeros,
// align_corners=True) on the grid tf @ (x, y, 1).
//
// Arithmetic (fixed order, -ffp-contract=off; tests/golden/bevdet4d_align_numpy.py restates it):
//   tf   per (frame, batch) entry in double (bda @ [R|t], closed-form affine inverse, the [0,1,3] slice and
//        inv(feat2bev) @ . @ feat2bev as written out in bs_transform), rounded to fp32 once.
//   grid gx = (tf00*x + tf01*y) + tf02; nx = (gx / (W-1)) * 2 - 1; ix = ((nx + 1) / 2) * (W-1); y alike.
//   sample corners floor(ix), floor(ix)+1 (rows alike); weights nw = (ix1-ix)*(iy1-iy), ne = (ix-ix0)*(iy1-iy),
//        sw = (ix1-ix)*(iy-iy0), se = (ix-ix0)*(iy-iy0); acc = 0, then acc += v*w over the in-range corners in
//        the order nw, ne, sw, se.  Coordinates are range-checked in float (NaN fails the test) before they are
//        converted to integers, so no non-finite or far-away coordinate becomes an address.
//
// Mapping: one 256-thread workgroup per (frame, batch, 64 consecutive output pixels of the H*W plane).
//   * source with stride_c == 1 (the channels-last view voxel_pooling_v2 returns): each bilinear corner is a
//     contiguous run of C floats.  Lanes run over channels for the loads (one 256-B read per corner and wave),
//     the weighted sums go to a 64 x 64 LDS tile (row pitch 65: conflict-free both ways), and lanes run over the
//     64 pixels for the stores (one 256-B row per channel and wave).
//   * any other source (contiguous NCHW, feat_prev): lanes over the 64 pixels, the 4 waves over channels
//     c = wave, wave + 4, ...; a small ego motion keeps neighbouring pixels' corners neighbours, the stores are
//     256-B rows.
// All offsets are 64-bit.
#include <cmath>

#include "common.hpp"

namespace {

constexpr int kMaxFrames = 16;
constexpr int kPix = 64;       // output pixels per workgroup
constexpr int kThreads = 256;  // 4 waves
constexpr int kChunk = 64;     // channels per LDS tile (channels-last path)

struct AlignArgs {
  const float* feat[kMaxFrames];
  int64_t stride[kMaxFrames][4];  // n, c, h, w in elements
  // adjacent frames only (index 1 .. F-1; entry 0 unused): camera 0's pose of batch entry b at ptr + b * batch stride
  const float* rot_cur[kMaxFrames];
  const float* tr_cur[kMaxFrames];
  const float* rot_adj[kMaxFrames];
  const float* tr_adj[kMaxFrames];
  const float* bda[kMaxFrames];
  const float* bda_adj[kMaxFrames];  // NULL: bda
  int64_t pose_stride[kMaxFrames][6];  // batch strides of rot_cur, tr_cur, rot_adj, tr_adj, bda, bda_adj
  int num_frame, first, batch, C, H, W;  // first = 0: frame 0 is copied into channels [0, C); 1: no current frame
  double sx, sy, lx, ly;  // feat2bev: grid_interval[0:2], grid_lower_bound[0:2]
  float* out;
  float* out_grid;  // [(F-1)*B, H, W, 2] or NULL
};

__device__ void load33(const float* p, double m[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) m[i][j] = (double)p[i * 3 + j];
}

// D @ R and D @ t, each sum as (a0 + a1) + a2
__device__ void affine(const double D[3][3], const double R[3][3], const double t[3], double A[3][3], double a[3]) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) A[i][j] = (D[i][0] * R[0][j] + D[i][1] * R[1][j]) + D[i][2] * R[2][j];
    a[i] = (D[i][0] * t[0] + D[i][1] * t[1]) + D[i][2] * t[2];
  }
}

// rows 0 and 1 of tf for one (frame, batch) entry; bs_transform in the restatement is the same text
__device__ void bs_transform(const AlignArgs& g, int f, int b, float tf[6]) {
  const int64_t* ps = g.pose_stride[f];
  double R0[3][3], R1[3][3], D[3][3], Da[3][3], t0[3], t1[3];
  load33(g.rot_cur[f] + b * ps[0], R0);
  load33(g.rot_adj[f] + b * ps[2], R1);
  load33(g.bda[f] + b * ps[4], D);
  load33(g.bda_adj[f] ? g.bda_adj[f] + b * ps[5] : g.bda[f] + b * ps[4], Da);
  for (int i = 0; i < 3; ++i) {
    t0[i] = (double)g.tr_cur[f][b * ps[1] + i];
    t1[i] = (double)g.tr_adj[f][b * ps[3] + i];
  }
  double A0[3][3], a0[3], A[3][3], a1[3];
  affine(D, R0, t0, A0, a0);   // c02l0 = bda4 @ [R0 t0; 0 1]
  affine(Da, R1, t1, A, a1);   // c12l0 = bda4' @ [R1 t1; 0 1]
  // inverse(c12l0) = [Bi, -Bi a1; 0 1], Bi = adj(A) / det(A)  (bda may scale or flip: no rigid shortcut)
  const double c00 = A[1][1] * A[2][2] - A[1][2] * A[2][1];
  const double c01 = A[1][2] * A[2][0] - A[1][0] * A[2][2];
  const double c02 = A[1][0] * A[2][1] - A[1][1] * A[2][0];
  const double det = (A[0][0] * c00 + A[0][1] * c01) + A[0][2] * c02;
  double Bi[3][3];
  Bi[0][0] = c00 / det;
  Bi[0][1] = (A[0][2] * A[2][1] - A[0][1] * A[2][2]) / det;
  Bi[0][2] = (A[0][1] * A[1][2] - A[0][2] * A[1][1]) / det;
  Bi[1][0] = c01 / det;
  Bi[1][1] = (A[0][0] * A[2][2] - A[0][2] * A[2][0]) / det;
  Bi[1][2] = (A[0][2] * A[1][0] - A[0][0] * A[1][2]) / det;
  Bi[2][0] = c02 / det;
  Bi[2][1] = (A[0][1] * A[2][0] - A[0][0] * A[2][1]) / det;
  Bi[2][2] = (A[0][0] * A[1][1] - A[0][1] * A[1][0]) / det;
  double bi[3];
  for (int i = 0; i < 3; ++i) bi[i] = -((Bi[i][0] * a1[0] + Bi[i][1] * a1[1]) + Bi[i][2] * a1[2]);
  // l02l1 = c02l0 @ inverse(c12l0), rows / columns [0, 1, 3]
  double T[2][3];
  for (int i = 0; i < 2; ++i) {
    for (int j = 0; j < 2; ++j) T[i][j] = (A0[i][0] * Bi[0][j] + A0[i][1] * Bi[1][j]) + A0[i][2] * Bi[2][j];
    T[i][2] = ((A0[i][0] * bi[0] + A0[i][1] * bi[1]) + A0[i][2] * bi[2]) + a0[i];
  }
  // tf = inv(feat2bev) @ T @ feat2bev, feat2bev = [[sx, 0, lx], [0, sy, ly], [0, 0, 1]]
  const double s[2] = {g.sx, g.sy}, l[2] = {g.lx, g.ly};
  for (int i = 0; i < 2; ++i) {
    tf[i * 3 + 0] = (float)((T[i][0] * g.sx) / s[i]);
    tf[i * 3 + 1] = (float)((T[i][1] * g.sy) / s[i]);
    tf[i * 3 + 2] = (float)((((T[i][0] * g.lx + T[i][1] * g.ly) + T[i][2]) - l[i]) / s[i]);
  }
}

// Bilinear set-up of one output pixel: base offset of the nw corner (h, w part), the four weights and the
// in-range mask (bit 0 nw, 1 ne, 2 sw, 3 se).  Writes the normalised grid when asked.
struct Tap {
  int64_t off;
  float w[4];
  int mask;
};

__device__ Tap bs_tap(const float tf[6], int p, int H, int W, int64_t sh, int64_t sw, float* grid_out) {
  const float x = (float)(p % W), y = (float)(p / W);
  const float gx = (tf[0] * x + tf[1] * y) + tf[2];
  const float gy = (tf[3] * x + tf[4] * y) + tf[5];
  const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
  const float nx = (gx / wm1) * 2.0f - 1.0f;
  const float ny = (gy / hm1) * 2.0f - 1.0f;
  if (grid_out) {
    grid_out[2 * (int64_t)p] = nx;
    grid_out[2 * (int64_t)p + 1] = ny;
  }
  const float ix = ((nx + 1.0f) / 2.0f) * wm1;
  const float iy = ((ny + 1.0f) / 2.0f) * hm1;
  Tap t;
  t.off = 0;
  t.mask = 0;
  t.w[0] = t.w[1] = t.w[2] = t.w[3] = 0.0f;
  // some corner is in range iff -1 <= ix < W and -1 <= iy < H; NaN fails both comparisons
  if (!(ix >= -1.0f && ix < (float)W && iy >= -1.0f && iy < (float)H)) return t;
  const float ix0 = floorf(ix), iy0 = floorf(iy);
  const float ix1 = ix0 + 1.0f, iy1 = iy0 + 1.0f;
  const int x0 = (int)ix0, y0 = (int)iy0;  // in [-1, W-1] x [-1, H-1]
  t.w[0] = (ix1 - ix) * (iy1 - iy);
  t.w[1] = (ix - ix0) * (iy1 - iy);
  t.w[2] = (ix1 - ix) * (iy - iy0);
  t.w[3] = (ix - ix0) * (iy - iy0);
  const bool xl = x0 >= 0, xr = x0 + 1 < W, yt = y0 >= 0, yb = y0 + 1 < H;
  t.mask = (xl && yt ? 1 : 0) | (xr && yt ? 2 : 0) | (xl && yb ? 4 : 0) | (xr && yb ? 8 : 0);
  t.off = (int64_t)y0 * sh + (int64_t)x0 * sw;  // may point before the plane; only masked corners are read
  return t;
}

// corner k of a tap at source pointer `src` (channel already applied)
__device__ __forceinline__ float bs_sample(const float* src, const Tap& t, int64_t sh, int64_t sw) {
  float acc = 0.0f;
  if (t.mask & 1) acc = acc + src[t.off] * t.w[0];
  if (t.mask & 2) acc = acc + src[t.off + sw] * t.w[1];
  if (t.mask & 4) acc = acc + src[t.off + sh] * t.w[2];
  if (t.mask & 8) acc = acc + src[t.off + sh + sw] * t.w[3];
  return acc;
}

__global__ void __launch_bounds__(kThreads) bev_align_kernel(AlignArgs g) {
  __shared__ float s_tf[6];
  __shared__ int64_t s_off[kPix];
  __shared__ float s_w[kPix][4];
  __shared__ int s_mask[kPix];
  __shared__ float s_tile[kChunk][kPix + 1];

  const int HW = g.H * g.W;
  const int fb = blockIdx.y;  // frame-major: (f - first, b)
  const int f = g.first + fb / g.batch, b = fb % g.batch;
  const int nout = g.num_frame - g.first;  // channel blocks of the output
  const int p0 = blockIdx.x * kPix;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int npix = min(kPix, HW - p0);
  const int64_t sn = g.stride[f][0], sc = g.stride[f][1], sh = g.stride[f][2], sw = g.stride[f][3];
  const float* src = g.feat[f] + (int64_t)b * sn;
  float* dst = g.out + ((int64_t)b * nout + (f - g.first)) * g.C * HW + p0;
  const bool chlast = sc == 1;

  if (f > 0) {
    if (tid == 0) bs_transform(g, f, b, s_tf);
    __syncthreads();
  }
  const int64_t HW64 = HW;

  if (!chlast) {
    // lanes over pixels, waves over channels
    if (lane >= npix) return;
    const int p = p0 + lane;
    if (f == 0) {
      const int64_t o = (int64_t)(p / g.W) * sh + (int64_t)(p % g.W) * sw;
      int c = wave;
      for (; c + 12 < g.C; c += 16) {  // four loads in flight before the stores (dst may alias src for the compiler)
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = src[(c + 4 * u) * sc + o];
#pragma unroll
        for (int u = 0; u < 4; ++u) dst[(c + 4 * u) * HW64 + lane] = v[u];
      }
      for (; c < g.C; c += 4) dst[c * HW64 + lane] = src[c * sc + o];
      return;
    }
    float tf[6];
    for (int k = 0; k < 6; ++k) tf[k] = s_tf[k];
    float* gout = (g.out_grid && wave == 0) ? g.out_grid + (int64_t)((f - 1) * g.batch + b) * HW * 2 : nullptr;
    const Tap t = bs_tap(tf, p, g.H, g.W, sh, sw, gout);
    int c = wave;
    for (; c + 12 < g.C; c += 16) {  // four channels' corner loads in flight before the stores
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = bs_sample(src + (c + 4 * u) * sc, t, sh, sw);
#pragma unroll
      for (int u = 0; u < 4; ++u) dst[(c + 4 * u) * HW64 + lane] = v[u];
    }
    for (; c < g.C; c += 4) dst[c * HW64 + lane] = bs_sample(src + c * sc, t, sh, sw);
    return;
  }

  // channels-last source: taps in LDS, lanes over channels for the loads, LDS transpose, lanes over pixels to store
  if (tid < kPix) {
    Tap t = {};
    if (tid < npix) {
      const int p = p0 + tid;
      if (f == 0) {
        t.off = (int64_t)(p / g.W) * sh + (int64_t)(p % g.W) * sw;
        t.mask = 0;
      } else {
        float tf[6];
        for (int k = 0; k < 6; ++k) tf[k] = s_tf[k];
        float* gout = g.out_grid ? g.out_grid + (int64_t)((f - 1) * g.batch + b) * HW * 2 : nullptr;
        t = bs_tap(tf, p, g.H, g.W, sh, sw, gout);
      }
    }
    s_off[tid] = t.off;
    s_mask[tid] = t.mask;
    for (int k = 0; k < 4; ++k) s_w[tid][k] = t.w[k];
  }
  __syncthreads();
  for (int c0 = 0; c0 < g.C; c0 += kChunk) {
    const int nc = min(kChunk, g.C - c0);
    for (int i = tid; i < kPix * kChunk; i += kThreads) {
      const int c = i % kChunk, q = i / kChunk;
      if (c >= nc || q >= npix) continue;
      const float* s = src + (int64_t)(c0 + c);  // sc == 1
      float v;
      if (f == 0) {
        v = s[s_off[q]];
      } else {
        Tap t;
        t.off = s_off[q];
        t.mask = s_mask[q];
        for (int k = 0; k < 4; ++k) t.w[k] = s_w[q][k];
        v = bs_sample(s, t, sh, sw);
      }
      s_tile[c][q] = v;
    }
    __syncthreads();
    for (int i = tid; i < kPix * kChunk; i += kThreads) {
      const int q = i % kPix, c = i / kPix;
      if (c < nc && q < npix) dst[(int64_t)(c0 + c) * HW64 + q] = s_tile[c][q];
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" {

int pd3_bevdet4d_align(const float* const* feats, const int64_t* strides, int num_frame, int with_current,
                       int batch, int channels, int feat_h, int feat_w, const float* const* rots_cur,
                       const float* const* trans_cur, const float* const* rots_adj, const float* const* trans_adj,
                       const float* const* bda, const float* const* bda_adj, const int64_t* pose_strides,
                       const float* grid_interval, const float* grid_lower_bound, float* out, float* out_grid,
                       void* stream) {
  if (!feats || !strides || !out || !grid_interval || !grid_lower_bound) return PD3_EINVAL;
  if (num_frame < 1 || batch < 1 || channels < 1 || feat_h < 1 || feat_w < 1) return PD3_EINVAL;
  if (!with_current && num_frame < 2) return PD3_EINVAL;
  if (num_frame > kMaxFrames) return PD3_EUNSUPPORTED;
  // the grid normalises by (W-1) and (H-1); the plane index is int; the workgroup grid's y is (frame, batch)
  if (feat_h < 2 || feat_w < 2 || (int64_t)feat_h * feat_w > (int64_t)1 << 30) return PD3_EUNSUPPORTED;
  if ((int64_t)num_frame * batch > 65535) return PD3_EUNSUPPORTED;
  AlignArgs g = {};
  g.first = with_current ? 0 : 1;
  for (int f = g.first; f < num_frame; ++f) {
    if (!feats[f]) return PD3_EINVAL;
    g.feat[f] = feats[f];
    for (int k = 0; k < 4; ++k) g.stride[f][k] = strides[f * 4 + k];
  }
  if (num_frame > 1 && (!rots_cur || !trans_cur || !rots_adj || !trans_adj || !bda || !pose_strides))
    return PD3_EINVAL;
  for (int f = 1; f < num_frame; ++f) {
    const int a = f - 1;
    if (!rots_cur[a] || !trans_cur[a] || !rots_adj[a] || !trans_adj[a] || !bda[a]) return PD3_EINVAL;
    g.rot_cur[f] = rots_cur[a];
    g.tr_cur[f] = trans_cur[a];
    g.rot_adj[f] = rots_adj[a];
    g.tr_adj[f] = trans_adj[a];
    g.bda[f] = bda[a];
    g.bda_adj[f] = bda_adj ? bda_adj[a] : nullptr;
    for (int k = 0; k < 6; ++k) g.pose_stride[f][k] = pose_strides[a * 6 + k];
  }
  if (!std::isfinite(grid_interval[0]) || !std::isfinite(grid_interval[1]) || grid_interval[0] == 0.0f ||
      grid_interval[1] == 0.0f)
    return PD3_EINVAL;
  g.num_frame = num_frame;
  g.batch = batch;
  g.C = channels;
  g.H = feat_h;
  g.W = feat_w;
  g.sx = grid_interval[0];
  g.sy = grid_interval[1];
  g.lx = grid_lower_bound[0];
  g.ly = grid_lower_bound[1];
  g.out = out;
  g.out_grid = out_grid;
  const int64_t hw = (int64_t)feat_h * feat_w;
  dim3 grid((unsigned)pd3::ceil_div(hw, kPix), (unsigned)((num_frame - g.first) * batch));
  hipLaunchKernelGGL(bev_align_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, g);
  return pd3::launch_status();
}

}  // extern "C"
