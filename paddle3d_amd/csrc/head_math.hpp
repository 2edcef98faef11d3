// Device helpers the head and set-abstraction kernels share.  Each is one fixed sequence of fp32 (or, where stated,
// double) operations: the arithmetic-order comments at the top of the .hip files and the numpy restatements under
// tests/golden/ rely on exactly these forms.
#pragma once
#include "libm_exact.hpp"

namespace pd3 {

// v > 0 ? v : +0, but a NaN stays a NaN (the reference's ReLU propagates it)
__device__ __forceinline__ float relu_keep_nan(float v) { return (v > 0.0f || v != v) ? v : 0.0f; }

// 1 / (1 + expf(-x)) with glibc's expf bits; `tab` reads the 32-entry exp2f table (lm::exp2f_tab_fill)
template <class Tab>
__device__ __forceinline__ float sigmoid_exact(float x, Tab tab) {
  return 1.0f / (1.0f + lm::expf_with(-x, tab));
}

// the inverse of a row-major 3x3 in double by the adjugate, rounded to fp32
static __device__ void inverse3(const float* __restrict__ m, float* out) {
  const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
  const double c00 = e * i - f * h, c01 = c * h - b * i, c02 = b * f - c * e;
  const double c10 = f * g - d * i, c11 = a * i - c * g, c12 = c * d - a * f;
  const double c20 = d * h - e * g, c21 = b * g - a * h, c22 = a * e - b * d;
  const double det = (a * c00 + b * c10) + c * c20;
  const double adj[9] = {c00, c01, c02, c10, c11, c12, c20, c21, c22};
  for (int k = 0; k < 9; ++k) out[k] = (float)(adj[k] / det);
}

// row r of the row-major 3x3 m times (p0, p1, p2)
__device__ __forceinline__ float mat3_row(const float* m, int r, float p0, float p1, float p2) {
  return (m[3 * r] * p0 + m[3 * r + 1] * p1) + m[3 * r + 2] * p2;
}

}  // namespace pd3
