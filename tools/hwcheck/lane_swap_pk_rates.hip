// Hardware check (gfx950): what the instructions cost that the F(4x4, 3x3) transforms could be rewritten with --
//   * v_permlane16_swap_b32 (one exchange of a (lo, hi) register pair between lanes l and l ^ 16) against the sequence the
//     pair transform uses for lanes l and l ^ 1: two v_mov_b32 quad_perm + two v_cndmask_b32;
//   * v_pk_add_f32 / v_pk_fma_f32 on an adjacent register pair against their two scalar twins;
// each ALONE (one wave per SIMD, nothing else) and as K units behind each of 36 v_mfma_f32_16x16x4_f32 of the same wave,
// fenced in place, as tools/hwcheck/mfma_valu_overlap.hip does for plain fmas.  A unit is one exchange of a pair, or one
// operation on both halves of a pair; the instructions per unit are in the table.
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

enum { FMA1, ADD1, SWAP16, SWAP16N, SEL4, PKADD, ADD2, PKFMA, FMA2, KINDS };
static const char* const kName[KINDS] = {"v_fma_f32 x1",
                                         "v_add_f32 x1",
                                         "v_permlane16_swap_b32 x1",
                                         "s_nop 1 + v_permlane16_swap x1",
                                         "v_mov dpp x2 + v_cndmask x2",
                                         "v_pk_add_f32 x1",
                                         "v_add_f32 x2",
                                         "v_pk_fma_f32 x1",
                                         "v_fma_f32 x2"};

// One unit on pair u % 8 (eight independent pairs: a unit never waits for the one before it, and the two wait states
// between a VALU write and a v_permlane16_swap / DPP read of the same register always lie between two units of one pair).
// The instructions are spelled out: left to the compiler, the scalar twins are paired up by the SLP vectoriser and the
// packed ones taken apart again.  SWAP16N carries the s_nop 1 the compiler puts in front of a swap whose operand was
// written by the instruction before it.
template <int KIND>
__device__ __forceinline__ void unit(float (&x)[8], float (&y)[8], f2 (&p)[8], const int u, const float b, const f2 b2,
                                     const f2 c2, const bool hf) {
  float &lo = x[u % 8], &hi = y[u % 8];
  f2& v = p[u % 8];
  if (KIND == FMA1 || KIND == FMA2) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(lo) : "v"(c2[0]), "v"(b));
  if (KIND == FMA2) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(hi) : "v"(c2[0]), "v"(b));
  if (KIND == ADD1 || KIND == ADD2) asm volatile("v_add_f32 %0, %0, %1" : "+v"(lo) : "v"(b));
  if (KIND == ADD2) asm volatile("v_add_f32 %0, %0, %1" : "+v"(hi) : "v"(b));
  if (KIND == SWAP16) asm volatile("v_permlane16_swap_b32 %0, %1" : "+v"(lo), "+v"(hi));
  if (KIND == SWAP16N) asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(lo), "+v"(hi));
  if (KIND == SEL4) {
    const float ph = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, hi), 0xB1, 0xf, 0xf, true));
    const float pl = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, lo), 0xB1, 0xf, 0xf, true));
    lo = hf ? ph : lo;
    hi = hf ? hi : pl;
  }
  if (KIND == PKADD) asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(v) : "v"(b2));
  if (KIND == PKFMA) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(v) : "v"(c2), "v"(b2));
}

// MF: 1 = K units behind each of 36 MFMAs, 0 = the units alone (36 x K per trip of the loop)
template <int KIND, int K, int MF>
__global__ __launch_bounds__(512) void k(float* out, long long* cyc, int iters) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wave >= 4) return;  // one wave per SIMD
  const float a = 1.0f + lane * 1e-3f, b = 0.5f - lane * 1e-3f;
  const bool hf = lane & 1;
  f4 acc[36];
  float x[8], y[8];
  f2 p[8];
  const f2 b2 = {b, b}, c2 = {1.0001f + lane * 1e-9f, 1.0001f};
#pragma unroll
  for (int c = 0; c < 36; ++c) acc[c] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    x[c] = a * (c + 1);
    y[c] = b * (c + 1);
    p[c] = (f2){x[c], y[c]};
  }
  const long long t0 = clock64();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int c = 0; c < 36; ++c) {
      if (MF) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[c], 0, 0, 0);
#pragma unroll
      for (int q = 0; q < K; ++q) unit<KIND>(x, y, p, c * K + q, b, b2, c2, hf);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  const long long t1 = clock64();
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < 36; ++c) s += acc[c][0] + acc[c][3];
#pragma unroll
  for (int c = 0; c < 8; ++c) s += p[c][0] + p[c][1] + x[c] + y[c];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
  if (blockIdx.x == 0 && lane == 0) cyc[wave] = t1 - t0;
}

template <int KIND, int K, int MF>
double run(float* out, long long* cyc) {
  const int iters = 100;
  for (int rep = 0; rep < 2; ++rep) {
    k<KIND, K, MF><<<256, 512>>>(out, cyc, iters);
    if (hipDeviceSynchronize() != hipSuccess) {
      printf("kernel failed\n");
      exit(1);
    }
  }
  long long h[4];
  (void)hipMemcpy(h, cyc, 32, hipMemcpyDeviceToHost);
  return (double)h[0] / (iters * 36);
}

template <int KIND>
void row(float* out, long long* cyc) {
  const double alone = run<KIND, 6, 0>(out, cyc) / 6;
  const double m1 = run<KIND, 1, 1>(out, cyc), m2 = run<KIND, 2, 1>(out, cyc), m3 = run<KIND, 3, 1>(out, cyc),
               m6 = run<KIND, 6, 1>(out, cyc);
  printf("%-30s | %6.2f | %5.1f | %5.1f | %5.1f | %5.1f | %5.2f\n", kName[KIND], alone, m1, m2, m3, m6, (m6 - m1) / 5);
}

int main() {
  float* out;
  long long* cyc;
  if (hipMalloc(&out, 256 * 512 * 4) != hipSuccess || hipMalloc(&cyc, 64) != hipSuccess) return 1;
  printf("bare stream of 36 v_mfma_f32_16x16x4_f32: %.1f cycles per MFMA\n", run<FMA1, 0, 1>(out, cyc));
  printf("unit                           | alone, cycles per unit | cycles per MFMA with K = 1 | 2 | 3 | 6 units behind it | per "
         "unit from K = 1 to 6\n");
  row<FMA1>(out, cyc);
  row<ADD1>(out, cyc);
  row<SWAP16>(out, cyc);
  row<SWAP16N>(out, cyc);
  row<SEL4>(out, cyc);
  row<PKADD>(out, cyc);
  row<ADD2>(out, cyc);
  row<PKFMA>(out, cyc);
  row<FMA2>(out, cyc);
  return 0;
}
