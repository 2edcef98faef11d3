// Hardware property the default hard_voxelize path rests on (voxelize_wave.hpp:125,296,345; voxelize_tiled.hpp:17-18):
// for ONE wave-wide returning LDS add (ds_add_rtn_u32), lanes that hit the same LDS word receive their "old" values
// in ASCENDING LANE ORDER, and successive LDS instructions of a wave execute in program order -- that is what makes
// the slot a point gets equal to the number of earlier points of its cell (the reference's sequential scan,
// voxelize_op.cc:47-78) without a sort.  The ISA documents neither; tools/hwcheck/lds_atomic_order.hip measured it
// (0 mismatches in 4.2 M on gfx950).  This entry point runs the same probe through the library, compiled with the
// library's flags, so that tests/test_properties_gpu.py::test_lds_atomic_lane_order can assert it on every GPU test run
// and a caller can assert it at start-up on a new part or driver.
#include "../../include/paddle3d_amd.h"
#include "block_topk.hpp"
#include "common.hpp"

namespace pd3 {

__global__ void lds_atomic_order_kernel(const uint32_t* __restrict__ addr, uint32_t* __restrict__ old, int rounds,
                                        int table) {
  extern __shared__ uint32_t sc_cnt[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t* c = sc_cnt + wave * table;
  for (int d = lane; d < table; d += 64) c[d] = 0;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const size_t base = ((size_t)blockIdx.x * (blockDim.x >> 6) + wave) * rounds * 64;
  for (int r = 0; r < rounds; ++r) {
    const uint32_t a = addr[base + r * 64 + lane];
    uint32_t o = 0xFFFFFFFFu;
    if (a != 0xFFFFFFFFu) o = atomicAdd(&c[a], 1u);  // the form the voxelizer uses: divergent lanes skip the add
    old[base + r * 64 + lane] = o;
  }
}

// The block top-K selection of block_topk.hpp on raw keys: one kTopkThreads workgroup per set runs block_topk_cut,
// one of the two compactions and block_topk_sort with the functors of the simplest caller (low(i, pos) = i), so that
// tests/test_topk_lattice_gpu.py can place every digit, tie and size border exactly -- through the heads a key is a
// sigmoid's bits, which cannot.  FORM 0: keys read from global memory, block_topk_compact (ssd_topk_kernel's shape);
// FORM 1: keys staged into LDS behind cp_topk_kernel's padding, block_topk_compact_chunks.
// The header's preconditions are the caller's to keep (more than K keys visited; a key left out sorts after every key
// taken); a launch that breaks one would run the compaction past the list's kTopkMaxK entries.  The probe counts
// instead of trusting: a set that breaks one gets 0xFFFFFFFF in every output word, the cut's two included.
constexpr int kProbeMaxLdsKeys = 16384;     // FORM 1: keys held in LDS (cp_topk_kernel's kTopkMaxHw)
constexpr uint32_t kProbeTakeAll = 0xFFFFFFFFu;  // skip_cut: the cut-off that takes every key below it

__device__ __forceinline__ int probe_kidx(int i) { return i + (i >> 4); }  // postprocess.hip kidx
static inline size_t probe_topk_lds(int form, int n) {
  const size_t ks = form ? ((size_t)n + n / 16 + 2) & ~(size_t)1 : 0;
  return (size_t)pd3::kTopkMaxK * 8 + ((size_t)pd3::kTopkHistWords + pd3::kTopkScratch + ks) * 4;
}

template <int FORM>
__global__ __launch_bounds__(kTopkThreads) void block_topk_probe_kernel(const uint32_t* __restrict__ keys, int n, int K,
                                                                        int key_bits, uint32_t leave_out,
                                                                        int has_leave_out, int skip_cut,
                                                                        uint32_t* __restrict__ idx,
                                                                        uint32_t* __restrict__ key_out,
                                                                        uint32_t* __restrict__ cut_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char probe_smem[];
  unsigned long long* list = reinterpret_cast<unsigned long long*>(probe_smem);  // [kTopkMaxK]
  int* hist = reinterpret_cast<int*>(list + kTopkMaxK);                          // [kTopkHistWords]
  int* scr = hist + kTopkHistWords;                                              // [kTopkScratch]
  uint32_t* ks = reinterpret_cast<uint32_t*>(scr + kTopkScratch);                // FORM 1: [n] behind probe_kidx
  const int set = blockIdx.x, t = threadIdx.x;
  const uint32_t* kg = keys + (int64_t)set * n;
  if (FORM == 1) {
    for (int i = t; i < n; i += kTopkThreads) ks[probe_kidx(i)] = kg[i];
    __syncthreads();
  }
  const auto key = [&](int i) { return FORM == 1 ? ks[probe_kidx(i)] : kg[i]; };
  const auto visit = [&](auto f) {
    for (int i = t; i < n; i += kTopkThreads) {
      const uint32_t k = key(i);
      if (!(has_leave_out && k == leave_out)) f(k);
    }
  };
  const auto refuse = [&]() {
    if (t < K) idx[(int64_t)set * K + t] = key_out[(int64_t)set * K + t] = 0xFFFFFFFFu;
    if (t == 0) cut_out[set * 2] = cut_out[set * 2 + 1] = 0xFFFFFFFFu;
  };
  // precondition of the cut: more than K keys counted; of the take-all cut: no more than K keys below it
  int mine = 0, total;
  if (skip_cut) {
    for (int i = t; i < n; i += kTopkThreads) mine += key(i) < kProbeTakeAll ? 1 : 0;
  } else {
    visit([&](uint32_t k) { mine += (k >> key_bits) == 0u ? 1 : 0; });
  }
  block_exclusive_scan<kTopkThreads>(mine, scr, total);
  if (skip_cut ? total > K : total <= K) return refuse();  // uniform
  const TopkCut cut = skip_cut ? TopkCut{kProbeTakeAll, 0} : block_topk_cut(K, key_bits, hist, scr, visit);
  // precondition of the compaction: what the cut takes fits the list (a left-out key below kc would be taken too)
  mine = 0;
  for (int i = t; i < n; i += kTopkThreads) mine += key(i) < cut.kc ? 1 : 0;
  block_exclusive_scan<kTopkThreads>(mine, scr, total);
  if (cut.r < 0 || total + cut.r > K) return refuse();  // uniform
  const auto low = [](int i, int) { return (uint32_t)i; };
  if (FORM == 1)
    block_topk_compact_chunks(cut, n, key, low, list, scr);
  else
    block_topk_compact(cut, n, key, low, list, scr);
  block_topk_sort(list, K);
  if (t < K) {
    idx[(int64_t)set * K + t] = (uint32_t)list[t];
    key_out[(int64_t)set * K + t] = (uint32_t)(list[t] >> 32);
  }
  if (t == 0) cut_out[set * 2] = cut.kc, cut_out[set * 2 + 1] = (uint32_t)cut.r;
}

}  // namespace pd3

extern "C" int pd3_selfcheck_block_topk(const uint32_t* keys, int sets, int n, int K, int key_bits, int form,
                                        int64_t leave_out, int skip_cut, uint32_t* idx, uint32_t* key, uint32_t* cut,
                                        void* stream) {
  if (!keys || !idx || !key || !cut || sets < 0 || n < 1 || K < 1 || K > pd3::kTopkMaxK || key_bits < 1 ||
      key_bits > 30 || form < 0 || form > 1 || (form == 1 && n > pd3::kProbeMaxLdsKeys) || leave_out > 0xFFFFFFFFll)
    return PD3_EINVAL;
  if (sets == 0) return PD3_OK;
  const auto kernel = form ? pd3::block_topk_probe_kernel<1> : pd3::block_topk_probe_kernel<0>;
  if (const int rc = pd3::launch_lds(kernel, (unsigned)sets, pd3::kTopkThreads, pd3::probe_topk_lds(form, n),
                                     static_cast<hipStream_t>(stream), keys, n, K, key_bits,
                                     (uint32_t)(leave_out < 0 ? 0 : leave_out), leave_out < 0 ? 0 : 1, skip_cut ? 1 : 0,
                                     idx, key, cut))
    return rc;
  return pd3::launch_status();
}

extern "C" int pd3_selfcheck_lds_atomic_order(const uint32_t* addr, uint32_t* old, int blocks, int waves_per_block,
                                              int rounds, int table, void* stream) {
  if (!addr || !old || blocks <= 0 || waves_per_block <= 0 || waves_per_block > 16 || rounds <= 0 || table <= 0 ||
      (size_t)waves_per_block * table * 4 > 64 * 1024)
    return PD3_EINVAL;
  pd3::lds_atomic_order_kernel<<<(unsigned)blocks, waves_per_block * 64, (size_t)waves_per_block * table * 4,
                                 static_cast<hipStream_t>(stream)>>>(addr, old, rounds, table);
  return pd3::launch_status();
}
