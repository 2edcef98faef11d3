// Exact top-K selection by one 1024-thread workgroup: the K smallest of a set of 32-bit keys, in ascending
// (key, index) order -- the order a stable sort of the keys gives.  The post-processing kernels (postprocess.hip
// cp_topk_kernel, ssd_head.hip ssd_topk_kernel, bevdet_postprocess.hip bd_select_decode_kernel) use it in place of a
// full sort when only the first K <= 1024 entries are needed.  Three steps, each a block-wide call:
//   1. block_topk_cut      radix select: the cut-off key kc and the number r of keys equal to kc that are taken
//   2. block_topk_compact  the taken entries, in index order, into an LDS list of (key << 32 | payload)
//      (block_topk_compact_chunks: the same for keys in LDS)
//   3. block_topk_sort     bitonic sort of that list
// The caller's memory access is passed in as functors: the keys may live in LDS or in global memory.
#pragma once
#include "common.hpp"

namespace pd3 {

constexpr int kTopkThreads = 1024;  // workgroup size of every caller
constexpr int kTopkMaxK = 1024;     // entries of the sorted list (one per thread)
constexpr int kTopkCopies = 8;      // histogram replicas (lane & 7): scores crowd into a handful of bins, and LDS
                                    // atomics of one wave on one address run one lane at a time
constexpr int kTopkHistWords = kTopkCopies * 1024;  // ints of the `hist` argument
constexpr int kTopkScratch = 48;                    // ints of the `scr` argument

// Taken: every key < kc, and the first r keys (in index order) equal to kc.
struct TopkCut {
  uint32_t kc;
  int r;
};

// A score in [0, 1] as a key: bits(1.0f) - bits(score), ascending key = descending score.
constexpr uint32_t kScoreKeyOne = 0x3F800000u;        // bits of 1.0f
constexpr uint32_t kScoreKeyAll = kScoreKeyOne + 2u;  // a cut-off that takes every key (one above a caller's NaN key)
constexpr int kScoreKeyBits = 30;                     // bits such a key can have

// Bits a score key bits(1.0f) - bits(score) can have when the scores taken are above (or at) `score_threshold`.
static inline int topk_key_bits(float score_threshold) {
  const uint32_t thr_bits = __builtin_bit_cast(uint32_t, score_threshold);
  const bool below_one = score_threshold > 0.f && thr_bits < kScoreKeyOne;
  return 32 - __builtin_clz(below_one ? kScoreKeyOne - thr_bits : kScoreKeyOne);  // 1 .. 30
}

// Cut-off of the K smallest keys.  `visit(f)` calls f(key) for every key of this thread that can be taken (any split
// of the keys over the threads); more than K keys must be visited in all.  Keys at or above 2^key_bits (1 <= key_bits
// <= 30) are never counted, so a sentinel above that costs no histogram atomics; a caller whose never-taken sentinel
// lies below 2^key_bits leaves it out in `visit`.  A key left out either way must sort after every key taken.
// Ten bits at a time from the top, over the bits a taken key can have (a digit from bits that are all zero would put
// every key into one bin); it stops as soon as the bin holding the cut-off is taken whole, which after two digits
// (16 k keys over a million bins) it nearly always is: then r = 0 and kc is the end of that bin.  Any exact select
// takes the same entries, whatever (kc, r) it returns for them.
// `hist`: kTopkHistWords ints of LDS, `scr`: kTopkScratch ints of LDS.  Ends with a block barrier.
template <typename Visit>
__device__ __forceinline__ TopkCut block_topk_cut(int K, int key_bits, int* hist, int* scr, Visit visit) {
  const int t = threadIdx.x;
  uint32_t prefix = 0;  // decided high bits
  int need = K;         // rank of the cut-off inside the still-undecided set (1-based)
  int hi = key_bits;    // bits [0, hi) are undecided
  int* const mine = hist + (t & (kTopkCopies - 1)) * 1024;
  while (hi > 0) {
    const int w = min(hi, 10), shift = hi - w;
#pragma unroll
    for (int c = 0; c < kTopkCopies; ++c) hist[c * 1024 + t] = 0;
    __syncthreads();
    visit([&](uint32_t k) {
      if ((k >> hi) == prefix) atomicAdd(&mine[(k >> shift) & ((1u << w) - 1u)], 1);
    });
    __syncthreads();
    int hh = 0;  // thread t owns bin t
#pragma unroll
    for (int c = 0; c < kTopkCopies; ++c) hh += hist[c * 1024 + t];
    int total;
    const int cum = block_exclusive_scan<kTopkThreads>(hh, scr, total);
    if (need > cum && need <= cum + hh) {  // exactly one bin holds rank `need`
      scr[kTopkScratch - 3] = hh;
      scr[kTopkScratch - 2] = t;
      scr[kTopkScratch - 1] = need - cum;
    }
    __syncthreads();
    const int in_bin = scr[kTopkScratch - 3];
    prefix = (prefix << w) | (uint32_t)scr[kTopkScratch - 2];
    need = scr[kTopkScratch - 1];
    hi = shift;
    __syncthreads();
    if (need == in_bin) {  // the whole bin is taken: every key below the next prefix, none at it
      prefix = (prefix + 1u) << hi;
      need = 0;
      break;
    }
  }
  return {prefix, need};
}

// Writes the entries `cut` takes of the n keys key(0) .. key(n - 1) to list[0 .. taken), those below kc first, then
// those equal to kc, each group in index order; entry = key << 32 | low(i, position in the list); the rest of the
// list is ~0 (sorts last).  Wave w walks a contiguous 16th of the indices, 64 neighbouring keys per step (coalesced
// reads of keys in global memory), and places its lanes' entries by ballot.  `scr`: kTopkScratch ints of LDS.  Ends
// with a block barrier: the list is complete.
template <typename Key, typename Low>
__device__ __forceinline__ void block_topk_compact(TopkCut cut, int n, Key key, Low low, unsigned long long* list,
                                                   int* scr) {
  static_assert(kTopkMaxK == kTopkThreads, "one list entry per thread");
  constexpr int kWaves = kTopkThreads / kWave;
  const int lane = lane_id(), wave = wave_id();
  const int per = (int)ceil_div(ceil_div(n, kWaves), kWave) * kWave;
  const int i0 = min(wave * per, n), i1 = min(i0 + per, n);
  const uint32_t kc = cut.kc;
  const unsigned long long below = (1ull << lane) - 1ull;
  int pos_less = 0, pos_eq = 0;  // entries < kc / == kc before the lane's current key
  constexpr int kQ = 4;  // keys per lane in flight
  const auto walk = [&](auto take) {
    for (int ib = i0; ib < i1; ib += kQ * kWave) {  // uniform trip count per wave: the ballots see the whole wave
      uint32_t kq[kQ];
#pragma unroll
      for (int q = 0; q < kQ; ++q) kq[q] = ib + q * kWave + lane < i1 ? key(ib + q * kWave + lane) : 0u;
#pragma unroll
      for (int q = 0; q < kQ; ++q) {
        const int i = ib + q * kWave + lane;
        const bool isl = i < i1 && kq[q] < kc, ise = i < i1 && kq[q] == kc;
        const unsigned long long bl = __ballot(isl), be = __ballot(ise);
        take(i, kq[q], isl, pos_less + __popcll(bl & below), ise, pos_eq + __popcll(be & below));
        pos_less += __popcll(bl);
        pos_eq += __popcll(be);
      }
    }
  };
  walk([](int, uint32_t, bool, int, bool, int) {});  // counts of the wave
  if (lane == 0) {
    scr[wave] = pos_less;
    scr[kWaves + wave] = pos_eq;
  }
  list[threadIdx.x] = ~0ull;
  __syncthreads();
  int tot_less = 0;
  pos_less = pos_eq = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {  // all reads issued at once, no branch per wave
    const int l = scr[w], e = scr[kWaves + w];
    pos_less += w < wave ? l : 0;
    pos_eq += w < wave ? e : 0;
    tot_less += l;
  }
  walk([&](int i, uint32_t k, bool isl, int pl, bool ise, int pe) {
    if (isl) list[pl] = ((unsigned long long)k << 32) | low(i, pl);
    if (ise && pe < cut.r) list[tot_less + pe] = ((unsigned long long)k << 32) | low(i, tot_less + pe);
  });
  __syncthreads();
}

// block_topk_compact for keys in LDS: thread t walks the contiguous indices [t * ept, (t + 1) * ept) and places its
// entries after two block scans of the per-thread counts.  The caller lays the keys out so that neighbouring threads'
// chunks start in different banks.  Measured on cp_topk_kernel (16 k keys): 2 us faster than the wave-ballot walk.
template <typename Key, typename Low>
__device__ __forceinline__ void block_topk_compact_chunks(TopkCut cut, int n, Key key, Low low,
                                                          unsigned long long* list, int* scr) {
  list[threadIdx.x] = ~0ull;
  const int ept = (n + kTopkThreads - 1) / kTopkThreads;
  const int c0 = threadIdx.x * ept, c1 = min(c0 + ept, n);
  int nless = 0, neq = 0;
  for (int i = c0; i < c1; ++i) {
    const uint32_t k = key(i);
    nless += k < cut.kc ? 1 : 0;
    neq += k == cut.kc ? 1 : 0;
  }
  int tot_less, tot_eq;
  int pl = block_exclusive_scan<kTopkThreads>(nless, scr, tot_less);
  int pe = tot_less + block_exclusive_scan<kTopkThreads>(neq, scr, tot_eq);
  for (int i = c0; i < c1; ++i) {
    const uint32_t k = key(i);
    if (k < cut.kc) {
      list[pl] = ((unsigned long long)k << 32) | low(i, pl);
      ++pl;
    } else if (k == cut.kc) {
      if (pe < tot_less + cut.r) list[pe] = ((unsigned long long)k << 32) | low(i, pe);
      ++pe;
    }
  }
  __syncthreads();
}

// Orders one wave's LDS accesses before this point against its accesses after it, across lanes: a convergent wave
// barrier between a wavefront-scope release and acquire.  It emits no instruction (a wave's LDS operations are
// performed in issue order); it only keeps the compiler from moving accesses across it.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Ascending bitonic sort of the first n2 entries of the list (n2: a power of two >= K, at least one wave's 64), one
// compare-exchange per thread and step.
// Why most steps need no block barrier: at a stride s <= 64, thread t = 64 w + u compares entries
// lo = 128 w + 2u - (u mod s) and lo + s, both in [128 w, 128 w + 128) -- the same 128 entries for every such step, and
// no other wave's.  A run of such steps is therefore private to each wave and needs only wave_lds_order between them.
// A step with a stride of 128 or more crosses waves, so a block barrier goes after it, and after the last step before
// it (stride 1 of the previous merge size).  At 1024 entries that is 10 barriers instead of one after each of the 55
// steps, plus the one after the network.  The barriers (px_lds_barrier) wait for LDS only: global loads the caller
// issued before the sort stay in flight across it.  Ends with a block barrier: the sorted list is visible to all.
__device__ __forceinline__ void block_topk_sort(unsigned long long* list, int K) {
  const int t = threadIdx.x;
  int n2 = 64;
  while (n2 < K) n2 <<= 1;  // uniform
  for (int size = 2; size <= n2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (t < (n2 >> 1)) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const unsigned long long a = list[lo], b = list[hi];
        if ((a > b) == up) {
          list[lo] = b;
          list[hi] = a;
        }
      }
      if (stride >= 2 * kWave || (stride == 1 && size >= 2 * kWave))
        px_lds_barrier();
      else
        wave_lds_order();
    }
  }
  px_lds_barrier();
}

}  // namespace pd3
