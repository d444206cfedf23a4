// select_dev.hpp — the device pieces that select.hip (one score vector: mhimx_select_mask, mhimx_select_rows), select_many.hip (the
// production select of many bags in one launch: mhimx_select_rows_many) and topk.hip (many vectors of different lengths in one launch
// chain: mhimx_topk_many) have in common: the order-preserving key, block scans, the register-resident radix select, the candidate stage
// and the LDS sort of the one-workgroup forms, the whole body of the one-workgroup select (threshold, candidates, both keyed subset draws,
// compaction, staged stores: select_small_body - one copy for select_small_kernel and select_many_kernel), and the digit-histogram
// threshold search of the multi-workgroup forms.
#pragma once
#include "common.hpp"

namespace mhimx {

constexpr int SEL_THREADS = 1024;
constexpr int SEL_WAVES = SEL_THREADS / 64;

MHIMX_DEV uint32_t mono32(float f, bool largest) {
  uint32_t b = __float_as_uint(f);
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);   // ascending fp32 order -> ascending uint32 order
  return largest ? b : ~b;                          // "largest key" == smallest value when !largest
}

// exclusive prefix count of `pred` over the 1024 threads in thread order; returns total via *total
MHIMX_DEV uint32_t block_prefix(bool pred, uint32_t* wave_tot /*[16] LDS*/, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(pred);
  const uint32_t in_wave = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wave_tot[wave] = __popcll(bal);
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < SEL_WAVES; ++w) {
    const uint32_t c = wave_tot[w];
    if (w < wave) base += c;
    tot += c;
  }
  __syncthreads();
  *total = tot;
  return base + in_wave;
}

// Wave64 integer scans / reductions on the DPP network (a __shfl_* is a ds_bpermute: an LDS-crossbar round trip per step,
// and this kernel is one long dependent chain).  row_shr:n = 0x110+n, row_bcast:15 = 0x142, row_bcast:31 = 0x143.
template <int CTRL, int ROW_MASK>
MHIMX_DEV uint32_t dpp_u32(uint32_t old, uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROW_MASK, 0xf, false);
}
MHIMX_DEV uint32_t wave_scan_incl(uint32_t v) {       // inclusive prefix sum in lane order
  v += dpp_u32<0x111, 0xf>(0u, v);
  v += dpp_u32<0x112, 0xf>(0u, v);
  v += dpp_u32<0x114, 0xf>(0u, v);
  v += dpp_u32<0x118, 0xf>(0u, v);                    // inclusive inside each 16-lane row
  v += dpp_u32<0x142, 0xa>(0u, v);                    // rows 1,3 += last lane of rows 0,2
  v += dpp_u32<0x143, 0xc>(0u, v);                    // rows 2,3 += lane 31
  return v;
}
MHIMX_DEV uint32_t wave_min_u32(uint32_t v) {
  uint32_t t;
  t = dpp_u32<0xB1, 0xf>(v, v); v = t < v ? t : v;
  t = dpp_u32<0x4E, 0xf>(v, v); v = t < v ? t : v;
  t = dpp_u32<0x141, 0xf>(v, v); v = t < v ? t : v;
  t = dpp_u32<0x140, 0xf>(v, v); v = t < v ? t : v;
  t = dpp_u32<0x142, 0xa>(v, v); v = t < v ? t : v;
  t = dpp_u32<0x143, 0xc>(v, v); v = t < v ? t : v;
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
MHIMX_DEV uint32_t wave_max_u32(uint32_t v) { return ~wave_min_u32(~v); }

// sum of the per-wave totals below `wave` and of all 16 (four 16-byte LDS reads)
MHIMX_DEV void wave_tot_combine(const uint32_t* wave_tot, int wave, uint32_t* below, uint32_t* total) {
  uint32_t w[SEL_WAVES];
#pragma unroll
  for (int q = 0; q < SEL_WAVES / 4; ++q) {
    const uint4 v = reinterpret_cast<const uint4*>(wave_tot)[q];
    w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
  }
  uint32_t b = 0, t = 0;
#pragma unroll
  for (int q = 0; q < SEL_WAVES; ++q) {
    b += q < wave ? w[q] : 0u;
    t += w[q];
  }
  *below = b;
  *total = t;
}

// exclusive prefix sum of one integer per thread over the 1024 threads (thread order); *total = block sum
MHIMX_DEV uint32_t block_scan_excl(uint32_t v, uint32_t* wave_tot /*[16] LDS, 16-byte aligned*/, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t inc = wave_scan_incl(v);
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  uint32_t base;
  wave_tot_combine(wave_tot, wave, &base, total);
  __syncthreads();
  return base + inc - v;
}

// radix select over register-resident keys: returns the k-th largest key T among the valid ones, in *remaining_out how
// many T-valued keys belong to the top-k and in *n_eq_out how many T-valued keys exist (remaining == n_eq: every tie is
// taken and the caller needs no tie ranking).
//   * Scores are low-entropy in their leading bits (a softmax-derived score in [0.5, 1) has 9 identical leading bits) and
//     a histogram pass over such a digit is 64 lanes x 10 keys of LDS atomics on ONE address: the passes start at the
//     highest bit in which the block's keys differ (min ^ max).  FULL32 (hashed keys) skips that pre-pass.
//   * One workgroup on one CU is a latency chain (a block barrier ~0.15 us, a pass ~7 of them): digits are 11 bits
//     (4 histogram copies of 2048 bins, wave w -> copy w & 3), and as soon as the threshold bin holds <= SEL_LIST keys
//     they are appended to an LDS list and the threshold is found by rank counting among them - for 1e4 continuous
//     scores that is ONE histogram pass + one list step instead of three or four passes.
// hist: [4][2048] LDS (also the list), wave_tot: [16], misc: [>=8] LDS.
constexpr int SEL_DIGIT = 11, SEL_BINS = 1 << SEL_DIGIT, SEL_COPIES = 4, SEL_LIST = 1024;

template <int KPT, bool FULL32>
MHIMX_DEV uint32_t radix_select_regs(const uint32_t (&key)[KPT], const bool (&valid)[KPT], uint32_t k, uint32_t* hist,
                                     uint32_t* wave_tot, uint32_t* misc, uint32_t* remaining_out, uint32_t* n_eq_out) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  uint32_t prefix = 0u, fixed_mask = 0u;
  int hb = 31;
  if (!FULL32) {
    // ---- block min / max of the valid keys
    uint32_t mn = 0xFFFFFFFFu, mx = 0u;
#pragma unroll
    for (int j = 0; j < KPT; ++j)
      if (valid[j]) { mn = key[j] < mn ? key[j] : mn; mx = key[j] > mx ? key[j] : mx; }
    mn = wave_min_u32(mn);
    mx = wave_max_u32(mx);
    if (lane == 0) { hist[wave] = mn; hist[SEL_WAVES + wave] = mx; }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < SEL_WAVES / 4; ++q) {
      const uint4 a = reinterpret_cast<const uint4*>(hist)[q], c = reinterpret_cast<const uint4*>(hist + SEL_WAVES)[q];
      mn = min(min(mn, min(a.x, a.y)), min(a.z, a.w));
      mx = max(max(mx, max(c.x, c.y)), max(c.z, c.w));
    }
    __syncthreads();
    const uint32_t diff = mn ^ mx;
    if (diff == 0u) {                          // every key equal: all of them are T-valued
      uint32_t nv = 0;
#pragma unroll
      for (int j = 0; j < KPT; ++j) nv += valid[j] ? 1u : 0u;
      uint32_t tot;
      block_scan_excl(nv, wave_tot, &tot);
      *remaining_out = k;
      *n_eq_out = tot;
      return mx;
    }
    hb = 31 - __clz(diff);                     // highest differing bit
    fixed_mask = hb >= 31 ? 0u : ~((2u << hb) - 1u);               // the common leading bits are decided
    prefix = mx & fixed_mask;
  }
  uint32_t remaining = k, n_eq = 0;
  int shift = hb - (SEL_DIGIT - 1) < 0 ? 0 : hb - (SEL_DIGIT - 1);
  uint32_t* copy = hist + (wave & (SEL_COPIES - 1)) * SEL_BINS;
  while (true) {
    {
      uint4* h4 = reinterpret_cast<uint4*>(hist);
      for (int i = tid; i < SEL_COPIES * SEL_BINS / 4; i += SEL_THREADS) h4[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < KPT; ++j)
      if (valid[j] && (key[j] & fixed_mask) == prefix) atomicAdd(&copy[(key[j] >> shift) & (SEL_BINS - 1)], 1u);
    __syncthreads();
    // thread t owns bins 2t, 2t+1; population ABOVE them = reversed block scan of the per-thread sums
    uint32_t c0 = 0, c1 = 0;
#pragma unroll
    for (int c = 0; c < SEL_COPIES; ++c) {
      const uint2 v = reinterpret_cast<const uint2*>(hist + c * SEL_BINS)[tid];
      c0 += v.x;
      c1 += v.y;
    }
    const uint32_t pre = wave_scan_incl(c0 + c1);                       // inclusive prefix in bin order
    if (lane == 63) wave_tot[wave] = pre;
    __syncthreads();
    uint32_t below, total;
    wave_tot_combine(wave_tot, wave, &below, &total);
    const uint32_t above = total - (below + pre);                       // population in the bins above 2t+1
    if (above < remaining && remaining <= above + c1) { misc[0] = 2u * tid + 1u; misc[1] = remaining - above; misc[3] = c1; }
    else if (above + c1 < remaining && remaining <= above + c1 + c0) { misc[0] = 2u * tid; misc[1] = remaining - above - c1; misc[3] = c0; }
    __syncthreads();
    prefix |= misc[0] << shift;
    remaining = misc[1];
    n_eq = misc[3];                            // keys in the threshold bin
    fixed_mask |= (uint32_t)(SEL_BINS - 1) << shift;
    if (shift == 0) break;                     // all bits decided: the bin IS the value T
    if (n_eq <= (uint32_t)SEL_LIST) {
      // ---- finish among the bin's keys: T = the remaining-th largest of the list
      if (tid == 0) misc[4] = 0;
      __syncthreads();                         // (also: everyone has read misc[0..3] and the histogram)
#pragma unroll
      for (int j = 0; j < KPT; ++j)
        if (valid[j] && (key[j] & fixed_mask) == prefix) hist[atomicAdd(&misc[4], 1u)] = key[j];
      __syncthreads();
      for (uint32_t j = tid; j < n_eq; j += SEL_THREADS) {
        const uint32_t mine = hist[j];
        uint32_t g = 0, e = 0;
        for (uint32_t q = 0; q < n_eq; ++q) {
          const uint32_t o = hist[q];
          g += o > mine ? 1u : 0u;
          e += o == mine ? 1u : 0u;
        }
        if (g < remaining && remaining <= g + e) { misc[5] = mine; misc[6] = remaining - g; misc[7] = e; }   // duplicates agree
      }
      __syncthreads();
      prefix = misc[5];
      remaining = misc[6];
      n_eq = misc[7];
      break;
    }
    __syncthreads();                           // misc / histogram are rewritten by the next pass
    shift = shift - SEL_DIGIT < 0 ? 0 : shift - SEL_DIGIT;
  }
  __syncthreads();
  *remaining_out = remaining;
  *n_eq_out = n_eq;
  return prefix;
}

// The candidate stage of every one-workgroup form (select_small_kernel, select_many_kernel, topk_small_kernel): thread t owns the
// CONTIGUOUS instances [t * KPT, (t + 1) * KPT) - scores are read from HBM exactly once (select_load_keys: the order-preserving keys and
// valid[j], instance t * KPT + j exists; a step of its own so that a kernel can put LDS set-up under the load's latency) and every
// order-dependent step costs ONE block scan of per-thread counts.  select_candidates leaves exactly k 64-bit keys
// (value image << 32 | ~index) in keys[0, k), in ascending row index: the
// k largest, ties lowest index first.  Ends with a barrier; `keys` may alias `hist`
// (radix_select_regs ends with one: the histogram is dead by then).
template <int KPT>
MHIMX_DEV void select_load_keys(const float* __restrict__ score, int N, bool lg, uint32_t (&key)[KPT], bool (&valid)[KPT]) {
  const int i0 = threadIdx.x * KPT;
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    valid[j] = (i0 + j) < N;
    key[j] = valid[j] ? mono32(score[i0 + j], lg) : 0u;
  }
}
template <int KPT>
MHIMX_DEV void select_candidates(const uint32_t (&key)[KPT], const bool (&valid)[KPT], uint32_t k, uint64_t* keys, uint32_t* hist,
                                 uint32_t* wave_tot, uint32_t* misc) {
  const int i0 = threadIdx.x * KPT;
  // ---- threshold
  uint32_t remaining, n_eq;
  const uint32_t T = radix_select_regs<KPT, false>(key, valid, k, hist, wave_tot, misc, &remaining, &n_eq);
  // ---- exactly k keys (ties: lowest index first)
  uint32_t eq_rank = 0;
  if (remaining != n_eq) {                 // only some of the T-valued keys belong to the top-k: rank them by index
    uint32_t neq = 0;
#pragma unroll
    for (int j = 0; j < KPT; ++j) neq += (valid[j] && key[j] == T) ? 1u : 0u;
    uint32_t tot;
    eq_rank = block_scan_excl(neq, wave_tot, &tot);
  }
  bool take[KPT];
  uint32_t ntake = 0;
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    bool t = valid[j] && key[j] > T;
    if (valid[j] && key[j] == T) { t = remaining == n_eq || eq_rank < remaining; ++eq_rank; }
    take[j] = t;
    ntake += t ? 1u : 0u;
  }
  // positions in THREAD order (one block scan): the device-drawn subsets pick candidates by their position in this list, so the list
  // must not depend on which wave reserves its slots first
  uint32_t tot;
  uint32_t pos = block_scan_excl(ntake, wave_tot, &tot);
#pragma unroll
  for (int j = 0; j < KPT; ++j)
    if (take[j]) keys[pos++] = ((uint64_t)key[j] << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)(i0 + j));
  __syncthreads();
}

// bitonic sort of a[0, P) in LDS, descending, in place; P a power of two; every thread of the workgroup calls it (the caller's barrier
// stands between its own writes of `a` and the call); ends with a barrier
MHIMX_DEV void lds_bitonic_desc(uint64_t* a, int P) {
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += SEL_THREADS) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const bool desc = ((lo & size) == 0);
        const uint64_t x = a[lo], y = a[hi];
        if ((x < y) == desc) { a[lo] = y; a[hi] = x; }
      }
      __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// The one-workgroup select of a bag of up to 16 384 rows (a bag of one slide at 20x is ~1e4 patches): select_small_kernel<KPT, LEAN>
// (select.hip: one bag, or one per plane of a bag-batched launch) and select_many_kernel<KPT> (select_many.hip: one bag of a by-value table
// per workgroup) are this body behind their own argument blocks.  Keys in registers, flags an LDS bitmap, the k candidates ordered by rank
// counting (k^2 / 1024 LDS compares per thread, no barriers) when k <= 2048.
// LEAN: the production call (device-drawn subsets, no injected permutation, no earlier mask, no id or top-k list) - the branches of every
// other form are compiled out, and so are the LDS arrays only they use.  The kernel runs once per step on one workgroup and is fetched cold by
// 16 waves: the lean instantiation is some 700 instructions shorter.
// The bits of every form are pinned by oracle/mhim_oracle.py select_rows (tests/test_select_oracle_gpu.py).
// ------------------------------------------------------------------------------------------------
struct SelectArgs {
  const float* score;
  int N, k, n_sel, largest;
  const int64_t *perm, *other;                 // full forms: an injected permutation of the candidates, an earlier mask to unite with
  int64_t n_other;
  int64_t *mask_ids, *len_keep_dev, *topk_out; // full forms
  int P;                                       // pow2 >= max(k, 2): places the LDS arrays only
  int use_rand;                                // 1: device-drawn subsets, rows = [stay | merge]; 2: [merge | stay]
  uint64_t rand_seed;                          // eff_seed of the launch
  int merge_R;
  int64_t* rows_out;
  int64_t* rows_img;   // optional: the same rows in the order of the projection's dPRE image when its producers write it -
                       // [rows that stay | 0 ... | rows to merge from position img_off | 0 ... to a multiple of 32]
  int img_off;
};

// dynamic LDS of the body: keys [P] u64 (+ sorted [P] u64 in the full forms) | hist [4][2048] | wave_tot [16] | misc [8] | bitmap [512] |
// klist [16384] u16; the row staging ([N] u16, last phase) aliases keys / hist.  8 P + 67 680 bytes LEAN, 16 P + 67 680 otherwise.
constexpr size_t select_lds_bytes(int P, bool lean) {
  return (size_t)(lean ? 1 : 2) * P * 8 + (size_t)(SEL_COPIES * SEL_BINS + SEL_WAVES + 8 + 512) * 4 + 16384 * 2;
}

template <int KPT, bool LEAN>
MHIMX_DEV void select_small_body(const SelectArgs& a, char* smem) {
  const int N = a.N, k = a.k, n_sel = a.n_sel, P = a.P, use_rand = a.use_rand, merge_R = a.merge_R;
  const int64_t* __restrict__ perm = a.perm;
  const int64_t* __restrict__ other = a.other;
  int64_t* __restrict__ mask_ids = a.mask_ids;
  int64_t* __restrict__ topk_out = a.topk_out;
  int64_t* __restrict__ rows_out = a.rows_out;
  int64_t* __restrict__ rows_img = a.rows_img;
  uint64_t* keys = reinterpret_cast<uint64_t*>(smem);                   // [P] the candidates, in ascending row index
  uint64_t* sorted = keys + P;                                          // [P] the same by (value desc, index asc): full forms only
  uint32_t* hist = reinterpret_cast<uint32_t*>(keys + (LEAN ? P : 2 * P));   // [4][2048]
  uint32_t* wave_tot = hist + SEL_COPIES * SEL_BINS;                    // [16]
  uint32_t* misc = wave_tot + SEL_WAVES;                                // [8]
  uint32_t* bitmap = misc + 8;                                          // [512] = 16384 bits
  uint16_t* klist = reinterpret_cast<uint16_t*>(bitmap + 512);          // [N] kept rows in ascending order (the Merge draw indexes it)
  uint16_t* stage = reinterpret_cast<uint16_t*>(smem);                  // [N] row list staging (aliases keys / sorted / hist: last phase)
  const int tid = threadIdx.x;
  const int i0 = tid * KPT;
  uint32_t key[KPT];
  bool valid[KPT];
  select_load_keys<KPT>(a.score, N, a.largest != 0, key, valid);
  for (int i = tid; i < 512; i += SEL_THREADS) bitmap[i] = 0;

  // ---- 1, 2. threshold; exactly k candidates in ascending row index
  select_candidates<KPT>(key, valid, (uint32_t)k, keys, hist, wave_tot, misc);

  // ---- 3. order the candidates: (value desc, index asc) == key desc
  // The device-drawn subset ALWAYS picks by position in `keys` - the candidates in ascending row index - whether or not the value-ordered
  // list is wanted as well: the same (seed, tick) masks the same rows with and without topk_out / LEAN.
  const bool dev_rand = LEAN || (use_rand && !perm && n_sel < k);
  if (LEAN || (dev_rand && !topk_out)) {
    // (no value-ordered list needed)
  } else if (k <= 2048) {
    for (int j = tid; j < k; j += SEL_THREADS) {
      const uint64_t mine = keys[j];
      int r = 0;
      for (int q = 0; q < k; ++q) r += keys[q] > mine ? 1 : 0;
      sorted[r] = mine;
    }
    __syncthreads();
  } else {
    for (int j = tid; j < P; j += SEL_THREADS) sorted[j] = j < k ? keys[j] : 0ull;
    __syncthreads();
    lds_bitonic_desc(sorted, P);
  }
  if (!LEAN && topk_out)
    for (int j = tid; j < k; j += SEL_THREADS) topk_out[j] = (int64_t)(0xFFFFFFFFu - (uint32_t)(sorted[j] & 0xFFFFFFFFull));

  // ---- 4. flags (LDS bitmap)
  const bool has_other = !LEAN && other != nullptr && a.n_other > 0;
  const int len_keep_simple = N - n_sel;
  if (dev_rand) {
    // masking.py:66-71 keeps a uniformly random n_sel-subset of the k candidates.  Drawn here without a host permutation and without
    // ranking random keys (k^2 / 1024 compares per thread were 3 us of this kernel): candidate pi(i), i < n_sel, of a keyed
    // pseudo-random permutation pi of the k list positions (common.hpp: feistel_small) - one short dependent chain per pick.
    // (both round keys depend on the WHOLE seed: with k1 a function of the high word alone, seeds that differ in the low word only - small
    // integers - shared it, and the 4-round network on a 6-bit domain masked one of 56 candidates 6.5 sigma off its share over 2000 seeds;
    // tools/feistel_sim.py, tests/test_round4_gpu.py::test_select_rows_draws_are_fair_on_small_lists)
    const uint32_t k0 = mix32((uint32_t)a.rand_seed ^ 0x9E3779B9u), k1 = mix32((uint32_t)(a.rand_seed >> 32) + 0x85EBCA6Bu + k0 * 0x632BE5ABu);
    const int bits = small_perm_bits((uint32_t)k);
    for (int i = tid; i < n_sel; i += SEL_THREADS) {
      const uint32_t j = feistel_small((uint32_t)i, (uint32_t)k, bits, k0, k1);
      const uint32_t idx = 0xFFFFFFFFu - (uint32_t)(keys[j] & 0xFFFFFFFFull);
      atomicOr(&bitmap[idx >> 5], 1u << (idx & 31));
      if (!LEAN && !has_other && mask_ids) mask_ids[len_keep_simple + i] = (int64_t)idx;
    }
  } else if (!LEAN) {
    for (int j = tid; j < n_sel; j += SEL_THREADS) {
      const int64_t src = perm ? perm[j] : (int64_t)j;
      const uint32_t idx = 0xFFFFFFFFu - (uint32_t)(sorted[src] & 0xFFFFFFFFull);
      atomicOr(&bitmap[idx >> 5], 1u << (idx & 31));
      if (!has_other && mask_ids) mask_ids[len_keep_simple + j] = (int64_t)idx;
    }
  }
  if (has_other)
    for (int64_t j = tid; j < a.n_other; j += SEL_THREADS) {
      const uint32_t idx = (uint32_t)other[j];
      atomicOr(&bitmap[idx >> 5], 1u << (idx & 31));
    }
  __syncthreads();

  // ---- 5. ordered compaction: kept ids ascending (and, for a union with an earlier mask, masked ids ascending)
  bool kv[KPT];
  uint32_t nkeep = 0;
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    const int i = i0 + j;
    kv[j] = valid[j] && !((bitmap[i >> 5] >> (i & 31)) & 1u);
    nkeep += kv[j] ? 1u : 0u;
  }
  uint32_t kept_total;
  uint32_t kpos = block_scan_excl(nkeep, wave_tot, &kept_total);
  const uint32_t kpos0 = kpos;
  if (!LEAN && mask_ids) {
#pragma unroll
    for (int j = 0; j < KPT; ++j)
      if (kv[j]) mask_ids[kpos++] = i0 + j;
    if (has_other) {
      uint32_t nm = 0;
#pragma unroll
      for (int j = 0; j < KPT; ++j) nm += (valid[j] && !kv[j]) ? 1u : 0u;
      uint32_t mt;
      uint32_t mpos = kept_total + block_scan_excl(nm, wave_tot, &mt);
#pragma unroll
      for (int j = 0; j < KPT; ++j)
        if (valid[j] && !kv[j]) mask_ids[mpos++] = i0 + j;
    }
  }
  if (!LEAN && tid == 0 && a.len_keep_dev) *a.len_keep_dev = (int64_t)kept_total;
  if (!LEAN && !rows_out) return;

  // ---- 6. Merge.masking (merge.py:158-176): a uniformly random R-subset of the kept rows is merged away.  Same device, the same
  // draw as step 4: the kept rows go to an LDS list in ascending order, row klist[pi2(i)], i < R, of a second keyed permutation (of the
  // Lrows list positions) is merged (flags in the bitmap, which step 5 has finished reading), then ordered compactions ->
  // rows_out = [kept rows that stay (ascending) | rows to merge (ascending)].  (A random key per kept row + a radix select of the R
  // largest was 4.1 us of this kernel.)  The pool is order independent, so the reference's random ORDER of the kept rows is not
  // reproduced (only fp summation order differs).
  const int Lrows = (int)kept_total;
  const int Lk = Lrows - merge_R;
  const bool partial = merge_R > 0 && merge_R < Lrows;
  if (partial) {
    uint32_t kp = kpos0;
#pragma unroll
    for (int j = 0; j < KPT; ++j)
      if (kv[j]) klist[kp++] = (uint16_t)(i0 + j);
    for (int i = tid; i < 512; i += SEL_THREADS) bitmap[i] = 0;
    __syncthreads();
    const uint32_t q1 = mix32((uint32_t)a.rand_seed * 0x9E3779B1u + 0xC2B2AE35u),
                   q0 = mix32(((uint32_t)(a.rand_seed >> 17) ^ 0x85EBCA6Bu) + q1 * 0x632BE5ABu);
    const int bits2 = small_perm_bits((uint32_t)Lrows);
    for (int i = tid; i < merge_R; i += SEL_THREADS) {
      const uint32_t row = klist[feistel_small((uint32_t)i, (uint32_t)Lrows, bits2, q0, q1)];
      atomicOr(&bitmap[row >> 5], 1u << (row & 31));
    }
    __syncthreads();
  }
  bool mrg[KPT];
  uint32_t nstay = 0, nmrg = 0;
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    const int i = i0 + j;
    const bool m = kv[j] && (merge_R >= Lrows || (partial && ((bitmap[i >> 5] >> (i & 31)) & 1u)));
    mrg[j] = m;
    nmrg += m ? 1u : 0u;
    nstay += (kv[j] && !m) ? 1u : 0u;
  }
  // one scan for both lists (each total <= 16384 fits 16 bits).
  // use_rand == 2: rows to merge FIRST ([merge | stay]: lets the caller keep [stay rows | merged tokens] contiguous)
  uint32_t t2;
  const uint32_t packed = block_scan_excl(nstay | (nmrg << 16), wave_tot, &t2);
  uint32_t spos = (use_rand == 2 ? (uint32_t)(Lrows - Lk) : 0u) + (packed & 0xFFFFu);
  uint32_t mpos2 = (use_rand == 2 ? 0u : (uint32_t)Lk) + (packed >> 16);
  // staged in LDS so the 8-byte row ids leave as full coalesced lines (a thread's own rows are 80 B apart from its
  // neighbour's: 10 scattered store instructions per wave otherwise)
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    if (!kv[j]) continue;
    if (mrg[j]) stage[mpos2++] = (uint16_t)(i0 + j);
    else stage[spos++] = (uint16_t)(i0 + j);
  }
  __syncthreads();
  for (int i = tid; i < Lrows; i += SEL_THREADS) rows_out[i] = (int64_t)stage[i];
  if (rows_img) {
    const int mrg_n = Lrows - Lk, stay0 = use_rand == 2 ? mrg_n : 0, mrg0 = use_rand == 2 ? 0 : Lk;
    const int end = (a.img_off + mrg_n + 31) / 32 * 32;
    for (int p = tid; p < end; p += SEL_THREADS)
      rows_img[p] = p < Lk ? (int64_t)stage[stay0 + p] : ((p >= a.img_off && p - a.img_off < mrg_n) ? (int64_t)stage[mrg0 + p - a.img_off] : (int64_t)0);
  }
}

constexpr int SELM_BINS = 2048;
// thread t owns bins 2t, 2t+1 of a 2048-bin histogram: find the bin in which the cumulative count FROM THE TOP reaches `remaining`
MHIMX_DEV void selm_find_bin(const uint32_t* __restrict__ h, uint32_t remaining, uint32_t* wave_tot, uint32_t* misc, uint32_t* bin_out,
                             uint32_t* rem_out) {
  const int tid = threadIdx.x;
  const uint2 v = reinterpret_cast<const uint2*>(h)[tid];
  uint32_t total;
  const uint32_t below = block_scan_excl(v.x + v.y, wave_tot, &total);
  const uint32_t above = total - (below + v.x + v.y);                 // population in the bins above 2t+1
  if (above < remaining && remaining <= above + v.y) { misc[0] = 2u * tid + 1u; misc[1] = remaining - above; }
  else if (above + v.y < remaining && remaining <= above + v.y + v.x) { misc[0] = 2u * tid; misc[1] = remaining - above - v.y; }
  __syncthreads();
  *bin_out = misc[0];
  *rem_out = misc[1];
  __syncthreads();
}

// digits fixed by the first `passes` histograms -> (prefix, remaining)
MHIMX_DEV void selm_prefix(const uint32_t* __restrict__ hist, int passes, uint32_t k, uint32_t* wave_tot, uint32_t* misc, uint32_t* prefix_out,
                           uint32_t* rem_out) {
  uint32_t prefix = 0, remaining = k, bin;
  if (passes >= 1) { selm_find_bin(hist, remaining, wave_tot, misc, &bin, &remaining); prefix = bin << 21; }
  if (passes >= 2) { selm_find_bin(hist + SELM_BINS, remaining, wave_tot, misc, &bin, &remaining); prefix |= bin << 10; }
  if (passes >= 3) { selm_find_bin(hist + 2 * SELM_BINS, remaining, wave_tot, misc, &bin, &remaining); prefix |= bin; }
  *prefix_out = prefix;
  *rem_out = remaining;
}

}  // namespace mhimx
