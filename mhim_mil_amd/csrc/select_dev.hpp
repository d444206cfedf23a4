// select_dev.hpp — the device pieces of the top-k selection that select.hip (one score vector: mhimx_select_mask, mhimx_select_rows)
// and topk.hip (many vectors of different lengths in one launch chain: mhimx_topk_many) have in common: the order-preserving key,
// block scans, the register-resident radix select and the digit-histogram threshold search.  Moved here text for text; every kernel of
// select.hip keeps its code (tools/kernel_meta.py --diff against the build before).
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
