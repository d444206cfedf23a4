// topk.hip — the k most (or least) attended instances of MANY score vectors of different lengths in one launch chain
// (mhimx_topk_many): what a validation pass does next with the per-instance attention / score vector of the ragged inference calls
// (replaces the per-slide torch.topk of CLAM/create_heatmaps.py:53 and the per-bag ranking of mhim_modules/masking.py:62, under the
// select's tie contract: value descending [ascending if !largest], then index ascending).
//
// Plane = segment.  The segment table travels by value (infer_tab.hpp's RG_PICK pattern: constant indices only), nothing is copied to
// the device, waited for or allocated; the launch count does not depend on n_segs:
//   small   one 1024-thread workgroup per segment.  N <= 16384: the whole job - the select's own candidate stage (select_dev.hpp
//           select_candidates: keys in registers, scores read from HBM once, threshold by radix_select_regs, exactly k_b 64-bit keys
//           value << 32 | ~index in index order), ordered in LDS (rank counting, or select_dev.hpp lds_bitonic_desc), idx / val / padding written.  A larger segment's workgroup exits at once; n_large further workgroups zero the digit
//           histograms of the large segments' workspace slots (a kernel of this stream, not a memset node: select.hip sel_zero_kernel).
//   Only if a segment is above 16384 rows (one workgroup walking 200 000 keys several times is 0.6 ms: select.hip), on a
//   (chunk, large segment) grid - up to 256 chunks of >= 4096 keys per segment, a segment's chunking depends on its own N alone:
//   hist x3 the 11/11/10-bit digit histograms of select.hip's multi-workgroup path, per segment (LDS histogram, then integer atomics)
//   count   T = k-th largest key, how many T-valued keys belong to the top-k; per-chunk counts of keys > T and == T
//   gather  exactly k keys at positions fixed by the counts (ties lowest index first)
//   final   one workgroup per large segment: the k candidates ordered in LDS, idx / val written
// 1 launch without, 7 with a large segment.  What one stage leaves for the next crosses a launch boundary; no workgroup waits for
// another.  Integer work only (the values leave as the inverse image of their keys: the same bits): a segment's result does not depend
// on where it stands in a call or on its neighbours.
#include "infer_tab.hpp"
#include "select_dev.hpp"

namespace mhimx {

constexpr int TK_SMALL_N = 16384;                 // rows one workgroup keeps in registers (16 per thread)
constexpr int TK_KPT = 16;
constexpr int TK_MAXG = 256, TK_CHUNK = 4096;     // chunks of a large segment: min(ceil(N / 4096), 256)
constexpr int TK_COUNT_K = 256;                   // up to here the candidates are ordered by rank counting, above by a bitonic sort
// a large segment's workspace slot: hist [3][2048] u32 | blk_gt [256] | blk_eq [256] | state (256 bytes) | cand [k] u64 (to 256 bytes)
constexpr int64_t TK_OFF_GT = 3 * SELM_BINS * 4, TK_OFF_EQ = TK_OFF_GT + TK_MAXG * 4, TK_OFF_STATE = TK_OFF_EQ + TK_MAXG * 4,
                  TK_OFF_CAND = TK_OFF_STATE + 256;
static int64_t tk_slot_bytes(int64_t k) { return TK_OFF_CAND + align_up(k * 8, 256); }

struct TopkTab {
  int64_t row0[MHIMX_INFER_MAX];
  int32_t N[MHIMX_INFER_MAX];
  int32_t large[MHIMX_INFER_MAX];                 // large[li] = the segment of workspace slot li
  int32_t n, n_large;
};
struct TopkSlot { uint32_t *hist, *blk_gt, *blk_eq, *state; uint64_t* cand; };
MHIMX_DEV TopkSlot tk_slot(char* ws, int li, int64_t slot_bytes) {
  char* p = ws + (int64_t)li * slot_bytes;
  TopkSlot s;
  s.hist = reinterpret_cast<uint32_t*>(p);
  s.blk_gt = reinterpret_cast<uint32_t*>(p + TK_OFF_GT);
  s.blk_eq = reinterpret_cast<uint32_t*>(p + TK_OFF_EQ);
  s.state = reinterpret_cast<uint32_t*>(p + TK_OFF_STATE);
  s.cand = reinterpret_cast<uint64_t*>(p + TK_OFF_CAND);
  return s;
}
// segment `seg` = tab.large[li] of a (chunk, large segment) grid: its N, row0, chunk count G and chunk length
#define TK_LARGE_SEG(li)                                                  \
  int seg = tab.large[0];                                                 \
  RG_PICK(seg, tab.large, li)                                             \
  int32_t N = tab.N[0];                                                   \
  int64_t row0 = tab.row0[0];                                             \
  RG_PICK(N, tab.N, seg) RG_PICK(row0, tab.row0, seg)                     \
  const int G = (N + TK_CHUNK - 1) / TK_CHUNK < TK_MAXG ? (N + TK_CHUNK - 1) / TK_CHUNK : TK_MAXG; \
  [[maybe_unused]] const int chunk = (N + G - 1) / G;

MHIMX_DEV float tk_unmono(uint32_t key, bool largest) {          // the inverse of mono32: the score's own bits
  uint32_t b = largest ? key : ~key;
  b = (b & 0x80000000u) ? (b ^ 0x80000000u) : ~b;
  return __uint_as_float(b);
}

// keys [0, kb) of LDS (distinct; room for the next power of two >= kb) -> descending order -> idx_row / val_row [0, k), padded behind kb
MHIMX_DEV void tk_order_write(uint64_t* keys, int kb, int k, bool largest, int64_t* __restrict__ idx_row, float* __restrict__ val_row) {
  const int tid = threadIdx.x;
  if (kb <= TK_COUNT_K) {
    uint64_t mine = 0ull;
    int r = 0;
    if (tid < kb) {
      mine = keys[tid];
      for (int q = 0; q < kb; ++q) r += keys[q] > mine ? 1 : 0;
    }
    __syncthreads();
    if (tid < kb) keys[r] = mine;
    __syncthreads();
  } else {
    int P = 2;
    while (P < kb) P <<= 1;
    for (int j = kb + tid; j < P; j += SEL_THREADS) keys[j] = 0ull;          // (0 is below every key)
    __syncthreads();
    lds_bitonic_desc(keys, P);
  }
  for (int j = tid; j < k; j += SEL_THREADS) {
    int64_t id = -1;
    float v = 0.f;
    if (j < kb) {
      const uint64_t key = keys[j];
      id = (int64_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull));
      v = tk_unmono((uint32_t)(key >> 32), largest);
    }
    idx_row[j] = id;
    if (val_row) val_row[j] = v;
  }
}

__global__ __launch_bounds__(SEL_THREADS) void topk_small_kernel(const float* __restrict__ score, TopkTab tab, int k, int largest,
                                                                int64_t* __restrict__ idx, float* __restrict__ val, char* __restrict__ ws,
                                                                int64_t slot_bytes) {
  __shared__ __attribute__((aligned(16))) uint32_t hist[SEL_COPIES * SEL_BINS];       // 32 KB; the candidate keys once the threshold is known
  __shared__ __attribute__((aligned(16))) uint32_t wave_tot[SEL_WAVES];
  __shared__ uint32_t misc[8];
  const int tid = threadIdx.x, b = blockIdx.x;
  if (b >= tab.n) {                          // the digit histograms of large slot b - n
    uint4* h = reinterpret_cast<uint4*>(ws + (int64_t)(b - tab.n) * slot_bytes);
    for (int i = tid; i < 3 * SELM_BINS / 4; i += SEL_THREADS) h[i] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  int32_t N = tab.N[0];
  int64_t row0 = tab.row0[0];
  RG_PICK(N, tab.N, b) RG_PICK(row0, tab.row0, b)
  if (N > TK_SMALL_N) return;
  const bool lg = largest != 0;
  const int kb = k < N ? k : N;
  const float* s = score + row0;
  // thread t owns the contiguous instances [16 t, 16 t + 16): exactly kb keys, in index order (ties: lowest index first), where the
  // histogram was
  uint64_t* keys = reinterpret_cast<uint64_t*>(hist);
  uint32_t key[TK_KPT];
  bool valid[TK_KPT];
  select_load_keys<TK_KPT>(s, N, lg, key, valid);
  select_candidates<TK_KPT>(key, valid, (uint32_t)kb, keys, hist, wave_tot, misc);
  tk_order_write(keys, kb, k, lg, idx + (int64_t)b * k, val ? val + (int64_t)b * k : nullptr);
}

template <int PASS>
__global__ __launch_bounds__(SEL_THREADS) void topk_hist_kernel(const float* __restrict__ score, TopkTab tab, int k, int largest,
                                                               char* __restrict__ ws, int64_t slot_bytes) {
  __shared__ uint32_t lh[SELM_BINS];
  __shared__ __attribute__((aligned(16))) uint32_t wave_tot[SEL_WAVES];
  __shared__ uint32_t misc[8];
  const int tid = threadIdx.x;
  TK_LARGE_SEG((int)blockIdx.y)
  if ((int)blockIdx.x >= G) return;
  const TopkSlot w = tk_slot(ws, blockIdx.y, slot_bytes);
  const bool lg = largest != 0;
  uint32_t prefix = 0, rem = 0;
  selm_prefix(w.hist, PASS, (uint32_t)k, wave_tot, misc, &prefix, &rem);
  const uint32_t fixed_mask = PASS == 0 ? 0u : (PASS == 1 ? 0xFFE00000u : 0xFFFFFC00u);
  const int shift = PASS == 0 ? 21 : (PASS == 1 ? 10 : 0);
  const uint32_t dmask = PASS == 2 ? 1023u : 2047u;
  for (int i = tid; i < SELM_BINS; i += SEL_THREADS) lh[i] = 0;
  __syncthreads();
  const float* s = score + row0;
  const int b0 = blockIdx.x * chunk, b1 = b0 + chunk < N ? b0 + chunk : N;
  for (int i = b0 + tid; i < b1; i += SEL_THREADS) {
    const uint32_t key = mono32(s[i], lg);
    if ((key & fixed_mask) == prefix) atomicAdd(&lh[(key >> shift) & dmask], 1u);
  }
  __syncthreads();
  uint32_t* gh = w.hist + PASS * SELM_BINS;
  for (int i = tid; i < SELM_BINS; i += SEL_THREADS)
    if (lh[i]) atomicAdd(&gh[i], lh[i]);
}

__global__ __launch_bounds__(SEL_THREADS) void topk_count_kernel(const float* __restrict__ score, TopkTab tab, int k, int largest,
                                                                char* __restrict__ ws, int64_t slot_bytes) {
  __shared__ __attribute__((aligned(16))) uint32_t wave_tot[SEL_WAVES];
  __shared__ uint32_t misc[8];
  const int tid = threadIdx.x;
  TK_LARGE_SEG((int)blockIdx.y)
  if ((int)blockIdx.x >= G) return;
  const TopkSlot w = tk_slot(ws, blockIdx.y, slot_bytes);
  const bool lg = largest != 0;
  uint32_t T, remaining;
  selm_prefix(w.hist, 3, (uint32_t)k, wave_tot, misc, &T, &remaining);
  if (blockIdx.x == 0 && tid == 0) { w.state[0] = T; w.state[1] = remaining; }
  const float* s = score + row0;
  const int b0 = blockIdx.x * chunk, b1 = b0 + chunk < N ? b0 + chunk : N;
  uint32_t gt = 0, eq = 0;
  for (int i = b0 + tid; i < b1; i += SEL_THREADS) {
    const uint32_t key = mono32(s[i], lg);
    gt += key > T ? 1u : 0u;
    eq += key == T ? 1u : 0u;
  }
  uint32_t tg, te;
  block_scan_excl(gt, wave_tot, &tg);
  block_scan_excl(eq, wave_tot, &te);
  if (tid == 0) { w.blk_gt[blockIdx.x] = tg; w.blk_eq[blockIdx.x] = te; }
}

__global__ __launch_bounds__(SEL_THREADS) void topk_gather_kernel(const float* __restrict__ score, TopkTab tab, int largest,
                                                                 char* __restrict__ ws, int64_t slot_bytes) {
  __shared__ __attribute__((aligned(16))) uint32_t wave_tot[SEL_WAVES];
  __shared__ uint32_t misc[8];
  const int tid = threadIdx.x, b = blockIdx.x;
  TK_LARGE_SEG((int)blockIdx.y)
  if (b >= G) return;
  const TopkSlot w = tk_slot(ws, blockIdx.y, slot_bytes);
  const bool lg = largest != 0;
  const uint32_t T = w.state[0], remaining = w.state[1];
  // positions: chunk b' < b took gt[b'] + min(max(remaining - eq_before[b'], 0), eq[b']) candidates
  if (tid == 0) {
    uint32_t eqb = 0, pos = 0;
    for (int q = 0; q < b; ++q) {
      const uint32_t e = w.blk_eq[q];
      const uint32_t room = remaining > eqb ? remaining - eqb : 0u;
      pos += w.blk_gt[q] + (e < room ? e : room);
      eqb += e;
    }
    misc[0] = eqb;
    misc[1] = pos;
  }
  __syncthreads();
  uint32_t eq_base = misc[0], pos_base = misc[1];
  __syncthreads();
  const float* s = score + row0;
  const int b0 = b * chunk, b1 = b0 + chunk < N ? b0 + chunk : N;
  for (int c0 = b0; c0 < b1; c0 += SEL_THREADS) {
    const int i = c0 + tid;
    uint32_t key = 0;
    bool gt = false, eq = false;
    if (i < b1) {
      key = mono32(s[i], lg);
      gt = key > T;
      eq = key == T;
    }
    uint32_t tot_eq, tot_take;
    const uint32_t erank = block_prefix(eq, wave_tot, &tot_eq);
    const bool take = gt || (eq && (eq_base + erank) < remaining);
    const uint32_t trank = block_prefix(take, wave_tot, &tot_take);
    if (take) w.cand[pos_base + trank] = ((uint64_t)key << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)i);
    eq_base += tot_eq;
    pos_base += tot_take;
  }
}

__global__ __launch_bounds__(SEL_THREADS) void topk_final_kernel(TopkTab tab, int k, int largest, int64_t* __restrict__ idx,
                                                                float* __restrict__ val, char* __restrict__ ws, int64_t slot_bytes) {
  __shared__ __attribute__((aligned(16))) uint64_t keys[MHIMX_TOPK_MAX_K];
  int seg = tab.large[0];
  RG_PICK(seg, tab.large, (int)blockIdx.x)
  const TopkSlot w = tk_slot(ws, blockIdx.x, slot_bytes);
  for (int j = threadIdx.x; j < k; j += SEL_THREADS) keys[j] = w.cand[j];           // (a large segment has more than k rows: k_b = k)
  __syncthreads();
  tk_order_write(keys, k, k, largest != 0, idx + (int64_t)seg * k, val ? val + (int64_t)seg * k : nullptr);
}

static int topk_check(const char* who, int32_t n_segs, const mhimx_topk_seg* segs, int64_t k) {
  MHIMX_CHECK_ARG(n_segs >= 1 && n_segs <= MHIMX_INFER_MAX, "%s: n_segs=%d must be in 1..%d", who, n_segs, MHIMX_INFER_MAX);
  MHIMX_CHECK_ARG(segs, "%s: null segment table", who);
  MHIMX_CHECK_ARG(k >= 1 && k <= MHIMX_TOPK_MAX_K, "%s: k=%lld must be in 1..%d", who, (long long)k, MHIMX_TOPK_MAX_K);
  for (int b = 0; b < n_segs; ++b) {
    MHIMX_CHECK_ARG(segs[b].N >= 1 && segs[b].N <= MHIMX_INFER_MAX_ROWS, "%s: segment %d: N must be in 1..%d", who, b, MHIMX_INFER_MAX_ROWS);
    MHIMX_CHECK_ARG(segs[b].row0 >= 0, "%s: segment %d: row0 must be >= 0", who, b);
  }
  return 0;
}
static int topk_n_large(int32_t n_segs, const mhimx_topk_seg* segs) {
  int n = 0;
  for (int b = 0; b < n_segs; ++b) n += segs[b].N > TK_SMALL_N ? 1 : 0;
  return n;
}

}  // namespace mhimx

using namespace mhimx;

extern "C" int64_t mhimx_topk_many_ws_bytes(int32_t n_segs, const mhimx_topk_seg* segs, int64_t k) {
  if (topk_check("mhimx_topk_many_ws_bytes", n_segs, segs, k)) return -1;
  return 256 + topk_n_large(n_segs, segs) * tk_slot_bytes(k);
}

extern "C" int mhimx_topk_many(void* stream, const float* score, int32_t n_segs, const mhimx_topk_seg* segs, int64_t k, int32_t largest,
                               int64_t* idx, float* val, void* ws, int64_t ws_bytes) {
  const char* who = "mhimx_topk_many";
  if (topk_check(who, n_segs, segs, k)) return -1;
  MHIMX_CHECK_ARG(score && idx, "%s: null score / idx", who);
  const int n_large = topk_n_large(n_segs, segs);
  const int64_t slot = tk_slot_bytes(k);
  if (rg_check_ws(who, ws, ws_bytes, 256 + n_large * slot)) return -1;
  TopkTab tab = {};
  int gmax = 1;
  for (int b = 0; b < n_segs; ++b) {
    tab.row0[b] = segs[b].row0;
    tab.N[b] = (int32_t)segs[b].N;
    if (segs[b].N > TK_SMALL_N) {
      tab.large[tab.n_large++] = b;
      const int g = (int)(cdiv(segs[b].N, TK_CHUNK) < TK_MAXG ? cdiv(segs[b].N, TK_CHUNK) : TK_MAXG);
      gmax = g > gmax ? g : gmax;
    }
  }
  tab.n = n_segs;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  hipLaunchKernelGGL(topk_small_kernel, dim3(n_segs + n_large), dim3(SEL_THREADS), 0, st, score, tab, (int)k, largest, idx, val, w, slot);
  if (n_large) {
    const dim3 grid(gmax, n_large);
    hipLaunchKernelGGL(topk_hist_kernel<0>, grid, dim3(SEL_THREADS), 0, st, score, tab, (int)k, largest, w, slot);
    hipLaunchKernelGGL(topk_hist_kernel<1>, grid, dim3(SEL_THREADS), 0, st, score, tab, (int)k, largest, w, slot);
    hipLaunchKernelGGL(topk_hist_kernel<2>, grid, dim3(SEL_THREADS), 0, st, score, tab, (int)k, largest, w, slot);
    hipLaunchKernelGGL(topk_count_kernel, grid, dim3(SEL_THREADS), 0, st, score, tab, (int)k, largest, w, slot);
    hipLaunchKernelGGL(topk_gather_kernel, grid, dim3(SEL_THREADS), 0, st, score, tab, largest, w, slot);
    hipLaunchKernelGGL(topk_final_kernel, dim3(n_large), dim3(SEL_THREADS), 0, st, tab, (int)k, largest, idx, val, w, slot);
  }
  MHIMX_LAUNCH_CHECK();
  return 0;
}
