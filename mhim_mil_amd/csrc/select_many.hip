// select_many.hip — mhimx_select_rows_many: the production hard-instance select (HAM mask + Merge split, mhimx_select_rows) of MANY score
// vectors of different lengths in one call: the row lists of every bag of a ragged accumulation window, or of a validation chunk
// (replaces the per-bag loop over mhim_modules/masking.py:9-88 + merge.py:158-176 that modules/mhim.py:341 runs once per slide).
//
// Bags of up to 16 384 rows: ONE launch, blockIdx.x = bag, of the device body select_small_kernel<KPT, LEAN = true> runs (select_dev.hpp:
// select_small_body - one copy of the threshold, the candidate list, both keyed draws, the compaction and the staged stores).  The bag
// table travels by value (infer_tab.hpp's RG_PICK pattern: constant indices only); nothing is copied to the device, waited for or
// allocated.  The launch uses ONE KPT - the class of its largest bag (4 / 10 / 16 keys per thread) - and one LDS size - from the largest
// P = next_pow2(k) - for every bag.  A bag's bits depend on neither: thread t owns the contiguous rows [t * KPT, (t + 1) * KPT), so the
// candidate list, the kept-row list and both compactions are in ascending row index for any KPT, the two Feistel draws index list
// positions only, and P only places the LDS arrays.  (One launch, not one per class: the workgroups of a launch run side by side, so the
// launch lasts as long as its largest bag on that bag's own class either way, and a second and third launch would only add their
// latency.)  Integer work only; no workgroup waits for another.
// Bags above 16 384 rows: select_large_rows per bag on the same stream - mhimx_random_perm, mhimx_select_mask, mhimx_random_perm and the
// [merge | stay] swap, the sequence mhimx_ragged_window_run and MHIM.student_rows issue for such a bag - out of the call's workspace.
#include "infer_tab.hpp"
#include "select_dev.hpp"

namespace mhimx {

constexpr int SM_SMALL_N = 16384, SM_SMALL_K = 4096, SM_LARGE_K = 16384;

// the small bags of a call (constant indices only: RG_PICK's rule)
struct SelManyTab {
  int64_t row0[MHIMX_INFER_MAX], out0[MHIMX_INFER_MAX];
  uint64_t seed[MHIMX_INFER_MAX];
  int32_t N[MHIMX_INFER_MAX], k[MHIMX_INFER_MAX], n_sel[MHIMX_INFER_MAX], merge_R[MHIMX_INFER_MAX];
};

static int sm_pow2(int v) {
  int p = 2;
  while (p < v) p <<= 1;
  return p;
}

// select_small_body<KPT, LEAN = true> (select_dev.hpp) with plane = bag: the steps of select_small_kernel's production form on the bag's own
// N, k, n_sel, merge_R and seed, largest scores first.
template <int KPT>
__global__ __launch_bounds__(SEL_THREADS) void select_many_kernel(const float* __restrict__ score_all, SelManyTab tab,
                                                                 const uint64_t* __restrict__ tick, int64_t* __restrict__ rows_all, int P,
                                                                 int merge_first) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int bag = blockIdx.x;
  int64_t row0 = tab.row0[0], out0 = tab.out0[0];
  uint64_t seed0 = tab.seed[0];
  int N = tab.N[0], k = tab.k[0], n_sel = tab.n_sel[0], merge_R = tab.merge_R[0];
  RG_PICK(row0, tab.row0, bag) RG_PICK(out0, tab.out0, bag) RG_PICK(seed0, tab.seed, bag)
  RG_PICK(N, tab.N, bag) RG_PICK(k, tab.k, bag) RG_PICK(n_sel, tab.n_sel, bag) RG_PICK(merge_R, tab.merge_R, bag)
  const SelectArgs a = {score_all + row0, N, k, n_sel, 1, nullptr, nullptr, 0, nullptr, nullptr, nullptr, P, merge_first ? 2 : 1,
                        eff_seed(seed0, tick), merge_R, rows_all + out0, nullptr, 0};
  select_small_body<KPT, true>(a, smem_raw);
}

// ------------------------------------------------------------------------------------------------ a bag above 16 384 rows
//   perm = pi_1 of 0 .. k-1 (masking.py:67's torch.randperm, keyed by (seed + 0x51ED270B, tick))
//   ids  = kept rows ascending ++ masked (mhimx_select_mask: the multi-workgroup select, the first n_sel entries of perm pick the masked)
//   rows = ids[pi_2(j)], j < len_keep (merge.py:165's shuffle of the kept rows, keyed by (seed ^ 0x3C6E.., tick)) = [stay (Lk) | merge (R)]
//   merge_first: rows_out = [merge | stay] (two copies); otherwise the second permutation writes rows_out itself.
int select_large_rows(hipStream_t st, const float* score, int64_t N, int64_t k, int64_t n_sel, uint64_t seed, const uint64_t* tick, int64_t merge_R,
                      int64_t* rows_out, int merge_first, const SelLargeWs& w) {
  const int64_t len_keep = N - n_sel, Lk = len_keep - merge_R;
  if (int r = mhimx_random_perm(st, k, seed + 0x51ED270Bull, tick, nullptr, w.perm)) return r;
  if (int r = mhimx_select_mask(st, score, N, k, n_sel, 1, n_sel < k ? w.perm : nullptr, nullptr, 0, w.ids, w.lk, nullptr, w.sel_ws, w.sel_ws_bytes))
    return r;
  if (!merge_first) return mhimx_random_perm(st, len_keep, seed ^ 0x3C6EF372FE94F82Bull, tick, w.ids, rows_out);
  if (int r = mhimx_random_perm(st, len_keep, seed ^ 0x3C6EF372FE94F82Bull, tick, w.ids, w.rows)) return r;
  if (merge_R) MHIMX_HIP(hipMemcpyAsync(rows_out, w.rows + Lk, (size_t)merge_R * 8, hipMemcpyDeviceToDevice, st));
  if (Lk) MHIMX_HIP(hipMemcpyAsync(rows_out + merge_R, w.rows, (size_t)Lk * 8, hipMemcpyDeviceToDevice, st));
  return 0;
}

// ------------------------------------------------------------------------------------------------ host
// the bag table's rules (mhimx.h), under the caller's name
int select_bags_check(const char* who, int32_t n_bags, const mhimx_select_bag* bags) {
  MHIMX_CHECK_ARG(n_bags >= 1 && n_bags <= MHIMX_INFER_MAX, "%s: n_bags=%d must be in 1..%d", who, n_bags, MHIMX_INFER_MAX);
  MHIMX_CHECK_ARG(bags, "%s: null bag table", who);
  for (int b = 0; b < n_bags; ++b) {
    const mhimx_select_bag& q = bags[b];
    MHIMX_CHECK_ARG(q.N >= 1 && q.N <= MHIMX_STEP_MAX_ROWS, "%s: bag %d: N=%lld must be in 1..%d", who, b, (long long)q.N, MHIMX_STEP_MAX_ROWS);
    const int64_t kcap = q.N <= SM_SMALL_N ? SM_SMALL_K : SM_LARGE_K, kmax = q.N < kcap ? q.N : kcap;
    MHIMX_CHECK_ARG(q.k >= 1 && q.k <= kmax, "%s: bag %d: k=%lld must be in 1..%lld (min(N, %lld) for a bag %s 16384 rows)", who, b, (long long)q.k,
                    (long long)kmax, (long long)kcap, q.N <= SM_SMALL_N ? "of up to" : "above");
    MHIMX_CHECK_ARG(q.n_sel >= 0 && q.n_sel <= q.k, "%s: bag %d: n_sel=%lld must be in 0..k", who, b, (long long)q.n_sel);
    MHIMX_CHECK_ARG(q.merge_R >= 0 && q.merge_R <= q.N - q.n_sel, "%s: bag %d: merge_R=%lld must be in 0..N - n_sel", who, b, (long long)q.merge_R);
    MHIMX_CHECK_ARG(q.row0 >= 0 && q.out0 >= 0, "%s: bag %d: row0 / out0 must be >= 0", who, b);
  }
  for (int b = 1; b < n_bags; ++b)
    for (int a = 0; a < b; ++a) {
      const int64_t a0 = bags[a].out0, a1 = a0 + bags[a].N - bags[a].n_sel, b0 = bags[b].out0, b1 = b0 + bags[b].N - bags[b].n_sel;
      MHIMX_CHECK_ARG(!(a0 < a1 && b0 < b1 && a0 < b1 && b0 < a1), "%s: bag %d: its output rows [%lld, %lld) overlap those of bag %d", who, b, (long long)b0, (long long)b1, a);
    }
  return 0;
}

// the large bags' scratch behind the first 256 bytes (the select_mask's len_keep word): one region each for the first permutation, the id
// list, the shuffled list and mhimx_select_mask's own workspace, sized for the largest large bag
struct SmLay { int64_t perm, ids, rows, sel_ws, sel_ws_bytes, total; };
static SmLay sm_layout(int32_t n_bags, const mhimx_select_bag* bags) {
  int64_t perm_n = 0, ids_n = 0, rows_n = 0, sel_b = 0;
  for (int b = 0; b < n_bags; ++b) {
    const mhimx_select_bag& q = bags[b];
    if (q.N <= SM_SMALL_N) continue;
    auto up = [](int64_t& a, int64_t v) { if (v > a) a = v; };
    up(perm_n, q.k); up(ids_n, q.N); up(rows_n, q.N - q.n_sel); up(sel_b, mhimx_select_ws_bytes(q.N));
  }
  SmLay l;
  Arena ar(nullptr, 0);
  ar.take<char>(256);
  l.perm = ar.off; ar.take<int64_t>(perm_n);
  l.ids = ar.off; ar.take<int64_t>(ids_n);
  l.rows = ar.off; ar.take<int64_t>(rows_n);
  l.sel_ws_bytes = sel_b; l.sel_ws = ar.off; ar.take<char>(sel_b);
  l.total = ar.off;
  return l;
}

// a table select_bags_check has taken: the small bags in one launch, then every large bag's sequence (w: their scratch)
int select_rows_many_launch(hipStream_t st, const float* score, int32_t n_bags, const mhimx_select_bag* bags, const uint64_t* tick,
                            int64_t* rows_out, const SelLargeWs& w, int merge_first) {
  SelManyTab tab = {};
  int n_small = 0, kmax = 1;
  int64_t nmax = 0;
  for (int b = 0; b < n_bags; ++b) {
    const mhimx_select_bag& q = bags[b];
    if (q.N > SM_SMALL_N) continue;
    tab.row0[n_small] = q.row0; tab.out0[n_small] = q.out0; tab.seed[n_small] = q.seed;
    tab.N[n_small] = (int32_t)q.N; tab.k[n_small] = (int32_t)q.k; tab.n_sel[n_small] = (int32_t)q.n_sel; tab.merge_R[n_small] = (int32_t)q.merge_R;
    ++n_small;
    if (q.N > nmax) nmax = q.N;
    if (q.k > kmax) kmax = (int)q.k;
  }
  if (n_small) {
    const int P = sm_pow2(kmax);
    const size_t sm = select_lds_bytes(P, true);
    MHIMX_ONCE_PER_DEVICE(
        MHIMX_HIP(hipFuncSetAttribute((const void*)select_many_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)select_lds_bytes(SM_SMALL_K, true)));
        MHIMX_HIP(hipFuncSetAttribute((const void*)select_many_kernel<10>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)select_lds_bytes(SM_SMALL_K, true)));
        MHIMX_HIP(hipFuncSetAttribute((const void*)select_many_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)select_lds_bytes(SM_SMALL_K, true))));
#define MHIMX_SEL_MANY(KPT) \
    hipLaunchKernelGGL(select_many_kernel<KPT>, dim3((unsigned)n_small), dim3(SEL_THREADS), sm, st, score, tab, tick, rows_out, P, merge_first ? 1 : 0)
    if (nmax <= 4096) MHIMX_SEL_MANY(4);                // every bag of the launch fits 1024 * KPT rows
    else if (nmax <= 10240) MHIMX_SEL_MANY(10);
    else MHIMX_SEL_MANY(16);
#undef MHIMX_SEL_MANY
    MHIMX_LAUNCH_CHECK();
  }
  for (int b = 0; b < n_bags; ++b) {
    const mhimx_select_bag& q = bags[b];
    if (q.N <= SM_SMALL_N) continue;
    if (int r = select_large_rows(st, score + q.row0, q.N, q.k, q.n_sel, q.seed, tick, q.merge_R, rows_out + q.out0, merge_first, w)) return r;
  }
  return 0;
}

}  // namespace mhimx

using namespace mhimx;

extern "C" int64_t mhimx_select_rows_many_ws_bytes(int32_t n_bags, const mhimx_select_bag* bags) {
  if (select_bags_check("mhimx_select_rows_many_ws_bytes", n_bags, bags)) return -1;
  return sm_layout(n_bags, bags).total;
}

extern "C" int mhimx_select_rows_many(void* stream, const float* score, int32_t n_bags, const mhimx_select_bag* bags, const uint64_t* tick,
                                      int64_t* rows_out, void* ws, int64_t ws_bytes, int32_t merge_first) {
  const char* who = "mhimx_select_rows_many";
  if (select_bags_check(who, n_bags, bags)) return -1;
  MHIMX_CHECK_ARG(score && rows_out, "%s: null score / rows_out", who);
  const SmLay l = sm_layout(n_bags, bags);
  if (rg_check_ws(who, ws, ws_bytes, l.total)) return -1;
  char* base = static_cast<char*>(ws);
  SelLargeWs w;
  w.lk = reinterpret_cast<int64_t*>(base);
  w.perm = reinterpret_cast<int64_t*>(base + l.perm);
  w.ids = reinterpret_cast<int64_t*>(base + l.ids);
  w.rows = reinterpret_cast<int64_t*>(base + l.rows);
  w.sel_ws = base + l.sel_ws;
  w.sel_ws_bytes = l.sel_ws_bytes;
  return select_rows_many_launch((hipStream_t)stream, score, n_bags, bags, tick, rows_out, w, merge_first);
}
