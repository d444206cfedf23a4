// infer_tab.hpp — what the ragged native calls share (mhimx_infer_run: infer.hip, mhimx_infer_dsmil_run: infer_dsmil.hip,
// mhimx_pure_window_run: pure_window.hip, mhimx_ragged_window_run: ragged_window.hip, their projection kernels: bag_project.hip): the
// per-bag table, ONE copy of the device pieces their kernels have in common (the bag lookup RG_PICK / RG_BAG / RG_FIND_BAG, the bf16 split
// rg_split, the 3-term bf16 k-loop rg_mma3, the {max, sum} merge of a bag's pool partials in index order rg_merge_stats) and ONE copy of
// the host checks and table fill (rg_check_*, rg_tab_*; for the three inference calls - mhimx_infer_transmil_run: infer_transmil.hip is the
// third - their whole common front rg_check_infer_front / rg_check_infer_bags / rg_check_infer_io and their table rg_tab_fill; the DSMIL
// launches 4 - 7 as host calls dsmil_rows_crit_pool / dsmil_finalize).  A piece is shared only where every kernel that uses it keeps its code,
// instruction for instruction (tools/kernel_meta.py --diff against the build before; profiles/ragged_shared.md names what stayed a copy).
#pragma once
#include <math.h>

#include "mma_tile.hpp"

namespace mhimx {

// Everything a kernel needs to know about a bag, as ONE by-value kernel argument: no host-to-device copy, nothing to wait for.
struct InferTab {
  const float* X[MHIMX_INFER_MAX];
  int64_t ldx[MHIMX_INFER_MAX], N[MHIMX_INFER_MAX];
  int64_t row0[MHIMX_INFER_MAX];                  // first row of the bag in the call's row space (feature rows, score, attn)
  int32_t tile0[MHIMX_INFER_MAX];                 // first 160-row projection tile
  int32_t part0[MHIMX_INFER_MAX];                 // first pool partial (= first 256-row scorer chunk)
  int32_t n, tiles, parts, pad;                   // pad: the element type of the rows X points to (mhimx.h MHIMX_X_*; 0 = fp32)
};
static_assert(MHIMX_PURE_WINDOW_MAX == MHIMX_INFER_MAX && MHIMX_RAGGED_WINDOW_MAX == MHIMX_INFER_MAX, "the window calls use the inference call's table");
// dst = arr[b] of a by-value per-bag array (constant indices only: a dynamically indexed by-value argument is copied to scratch)
#define RG_PICK(dst, arr, b)                                     \
  _Pragma("unroll") for (int q_ = 0; q_ < MHIMX_INFER_MAX; ++q_) \
    if (q_ == (b)) dst = (arr)[q_];

// The element type XT (MHIMX_X_*) of the bags' rows in the two kernels that read X (infer_project_body: bag_project.hip; pw_tn_kernel:
// pure_window.hip): what 4 / 2 consecutive elements are loaded as, and their widening to fp32 - exact for every fp16 and bf16 value,
// subnormals included (v_cvt_f32_f16 honours fp16 denormals; a bf16 IS the upper half of an fp32).  XT = 0 is the identity.
typedef float x_f2 __attribute__((ext_vector_type(2)));
typedef unsigned x_u2 __attribute__((ext_vector_type(2)));
typedef _Float16 x_h2 __attribute__((ext_vector_type(2)));
template <int XT> struct XRow { typedef float elt; typedef f32x4 v4; typedef x_f2 v2; };
template <> struct XRow<1> { typedef _Float16 elt; typedef x_u2 v4; typedef unsigned v2; };
template <> struct XRow<2> { typedef unsigned short elt; typedef x_u2 v4; typedef unsigned v2; };
template <int XT> MHIMX_DEV x_f2 x_widen(unsigned w) {          // two 2-byte elements of one dword
  if constexpr (XT == 1) {
    const x_h2 h = __builtin_bit_cast(x_h2, w);
    return x_f2{(float)h[0], (float)h[1]};
  } else {
    return x_f2{__builtin_bit_cast(float, w << 16), __builtin_bit_cast(float, w & 0xffff0000u)};
  }
}
template <int XT> MHIMX_DEV f32x4 x_widen(const x_u2& w) {
  const x_f2 a = x_widen<XT>(w[0]), b = x_widen<XT>(w[1]);
  return f32x4{a[0], a[1], b[0], b[1]};
}
template <int XT> MHIMX_DEV const f32x4& x_widen(const f32x4& v) { return v; }
template <int XT> MHIMX_DEV const x_f2& x_widen(const x_f2& v) { return v; }

constexpr int INFER_TILE_ROWS = 160;              // rows of a projection tile (bag-major tile numbering: InferTab.tile0)
constexpr int IE = 512;                           // feature width of the ragged path
constexpr int RG_ROWS = 32;                       // rows of a scorer / pool tile in LDS
constexpr int RG_CHUNK = 256;                     // rows of a pool partial (InferTab.part0 counts them)
constexpr int RG_LD = IE + 4;                     // pitch of a feature row in LDS
constexpr int RG_T = 256;                         // threads of the kernels that walk 32-row tiles
constexpr int RG_FIN_T = 512;                     // threads of the kernels that merge a bag's partials (one per pooled column)

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------------------------------------ device: which bag, and its numbers
// Inside a kernel whose by-value table argument is called `tab`.  RG_BAG(b) declares bag b's N, orow0 (its first row in the call's row
// space) and p0 (its first pool partial); RG_FIND_BAG(key, first) declares `bag` = the last bag b with tab.first[b] <= key - the owner of pool
// partial `key` (first = part0) or of row `key` of the row space (first = row0); RG_BAG_OF is the two together.  Macros, not functions: a
// function that takes the table by reference makes the compiler copy the whole by-value argument first (infer_score_kernel: 23 more
// instructions); these expand to the text every kernel used to carry, and the kernels keep their code.
#define RG_BAG(b)                                                             \
  [[maybe_unused]] int64_t N = tab.N[0], orow0 = tab.row0[0];                 \
  [[maybe_unused]] int p0 = tab.part0[0];                                     \
  RG_PICK(N, tab.N, b) RG_PICK(orow0, tab.row0, b) RG_PICK(p0, tab.part0, b)
#define RG_FIND_BAG(key, first)                                               \
  int bag = 0;                                                                \
  _Pragma("unroll") for (int b_ = 1; b_ < MHIMX_INFER_MAX; ++b_)              \
    if (b_ < tab.n && (key) >= tab.first[b_]) bag = b_;
#define RG_BAG_OF(key, first) RG_FIND_BAG(key, first) RG_BAG(bag)
MHIMX_DEV int rg_parts(int64_t N) { return (int)((N + RG_CHUNK - 1) / RG_CHUNK); }      // pool partials of a bag of N rows

// ------------------------------------------------------------------------------------------------ device: 3-term bf16 k-loop
// bf16 hi / lo halves of 8 floats
MHIMX_DEV void rg_split(const f32x4& a, const f32x4& b, bf8& hi, bf8& lo) {
  const float x[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const __bf16 h = (__bf16)x[i];
    hi[i] = h;
    lo[i] = (__bf16)(x[i] - (float)h);
  }
}
// A[32 rows of LDS, K] B^T for one wave's 32 columns: v_mfma_f32_32x32x16_bf16, A split on the fly, B a prep kind-4 image, one accumulator
// per bf16x3 term; returns the terms added as hi*hi + (lo*hi + hi*lo).  aptr = tile + (lane & 31) * ld + 8 * (lane >> 5); fptr = image +
// ((wave * (K / 16) * 64 + lane) * 8 floats (+ ks * 128: hi, + 1: lo).  Element i of the result: row 8 (i >> 2) + 4 (lane >> 5) + (i & 3).
template <int K>
MHIMX_DEV f32x16 rg_mma3(const float* aptr, const f32x4* fptr) {
  f32x16 acc, acc2, acc3;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc[i] = 0.f; acc2[i] = 0.f; acc3[i] = 0.f; }
  f32x4 bh = fptr[0], bl = fptr[1];
#pragma unroll 4
  for (int ks = 0; ks < K / 16; ++ks) {
    const int kn = ks + 1 < K / 16 ? ks + 1 : ks;
    const f32x4 nbh = fptr[128 * kn], nbl = fptr[128 * kn + 1];
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(aptr + 16 * ks), a1 = *reinterpret_cast<const f32x4*>(aptr + 16 * ks + 4);
    bf8 ah, al;
    rg_split(a0, a1, ah, al);
    const bf8 bh8 = __builtin_bit_cast(bf8, bh), bl8 = __builtin_bit_cast(bf8, bl);
    acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh8, acc2, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh8, acc, 0, 0, 0);
    acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl8, acc3, 0, 0, 0);
    bh = nbh;
    bl = nbl;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] += acc2[i] + acc3[i];
  return acc;
}

// ------------------------------------------------------------------------------------------------ device: merge of a bag's pool partials
// {max, sum} of a bag's G partials pm / pl [g * stride], by RG_FIN_T threads (red: 8 floats of LDS): every block that calls this for a bag
// gets the same bits - the per-thread order, the wave reductions and the order of the 8 wave results are fixed.
MHIMX_DEV void rg_merge_stats(const float* __restrict__ pm, const float* __restrict__ pl, int G, int stride, float* red, float& mx, float& L) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float m = -INFINITY;
  for (int b = tid; b < G; b += RG_FIN_T) m = fmaxf(m, pm[(int64_t)b * stride]);
  m = wave_max(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  float mxv = red[0];
#pragma unroll
  for (int w = 1; w < 8; ++w) mxv = fmaxf(mxv, red[w]);
  __syncthreads();
  float lp = 0.f;
  for (int b = tid; b < G; b += RG_FIN_T) lp += pl[(int64_t)b * stride] * __expf(pm[(int64_t)b * stride] - mxv);
  lp = wave_sum(lp);
  if (lane == 0) red[wave] = lp;
  __syncthreads();
  float Lv = 0.f;
#pragma unroll
  for (int w = 0; w < 8; ++w) Lv += red[w];                   // fixed order: deterministic
  mx = mxv;
  L = Lv;
}

// ------------------------------------------------------------------------------------------------ host: checks and table fill
// What differs between the calls' per-bag checks.  The inference calls cap the pitch at 2^20 elements for every element type and do not
// bound a bag's bytes; the window calls (`window`) bound N * ldx * element size below 2^32 - 32-bit byte offsets in the d W1 launch - and
// cap the pitch only for the 2-byte types.  max_n: the most rows of one bag (0: the caller has checked N itself).
struct RgRules { int64_t max_n; bool window; };
inline int rg_check_xdt(const char* who, int32_t xdt) {
  MHIMX_CHECK_ARG(xdt >= MHIMX_X_F32 && xdt <= MHIMX_X_BF16, "%s: x_dtype %d is none of MHIMX_X_F32 / F16 / BF16", who, xdt);
  return 0;
}
inline int rg_check_bag(const char* who, int b, int64_t N, int64_t ldx, int64_t D, int32_t xdt, const RgRules& rules) {
  if (rules.max_n) MHIMX_CHECK_ARG(N >= 1 && N <= rules.max_n, "%s: bag %d: N must be in 1..%lld", who, b, (long long)rules.max_n);
  const bool f32 = xdt == MHIMX_X_F32;
  const int mult = f32 ? 4 : 8, elt = f32 ? 4 : 2;
  const bool capped = !(rules.window && f32);
  const bool pitch_ok = ldx >= D && ldx % mult == 0 && (!capped || ldx <= (1 << 20));
  if (f32) MHIMX_CHECK_ARG(pitch_ok, "%s: bag %d: row pitch below D or not a multiple of 4 floats", who, b);
  else MHIMX_CHECK_ARG(pitch_ok, "%s: bag %d: row pitch below D%s or not a multiple of 8 two-byte elements", who, b, rules.window ? ", above 2^20" : "");
  if (rules.window) MHIMX_CHECK_ARG(N * ldx * elt < ((int64_t)1 << 32), "%s: bag %d: N * ldx * %d must stay below 2^32", who, b, elt);
  return 0;
}
inline int rg_check_ws(const char* who, const void* ws, int64_t ws_bytes, int64_t need) {
  MHIMX_CHECK_ARG(ws && (reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: the workspace must be 256-byte aligned", who);
  MHIMX_CHECK_ARG(ws_bytes >= need, "%s: workspace too small (%lld bytes, need %lld)", who, (long long)ws_bytes, (long long)need);
  return 0;
}
// The table, bag after bag: bag b starts at the running row / tile / partial counts and takes slot_rows rows of the row space (N in the
// inference calls; N, or N + k, rounded up to 32 in the window calls).  tab may be null (layout only: the counts are what is wanted).
struct RgCount { int64_t rows = 0, tiles = 0, parts = 0; };
inline void rg_tab_add(InferTab* tab, RgCount& n, int b, const float* X, int64_t ldx, int64_t N, int64_t slot_rows) {
  if (tab) {
    tab->X[b] = X; tab->ldx[b] = ldx; tab->N[b] = N;
    tab->row0[b] = n.rows; tab->tile0[b] = (int32_t)n.tiles; tab->part0[b] = (int32_t)n.parts;
  }
  n.rows += slot_rows;
  n.tiles += cdiv(N, INFER_TILE_ROWS);
  n.parts += cdiv(N, RG_CHUNK);
}
inline void rg_tab_close(InferTab* tab, const RgCount& n, int n_bags) {
  if (tab) { tab->n = n_bags; tab->tiles = (int32_t)n.tiles; tab->parts = (int32_t)n.parts; }
}
// the table of an inference call: every bag takes its own N rows of the row space
inline RgCount rg_tab_fill(InferTab* tab, int32_t n_bags, const mhimx_infer_bag* bags) {
  RgCount n;
  for (int b = 0; b < n_bags; ++b) rg_tab_add(tab, n, b, bags[b].X, bags[b].ldx, bags[b].N, bags[b].N);
  rg_tab_close(tab, n, n_bags);
  return n;
}
// The checks the three inference calls (`who`: infer, infer_dsmil, infer_transmil) make alike, in the order they refuse: the element type,
// null arguments, the bag count (`got`: the message names n_bags) - rg_check_infer_front; the call's own shape and activation lines; every
// bag's N and pitch, the rows of the call - rg_check_infer_bags.  And what only the *_run entry points ask, behind their parameter
// checks: every bag's address, the outputs the call cannot do without (`outputs`, else "<who>: <outputs_text>"), labels for the loss.
inline int rg_check_infer_front(const char* who, int32_t xdt, const void* cfg, int32_t n_bags, const mhimx_infer_bag* bags, bool got) {
  if (int r = rg_check_xdt(who, xdt)) return r;
  MHIMX_CHECK_ARG(cfg && bags, "%s: null configuration / bag list", who);
  if (got) MHIMX_CHECK_ARG(n_bags >= 1 && n_bags <= MHIMX_INFER_MAX, "%s: 1..%d bags per call (got %d)", who, MHIMX_INFER_MAX, n_bags);
  MHIMX_CHECK_ARG(n_bags >= 1 && n_bags <= MHIMX_INFER_MAX, "%s: 1..%d bags per call", who, MHIMX_INFER_MAX);
  return 0;
}
inline int rg_check_infer_bags(const char* who, int64_t D, int32_t n_bags, const mhimx_infer_bag* bags, int32_t xdt) {
  int64_t rows = 0;
  for (int b = 0; b < n_bags; ++b) {
    if (int r = rg_check_bag(who, b, bags[b].N, bags[b].ldx, D, xdt, RgRules{MHIMX_INFER_MAX_ROWS, false})) return r;
    rows += bags[b].N;
  }
  MHIMX_CHECK_ARG(rows <= MHIMX_INFER_MAX_ROWS, "%s: more than %d rows in one call", who, MHIMX_INFER_MAX_ROWS);
  return 0;
}
inline int rg_check_infer_io(const char* who, int32_t n_bags, const mhimx_infer_bag* bags, bool outputs, const char* outputs_text, const void* loss,
                             const void* labels) {
  for (int b = 0; b < n_bags; ++b) MHIMX_CHECK_ARG(bags[b].X && aligned16(bags[b].X), "%s: bag %d: null or unaligned rows", who, b);
  MHIMX_CHECK_ARG(outputs, "%s: %s", who, outputs_text);
  MHIMX_CHECK_ARG(!loss || labels, "%s: the loss output needs labels", who);
  return 0;
}

// what the TRAIN-mode ragged projection (mhimx_pure_window_run) needs beyond the table: every bag's dropout seed, the device tick the
// seeds are mixed with, the dropout probability and the fp16 d out / d pre rows (row space of the call, like the feature rows)
struct PureWinDrop {
  uint64_t seed[MHIMX_INFER_MAX];
  const uint64_t* tick;
  _Float16* dact;
  float drop_p, pad;
};
int pure_window_project(hipStream_t st, const InferTab& tab, const PureWinDrop& dr, int D, const float* w1p, const float* b1, int act, float* Hout);
// the same launch with the gemm epilogues' per-element dropout law (the mask ops.gemm_nt draws for the same seed, tick, row, column)
int pure_window_project_elem(hipStream_t st, const InferTab& tab, const PureWinDrop& dr, int D, const float* w1p, const float* b1, int act, float* Hout);
// the ragged scorer + pool-partial launch of infer.hip (one workgroup per 256-row chunk of one bag; InferTab.part0 / .parts / .row0)
int infer_score(hipStream_t st, const InferTab& tab, const float* H, const float* wa_frag, const float* wc, int act, float* s, float* pm, float* pl,
                float* pz);

// the same launch + the class projections of the pseudo score, cproj [rows of the row space][4] = h . Wp_c (C <= 4), taken while the rows are
// LDS-resident (infer_score_kernel<true>; mhimx_ragged_window_run's teacher)
int infer_score_cproj(hipStream_t st, const InferTab& tab, const float* H, const float* wa_frag, const float* wc, int act, float* s, float* pm,
                      float* pl, float* pz, const float* wp, int C, float* cproj);
// pure_window.hip's split-K rule, d W1 = sum_b dPRE_b^T X_b launch (pw_tn_kernel<true, XT>) and index-order reduction launch as host calls
int pw_split_k(int steps, int want_max, int div, int32_t* S, int32_t* per);
int pw_wgrad_bagx(hipStream_t st, const InferTab& tab, const float* dpre, int D, int steps, int S, int per, float* slabs);
int pw_reduce(hipStream_t st, int n, const float* const* parts, const int32_t* G, const int64_t* W, float* const* out);
// the same product with both operands as fp32 rows of the row space (pw_tn_kernel<false, 0>): slabs[z][M][Nc] = sum over the k-steps of slab z
// of A[rows, M]^T B[rows, Nc]; M and Nc multiples of 128, padding rows of both operands finite and zero in A
int pw_wgrad_rows(hipStream_t st, const InferTab& tab, const float* A, int lda, int M, const float* B, int ldb, int Nc, int steps, int S, int per,
                  float* slabs);
// infer_dsmil.hip's launches 4, 5, 6 over a table (row space, chunks) as a host call: per-row Q / classes and the arg-max partials, the
// critical rows (crit, logits_ins, q_max), the softmax-pool partials {pm, pl, pB}; C <= 16
// score (optional, rows of the row space): max_c classes of every row - the instance score of a model with cls_attn
int dsmil_rows_crit_pool(hipStream_t st, const InferTab& tab, const float* H, const float* V, const float* q0f, const float* bq0, const float* q2f,
                         const float* bq2, const float* wi, const float* bi, int C, float* Q, float* cls, float* pmax, int32_t* parg, float* qmax,
                         float* logits_ins, int64_t* crit, float* pm, float* pl, float* pB, float* score = nullptr);
// infer_dsmil.hip's launch 7 over a table as a host call: plane = bag, the partials merged in index order -> B [n, C, 512], logits_bag,
// logits [n, C]; attn (optional, rows of the row space): max_c A of every row (no_norm: max_c a); loss (optional, needs labels) [n]
int dsmil_finalize(hipStream_t st, const InferTab& tab, const float* pm, const float* pl, const float* pB, const float* Q, const float* qmax,
                   const float* wfcc, const float* bfcc, int C, const float* logits_ins, float* logits_bag, float* logits, float* B, float* attn,
                   int no_norm = 0, const int64_t* labels = nullptr, float* loss = nullptr);
// (the DSMIL student of the two DSMIL train calls - head kernel, layout share, forward, backward, reductions, checks: dsmil_student.hpp)
// ragged_window.hip's launch C.5 as a host call: q <- mm^n q + (1 - mm) sum_b mm^(n-1-b) z_b, z_b = the k rows of Hs from row tok[b] on
int rw_q_chain(hipStream_t st, float* q, const float* Hs, int n_bags, const int64_t* tok, double mm, int n_floats);
// step.hip: the checks mhimx_step_run makes on (cfg, N, counts)
int step_check_cfg(const mhimx_step_cfg* c, int64_t N, const mhimx_step_counts* n);

// select_many.hip: the select of a bag above 16 384 rows as ONE helper with explicit pointers (mhimx_random_perm, mhimx_select_mask,
// mhimx_random_perm, the [merge | stay] swap) - w.perm [k], w.ids [N], w.rows [N - n_sel] (merge_first only), w.lk [1], w.sel_ws
// (mhimx_select_ws_bytes(N)); the bag table's checks under the caller's name `who`; and the many-select of a table that passed them (the
// small bags in one launch, then every large bag through the helper out of the one scratch set w).  mhimx_select_rows_many is check,
// pointer and workspace checks, launch; mhimx_ragged_window_run checks and launches with its own workspace regions.
struct SelLargeWs { int64_t *perm, *ids, *rows, *lk; void* sel_ws; int64_t sel_ws_bytes; };
int select_large_rows(hipStream_t st, const float* score, int64_t N, int64_t k, int64_t n_sel, uint64_t seed, const uint64_t* tick, int64_t merge_R,
                      int64_t* rows_out, int merge_first, const SelLargeWs& w);
int select_bags_check(const char* who, int32_t n_bags, const mhimx_select_bag* bags);
int select_rows_many_launch(hipStream_t st, const float* score, int32_t n_bags, const mhimx_select_bag* bags, const uint64_t* tick, int64_t* rows_out,
                            const SelLargeWs& w, int merge_first);

// the ragged one-model projection launch (bag_project.hip): Hout[row0[b] + m, :] = act(X_b[m, :] W1^T + b1) for every bag b of the table
int infer_project(hipStream_t st, const InferTab& tab, int D, const float* w1p, const float* b1, int act, float* Hout);

}  // namespace mhimx
