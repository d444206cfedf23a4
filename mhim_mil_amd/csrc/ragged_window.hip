// ragged_window.hip — mhimx_ragged_window_run: ONE optimiser update of the full MHIM(ABMIL) model (teacher, HAM select, Merge, student,
// distillation, EMA teacher) over up to MHIMX_RAGGED_WINDOW_MAX bags of DIFFERENT row counts behind one C call (include/mhimx.h).
// replaces: engines/base_engine.py:29-51,76-167 (the accumulation window, its one optimizer.step() and the per-parameter EMA) around
//           engines/common_mil.py:14-48 (forward_func: model_ema.forward_teacher -> model(bag, score, teacher_feat)), i.e.
//           modules/mhim.py:181-227 (forward_teacher), :109-179 (get_mask), :318-378 (forward) and their autograd, with the loader's
//           different N per slide (datasets/dataset_feat.py:93-111) - and, on this side of the boundary, FusedTrainer.window_step's stream
//           form (_nat_prep / _nat_bag per bag from Python) for windows mhimx_window_run's one-shape rule refuses.
//
// The call's row space: bag b owns a slot of 32 * ceil((N_b + k) / 32) rows (its N feature rows, the k Merge tokens where the per-bag entry
// points expect them - H_student + N * E - then zero rows), so that a 32-row tile / k-step lies inside one bag.  Three parts:
//
//   A. the teacher half and every bag's row list, window-wide (7 launches whatever n_bags is; + 5 per bag above 16 384 rows)
//      1  mhimx_prep_batch            counters, both W1 paired-plane images, both Wa fragment images, the student's transposed images, the
//                                     query snapshot
//      2  pure_window_project_kernel  (bag_project.hip, as it is) the teacher's feature rows: drop_p_teacher, per-bag seed
//      3  pure_window_project_kernel  the student's feature rows + fp16 d out / d pre (the teacher launch's d out / d pre rows land in the
//                                     same buffer first and are overwritten: TWO launches of the existing body, not a two-head instantiation)
//      4  rw_pad_kernel               zero rows between a bag's 32-row boundary and the end of its slot (feature rows of both models,
//                                     d out / d pre), the kept-row map cleared
//      5  infer_score_kernel<false> / <true>   (infer.hip) the teacher's scores + one pool partial per 256 rows; attn2score = 1:
//                                     the instantiation that also takes the class projections h . Wp_c while the rows are LDS-resident
//      6  rw_finalize_kernel          plane = bag: the partials merged in index order -> {max, sum}, z_teacher; every row's instance score
//                                     (attention, or the pseudo score of scoring.py:37-58 with its bp[0] quirk)
//      7  select_many_kernel<KPT>     (select_many.hip) plane = bag: HAM mask + Merge split of every bag of up to 16 384 rows, the ragged form
//                                     of mhimx_select_rows' production kernel; a bag above 16 384 rows: select_large_rows behind it
//                                     (random_perm, select_mask, random_perm, two copies) out of the call's select scratch.  The select
//                                     reads the bag's scores, its seed and *tick (which moves once, in A.1): the same bits as inside the loop
//   B. the middle, bag after bag: mhimx_step_run's entry points in its order with pointers into the bag's slot (12 launches per bag;
//      launches 2-9 through step_mid.hpp's one copy: mid_student_fwd, mid_head, mid_bwd_rows)
//      1     mhimx_prep_batch        the row list's constant tail, the parameter-only part of this bag's Merge (its workspace is shared)
//      2     mhimx_abmil_pool_fwd    phase 1: student scorer over the rows that stay, Merge's rows pass riding
//      3-5   mhimx_merge_fwd         partial merge | O | to_out (the queries' EMA goes to scratch: the window's first queries stay)
//      6     mhimx_abmil_pool_fwd    phase 2: the finalize that scores the tokens
//      7     mhimx_head_fwd_bwd      loss scale 1 / n_bags
//      8     mhimx_abmil_pool_bwd    fp32 dH rows (pg.img = NULL): the stay rows' gradient exists as rows of the bag's slot
//      9     mhimx_merge_bwd         rows backward + the parked scorer-weight-gradient product
//      10-12 mhimx_reduce_flush      the Merge tail's stages + the bag's queued reductions
//      The small gradients accumulate in bag order on the one stream: bag 0 overwrites cfg->grad, every later bag adds (accumulate = 1).
//      A bag runs forward and backward before the next starts: the Merge and pool workspaces exist once, sized for the largest bag.
//   C. the backward tail, window-wide (6 launches; 5 with update = 0)
//      1  rw_keep_kernel             the kept-row map: keep[row0_b + rows_all_b[j]] = 1, j < len_keep_b
//      2  rw_dpre_kernel             one workgroup per 32-row tile of the row space: dPRE = dH * d out / d pre on kept rows, zero rows
//                                    elsewhere (masked, padding and token rows), IN PLACE on the gradient rows; the tile's column sums
//      3  pw_tn_kernel<true, XT>     (pure_window.hip, as it is) d W1 = sum_b dPRE_b^T X_b over the row space: masked rows ride as zero
//                                    rows (<= n_sel / N of wasted k-steps, 1.5 % at the default ratios) instead of a gather
//      4  pw_reduce_kernel           (pure_window.hip) d W1's slabs and d b1's per-tile partials in index order
//      5  rw_q_chain_kernel          q <- mm^n q + (1 - mm) sum_b mm^(n-1-b) z_b on the bags' tokens
//      6  mhimx_optim_step           Adam + EMA teacher (update = 1)
// Launch count: 13 (window-wide: 7 + 6) + 12 x n_bags (+ 5 window-wide for a bag above 16 384 rows).  No floating-point atomics, no workgroup waits for another, every sum has a fixed order.
#include <math.h>
#include <string.h>

#include "infer_tab.hpp"
#include "step_mid.hpp"
#include "surv_dev.hpp"

namespace mhimx {

namespace {

constexpr int RW_ROWS = RG_ROWS, RW_T = 256;                     // tile of the row space
constexpr int FIN_SCORE_BLOCKS = 8;
constexpr int RW_MAX = MHIMX_RAGGED_WINDOW_MAX;                  // (= MHIMX_INFER_MAX: the by-value bag table is the inference call's)

typedef _Float16 rw_h4 __attribute__((ext_vector_type(4)));

// per-bag counts the window-wide launches need beyond the table (constant indices only: RG_PICK's rule)
struct RwCnt { int32_t len_keep[RW_MAX]; int32_t slot[RW_MAX]; };

// ------------------------------------------------------------------------------------------------ A4. zero rows of a slot, kept-row map
// blockIdx.x = bag.  The ragged projection zeroes a bag's rows up to the next multiple of 32; a slot of 32 * ceil((N + k) / 32) rows may
// hold one more 32-row tile.  Its rows are zero rows here (the k tokens among them are written later, by the bag's Merge).
__global__ __launch_bounds__(RW_T) void rw_pad_kernel(InferTab tab, RwCnt cn, float* __restrict__ Ht, float* __restrict__ Hs,
                                                      _Float16* __restrict__ dact, uint8_t* __restrict__ keep) {
  const int bag = blockIdx.x;
  int64_t N = tab.N[0], orow0 = tab.row0[0];
  int slot = cn.slot[0];
  RG_PICK(N, tab.N, bag) RG_PICK(orow0, tab.row0, bag) RG_PICK(slot, cn.slot, bag)
  for (int r = threadIdx.x + blockIdx.y * RW_T; r < slot; r += RW_T * gridDim.y) keep[orow0 + r] = 0;
  if (blockIdx.y != 0) return;
  const int64_t p0 = (N + 31) & ~(int64_t)31;
  const int pad = (int)(slot - p0);                            // 0 or 32
  const f32x4 z4 = f32x4{0.f, 0.f, 0.f, 0.f};
  const rw_h4 zh = rw_h4{(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
  for (int f = threadIdx.x; f < pad * (IE / 4); f += RW_T) {
    const int64_t o = (orow0 + p0) * IE + 4 * (int64_t)f;
    *reinterpret_cast<f32x4*>(Ht + o) = z4;
    *reinterpret_cast<f32x4*>(Hs + o) = z4;
    *reinterpret_cast<rw_h4*>(dact + o) = zh;
  }
}

// ------------------------------------------------------------------------------------------------ A6. ragged teacher finalize
// blockIdx.x = bag (infer_finalize_kernel's merge: every block of a bag derives {max, sum} from the bag's partials in the same fixed order).
// blockIdx.y = 0: the pooled row z_teacher, stats.  blockIdx.y > 0: every row's instance score - the attention weight (attn2score = 0) or
// mhimx_pseudo_score's arithmetic, score_n = 1 / sum_c exp(cam_c - max_c cam), cam_c = attn_n cproj[n, c] + bp[0] (scoring.py:37-58, the
// class-0 bias for every class: :54).
__global__ __launch_bounds__(RG_FIN_T) void rw_finalize_kernel(InferTab tab, const float* __restrict__ pm, const float* __restrict__ pl,
                                                            const float* __restrict__ pz, const float* __restrict__ s,
                                                            const float* __restrict__ cproj, const float* __restrict__ bp, int C,
                                                            int attn2score, float* __restrict__ z_out, float* __restrict__ stats,
                                                            float* __restrict__ score) {
  __shared__ float red[8];
  __shared__ float wgt[RG_FIN_T];
  const int bag = blockIdx.x;
  RG_BAG(bag)
  const int G = rg_parts(N);
  const int tid = threadIdx.x;
  pm += p0; pl += p0; pz += (int64_t)p0 * IE;
  float mx, L;
  rg_merge_stats(pm, pl, G, 1, red, mx, L);
  const float invL = 1.f / L;
  if (blockIdx.y > 0) {
    const float* sb = s + orow0;
    float* ob = score + orow0;
    const float b0 = attn2score ? bp[0] : 0.f;
    const int64_t step = (int64_t)(gridDim.y - 1) * RG_FIN_T;
    for (int64_t r = (int64_t)(blockIdx.y - 1) * RG_FIN_T + tid; r < N; r += step) {
      const float an = __expf(sb[r] - mx) * invL;
      if (!attn2score) { ob[r] = an; continue; }
      const f32x4 cp = *reinterpret_cast<const f32x4*>(cproj + (orow0 + r) * 4);
      float cm = -INFINITY;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C) cm = fmaxf(cm, an * cp[c] + b0);
      float den = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C) den += expf((an * cp[c] + b0) - cm);
      ob[r] = 1.f / den;
    }
    return;
  }
  if (tid == 0) { stats[2 * bag] = mx; stats[2 * bag + 1] = L; }
  float acc = 0.f;                                            // column tid of the pooled row
  for (int base = 0; base < G; base += RG_FIN_T) {
    __syncthreads();
    wgt[tid] = base + tid < G ? __expf(pm[base + tid] - mx) : 0.f;
    __syncthreads();
    const int cnt = G - base < RG_FIN_T ? G - base : RG_FIN_T;
#pragma unroll 8
    for (int j = 0; j < cnt; ++j) acc += pz[(int64_t)(base + j) * IE + tid] * wgt[j];
  }
  z_out[(int64_t)bag * IE + tid] = acc * invL;
}

// ------------------------------------------------------------------------------------------------ C1. the kept-row map
// blockIdx.x = bag: keep[row0 + rows_all[j]] = 1 for the bag's kept rows j < len_keep (rw_pad_kernel cleared the map; row ids inside [0, N)
// come from the select, anything else is dropped: no write outside the bag's slot)
__global__ __launch_bounds__(RW_T) void rw_keep_kernel(InferTab tab, RwCnt cn, const int64_t* __restrict__ rows_all, uint8_t* __restrict__ keep) {
  const int bag = blockIdx.x;
  int64_t N = tab.N[0], orow0 = tab.row0[0];
  int len_keep = cn.len_keep[0];
  RG_PICK(N, tab.N, bag) RG_PICK(orow0, tab.row0, bag) RG_PICK(len_keep, cn.len_keep, bag)
  const int64_t* rows = rows_all + orow0;
  for (int j = threadIdx.x + blockIdx.y * RW_T; j < len_keep; j += RW_T * gridDim.y) {
    const int64_t r = rows[j];
    if (r >= 0 && r < N) keep[orow0 + r] = 1;
  }
}

// ------------------------------------------------------------------------------------------------ C2. ragged dPRE rows, in place
// blockIdx.x = 32-row tile of the row space.  Thread t owns the 4 columns 4 (t & 127) .. + 3 of the rows of parity t >> 7: 16-byte loads of
// the gradient rows, 8-byte loads of the fp16 d out / d pre rows, 16-byte stores; rows that are not kept are neither read (their gradient
// rows hold nothing) nor anything but zero afterwards.  part[tile][512]: the tile's column sums (d b1's partials; rows in index order).
__global__ __launch_bounds__(RW_T) void rw_dpre_kernel(const uint8_t* __restrict__ keep, float* __restrict__ dH, const _Float16* __restrict__ dact,
                                                       float* __restrict__ part) {
  __shared__ f32x4 half[IE / 4];
  __shared__ uint8_t kf[RW_ROWS];
  const int tile = blockIdx.x, tid = threadIdx.x;
  const int64_t r0 = (int64_t)tile * RW_ROWS;
  if (tid < RW_ROWS) kf[tid] = keep[r0 + tid];
  __syncthreads();
  const int c4 = tid & 127, par = tid >> 7;
  f32x4 sum = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int i = 0; i < RW_ROWS / 2; ++i) {
    const int r = 2 * i + par;
    f32x4* gp = reinterpret_cast<f32x4*>(dH + (r0 + r) * IE) + c4;
    f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
    if (kf[r]) {                                              // (uniform over the two waves that share the row)
      const f32x4 g = *gp;
      const rw_h4 a = *(reinterpret_cast<const rw_h4*>(dact + (r0 + r) * IE) + c4);
#pragma unroll
      for (int q = 0; q < 4; ++q) d[q] = g[q] * (float)a[q];
    }
    *gp = d;
#pragma unroll
    for (int q = 0; q < 4; ++q) sum[q] += d[q];
  }
  if (par == 1) half[c4] = sum;
  __syncthreads();
  if (par == 0) {
    const f32x4 o = half[c4];
#pragma unroll
    for (int q = 0; q < 4; ++q) sum[q] += o[q];
    *(reinterpret_cast<f32x4*>(part + (int64_t)tile * IE) + c4) = sum;
  }
}

// ------------------------------------------------------------------------------------------------ C5. the queries' EMA chain
// q <- wq q + sum_b w[b] z_b, z_b = bag b's k tokens (rows tok[b] .. of the student's feature rows): merge.py:142-143 applied bag after bag
// on tokens that were all computed from the window's first queries (window_q_chain_kernel's contract, step.hip; bag order)
struct RwChain { int64_t tok[RW_MAX]; float w[RW_MAX]; float wq; int32_t n; };
__global__ __launch_bounds__(RW_T) void rw_q_chain_kernel(float* __restrict__ q, const float* __restrict__ Hs, RwChain ch, int n) {
  const int i = blockIdx.x * RW_T + threadIdx.x;
  if (i >= n) return;
  float acc = 0.f;
#pragma unroll
  for (int b = 0; b < RW_MAX; ++b)
    if (b < ch.n) acc += Hs[ch.tok[b] * IE + i] * ch.w[b];
  q[i] = q[i] * ch.wq + acc;
}

// ------------------------------------------------------------------------------------------------ host
struct RwLay {
  int64_t w1p_t, wa_frag_t, w1p_s, wa_frag_s, wa_t, wa_t_frag, wo_t, q_old, q_scr;
  int64_t logits, losses, z_t, z_s, stats_t;
  int64_t H_t, H_s, dact, dH, rows_all, s_t, score, cproj, keep, db1_part, pm, pl, pz, slab_1;
  int64_t merge_ws, merge_ws_bytes, sel_ws, sel_ws_bytes, sel_perm, sel_ids, sel_rows, sel_lk, s_s, stats_s, pool_ws_s, pool_ws_s_bytes, g_z;
  int64_t total, rows;
  int32_t steps, s1, s1_per;
};

int64_t slot_rows(int64_t N, int64_t k) { return align_up(N + k, RW_ROWS); }

// xdt: the element type of the bags' rows (MHIMX_X_*); the 2-byte types have their own pitch rule (16-byte rows: 8 elements)
int check_rw(const mhimx_step_cfg* c, int32_t n_bags, const mhimx_ragged_window_bag* bags, int32_t xdt = MHIMX_X_F32) {
  if (int r = rg_check_xdt("ragged_window", xdt)) return r;
  MHIMX_CHECK_ARG(c && bags, "ragged_window: null configuration / bag list");
  MHIMX_CHECK_ARG(n_bags >= 1 && n_bags <= RW_MAX, "ragged_window: 1..%d bags per window (got %d)", RW_MAX, n_bags);
  MHIMX_CHECK_ARG(!c->q_out && !c->side_stream && !c->time_project, "ragged_window: q_out / side_stream / time_project are single-step options");
  MHIMX_CHECK_ARG(c->D > 0 && c->D <= (1 << 20), "ragged_window: D outside 1..2^20");
  int64_t rows = 0;
  for (int b = 0; b < n_bags; ++b) {
    const mhimx_ragged_window_bag& q = bags[b];
    if (step_check_cfg(c, q.N, &q.cnt)) {
      const std::string why = last_error();
      return fail(-1, "ragged_window: bag %d (N = %lld): %s", b, (long long)q.N, why.c_str());
    }
    if (int r = rg_check_bag("ragged_window", b, q.N, q.ldx, c->D, xdt, RgRules{0, true})) return r;      // (N: step_check_cfg has checked it)
    rows += slot_rows(q.N, c->k);
    MHIMX_CHECK_ARG(rows <= MHIMX_RAGGED_WINDOW_MAX_ROWS, "ragged_window: bag %d: %lld rows in the window's row space up to this bag, at most %d", b,
                    (long long)rows, MHIMX_RAGGED_WINDOW_MAX_ROWS);
  }
  const mhimx_step_params &s = c->student, &t = c->teacher;
  MHIMX_CHECK_ARG(aligned16(s.w1) && aligned16(s.b1) && aligned16(s.wa) && aligned16(t.w1) && aligned16(t.b1) && aligned16(t.wa) &&
                      (!c->attn2score || aligned16(t.wp)),
                  "ragged_window: feature / scorer / teacher predictor weights must be 16-byte aligned");
  MHIMX_CHECK_ARG(c->act >= MHIMX_ACT_NONE && c->act <= MHIMX_ACT_TANH && c->da_act >= MHIMX_ACT_NONE && c->da_act <= MHIMX_ACT_TANH,
                  "ragged_window: unknown activation");
  MHIMX_CHECK_ARG(c->drop_p_student >= 0.f && c->drop_p_student < 1.f && c->drop_p_teacher >= 0.f && c->drop_p_teacher < 1.f,
                  "ragged_window: dropout probability outside [0,1)");
  return 0;
}

void rw_layout(const mhimx_step_cfg* c, int32_t n_bags, const mhimx_ragged_window_bag* bags, RwLay* w, InferTab* tab, RwCnt* cn, int64_t* row0_out) {
  const int64_t E = c->E, D = c->D, A = c->A, k = c->k, n = n_bags, I = 512;
  RgCount cnt;
  int64_t merge_b = 0, sel_b = 0, pool_b = 0, perm_n = 0, ids_n = 0, rows_n = 0, M_max = 0;
  for (int b = 0; b < n_bags; ++b) {
    const mhimx_ragged_window_bag& q = bags[b];
    if (cn) { cn->len_keep[b] = (int32_t)q.cnt.len_keep; cn->slot[b] = (int32_t)slot_rows(q.N, k); }
    if (row0_out) row0_out[b] = cnt.rows;
    rg_tab_add(tab, cnt, b, q.X, q.ldx, q.N, slot_rows(q.N, k));
    const int64_t M = q.cnt.Lk + k;
    auto up = [](int64_t& a, int64_t v) { if (v > a) a = v; };
    up(merge_b, mhimx_merge_ws_bytes(q.cnt.R, E, k, 8, 64));
    up(sel_b, mhimx_select_ws_bytes(q.N));
    up(pool_b, mhimx_abmil_pool_ws_bytes(M, E, A, 0));
    up(M_max, M);
    if (q.N > 16384) { up(perm_n, q.cnt.k_top); up(ids_n, q.N); up(rows_n, q.cnt.len_keep); }
  }
  rg_tab_close(tab, cnt, n_bags);
  const int64_t rows = cnt.rows, parts = cnt.parts;
  w->rows = rows;
  w->steps = (int32_t)(rows / RW_ROWS);
  const int s1_room = pw_split_k(w->steps, 8, 8, &w->s1, &w->s1_per);
  Arena ar(nullptr, 0);
  w->w1p_t = ar.off; ar.take<float>(E * D);
  w->wa_frag_t = ar.off; ar.take<float>(A * E);
  w->w1p_s = ar.off; ar.take<float>(E * D);
  w->wa_frag_s = ar.off; ar.take<float>(A * E);
  w->wa_t = ar.off; ar.take<float>(E * A);
  w->wa_t_frag = ar.off; ar.take<float>(E * A);
  w->wo_t = ar.off; ar.take<float>(I * E);
  w->q_old = ar.off; ar.take<float>(k * E);
  w->q_scr = ar.off; ar.take<float>(k * E);
  w->logits = ar.off; ar.take<float>(n * 16);
  w->losses = ar.off; ar.take<float>(n * 4);
  w->z_t = ar.off; ar.take<float>(n * E);
  w->z_s = ar.off; ar.take<float>(n * E);
  w->stats_t = ar.off; ar.take<float>(n * 2);
  w->H_t = ar.off; ar.take<float>(rows * E);
  w->H_s = ar.off; ar.take<float>(rows * E);
  w->dact = ar.off; ar.take<_Float16>(rows * E);
  w->dH = ar.off; ar.take<float>(rows * E);
  w->rows_all = ar.off; ar.take<int64_t>(rows);
  w->s_t = ar.off; ar.take<float>(rows);
  w->score = ar.off; ar.take<float>(rows);
  w->cproj = ar.off; ar.take<float>(rows * 4);
  w->keep = ar.off; ar.take<uint8_t>(rows);
  w->db1_part = ar.off; ar.take<float>((int64_t)w->steps * E);
  w->pm = ar.off; ar.take<float>(parts);
  w->pl = ar.off; ar.take<float>(parts);
  w->pz = ar.off; ar.take<float>(parts * E);
  w->slab_1 = ar.off; ar.take<float>((int64_t)s1_room * E * D);
  // the per-bag scratch, once, sized for the largest bag
  w->merge_ws_bytes = merge_b; w->merge_ws = ar.off; ar.take<char>(merge_b);
  w->sel_ws_bytes = sel_b; w->sel_ws = ar.off; ar.take<char>(sel_b);
  w->sel_perm = ar.off; ar.take<int64_t>(perm_n);
  w->sel_ids = ar.off; ar.take<int64_t>(ids_n);
  w->sel_rows = ar.off; ar.take<int64_t>(rows_n);
  w->sel_lk = ar.off; ar.take<int64_t>(1);
  w->s_s = ar.off; ar.take<float>(M_max);
  w->stats_s = ar.off; ar.take<float>(2);
  w->pool_ws_s_bytes = pool_b; w->pool_ws_s = ar.off; ar.take<char>(pool_b);
  w->g_z = ar.off; ar.take<float>(E);
  w->total = ar.off;
}

}  // namespace

// launch C.5 for mhimx_dsmil_mhim_window_run (dsmil_mhim.hip): the same kernel on that call's token rows
int rw_q_chain(hipStream_t st, float* q, const float* Hs, int n_bags, const int64_t* tok, double mm, int n_floats) {
  RwChain ch = {};
  ch.n = n_bags;
  q_chain_weights(mm, n_bags, &ch.wq, ch.w);
  for (int b = 0; b < n_bags; ++b) ch.tok[b] = tok[b];
  hipLaunchKernelGGL(rw_q_chain_kernel, dim3((unsigned)cdiv(n_floats, RW_T)), dim3(RW_T), 0, st, q, Hs, ch, n_floats);
  MHIMX_LAUNCH_CHECK();
  return 0;
}

}  // namespace mhimx

using namespace mhimx;

extern "C" int mhimx_ragged_window_layout_of(const mhimx_step_cfg* cfg, int32_t n_bags, const mhimx_ragged_window_bag* bags,
                                             mhimx_ragged_window_layout* out) {
  MHIMX_CHECK_ARG(out, "ragged_window_layout: null output");
  if (int r = check_rw(cfg, n_bags, bags)) return r;
  RwLay w;
  memset(out, 0, sizeof(*out));
  rw_layout(cfg, n_bags, bags, &w, nullptr, nullptr, out->row0);
  out->total = w.total; out->rows = w.rows; out->logits = w.logits; out->losses = w.losses; out->score = w.score; out->rows_all = w.rows_all;
  out->H_teacher = w.H_t; out->H_student = w.H_s; out->dact = w.dact; out->dpre = w.dH; out->z_teacher = w.z_t; out->z_student = w.z_s;
  return 0;
}

extern "C" int mhimx_ragged_window_run(void* stream, const mhimx_step_cfg* cfg, int32_t n_bags, const mhimx_ragged_window_bag* bags,
                                       int64_t host_step, void* ws, int64_t ws_bytes, int32_t update) {
  return mhimx_ragged_window_run_x(stream, cfg, n_bags, bags, host_step, ws, ws_bytes, update, MHIMX_X_F32);
}

extern "C" int mhimx_ragged_window_run_x(void* stream, const mhimx_step_cfg* cfg, int32_t n_bags, const mhimx_ragged_window_bag* bags,
                                         int64_t host_step, void* ws, int64_t ws_bytes, int32_t update, int32_t x_dtype) {
  return mhimx::ragged_window_run(stream, cfg, n_bags, bags, host_step, ws, ws_bytes, update, x_dtype, nullptr);
}

extern "C" int mhimx_ragged_window_run_surv(void* stream, const mhimx_step_cfg* cfg, int32_t n_bags, const mhimx_ragged_window_bag* bags,
                                            int64_t host_step, void* ws, int64_t ws_bytes, int32_t update, int32_t x_dtype,
                                            const mhimx_surv_spec* surv) {
  MHIMX_CHECK_ARG(surv, "ragged_window: null survival description (mhimx_ragged_window_run_x is the classification call)");
  return mhimx::ragged_window_run(stream, cfg, n_bags, bags, host_step, ws, ws_bytes, update, x_dtype, surv);
}

// the one body of mhimx_ragged_window_run(_x) (surv NULL: cross entropy) and mhimx_ragged_window_run_surv
int mhimx::ragged_window_run(void* stream, const mhimx_step_cfg* cfg, int32_t n_bags, const mhimx_ragged_window_bag* bags, int64_t host_step,
                             void* ws, int64_t ws_bytes, int32_t update, int32_t x_dtype, const mhimx_surv_spec* surv) {
  if (int r = check_rw(cfg, n_bags, bags, x_dtype)) return r;
  if (surv)
    if (int r = surv_spec_check("ragged_window", n_bags, surv)) return r;
  for (int b = 0; b < n_bags; ++b) {
    MHIMX_CHECK_ARG(bags[b].X && aligned16(bags[b].X), "ragged_window: bag %d: null or unaligned rows", b);
    MHIMX_CHECK_ARG(bags[b].label_dev, "ragged_window: bag %d: null label", b);
  }
  MHIMX_CHECK_ARG(!update || (cfg->p && cfg->g && cfg->m && cfg->v && cfg->n_train > 0 && cfg->n_all >= cfg->n_train),
                  "ragged_window: update needs the flat optimiser buffers");
  RwLay w;
  InferTab tab = {};
  RwCnt cn = {};
  rw_layout(cfg, n_bags, bags, &w, &tab, &cn, nullptr);
  tab.pad = x_dtype;                           // read by the launches that read X: both projections and d W1
  if (int r = rg_check_ws("ragged_window", ws, ws_bytes, w.total)) return r;
  const mhimx_step_cfg& c = *cfg;
  const mhimx_step_params &S = c.student, &T = c.teacher;
  const int64_t D = c.D, E = c.E, C = c.C, k = c.k;
  hipStream_t st = (hipStream_t)stream;
  char* base = static_cast<char*>(ws);
  auto F = [&](int64_t off) { return reinterpret_cast<float*>(base + off); };
  const MidImages im = {F(w.w1p_t), F(w.wa_frag_t), F(w.w1p_s), F(w.wa_frag_s), F(w.wa_t), F(w.wa_t_frag), F(w.wo_t), F(w.q_old)};
  float *H_t = F(w.H_t), *H_s = F(w.H_s), *dHall = F(w.dH), *s_t = F(w.s_t), *score_all = F(w.score), *cproj = F(w.cproj);
  _Float16* dact = reinterpret_cast<_Float16*>(base + w.dact);
  int64_t* rows_space = reinterpret_cast<int64_t*>(base + w.rows_all);
  uint8_t* keep = reinterpret_cast<uint8_t*>(base + w.keep);
  void* merge_ws = base + w.merge_ws;
  const uint64_t* tick = c.tick;

  // ================================================================================================ A. the teacher half, window-wide
  const mhimx_merge mw_prep = mid_merge_params(c);            // (read while enqueueing, by every bag's kind-6 job: alive until the last bag's)
  {
    mhimx_prep_job jobs[10];
    int n = mid_prep_head(c, im, jobs);
    n += mid_prep_student(c, im, jobs + n);
    if (int r = mhimx_prep_batch(stream, jobs, n)) return r;
  }
  // both models' feature rows into the row space (mhim.py:186 and :335-336): the teacher first - its d out / d pre rows are overwritten by
  // the student's
  {
    PureWinDrop dr = {};
    dr.tick = tick; dr.dact = dact;
    for (int b = 0; b < n_bags; ++b) dr.seed[b] = bags[b].seeds.drop_teacher;
    dr.drop_p = c.drop_p_teacher;
    if (int r = pure_window_project(st, tab, dr, (int)D, im.w1p_t, T.b1, c.act, H_t)) return r;
    for (int b = 0; b < n_bags; ++b) dr.seed[b] = bags[b].seeds.drop_student;
    dr.drop_p = c.drop_p_student;
    if (int r = pure_window_project(st, tab, dr, (int)D, im.w1p_s, S.b1, c.act, H_s)) return r;
  }
  hipLaunchKernelGGL(rw_pad_kernel, dim3((unsigned)n_bags, 4), dim3(RW_T), 0, st, tab, cn, H_t, H_s, dact, keep);
  MHIMX_LAUNCH_CHECK();
  // the teacher's scores, pool partials and (attn2score) class projections; then plane = bag: stats, z_teacher, every row's instance score
  if (c.attn2score) {
    if (int r = infer_score_cproj(st, tab, H_t, im.wa_frag_t, T.wc, c.da_act, s_t, F(w.pm), F(w.pl), F(w.pz), T.wp, (int)C, cproj)) return r;
  } else if (int r = infer_score(st, tab, H_t, im.wa_frag_t, T.wc, c.da_act, s_t, F(w.pm), F(w.pl), F(w.pz)))
    return r;
  hipLaunchKernelGGL(rw_finalize_kernel, dim3((unsigned)n_bags, 1 + FIN_SCORE_BLOCKS), dim3(RG_FIN_T), 0, st, tab, F(w.pm), F(w.pl), F(w.pz), s_t, cproj, T.bp,
                     (int)C, (int)c.attn2score, F(w.z_t), F(w.stats_t), score_all);
  MHIMX_LAUNCH_CHECK();
  // ---- HAM mask + Merge split of every bag: rows_all = [rows to merge (R) | rows that stay (Lk) | N .. N + k - 1].  The select reads the
  // bag's scores, its seed and *tick only (the tick moves once, in A.1): every bag's row list exists before the first bag's middle starts
  {
    mhimx_select_bag sb[RW_MAX];
    for (int b = 0; b < n_bags; ++b) {
      const mhimx_step_counts& cnt = bags[b].cnt;
      sb[b] = mhimx_select_bag{tab.row0[b], bags[b].N, cnt.k_top, cnt.n_sel, cnt.R, tab.row0[b], bags[b].seeds.select};
    }
    SelLargeWs lw;
    lw.perm = reinterpret_cast<int64_t*>(base + w.sel_perm); lw.ids = reinterpret_cast<int64_t*>(base + w.sel_ids);
    lw.rows = reinterpret_cast<int64_t*>(base + w.sel_rows); lw.lk = reinterpret_cast<int64_t*>(base + w.sel_lk);
    lw.sel_ws = base + w.sel_ws; lw.sel_ws_bytes = w.sel_ws_bytes;
    if (int r = select_bags_check("ragged_window", n_bags, sb)) return r;
    if (int r = select_rows_many_launch(st, score_all, n_bags, sb, tick, rows_space, lw, 1)) return r;
  }

  // ================================================================================================ B. the middle, bag after bag
  const float inv_n = 1.f / (float)n_bags;
  for (int b = 0; b < n_bags; ++b) {
    const mhimx_ragged_window_bag& g = bags[b];
    const int64_t N = g.N, R = g.cnt.R, row0 = tab.row0[b];
    int64_t* rows_all = rows_space + row0;
    const int acc = b > 0 ? 1 : 0;
    {
      mhimx_prep_job jobs[2];
      jobs[0] = mhimx_prep_job{10, nullptr, reinterpret_cast<float*>(rows_all + g.cnt.len_keep), N, k};
      jobs[1] = mhimx_prep_job{6, reinterpret_cast<const float*>(&mw_prep), static_cast<float*>(merge_ws), R, w.merge_ws_bytes};
      if (int r = mhimx_prep_batch(stream, jobs, 2)) return r;
    }
    // ---- the student's forward (the queries' EMA goes to scratch), the head with this bag's loss / n_bags (base_engine.py:102), the
    // backward down to the gradient rows of the bag's slot (no fused dPRE image: part C makes it for the whole row space)
    const MidBag mb = {H_s + row0 * E, dHall + row0 * E, rows_all, N, R, g.cnt.Lk, g.seeds.mca, F(w.q_scr), F(w.s_s), F(w.stats_s), F(w.z_s) + (int64_t)b * E,
                       F(w.g_z), base + w.pool_ws_s, w.pool_ws_s_bytes, merge_ws, w.merge_ws_bytes};
    MidFwd fwd;
    if (int r = mid_student_fwd(stream, c, im, mw_prep, mb, nullptr, &fwd)) return r;
    const MidSurv sv = {surv ? surv->censor_dev[b] : nullptr, surv ? surv->alpha : 0.f, surv ? surv->eps : 0.f, surv && surv->risk ? surv->risk + b : nullptr};
    if (int r = mid_head(stream, c, mb, F(w.z_t) + (int64_t)b * E, g.label_dev, inv_n, F(w.logits) + 16 * b, F(w.losses) + 4 * b, c.grad, acc,
                         surv ? &sv : nullptr))
      return r;
    mhimx_reduce_list lst;
    memset(&lst, 0, sizeof(lst));
    if (int r = mid_bwd_rows(stream, im, fwd, mb, c.grad, acc, nullptr, nullptr, &lst)) return r;
    if (int r = mhimx_reduce_flush(stream, &lst)) return r;      // (the per-bag workspaces are the next bag's: nothing stays queued)
  }

  // ================================================================================================ C. the backward tail, window-wide
  hipLaunchKernelGGL(rw_keep_kernel, dim3((unsigned)n_bags, 8), dim3(RW_T), 0, st, tab, cn, rows_space, keep);
  MHIMX_LAUNCH_CHECK();
  hipLaunchKernelGGL(rw_dpre_kernel, dim3((unsigned)w.steps), dim3(RW_T), 0, st, keep, dHall, dact, F(w.db1_part));
  MHIMX_LAUNCH_CHECK();
  if (int r = pw_wgrad_bagx(st, tab, dHall, (int)D, w.steps, w.s1, w.s1_per, F(w.slab_1))) return r;
  {
    const float* parts[2] = {F(w.slab_1), F(w.db1_part)};
    const int32_t G[2] = {w.s1, w.steps};
    const int64_t W[2] = {E * D, E};
    float* out[2] = {c.grad.w1, c.grad.b1};
    if (int r = pw_reduce(st, 2, parts, G, W, out)) return r;
  }
  {
    int64_t tok[RW_MAX];
    for (int b = 0; b < n_bags; ++b) tok[b] = tab.row0[b] + bags[b].N;
    if (int r = rw_q_chain(st, S.q, H_s, n_bags, tok, (double)c.merge_mm, (int)(k * E))) return r;
  }
  if (!update) return 0;
  const mhimx_optim_args o = optim_args_of(c, host_step, true);
  return mhimx_optim_step(stream, &o);
}
