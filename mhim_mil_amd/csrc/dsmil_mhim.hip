// dsmil_mhim.hip — mhimx_dsmil_mhim_window_run: ONE optimiser update of the full MHIM(DSMIL) model (EMA teacher, hard-instance select,
// Merge, DSMIL student, per-class distillation) over up to MHIMX_DSMIL_MHIM_WINDOW_MAX bags of DIFFERENT row counts behind one C call
// (include/mhimx.h); n_bags = 1 is the single-bag step.
// replaces: engines/base_engine.py:29-51,76-167 (the accumulation window, its one optimizer.step() and the per-parameter EMA) around
//           engines/common_mil.py:14-48 (forward_func), modules/mhim.py:181-227 (forward_teacher), :109-179 (get_mask), :318-378 (forward,
//           baseline 'dsmil'), mhim_modules/merge.py:127-203 and mhim_modules/baseline.py:112-194 (BClassifier / DSMIL) with their
//           autograd - and, on this side of the boundary, FusedTrainer's per-op autograd route (_dsmil_forward_backward over dsmil.py).
//
// Two row spaces.  The BAG space holds every bag's N rows from a multiple of 32 on (mhimx_dsmil_window_run's).  The TOKEN space is
// compact: bag b owns 32 * ceil((Lk_b + k) / 32) rows - its Lk rows that stay, the k Merge tokens, zero rows - and a second by-value table
// over it (N_b = Lk_b + k) lets the DSMIL kernels of infer_dsmil.hip / dsmil_window.hip run on the student as they are.  The rows to
// merge of bag b lie contiguously in a third buffer, where the per-bag Merge entry points read them.
//
//   A. forward, window-wide (10 launches; more for every bag above 16 384 rows: select_large_rows' sequence)
//      1  mhimx_prep_batch             counters; both W1 paired-plane images; the teacher's Wv / Wq0 / Wq2 images; the student's Wv, Wv^T,
//                                      Wq0, Wq2, Wq2^T, Wq0^T images; Wo^T of the Merge; the parameter-only part of the first 8 bags'
//                                      Merge (job kind 6: every bag owns its Merge workspace); q -> q_out when given
//      2  pure_window_project_kernel   (bag_project.hip) the teacher's feature rows: drop_p_teacher, per-bag seed
//      3  pure_window_project_kernel   the student's feature rows + fp16 d out / d pre (the teacher launch's d out / d pre rows are overwritten)
//      4  infer_project_kernel         the teacher's h -> V
//      5-7  dsmil_rows / crit / pool   (infer_dsmil.hip) the teacher's Q, classes (cls_attn: the instance score max_c classes), critical
//                                      rows, pool partials
//      8  dsmil_finalize_kernel        plane = bag: B_teacher [C, E]; the instance score max_c A otherwise
//      9  select_many_kernel<KPT>      (select_many.hip) every bag's row list [stay (Lk) | merge (R)]; a bag above 16 384 rows: select_large_rows
//     10  dm_gather_kernel             NEW: stay rows of the student's feature rows -> the token space, rows to merge -> the merge buffer,
//                                      the token slots' zero rows, every kept row's position in its list
//   B. Merge forward, bag after bag (4 launches per bag: rows pass, partial merge, O, to_out; + 1 mhimx_prep_batch per 8 bags past the
//      first 8): the k tokens land in the bag's token slot.  Every bag attends with the call's first queries.
//   C. the student, token-space-wide (12 launches, through dsmil_student.hpp's ds_forward, ds_head and ds_backward)
//      1  infer_project_kernel         tokens -> V
//      2-4  dsmil_rows / crit / pool   Q, classes, critical rows, pool partials
//      5  ds_head_kernel<DsDist>       (dsmil_student.hpp) the teacher-free head + the distillation: B, fcc, the mix, CE, cl = mean_c SoftTargetCE(B[c],
//                                      B_teacher[c], temp_t); d B = Wfcc^T g_lb + aux_alpha / (n C) (softmax(B[c]) - softmax(B_t[c] / temp_t))
//      6  dw_rows1_kernel              (dsmil_window.hip) d a, d PreV over V in place, the tiles' d bv and d q_max partials
//      7  infer_project_kernel         d PreV Wv
//      8  dw_dqmax_kernel              per bag: d q_max
//      9  dw_rows2_kernel<true>        NEW instantiation: plain d tokens over launch 7's rows in place (the token rows' d out / d pre
//                                      lives in the bag space, the k tokens have none), no d b1 partials
//     10-12  pw_tn_kernel              d Wv = dPreV^T tokens, d Wq2 = dPreQ^T U1, d Wq0 = dPre1^T tokens (pure_window.hip)
//   D. Merge backward, bag after bag (5 launches per bag: parameters x dz, rows, the parameter-gradient tail's two stages, its last stage
//      with the queued reductions in mhimx_reduce_flush): d X of the R merged rows from the k tokens' gradient rows; bag 0 overwrites the
//      six Merge gradients, every later bag adds.
//   E. the tail, window-wide (6 launches; 5 with update = 0)
//      1  dm_scatter_kernel            NEW: one workgroup per 32-row tile of the bag space: dPRE[row] = d tokens[j] * d out / d pre[row] for a
//                                      stay row, d X[j - Lk] * d out / d pre[row] for a merged row (j: the row's position in its bag's list);
//                                      masked and padding rows are zero rows; the tile's d b1 column sums
//      2  pw_tn_kernel<true, XT>       d W1 = sum_b dPRE_b^T X_b with X read where it lies (masked rows ride as zero rows)
//      3-4  pw_reduce_kernel           the twelve partial buffers in index order into the gradient views
//      5  rw_q_chain_kernel            (ragged_window.hip) q <- mm^n q + (1 - mm) sum_b mm^(n-1-b) z_b on the bags' tokens
//      6  mhimx_optim_step             Adam + EMA teacher (update = 1)
// Launch count: 28 window-wide (10 + 12 + 6) + 9 per bag (+ 1 per 8 bags past the first 8; + select_large_rows' launches per bag above
// 16 384 rows: 12 counted by the profiler).  One bag: 37; 8 whole-slide bags, three of them above 16 384 rows: 136.  No floating-point
// atomics, no workgroup waits for another, every sum has a fixed order.
#include <math.h>
#include <string.h>

#include "dsmil_student.hpp"

namespace mhimx {

bool merge2_ok(const mhimx_merge* m, int64_t R);                  // mca2.hip: the projection-free Merge and its workspace
int64_t merge2_ws_bytes(int64_t R, int64_t k);

namespace {

constexpr int DM_Q = DS_Q, DM_MAXC = DS_MAXC, DM_ROWS = RG_ROWS, DM_T = 256;
constexpr int DM_MAX = MHIMX_DSMIL_MHIM_WINDOW_MAX;
constexpr int DM_GATHER_Y = 64;                                  // gather workgroups per bag
static_assert(DM_MAX == MHIMX_INFER_MAX, "the by-value bag table is the inference call's");

typedef _Float16 dm_h4 __attribute__((ext_vector_type(4)));

// per-bag numbers the new kernels need beyond the tables (constant indices only: RG_PICK's rule)
struct DmCnt {
  int64_t tok0[DM_MAX], mrg0[DM_MAX];                            // first row of the bag in the token space / in the merge buffer
  int32_t len_keep[DM_MAX], Lk[DM_MAX], tslot[DM_MAX];           // tslot: rows of the bag's token slot
};

// ------------------------------------------------------------------------------------------------ A10. gather
// blockIdx.x = bag, blockIdx.y = a share of the bag's list.  One wave per list entry j: row rows[j] of the student's feature rows goes to
// token row j (j < Lk) or to row j - Lk of the bag's merge block; pos[row] = j.  A row id outside [0, N) (the select writes none) gives a
// zero row and no pos entry: nothing is read or written outside the bag's slots.  blockIdx.y == 0 also clears the token slot's rows
// behind the k Merge tokens.
__global__ __launch_bounds__(DM_T) void dm_gather_kernel(InferTab tab, DmCnt cn, const float* __restrict__ Hs, const int64_t* __restrict__ rows_all,
                                                         int k, float* __restrict__ T, float* __restrict__ Xm, int32_t* __restrict__ pos) {
  const int bag = blockIdx.x;
  int64_t N = tab.N[0], orow0 = tab.row0[0], tok0 = cn.tok0[0], mrg0 = cn.mrg0[0];
  int len_keep = cn.len_keep[0], Lk = cn.Lk[0], tslot = cn.tslot[0];
  RG_PICK(N, tab.N, bag) RG_PICK(orow0, tab.row0, bag) RG_PICK(tok0, cn.tok0, bag) RG_PICK(mrg0, cn.mrg0, bag)
  RG_PICK(len_keep, cn.len_keep, bag) RG_PICK(Lk, cn.Lk, bag) RG_PICK(tslot, cn.tslot, bag)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t* rows = rows_all + orow0;
  const f32x4 z4 = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int j = blockIdx.y * (DM_T / 64) + wave; j < len_keep; j += (DM_T / 64) * gridDim.y) {
    const int64_t r = rows[j];
    const bool ok = r >= 0 && r < N;
    const f32x4* src = reinterpret_cast<const f32x4*>(Hs + (orow0 + (ok ? r : 0)) * IE);
    f32x4* dst = reinterpret_cast<f32x4*>(j < Lk ? T + (tok0 + j) * IE : Xm + (mrg0 + (j - Lk)) * IE);
    f32x4 v0 = src[lane], v1 = src[lane + 64];
    if (!ok) { v0 = z4; v1 = z4; }
    dst[lane] = v0;
    dst[lane + 64] = v1;
    if (ok && lane == 0) pos[orow0 + r] = j;
  }
  if (blockIdx.y == 0) {
    const int first = Lk + k;
    f32x4* dst = reinterpret_cast<f32x4*>(T + (tok0 + first) * IE);
    for (int f = tid; f < (tslot - first) * (IE / 4); f += DM_T) dst[f] = z4;
  }
}

// ------------------------------------------------------------------------------------------------ E1. scatter: dPRE rows of the bag space
// blockIdx.x = 32-row tile of the bag space (inside ONE bag).  Row r of the bag is kept iff its list position p = pos[r] is inside
// [0, len_keep) and rows[p] == r: pos entries of masked rows hold whatever the workspace held, and a position that names another row is
// not this row's (the ids of a list are distinct), so the map needs no clearing.  Kept: dPRE = (p < Lk ? d tokens[p] : d X[p - Lk]) *
// d out / d pre; else a zero row.  Thread t owns the 4 columns 4 (t & 127) .. + 3 of the rows of parity t >> 7 (rw_dpre_kernel's
// shape); part[tile][512]: the tile's column sums, rows in index order.
__global__ __launch_bounds__(DM_T) void dm_scatter_kernel(InferTab tab, DmCnt cn, const int64_t* __restrict__ rows_all, const int32_t* __restrict__ pos,
                                                          const float* __restrict__ dT, const float* __restrict__ dXm,
                                                          const _Float16* __restrict__ dact, float* __restrict__ dpre, float* __restrict__ part) {
  __shared__ f32x4 half[IE / 4];
  __shared__ int64_t srow[DM_ROWS];                             // >= 0: row of dT; <= -2: row -2 - s of dXm; -1: a zero row
  const int tile = blockIdx.x, tid = threadIdx.x;
  const int64_t r0 = (int64_t)tile * DM_ROWS;
  RG_FIND_BAG(r0, row0)
  int64_t N = tab.N[0], orow0 = tab.row0[0], tok0 = cn.tok0[0], mrg0 = cn.mrg0[0];
  int len_keep = cn.len_keep[0], Lk = cn.Lk[0];
  RG_PICK(N, tab.N, bag) RG_PICK(orow0, tab.row0, bag) RG_PICK(tok0, cn.tok0, bag) RG_PICK(mrg0, cn.mrg0, bag)
  RG_PICK(len_keep, cn.len_keep, bag) RG_PICK(Lk, cn.Lk, bag)
  if (tid < DM_ROWS) {
    const int64_t rin = r0 - orow0 + tid;
    int64_t s = -1;
    if (rin < N) {
      const int p = pos[r0 + tid];
      if (p >= 0 && p < len_keep && rows_all[orow0 + p] == rin) s = p < Lk ? tok0 + p : -2 - (mrg0 + (p - Lk));
    }
    srow[tid] = s;
  }
  __syncthreads();
  const int c4 = tid & 127, par = tid >> 7;
  f32x4 sum = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int i = 0; i < DM_ROWS / 2; ++i) {
    const int r = 2 * i + par;
    const int64_t s = srow[r];                                  // (uniform over the two waves that share the row)
    f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
    if (s != -1) {
      const float* src = s >= 0 ? dT + s * IE : dXm + (-2 - s) * IE;
      const f32x4 g = reinterpret_cast<const f32x4*>(src)[c4];
      const dm_h4 a = *(reinterpret_cast<const dm_h4*>(dact + (r0 + r) * IE) + c4);
#pragma unroll
      for (int q = 0; q < 4; ++q) d[q] = g[q] * (float)a[q];
    }
    *(reinterpret_cast<f32x4*>(dpre + (r0 + r) * IE) + c4) = d;
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

// ------------------------------------------------------------------------------------------------ host
struct DmLay {
  DsLay s;                                    // the student's share, over the token space (dsmil_student.hpp)
  // weight images
  int64_t w1p_t, w1p_s, vp_t, q0f_t, q2f_t, wo_t;
  // the teacher's per-bag heads
  int64_t B_t, lb_t, lg_t, li_t, crit_t, qmax_t;
  // bag space
  int64_t H_t, H_s, dact, V_t, Q_t, cls_t, score, rows_all, pos, db1_part, pmax_t, parg_t, pm_t, pl_t, pB_t, slab_1;
  // the tokens
  int64_t T;
  // the rows to merge and the per-bag Merge workspaces; the select's scratch
  int64_t Xm, dXm, merge_ws[DM_MAX], merge_ws_bytes[DM_MAX], sel_ws, sel_ws_bytes, sel_perm, sel_ids, sel_rows, sel_lk;
  int64_t total, rows, trows, mrows;
  int32_t steps, s1, s1_per;
};

mhimx_merge dm_merge_params(const mhimx_dsmil_mhim_cfg& c) {
  mhimx_merge m = {};
  m.E = c.base.E; m.k = c.k; m.heads = 8; m.dim_head = 64;
  m.q_param = c.q; m.ln_w = c.merge.ln_w; m.ln_b = c.merge.ln_b; m.wkv = c.merge.wkv; m.wq = c.merge.wq; m.wo = c.merge.wo; m.bo = c.merge.bo;
  m.mm = c.merge_mm; m.prec = MHIMX_PREC_BF16X3; m.drop_tick = c.base.tick; m.rep = 1.f; m.drop_p = c.merge_drop_p;
  return m;
}

int check_dm(const mhimx_dsmil_mhim_cfg* cfg, int32_t n_bags, const mhimx_ragged_window_bag* bags, int32_t xdt = MHIMX_X_F32) {
  const char* who = "dsmil_mhim_window";
  const mhimx_dsmil_train_cfg* c = cfg ? &cfg->base : nullptr;
  if (int r = ds_check_base(who, c, xdt, n_bags, DM_MAX, bags, "student ")) return r;
  MHIMX_CHECK_ARG(cfg->k >= 1 && 8 * cfg->k <= 48, "dsmil_mhim_window: merge_k outside 1..6 (8 k <= 48)");
  MHIMX_CHECK_ARG(cfg->drop_p_teacher >= 0.f && cfg->drop_p_teacher < 1.f && cfg->merge_drop_p >= 0.f && cfg->merge_drop_p < 1.f,
                  "dsmil_mhim_window: dropout probability outside [0,1)");
  MHIMX_CHECK_ARG(cfg->temp_t > 0.f, "dsmil_mhim_window: the distillation temperature must be positive");
  MHIMX_CHECK_ARG(ds_params_ok(cfg->teacher), "dsmil_mhim_window: null teacher parameter");
  MHIMX_CHECK_ARG(ds_params_aligned(cfg->teacher),
                  "dsmil_mhim_window: the feature, i_classifier, q and v weights of the teacher model must be 16-byte aligned");
  const mhimx_dsmil_merge_params& m = cfg->merge;
  MHIMX_CHECK_ARG(m.ln_w && m.ln_b && m.wkv && m.wq && m.wo && m.bo && cfg->q, "dsmil_mhim_window: null Merge parameter / global queries");
  MHIMX_CHECK_ARG(aligned16(m.ln_w) && aligned16(m.ln_b) && aligned16(m.wkv) && aligned16(m.wq) && aligned16(m.wo) && aligned16(cfg->q) &&
                      (!cfg->q_out || aligned16(cfg->q_out)),
                  "dsmil_mhim_window: the Merge weights and the global queries must be 16-byte aligned");
  const mhimx_dsmil_merge_grads& mg = cfg->merge_grad;
  MHIMX_CHECK_ARG(mg.ln_w && mg.ln_b && mg.wkv && mg.wq && mg.wo && mg.bo, "dsmil_mhim_window: null Merge gradient view");
  const mhimx_merge mw = dm_merge_params(*cfg);
  int64_t rows = 0;
  for (int b = 0; b < n_bags; ++b) {
    const mhimx_ragged_window_bag& q = bags[b];
    const mhimx_step_counts& n = q.cnt;
    if (int r = rg_check_bag(who, b, q.N, q.ldx, c->D, xdt, RgRules{MHIMX_STEP_MAX_ROWS, true})) return r;
    MHIMX_CHECK_ARG(q.N >= 64 && n.k_top >= 1 && n.k_top <= (q.N <= 16384 ? 4096 : 16384) && n.n_sel >= 1 && n.n_sel <= n.k_top &&
                        n.len_keep == q.N - n.n_sel && n.Lk >= 1 && n.R >= 1 && n.R <= 32768 && n.Lk + n.R == n.len_keep,
                    "dsmil_mhim_window: bag %d (N = %lld): row counts outside the device-drawn select (64 <= N <= %d, k_top <= 4096 up to 16384 rows / "
                    "16384 above, 1 <= n_sel <= k_top, len_keep = N - n_sel, rows that stay >= 1, 1 <= rows to merge <= 32768, Lk + R = len_keep)",
                    b, (long long)q.N, MHIMX_STEP_MAX_ROWS);
    MHIMX_CHECK_ARG(merge2_ok(&mw, n.R), "dsmil_mhim_window: bag %d: the Merge entry points' projection-free form does not take R = %lld", b,
                    (long long)n.R);
    rows += align_up(q.N, DM_ROWS);
    MHIMX_CHECK_ARG(rows <= MHIMX_DSMIL_MHIM_WINDOW_MAX_ROWS, "dsmil_mhim_window: bag %d: %lld rows in the window's bag space up to this bag, at most %d", b,
                    (long long)rows, MHIMX_DSMIL_MHIM_WINDOW_MAX_ROWS);
  }
  return 0;
}

// tab: the bag space; tab2: the token space (X / ldx are filled where a launch reads its rows as "bags"); either may be null (layout only)
void dm_layout(const mhimx_dsmil_mhim_cfg* cfg, int32_t n_bags, const mhimx_ragged_window_bag* bags, DmLay* w, InferTab* tab, InferTab* tab2, DmCnt* cn,
               int64_t* row0_out, int64_t* tok0_out) {
  const int64_t E = cfg->base.E, D = cfg->base.D, C = cfg->base.C, k = cfg->k, n = n_bags;
  RgCount cnt, cnt2;
  int64_t mrows = 0, sel_b = 0, perm_n = 0, ids_n = 0, rows_n = 0;
  for (int b = 0; b < n_bags; ++b) {
    const mhimx_ragged_window_bag& q = bags[b];
    const int64_t M = q.cnt.Lk + k, tslot = align_up(M, DM_ROWS);
    if (row0_out) row0_out[b] = cnt.rows;
    if (tok0_out) tok0_out[b] = cnt2.rows;
    if (cn) {
      cn->tok0[b] = cnt2.rows; cn->mrg0[b] = mrows; cn->len_keep[b] = (int32_t)q.cnt.len_keep; cn->Lk[b] = (int32_t)q.cnt.Lk;
      cn->tslot[b] = (int32_t)tslot;
    }
    rg_tab_add(tab, cnt, b, q.X, q.ldx, q.N, align_up(q.N, DM_ROWS));
    rg_tab_add(tab2, cnt2, b, nullptr, IE, M, tslot);
    mrows += q.cnt.R;
    auto up = [](int64_t& a, int64_t v) { if (v > a) a = v; };
    up(sel_b, mhimx_select_ws_bytes(q.N));
    if (q.N > 16384) { up(perm_n, q.cnt.k_top); up(ids_n, q.N); up(rows_n, q.cnt.len_keep); }
  }
  rg_tab_close(tab, cnt, n_bags);
  rg_tab_close(tab2, cnt2, n_bags);
  const int64_t rows = cnt.rows, parts = cnt.parts, trows = cnt2.rows, tparts = cnt2.parts;
  w->rows = rows; w->trows = trows; w->mrows = mrows;
  w->steps = (int32_t)(rows / DM_ROWS);
  // d W1's split-K slabs over the bag space (dsmil_window.hip's rule); the student's three over the token space
  const int s1_room = pw_split_k(w->steps, 8, 8, &w->s1, &w->s1_per);
  Arena ar(nullptr, 0);
  w->w1p_t = ar.off; ar.take<float>(E * D);
  w->w1p_s = ar.off; ar.take<float>(E * D);
  w->vp_t = ar.off; ar.take<float>(E * E);
  w->q0f_t = ar.off; ar.take<float>(DM_Q * E);
  w->q2f_t = ar.off; ar.take<float>(DM_Q * DM_Q);
  w->wo_t = ar.off; ar.take<float>(512 * E);
  w->B_t = ar.off; ar.take<float>(n * C * E);
  w->lb_t = ar.off; ar.take<float>(n * C);
  w->lg_t = ar.off; ar.take<float>(n * C);
  w->li_t = ar.off; ar.take<float>(n * C);
  w->crit_t = ar.off; ar.take<int64_t>(n * C);
  w->qmax_t = ar.off; ar.take<float>(n * DM_MAXC * DM_Q);
  // ---- the bag space (V_t: the teacher's V rows, and - the teacher is done by then - the dPRE rows of the tail)
  w->H_t = ar.off; ar.take<float>(rows * E);
  w->H_s = ar.off; ar.take<float>(rows * E);
  w->dact = ar.off; ar.take<_Float16>(rows * E);
  w->V_t = ar.off; ar.take<float>(rows * E);
  w->Q_t = ar.off; ar.take<float>(rows * DM_Q);
  w->cls_t = ar.off; ar.take<float>(rows * DM_MAXC);
  w->score = ar.off; ar.take<float>(rows);
  w->rows_all = ar.off; ar.take<int64_t>(rows);
  w->pos = ar.off; ar.take<int32_t>(rows);
  w->db1_part = ar.off; ar.take<float>((int64_t)w->steps * E);
  w->pmax_t = ar.off; ar.take<float>(parts * DM_MAXC);
  w->parg_t = ar.off; ar.take<int32_t>(parts * DM_MAXC);
  w->pm_t = ar.off; ar.take<float>(parts * DM_MAXC);
  w->pl_t = ar.off; ar.take<float>(parts * DM_MAXC);
  w->pB_t = ar.off; ar.take<float>(parts * C * E);
  w->slab_1 = ar.off; ar.take<float>((int64_t)s1_room * E * D);
  // ---- the token space: the tokens and the student's share
  w->T = ar.off; ar.take<float>(trows * E);
  ds_take(ar, &w->s, n, C, trows, tparts, (int32_t)(trows / DM_ROWS));
  // ---- the rows to merge, their gradient rows, every bag's own Merge workspace (the forward leaves there what the backward reads)
  w->Xm = ar.off; ar.take<float>(mrows * E);
  w->dXm = ar.off; ar.take<float>(mrows * E);
  for (int b = 0; b < n_bags; ++b) {
    w->merge_ws_bytes[b] = merge2_ws_bytes(bags[b].cnt.R, k);
    w->merge_ws[b] = ar.off; ar.take<char>(w->merge_ws_bytes[b]);
  }
  // ---- the select's scratch, once, sized for the largest bag
  w->sel_ws_bytes = sel_b; w->sel_ws = ar.off; ar.take<char>(sel_b);
  w->sel_perm = ar.off; ar.take<int64_t>(perm_n);
  w->sel_ids = ar.off; ar.take<int64_t>(ids_n);
  w->sel_rows = ar.off; ar.take<int64_t>(rows_n);
  w->sel_lk = ar.off; ar.take<int64_t>(1);
  w->total = ar.off;
}

}  // namespace

}  // namespace mhimx

using namespace mhimx;

extern "C" int mhimx_dsmil_mhim_window_layout_of(const mhimx_dsmil_mhim_cfg* cfg, int32_t n_bags, const mhimx_ragged_window_bag* bags,
                                                 mhimx_dsmil_mhim_window_layout* out) {
  MHIMX_CHECK_ARG(out, "dsmil_mhim_window_layout: null output");
  if (int r = check_dm(cfg, n_bags, bags)) return r;
  DmLay w;
  memset(out, 0, sizeof(*out));
  dm_layout(cfg, n_bags, bags, &w, nullptr, nullptr, nullptr, out->row0, out->tok0);
  out->total = w.total; out->rows = w.rows; out->tok_rows = w.trows; out->logits = w.s.logits; out->losses = w.s.losses; out->logits_bag = w.s.logits_bag;
  out->logits_ins = w.s.logits_ins; out->B = w.s.B; out->crit = w.s.crit; out->B_teacher = w.B_t; out->H_teacher = w.H_t; out->H_student = w.H_s;
  out->dact = w.dact; out->score = w.score; out->rows_all = w.rows_all; out->tokens = w.T;
  return 0;
}

extern "C" int64_t mhimx_dsmil_mhim_window_ws_bytes(const mhimx_dsmil_mhim_cfg* cfg, int32_t n_bags, const mhimx_ragged_window_bag* bags) {
  if (int r = check_dm(cfg, n_bags, bags)) return r;
  DmLay w;
  dm_layout(cfg, n_bags, bags, &w, nullptr, nullptr, nullptr, nullptr, nullptr);
  return w.total;
}

extern "C" int mhimx_dsmil_mhim_window_run(void* stream, const mhimx_dsmil_mhim_cfg* cfg, int32_t n_bags, const mhimx_ragged_window_bag* bags,
                                           int64_t host_step, void* ws, int64_t ws_bytes, int32_t update, int32_t x_dtype) {
  if (int r = check_dm(cfg, n_bags, bags, x_dtype)) return r;
  for (int b = 0; b < n_bags; ++b) {
    MHIMX_CHECK_ARG(bags[b].X && aligned16(bags[b].X), "dsmil_mhim_window: bag %d: null or unaligned rows", b);
    MHIMX_CHECK_ARG(bags[b].label_dev, "dsmil_mhim_window: bag %d: null label", b);
  }
  const mhimx_dsmil_train_cfg& c = cfg->base;
  MHIMX_CHECK_ARG(!update || (c.p && c.g && c.m && c.v && c.n_train > 0 && c.n_all >= c.n_train), "dsmil_mhim_window: update needs the flat optimiser buffers");
  DmLay w;
  InferTab tab = {}, tab2 = {};
  DmCnt cn = {};
  dm_layout(cfg, n_bags, bags, &w, &tab, &tab2, &cn, nullptr, nullptr);
  tab.pad = x_dtype;                           // read by the launches that read X: both projections (A.2, A.3) and d W1 (E.2)
  tab2.pad = MHIMX_X_F32;
  if (int r = rg_check_ws("dsmil_mhim_window", ws, ws_bytes, w.total)) return r;
  const mhimx_dsmil_params &P = c.param, &Tp = cfg->teacher;
  hipStream_t st = (hipStream_t)stream;
  char* base = static_cast<char*>(ws);
  auto F = [&](int64_t off) { return reinterpret_cast<float*>(base + off); };
  const int D = (int)c.D, C = (int)c.C;
  const int64_t k = cfg->k;
  float *H_t = F(w.H_t), *H_s = F(w.H_s), *V_t = F(w.V_t), *Q_t = F(w.Q_t), *score = F(w.score);
  float *T = F(w.T), *dhv = F(w.s.dhv), *Xm = F(w.Xm), *dXm = F(w.dXm);
  float* dpre = V_t;                           // (the teacher's V rows are dead behind A.8)
  _Float16* dact = reinterpret_cast<_Float16*>(base + w.dact);
  int64_t* rows_space = reinterpret_cast<int64_t*>(base + w.rows_all);
  int32_t* pos = reinterpret_cast<int32_t*>(base + w.pos);
  const uint64_t* tick = c.tick;
  float* q_dst = cfg->q_out ? cfg->q_out : cfg->q;

  // ================================================================================================ A. forward, window-wide
  // ---- 1. counters, weight images, the parameter-only part of every bag's Merge (8 bags per launch: the first 8 ride here)
  mhimx_merge mw_prep = dm_merge_params(*cfg);      // (read while enqueueing by the kind-6 jobs: alive until the last of them is enqueued)
  {
    mhimx_prep_job jobs[24];
    int n = 0;
    jobs[n++] = mhimx_prep_job{3, nullptr, reinterpret_cast<float*>(c.tick), 1, 1};
    if (c.opt_step) jobs[n++] = mhimx_prep_job{3, nullptr, reinterpret_cast<float*>(c.opt_step), 1, 1};
    jobs[n++] = mhimx_prep_job{1, Tp.w1, F(w.w1p_t), c.E, c.D};
    jobs[n++] = mhimx_prep_job{1, P.w1, F(w.w1p_s), c.E, c.D};
    jobs[n++] = mhimx_prep_job{1, Tp.wv, F(w.vp_t), c.E, c.E};
    jobs[n++] = mhimx_prep_job{4, Tp.wq0, F(w.q0f_t), DM_Q, c.E};
    jobs[n++] = mhimx_prep_job{4, Tp.wq2, F(w.q2f_t), DM_Q, DM_Q};
    n += ds_prep_jobs(P, base, w.s, jobs + n);
    jobs[n++] = mhimx_prep_job{0, cfg->merge.wo, F(w.wo_t), c.E, 512};
    if (cfg->q_out) jobs[n++] = mhimx_prep_job{2, cfg->q, cfg->q_out, 1, k * c.E};
    for (int b = 0; b < n_bags && b < 8; ++b)
      jobs[n++] = mhimx_prep_job{6, reinterpret_cast<const float*>(&mw_prep), reinterpret_cast<float*>(base + w.merge_ws[b]), bags[b].cnt.R, w.merge_ws_bytes[b]};
    if (int r = mhimx_prep_batch(stream, jobs, n)) return r;
  }
  // ---- 2., 3. both models' feature rows into the bag space: the teacher first - its d out / d pre rows are overwritten by the student's
  {
    PureWinDrop dr = {};
    dr.tick = tick; dr.dact = dact;
    for (int b = 0; b < n_bags; ++b) dr.seed[b] = bags[b].seeds.drop_teacher;
    dr.drop_p = cfg->drop_p_teacher;
    if (int r = pure_window_project(st, tab, dr, D, F(w.w1p_t), Tp.b1, c.act, H_t)) return r;
    for (int b = 0; b < n_bags; ++b) dr.seed[b] = bags[b].seeds.drop_student;
    dr.drop_p = c.drop_p;
    if (int r = pure_window_project(st, tab, dr, D, F(w.w1p_s), P.b1, c.act, H_s)) return r;
  }
  // ---- 4. - 8. the teacher's DSMIL forward: V, Q / classes, critical rows, pool partials, B_teacher and every row's instance score
  InferTab tabv = tab;
  for (int b = 0; b < n_bags; ++b) { tabv.X[b] = H_t + tab.row0[b] * IE; tabv.ldx[b] = IE; }
  tabv.pad = MHIMX_X_F32;
  if (int r = infer_project(st, tabv, IE, F(w.vp_t), Tp.bv, MHIMX_ACT_RELU, V_t)) return r;
  if (int r = dsmil_rows_crit_pool(st, tab, H_t, V_t, F(w.q0f_t), Tp.bq0, F(w.q2f_t), Tp.bq2, Tp.wi, Tp.bi, C, Q_t, F(w.cls_t), F(w.pmax_t),
                                   reinterpret_cast<int32_t*>(base + w.parg_t), F(w.qmax_t), F(w.li_t), reinterpret_cast<int64_t*>(base + w.crit_t),
                                   F(w.pm_t), F(w.pl_t), F(w.pB_t), cfg->cls_attn ? score : nullptr))
    return r;
  if (int r = dsmil_finalize(st, tab, F(w.pm_t), F(w.pl_t), F(w.pB_t), Q_t, F(w.qmax_t), Tp.wfcc, Tp.bfcc, C, F(w.li_t), F(w.lb_t), F(w.lg_t), F(w.B_t),
                             cfg->cls_attn ? nullptr : score))
    return r;
  // ---- 9. every bag's row list [rows that stay (Lk) | rows to merge (R)] at the bag's first row of the bag space.  The select reads the
  // bag's scores, its seed and *tick only (the tick moves once, in A.1)
  {
    mhimx_select_bag sb[DM_MAX];
    for (int b = 0; b < n_bags; ++b) {
      const mhimx_step_counts& n = bags[b].cnt;
      sb[b] = mhimx_select_bag{tab.row0[b], bags[b].N, n.k_top, n.n_sel, n.R, tab.row0[b], bags[b].seeds.select};
    }
    SelLargeWs lw;
    lw.perm = reinterpret_cast<int64_t*>(base + w.sel_perm); lw.ids = reinterpret_cast<int64_t*>(base + w.sel_ids);
    lw.rows = reinterpret_cast<int64_t*>(base + w.sel_rows); lw.lk = reinterpret_cast<int64_t*>(base + w.sel_lk);
    lw.sel_ws = base + w.sel_ws; lw.sel_ws_bytes = w.sel_ws_bytes;
    if (int r = select_bags_check("dsmil_mhim_window", n_bags, sb)) return r;
    if (int r = select_rows_many_launch(st, score, n_bags, sb, tick, rows_space, lw, 0)) return r;
  }
  // ---- 10. stay rows -> the token space, rows to merge -> the merge buffer
  hipLaunchKernelGGL(dm_gather_kernel, dim3((unsigned)n_bags, DM_GATHER_Y), dim3(DM_T), 0, st, tab, cn, H_s, rows_space, (int)k, T, Xm, pos);
  MHIMX_LAUNCH_CHECK();

  // ================================================================================================ B. Merge forward, bag after bag
  for (int b = 0; b < n_bags; ++b) {
    if (b >= 8 && b % 8 == 0) {
      mhimx_prep_job jobs[8];
      int n = 0;
      for (int q = b; q < n_bags && q < b + 8; ++q)
        jobs[n++] = mhimx_prep_job{6, reinterpret_cast<const float*>(&mw_prep), reinterpret_cast<float*>(base + w.merge_ws[q]), bags[q].cnt.R, w.merge_ws_bytes[q]};
      if (int r = mhimx_prep_batch(stream, jobs, n)) return r;
    }
    mhimx_merge mw = mw_prep;
    mw.drop_seed = bags[b].seeds.mca; mw.prepared = 1;
    if (int r = mhimx_merge_fwd(stream, &mw, Xm + cn.mrg0[b] * IE, bags[b].cnt.R, T + (cn.tok0[b] + cn.Lk[b]) * IE, nullptr, 0, base + w.merge_ws[b],
                                w.merge_ws_bytes[b]))
      return r;
  }

  // ================================================================================================ C. the student, token-space-wide
  // the tokens have no d out / d pre of their own (it lives in the bag space; the k Merge tokens have none): plain d tokens, no d b1 partials.
  // The head is always the distillation instantiation; Bt NULL when aux_alpha == 0
  if (int r = ds_forward(st, tab2, base, w.s, P, C, T)) return r;
  {
    DsLabels lab = {};
    for (int b = 0; b < n_bags; ++b) lab.p[b] = bags[b].label_dev;
    const DsDist dist = {cfg->aux_alpha != 0.f ? F(w.B_t) : nullptr, cfg->temp_t, cfg->aux_alpha};
    if (int r = ds_head(st, tab2, base, w.s, P, C, T, lab, c.main_alpha, dist)) return r;
  }
  if (int r = ds_backward(st, tab2, base, w.s, P, C, T, nullptr, nullptr)) return r;

  // ================================================================================================ D. Merge backward, bag after bag
  // d X of the bag's R merged rows from its k tokens' gradient rows; the six Merge gradients accumulate in bag order on the one stream:
  // bag 0 overwrites, every later bag adds.  A bag's reductions are flushed before the next bag queues its own (ragged_window.hip part B).
  for (int b = 0; b < n_bags; ++b) {
    mhimx_merge mwb = mw_prep;
    mwb.drop_seed = bags[b].seeds.mca; mwb.wo_t = F(w.wo_t); mwb.prepared = 0;
    mhimx_reduce_list lst;
    memset(&lst, 0, sizeof(lst));
    mhimx_merge_grad mg = {};
    const mhimx_dsmil_merge_grads& G_ = cfg->merge_grad;
    mg.d_ln_w = G_.ln_w; mg.d_ln_b = G_.ln_b; mg.d_wkv = G_.wkv; mg.d_wq = G_.wq; mg.d_wo = G_.wo; mg.d_bo = G_.bo;
    mg.accumulate = b > 0 ? 1 : 0; mg.splits = 8; mg.defer = &lst;
    if (int r = mhimx_merge_bwd(stream, &mwb, Xm + cn.mrg0[b] * IE, bags[b].cnt.R, dhv + (cn.tok0[b] + cn.Lk[b]) * IE, dXm + cn.mrg0[b] * IE, &mg,
                                base + w.merge_ws[b], w.merge_ws_bytes[b]))
      return r;
    if (int r = mhimx_reduce_flush(stream, &lst)) return r;
  }

  // ================================================================================================ E. the tail, window-wide
  hipLaunchKernelGGL(dm_scatter_kernel, dim3((unsigned)w.steps), dim3(DM_T), 0, st, tab, cn, rows_space, pos, dhv, dXm, dact, dpre, F(w.db1_part));
  MHIMX_LAUNCH_CHECK();
  if (int r = pw_wgrad_bagx(st, tab, dpre, D, w.steps, w.s1, w.s1_per, F(w.slab_1))) return r;
  if (int r = ds_reduce(st, base, w.s, c.grad, D, C, n_bags, F(w.slab_1), w.s1, F(w.db1_part), w.steps)) return r;
  {
    int64_t tok[DM_MAX];
    for (int b = 0; b < n_bags; ++b) tok[b] = cn.tok0[b] + cn.Lk[b];
    if (int r = rw_q_chain(st, q_dst, T, n_bags, tok, (double)cfg->merge_mm, (int)(k * c.E))) return r;
  }
  if (!update) return 0;
  mhimx_optim_args o = optim_args_of(c, host_step);
  o.teacher = cfg->p_teacher; o.ema_mm = cfg->ema_mm; o.mm_table = cfg->mm_table; o.mm_len = cfg->mm_len;
  return mhimx_optim_step(stream, &o);
}
