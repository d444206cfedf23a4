// step_mid.hpp — ONE copy of the student's middle that the three native train calls of the full MHIM(ABMIL) model enqueue
// (mhimx_step_run, mhimx_window_run: step.hip; mhimx_ragged_window_run_x: ragged_window.hip): the Merge description, the weight-image
// preparation jobs, the scorer descriptors, the student's forward, the head and the backward down to the gradient rows.  Host code, defined
// in step.hip; every launch goes through the library's own extern "C" entry points, which set the error messages: the helpers add none.
// What a caller keeps: which launch carries which preparation jobs, the teacher half, the select, the projection's gradient pair, its
// reduction list and the update.
#pragma once
#include "common.hpp"

namespace mhimx {

// the parameter images a call prepares once (pointers into its workspace)
struct MidImages { float *w1p_t, *wa_frag_t, *w1p_s, *wa_frag_s, *wa_t, *wa_t_frag, *wo_t, *q_old; };

// one bag's share of the workspace: the student's feature rows [N + k, E] (Merge's tokens land behind the bag's rows) and their gradient
// rows, the row list [rows to merge (R) | rows that stay (Lk) | N .. N + k - 1], Merge's dropout seed, where the forward's EMA of the
// global queries goes, the student pool's outputs, the head's g_z, the pool's and Merge's workspaces
struct MidBag {
  float *Hbuf, *dH;
  int64_t* rows_all;
  int64_t N, R, Lk;
  uint64_t mca_seed;
  float* q_out;
  float *s_s, *stats_s, *z_s, *g_z;
  void* pool_ws; int64_t pool_ws_bytes;
  void* merge_ws; int64_t merge_ws_bytes;
};
// mhimx_step_run's DAG form (side_stream): the two streams and the step's fork / join events.  NULL: the one-stream chain
struct MidDag { hipStream_t main_st, side_st; hipEvent_t* ev; };
// what the forward leaves for the backward
struct MidFwd { mhimx_merge mw; mhimx_scorer sc_s; mhimx_pool_io io_s; };
// the stay rows' share of the projection's dPRE image written by the scorer backward itself (mhimx_pool_grad.img ..).  NULL: fp32 rows
struct MidImg { void* img; const void* dact; float* part; };

// the parameter-only part of the student's Merge.  Prep job kind 6 reads it WHILE ENQUEUEING: it stays in the caller's frame until the
// launch that carries that job is enqueued
mhimx_merge mid_merge_params(const mhimx_step_cfg& c);
// preparation jobs into j[], in the one order every call uses; the count is returned.  head: {tick, opt_step?, T.w1, T.wa frag, S.w1}
// (<= 5); student: {S.wa frag, S.wa^T, S.wa^T frag, S.wo^T, q snapshot} (5)
int mid_prep_head(const mhimx_step_cfg& c, const MidImages& im, mhimx_prep_job* j);
int mid_prep_student(const mhimx_step_cfg& c, const MidImages& im, mhimx_prep_job* j);
// a model's scorer (teacher: c.teacher, im.wa_frag_t; student: c.student, im.wa_frag_s)
mhimx_scorer mid_scorer(const mhimx_step_cfg& c, const mhimx_step_params& p, const float* wa_frag);
// phase-1 scorer over the rows that stay with Merge's row tiles riding -> mhimx_merge_fwd's tail -> the phase-2 finalize that scores the
// tokens.  dag: the scorer on the side stream beside Merge's whole chain on the main one (nothing rides), joined before the finalize
int mid_student_fwd(void* stream, const mhimx_step_cfg& c, const MidImages& im, const mhimx_merge& mw_prep, const MidBag& g, const MidDag* dag, MidFwd* f);
// a bag's survival head (mhimx_ragged_window_run_surv): its censorship flag, NLLSurvLoss(alpha), the clamp, where its risk goes (or NULL)
struct MidSurv { const float* censor; float alpha, eps; float* risk; };
// predictor, CE, distillation against z_t (not read when aux_alpha == 0) and their gradients: g.g_z, gr.wp / gr.bp.  sv: the survival
// criterion in place of the cross entropy (mhimx_head_surv_fwd_bwd); NULL: mhimx_head_fwd_bwd
int mid_head(void* stream, const mhimx_step_cfg& c, const MidBag& g, const float* z_t, const int64_t* label, float loss_scale, float* logits,
             float* losses, const mhimx_step_grads& gr, int accumulate, const MidSurv* sv = nullptr);
// mhimx_merge_bwd_park, mhimx_abmil_pool_bwd, mhimx_merge_bwd with their reductions queued on the caller's list.  dag: the side branch's
// two halves (the parked scorer-weight-gradient product, then the Merge parameter-gradient tail) are flushed from here
int mid_bwd_rows(void* stream, const MidImages& im, const MidFwd& f, const MidBag& g, const mhimx_step_grads& gr, int accumulate, const MidImg* img,
                 const MidDag* dag, mhimx_reduce_list* lst);
// the weights of a window's EMA chain of the global queries, q <- wq q + sum_b w[b] z_b: wq = mm^n, w[b] = (1 - mm) mm^(n-1-b), in double
void q_chain_weights(double mm, int n, float* wq, float* w);

}  // namespace mhimx
