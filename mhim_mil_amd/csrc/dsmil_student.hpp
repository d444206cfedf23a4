// dsmil_student.hpp — ONE copy of the DSMIL student that the two ragged native train calls enqueue (mhimx_dsmil_window_run:
// dsmil_window.hip, over the bag space; mhimx_dsmil_mhim_window_run: dsmil_mhim.hip, over the token space): the head kernel, the student's
// share of the workspace, its weight-image preparation jobs, forward, head launch, backward down to the gradient rows and the weight
// gradients' slabs, the two reduction launches, and the checks both calls make on mhimx_dsmil_train_cfg.  The host helpers work over
// (workspace base, DsLay, table), are defined in dsmil_window.hip and add no error messages of their own; the head kernel's body lives here,
// so each translation unit instantiates what it launches.  What a caller keeps: the feature rows and their d out / d pre, the counters and
// W1 images of the preparation launch, the teacher, select, Merge and scatter, d W1 with its slabs and bias partials, the update.
#pragma once
#include "infer_tab.hpp"

namespace mhimx {

constexpr int DS_Q = 128, DS_MAXC = 16;                          // width of q; most classes

struct DsLabels { const int64_t* p[MHIMX_INFER_MAX]; };
// the per-class distillation of mhimx_dsmil_mhim_window_run: the teacher's B [n, C, 512] (NULL: no distillation term), temperature, weight
struct DsDist { const float* Bt; float temp_t, aux_alpha; };
template <class T>
MHIMX_DEV const T& ds_dist_of(const T& d) { return d; }

// {max, sum} style block reductions of the distillation: wave results combined in index order (red: 8 floats of LDS)
MHIMX_DEV float ds_blk_max(float v, float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_max(v);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int w = 1; w < 8; ++w) r = fmaxf(r, red[w]);
  __syncthreads();
  return r;
}
MHIMX_DEV float ds_blk_sum(float v, float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_sum(v);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float r = 0.f;
#pragma unroll
  for (int w = 0; w < 8; ++w) r += red[w];
  __syncthreads();
  return r;
}

// ------------------------------------------------------------------------------------------------ merge + fcc + mix + CE + head gradients
// blockIdx.x = bag; thread e = column e.  The forward half is dsmil_finalize_kernel's y = 0 plane (same order of every sum).  The trailing
// pack DIST is the distillation.  Empty: the teacher-free head.  One DsDist: the per-class distillation of mhimx_dsmil_head (optim.hip:
// dsmil_head_kernel) between the forward and the head gradients: cl = mean_c [ - sum_e softmax(Bt[c] / temp_t)_e log_softmax(B[c])_e ],
// d B[c] += aux_alpha inv_n / C (softmax(B[c]) - softmax(Bt[c] / temp_t)); Bt NULL: d B[c] += 0.  Everything around it is one text.
template <class... DIST>
__global__ __launch_bounds__(RG_FIN_T) void ds_head_kernel(InferTab tab, DsLabels lab, const float* __restrict__ pm, const float* __restrict__ pl,
                                                         const float* __restrict__ pB, const float* __restrict__ H,
                                                         const float* __restrict__ wfcc, const float* __restrict__ bfcc,
                                                         const float* __restrict__ logits_ins, const int64_t* __restrict__ crit, int C,
                                                         float main_alpha, float inv_n, float* __restrict__ logits_bag,
                                                         float* __restrict__ logits, float* __restrict__ losses, float* __restrict__ B_out,
                                                         float* __restrict__ stats, float* __restrict__ gli, float* __restrict__ dB,
                                                         float* __restrict__ delta, float* __restrict__ dwfcc_part,
                                                         float* __restrict__ dbfcc_part, float* __restrict__ dwi_part,
                                                         float* __restrict__ dbi_part, DIST... dist) {
  constexpr bool DISTIL = sizeof...(DIST) == 1;
  __shared__ float red[8];
  __shared__ float wgt[RG_FIN_T];
  __shared__ float smx[DS_MAXC], sinv[DS_MAXC], lg[DS_MAXC], gl[DS_MAXC];
  __shared__ float dl[DS_MAXC][8];
  __shared__ __attribute__((aligned(16))) float big[DS_MAXC * IE];   // B [C][512]
  const int bag = blockIdx.x;
  RG_BAG(bag)
  const int64_t* label = lab.p[0];
  RG_PICK(label, lab.p, bag)
  const int G = rg_parts(N);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  pm += (int64_t)p0 * DS_MAXC; pl += (int64_t)p0 * DS_MAXC; pB += (int64_t)p0 * C * IE;
  for (int c = 0; c < C; ++c) {
    float mx, Ls;
    rg_merge_stats(pm + c, pl + c, G, DS_MAXC, red, mx, Ls);
    if (tid == 0) {
      smx[c] = mx; sinv[c] = 1.f / Ls;
      stats[((int64_t)bag * DS_MAXC + c) * 2] = mx;
      stats[((int64_t)bag * DS_MAXC + c) * 2 + 1] = 1.f / Ls;
    }
    __syncthreads();
  }
  for (int c = 0; c < C; ++c) {
    const float mx = smx[c];
    float acc = 0.f;                                            // column tid of B[c]
    for (int base = 0; base < G; base += RG_FIN_T) {
      __syncthreads();
      wgt[tid] = base + tid < G ? __expf(pm[(int64_t)(base + tid) * DS_MAXC + c] - mx) : 0.f;
      __syncthreads();
      const int cnt = G - base < RG_FIN_T ? G - base : RG_FIN_T;
#pragma unroll 8
      for (int j = 0; j < cnt; ++j) acc += pB[((int64_t)(base + j) * C + c) * IE + tid] * wgt[j];
    }
    const float bv = acc * sinv[c];
    big[c * IE + tid] = bv;
    B_out[((int64_t)bag * C + c) * IE + tid] = bv;
  }
  __syncthreads();
  for (int o = wave; o < C; o += RG_FIN_T / 64) {
    float d = 0.f;
    for (int c = 0; c < C; ++c) {
      const float* w = wfcc + ((int64_t)o * C + c) * IE;
#pragma unroll
      for (int q = 0; q < IE / 64; ++q) d += big[c * IE + lane + 64 * q] * w[lane + 64 * q];
    }
    d = wave_sum(d);
    if (lane == 0) {
      const float lb = d + bfcc[o];
      const float mix = 0.5f * lb + 0.5f * logits_ins[(int64_t)bag * C + o];
      logits_bag[(int64_t)bag * C + o] = lb;
      logits[(int64_t)bag * C + o] = mix;
      lg[o] = mix;
    }
  }
  __syncthreads();
  // ---- distillation: this thread's column of d cl / d B[c] (scaled) stays in dk[c]; every thread ends with the same cl
  [[maybe_unused]] float cl = 0.f, aux_alpha = 0.f;
  [[maybe_unused]] float dk[DS_MAXC];
  if constexpr (DISTIL) {
    const DsDist& ds = ds_dist_of(dist...);
    aux_alpha = ds.aux_alpha;
#pragma unroll
    for (int c = 0; c < DS_MAXC; ++c) dk[c] = 0.f;
    if (ds.Bt) {
      const float gs = aux_alpha * inv_n / (float)C;
#pragma unroll
      for (int c = 0; c < DS_MAXC; ++c)
        if (c < C) {
          const float s = big[c * IE + tid], t = ds.Bt[((int64_t)bag * C + c) * IE + tid] / ds.temp_t;
          const float s_mx = ds_blk_max(s, red), t_mx = ds_blk_max(t, red);
          const float es = expf(s - s_mx), et = expf(t - t_mx);
          const float s_den = ds_blk_sum(es, red), t_den = ds_blk_sum(et, red);
          const float pt = et / t_den;
          cl -= ds_blk_sum(pt * (s - s_mx - logf(s_den)), red) / (float)C;
          dk[c] = gs * (es / s_den - pt);
        }
    }
  }
  if (tid == 0) {
    // torch.nn.CrossEntropyLoss on one row (a label outside [0, C): NaN, where torch raises); g_lb = g_li = 0.5 g_logits
    float cm = lg[0];
    for (int c = 1; c < C; ++c) cm = fmaxf(cm, lg[c]);
    float den = 0.f;
    for (int c = 0; c < C; ++c) den += expf(lg[c] - cm);
    const int64_t y = label[0];
    const bool ok = y >= 0 && y < C;
    const float ce = ok ? (cm + logf(den)) - lg[ok ? y : 0] : NAN;
    if constexpr (DISTIL) {
      losses[3 * bag] = main_alpha * ce + aux_alpha * cl;
      losses[3 * bag + 1] = ce;
      losses[3 * bag + 2] = cl;
    } else {
      losses[3 * bag] = main_alpha * ce;
      losses[3 * bag + 1] = ce;
      losses[3 * bag + 2] = 0.f;
    }
    for (int c = 0; c < DS_MAXC; ++c) {
      const float g = c < C ? (ok ? 0.5f * (main_alpha * (expf(lg[c] - cm) / den - (c == y ? 1.f : 0.f)) * inv_n) : NAN) : 0.f;
      gl[c] = g;
      gli[(int64_t)bag * DS_MAXC + c] = g;
      if (c < C) { dbfcc_part[(int64_t)bag * C + c] = g; dbi_part[(int64_t)bag * C + c] = g; }
    }
  }
  __syncthreads();
  // class c's d B row, d fcc / d i_classifier partials and delta's wave sums.  The teacher-free form loops c < C; the distillation form
  // is fully unrolled with `if (c < C)`, so that dk[] stays in registers
  auto one_class = [&](int c) {
    const float b = big[c * IE + tid];
    float db = 0.f;
    for (int o = 0; o < C; ++o) {
      db = fmaf(wfcc[((int64_t)o * C + c) * IE + tid], gl[o], db);
      dwfcc_part[(((int64_t)bag * C + o) * C + c) * IE + tid] = gl[o] * b;
    }
    if constexpr (DISTIL) db += dk[c];
    dB[((int64_t)bag * DS_MAXC + c) * IE + tid] = db;
    int64_t cr = crit[(int64_t)bag * C + c];
    if (cr < 0 || cr >= N) cr = 0;                              // (a class whose logits are all NaN has no critical row)
    dwi_part[((int64_t)bag * C + c) * IE + tid] = gl[c] * H[(orow0 + cr) * IE + tid];
    const float d = wave_sum(db * b);
    if (lane == 0) dl[c][wave] = d;
  };
  if constexpr (DISTIL) {
#pragma unroll
    for (int c = 0; c < DS_MAXC; ++c)
      if (c < C) one_class(c);
  } else {
    for (int c = 0; c < C; ++c) one_class(c);
  }
  __syncthreads();
  if (tid < DS_MAXC) {
    float t = 0.f;
    if (tid < C) {
#pragma unroll
      for (int w = 0; w < 8; ++w) t += dl[tid][w];
    }
    delta[(int64_t)bag * DS_MAXC + tid] = t;
  }
}

// ------------------------------------------------------------------------------------------------ host: the student's share of a workspace
// byte offsets: the six weight images, the per-bag head regions, the rows of the student's row space (the bag space of
// mhimx_dsmil_window_run, the token space of mhimx_dsmil_mhim_window_run), the pool / bias / d q_max partials and the three split-K slabs
struct DsLay {
  int64_t vp, vtp, q0f, q2f, q2tf, q0tf;
  int64_t logits, losses, logits_bag, logits_ins, B, crit, qmax, stats, gli, dB, delta, dqmax, dwfcc_part, dbfcc_part, dwi_part, dbi_part;
  int64_t V, Q, cls, da, dhv, U1, dPQ, dP1;
  int64_t pmax, parg, pm, pl, pB, dbv_part, dbq0_part, dbq2_part, dqm_part, slab_v, slab_q0, slab_q2;
  int32_t steps, sv, sv_per, sq0, sq0_per, sq2, sq2_per;       // 32-row tiles of the row space; the split-K numbers of the three slabs
};
// n bags, C classes; rows, parts, steps: the student's row space, its pool partials and its 32-row tiles
void ds_take(Arena& ar, DsLay* s, int64_t n, int64_t C, int64_t rows, int64_t parts, int32_t steps);

// the six weight-image jobs {vp, vtp, q0f, q2f, q2tf, q0tf} into j[]; returns 6
int ds_prep_jobs(const mhimx_dsmil_params& P, char* base, const DsLay& s, mhimx_prep_job* j);
// V = relu(h Wv^T + bv) over the rows H of the table's row space; Q, classes, critical rows, pool partials (infer_dsmil.hip)
int ds_forward(hipStream_t st, const InferTab& tab, char* base, const DsLay& s, const mhimx_dsmil_params& P, int C, const float* H);
// rows pass 1, d PreV Wv, d q_max, rows pass 2, d Wv / d Wq2 / d Wq0 slabs.  dact and db1_part: the rows' d out / d pre is applied over dhv
// in place and the tiles' d b1 partials are written; both NULL: d h as it is, zero rows past a bag's N
int ds_backward(hipStream_t st, const InferTab& tab, char* base, const DsLay& s, const mhimx_dsmil_params& P, int C, const float* H,
                const _Float16* dact, float* db1_part);
// the twelve partial buffers in index order into the gradient views; d W1's slabs, their count and the d b1 partials of steps1 tiles are
// the caller's
int ds_reduce(hipStream_t st, char* base, const DsLay& s, const mhimx_dsmil_grads& g, int64_t D, int C, int n_bags, const float* slab_1,
              int32_t s1, const float* db1_part, int32_t steps1);
inline bool ds_params_ok(const mhimx_dsmil_params& p) {
  return p.w1 && p.b1 && p.wi && p.bi && p.wq0 && p.bq0 && p.wq2 && p.bq2 && p.wv && p.bv && p.wfcc && p.bfcc;
}
inline bool ds_params_aligned(const mhimx_dsmil_params& p) {
  return aligned16(p.w1) && aligned16(p.b1) && aligned16(p.wi) && aligned16(p.wq0) && aligned16(p.wq2) && aligned16(p.wv) && aligned16(p.bv);
}
// what both calls check on (x_dtype, cfg, bag list, bag count) under the caller's name: null arguments, 1..max_bags bags, the shapes, the
// activation, the student's dropout, its twelve parameters ("null <student>parameter") and their alignment, the gradient views, the tick
int ds_check_base(const char* who, const mhimx_dsmil_train_cfg* c, int32_t xdt, int32_t n_bags, int32_t max_bags, const void* bags,
                  const char* student);

// the head launch: the partials merged, B, fcc, the mix, CE (+ the distillation `dist`: one DsDist, or nothing) and the head gradients
template <class... DIST>
int ds_head(hipStream_t st, const InferTab& tab, char* base, const DsLay& s, const mhimx_dsmil_params& P, int C, const float* H, const DsLabels& lab,
            float main_alpha, DIST... dist) {
  auto F = [&](int64_t off) { return reinterpret_cast<float*>(base + off); };
  hipLaunchKernelGGL(ds_head_kernel<DIST...>, dim3((unsigned)tab.n), dim3(RG_FIN_T), 0, st, tab, lab, F(s.pm), F(s.pl), F(s.pB), H, P.wfcc, P.bfcc,
                     F(s.logits_ins), reinterpret_cast<const int64_t*>(base + s.crit), C, main_alpha, 1.f / (float)tab.n, F(s.logits_bag), F(s.logits),
                     F(s.losses), F(s.B), F(s.stats), F(s.gli), F(s.dB), F(s.delta), F(s.dwfcc_part), F(s.dbfcc_part), F(s.dwi_part), F(s.dbi_part),
                     dist...);
  MHIMX_LAUNCH_CHECK();
  return 0;
}

}  // namespace mhimx
