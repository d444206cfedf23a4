// dsmil_window.hip — ONE optimiser update over up to MHIMX_DSMIL_WINDOW_MAX bags of DIFFERENT row counts for the teacher-free DSMIL model
// ('mhim_pure' with baseline 'dsmil'; n_bags = 1 is the single-bag step) behind one C call: mhimx_dsmil_window_run.
// replaces: engines/base_engine.py:29-51,76-120 (the accumulation window) around engines/common_mil.py:26-28,32-37, modules/mhim.py:274-298
//           `pure` and mhim_modules/baseline.py:112-194 (BClassifier / DSMIL) with their autograd, for bags b = 0 .. n-1:
//
//     h = dropout_b(act(X W1^T + b1)),  classes = h Wi^T + bi,  V = relu(h Wv^T + bv),  U1 = relu(h Wq0^T + bq0),  Q = tanh(U1 Wq2^T + bq2)
//     crit[c] = arg max_m classes[m,c],  q_max[c] = Q[crit[c]],  a = Q q_max^T / sqrt(128),  A = softmax_m(a),  B = A^T V
//     logits = 0.5 fcc(B) + 0.5 max_m classes,  loss_b = main_alpha CE(logits, label_b) / n,  g = sum_b d loss_b / d theta,  one Adam step
//
// The row space, the by-value table and the train-mode projection are mhimx_pure_window_run's (every bag starts at a multiple of 32; the
// rows between a bag's N and its next multiple of 32 are zero rows); the forward's middle is mhimx_infer_dsmil_run's kernels as they are.
// Eighteen launches whatever n and the sizes are:
//   1  mhimx_prep_batch            counters; paired-plane images of W1, Wv and Wv^T; fragment images of Wq0, Wq2, Wq2^T and Wq0^T
//   2  pure_window_project_elem_kernel  (bag_project.hip) X -> h with per-bag dropout and the fp16 d out / d pre rows; the keep-mask is the
//                                  gemm epilogues' per-element law: the mask the autograd route (ops.gemm_nt) draws for the same seed and tick
//   3  infer_project_kernel        h -> V (the feature rows as fp32 "bags" of pitch 512)
//   4  dsmil_rows_kernel           (infer_dsmil.hip, as it is) Q, classes, per-chunk arg-max partials
//   5  dsmil_crit_kernel           crit, logits_ins, q_max
//   6  dsmil_pool_kernel           per-chunk softmax-pool partials
//   7  dw_head_kernel              plane = bag: merge of the partials in index order -> B, fcc, the mix, CE; g_lb = g_li = 0.5 g_logits,
//                                  d B = Wfcc^T g_lb, delta_c = d B[c] . B[c], the bag's d fcc / d i_classifier partials
//   8  dw_rows1_kernel             one workgroup per 32-row tile: A again from Q and q_max, d A = V d B^T, d a = A (d A - delta),
//                                  d PreV = (A d B) [V > 0] over V in place, the tile's d bv and d q_max partials
//   9  infer_project_kernel        d PreV Wv: the ragged projection on the d PreV rows with the paired image of Wv^T
//  10  dw_dqmax_kernel             per bag: the tiles' d q_max partials in index order
//  11  dw_rows2_kernel             per tile: d Q = s d a q_max + the critical rows' d q_max, d PreQ = d Q (1 - Q^2); U1 again on the matrix
//                                  cores; d Pre1 = (d PreQ Wq2) [U1 > 0] and d Pre1 Wq0 on the matrix cores; d h = that + launch 9's rows +
//                                  g_li Wi on the critical rows; dPRE = d h * d out / d pre over launch 9's rows in place; bias partials
//  12-15  pw_tn_kernel             d Wv = dPreV^T h, d Wq2 = dPreQ^T U1, d Wq0 = dPre1^T h, d W1 = sum_b dPRE_b^T X_b (pure_window.hip)
//  16-17  pw_reduce_kernel         the twelve partial buffers in index order into the gradient views
//  18  mhimx_optim_step            Adam (update = 1)
// No floating-point atomics, no workgroup waits for another, every sum has a fixed order.  What is written per bag depends on that bag's
// N, seed and the tick alone.
#include <math.h>
#include <string.h>

#include "infer_tab.hpp"

namespace mhimx {

namespace {

constexpr int DW_Q = 128, DW_MAXC = 16, DW_ROWS = RG_ROWS, DW_T = RG_T;
constexpr int DW_ULD = DW_Q + 4;                                 // pitch of a [32][128] tile in LDS
constexpr float DW_SCALE = 0.08838834764831845f;                 // 1 / sqrt(128)
constexpr size_t DW_R1_SMEM = (size_t)(DW_ROWS * RG_LD + DW_MAXC * DW_Q + DW_ROWS * DW_ULD + 2 * DW_ROWS * DW_MAXC) * sizeof(float);
constexpr size_t DW_R2_SMEM = (size_t)(DW_ROWS * RG_LD) * sizeof(float);
static_assert(3 * DW_ROWS * DW_ULD <= DW_ROWS * RG_LD, "U1, d PreQ and d Pre1 tiles reuse the feature tile's LDS");

struct DwLabels { const int64_t* p[MHIMX_INFER_MAX]; };

// ------------------------------------------------------------------------------------------------ 7. merge + fcc + mix + CE + head gradients
// blockIdx.x = bag; thread e = column e.  The forward half is dsmil_finalize_kernel's y = 0 plane (same order of every sum).
__global__ __launch_bounds__(RG_FIN_T) void dw_head_kernel(InferTab tab, DwLabels lab, const float* __restrict__ pm, const float* __restrict__ pl,
                                                         const float* __restrict__ pB, const float* __restrict__ H,
                                                         const float* __restrict__ wfcc, const float* __restrict__ bfcc,
                                                         const float* __restrict__ logits_ins, const int64_t* __restrict__ crit, int C,
                                                         float main_alpha, float inv_n, float* __restrict__ logits_bag,
                                                         float* __restrict__ logits, float* __restrict__ losses, float* __restrict__ B_out,
                                                         float* __restrict__ stats, float* __restrict__ gli, float* __restrict__ dB,
                                                         float* __restrict__ delta, float* __restrict__ dwfcc_part,
                                                         float* __restrict__ dbfcc_part, float* __restrict__ dwi_part,
                                                         float* __restrict__ dbi_part) {
  __shared__ float red[8];
  __shared__ float wgt[RG_FIN_T];
  __shared__ float smx[DW_MAXC], sinv[DW_MAXC], lg[DW_MAXC], gl[DW_MAXC];
  __shared__ float dl[DW_MAXC][8];
  __shared__ __attribute__((aligned(16))) float big[DW_MAXC * IE];   // B [C][512]
  const int bag = blockIdx.x;
  RG_BAG(bag)
  const int64_t* label = lab.p[0];
  RG_PICK(label, lab.p, bag)
  const int G = rg_parts(N);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  pm += (int64_t)p0 * DW_MAXC; pl += (int64_t)p0 * DW_MAXC; pB += (int64_t)p0 * C * IE;
  for (int c = 0; c < C; ++c) {
    float mx, Ls;
    rg_merge_stats(pm + c, pl + c, G, DW_MAXC, red, mx, Ls);
    if (tid == 0) {
      smx[c] = mx; sinv[c] = 1.f / Ls;
      stats[((int64_t)bag * DW_MAXC + c) * 2] = mx;
      stats[((int64_t)bag * DW_MAXC + c) * 2 + 1] = 1.f / Ls;
    }
    __syncthreads();
  }
  for (int c = 0; c < C; ++c) {
    const float mx = smx[c];
    float acc = 0.f;                                            // column tid of B[c]
    for (int base = 0; base < G; base += RG_FIN_T) {
      __syncthreads();
      wgt[tid] = base + tid < G ? __expf(pm[(int64_t)(base + tid) * DW_MAXC + c] - mx) : 0.f;
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
  if (tid == 0) {
    // torch.nn.CrossEntropyLoss on one row (a label outside [0, C): NaN, where torch raises); g_lb = g_li = 0.5 g_logits
    float cm = lg[0];
    for (int c = 1; c < C; ++c) cm = fmaxf(cm, lg[c]);
    float den = 0.f;
    for (int c = 0; c < C; ++c) den += expf(lg[c] - cm);
    const int64_t y = label[0];
    const bool ok = y >= 0 && y < C;
    const float ce = ok ? (cm + logf(den)) - lg[ok ? y : 0] : NAN;
    losses[3 * bag] = main_alpha * ce;
    losses[3 * bag + 1] = ce;
    losses[3 * bag + 2] = 0.f;
    for (int c = 0; c < DW_MAXC; ++c) {
      const float g = c < C ? (ok ? 0.5f * (main_alpha * (expf(lg[c] - cm) / den - (c == y ? 1.f : 0.f)) * inv_n) : NAN) : 0.f;
      gl[c] = g;
      gli[(int64_t)bag * DW_MAXC + c] = g;
      if (c < C) { dbfcc_part[(int64_t)bag * C + c] = g; dbi_part[(int64_t)bag * C + c] = g; }
    }
  }
  __syncthreads();
  for (int c = 0; c < C; ++c) {
    const float b = big[c * IE + tid];
    float db = 0.f;
    for (int o = 0; o < C; ++o) {
      db = fmaf(wfcc[((int64_t)o * C + c) * IE + tid], gl[o], db);
      dwfcc_part[(((int64_t)bag * C + o) * C + c) * IE + tid] = gl[o] * b;
    }
    dB[((int64_t)bag * DW_MAXC + c) * IE + tid] = db;
    int64_t cr = crit[(int64_t)bag * C + c];
    if (cr < 0 || cr >= N) cr = 0;                              // (a class whose logits are all NaN has no critical row)
    dwi_part[((int64_t)bag * C + c) * IE + tid] = gl[c] * H[(orow0 + cr) * IE + tid];
    const float d = wave_sum(db * b);
    if (lane == 0) dl[c][wave] = d;
  }
  __syncthreads();
  if (tid < DW_MAXC) {
    float t = 0.f;
    if (tid < C) {
#pragma unroll
      for (int w = 0; w < 8; ++w) t += dl[tid][w];
    }
    delta[(int64_t)bag * DW_MAXC + tid] = t;
  }
}

// ------------------------------------------------------------------------------------------------ 8. rows pass 1
// blockIdx.x = 32-row tile of the row space (inside ONE bag).  Threads (row = tid >> 3, seg = tid & 7): 8 lanes per row for the two row dots
// (scores against q_max, V against d B), added in a fixed xor tree; then thread t owns columns t, t + 256 of d PreV and column t & 127,
// classes 8 (t >> 7) .. + 8 of the tile's d q_max partial.
__global__ __launch_bounds__(DW_T) void dw_rows1_kernel(InferTab tab, float* __restrict__ V, const float* __restrict__ Q, const float* __restrict__ qmax,
                                                      const float* __restrict__ stats, const float* __restrict__ dB, const float* __restrict__ delta,
                                                      int C, float* __restrict__ da_out, float* __restrict__ dbv_part, float* __restrict__ dqm_part) {
  extern __shared__ __attribute__((aligned(16))) float dw_sm[];
  float* Vs = dw_sm;                            // [32][516]
  float* qs = Vs + DW_ROWS * RG_LD;             // [16][128] q_max of the bag (classes past C: zeros)
  float* Qs = qs + DW_MAXC * DW_Q;              // [32][132]
  float* As = Qs + DW_ROWS * DW_ULD;            // [32][16] softmax weights
  float* das = As + DW_ROWS * DW_MAXC;          // [32][16] d a
  const int tile = blockIdx.x;
  const int64_t r0 = (int64_t)tile * DW_ROWS;
  RG_FIND_BAG(r0, row0)
  int64_t N = tab.N[0], orow0 = tab.row0[0];
  RG_PICK(N, tab.N, bag) RG_PICK(orow0, tab.row0, bag)
  const int64_t left = N - (r0 - orow0);
  const int M = left < DW_ROWS ? (int)left : DW_ROWS;           // real rows of the tile (>= 1)
  const int tid = threadIdx.x;
  float* Vt = V + r0 * IE;
  const float* Qt = Q + r0 * DW_Q;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int f = tid + DW_T * i, r = f >> 7, c4 = f & 127;
    f32x4 v = reinterpret_cast<const f32x4*>(Vt + (int64_t)(r < M ? r : M - 1) * IE)[c4];
    if (r >= M) v = f32x4{0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(Vs + r * RG_LD + 4 * c4) = v;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int f = tid + DW_T * i, r = f >> 5, c4 = f & 31;
    f32x4 v = reinterpret_cast<const f32x4*>(Qt + (int64_t)(r < M ? r : M - 1) * DW_Q)[c4];
    if (r >= M) v = f32x4{0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(Qs + r * DW_ULD + 4 * c4) = v;
  }
  for (int i = tid; i < DW_MAXC * DW_Q; i += DW_T) qs[i] = (i >> 7) < C ? qmax[(int64_t)bag * DW_MAXC * DW_Q + i] : 0.f;
  __syncthreads();
  {
    const int row = tid >> 3, seg = tid & 7;
    float a[DW_MAXC], dA[DW_MAXC];
#pragma unroll
    for (int c = 0; c < DW_MAXC; ++c) { a[c] = 0.f; dA[c] = 0.f; }
    const f32x4* qr = reinterpret_cast<const f32x4*>(Qs + row * DW_ULD);
#pragma unroll
    for (int g = 0; g < DW_Q / 32; ++g) {
      const f32x4 q = qr[seg + 8 * g];
#pragma unroll
      for (int c = 0; c < DW_MAXC; ++c)
        if (c < C) {
          const f32x4 w = reinterpret_cast<const f32x4*>(qs + c * DW_Q)[seg + 8 * g];
          a[c] = fmaf(q[3], w[3], fmaf(q[2], w[2], fmaf(q[1], w[1], fmaf(q[0], w[0], a[c]))));
        }
    }
    const f32x4* vr = reinterpret_cast<const f32x4*>(Vs + row * RG_LD);
    const f32x4* d4 = reinterpret_cast<const f32x4*>(dB + (int64_t)bag * DW_MAXC * IE);
#pragma unroll 2
    for (int g = 0; g < IE / 32; ++g) {
      const f32x4 v = vr[seg + 8 * g];
#pragma unroll
      for (int c = 0; c < DW_MAXC; ++c)
        if (c < C) {
          const f32x4 w = d4[c * (IE / 4) + seg + 8 * g];
          dA[c] = fmaf(v[3], w[3], fmaf(v[2], w[2], fmaf(v[1], w[1], fmaf(v[0], w[0], dA[c]))));
        }
    }
    const bool live = row < M;
#pragma unroll
    for (int c = 0; c < DW_MAXC; ++c) {
      a[c] += __shfl_xor(a[c], 1);   a[c] += __shfl_xor(a[c], 2);   a[c] += __shfl_xor(a[c], 4);
      dA[c] += __shfl_xor(dA[c], 1); dA[c] += __shfl_xor(dA[c], 2); dA[c] += __shfl_xor(dA[c], 4);
      float Av = 0.f, dav = 0.f;
      if (c < C && live) {
        const float mx = stats[((int64_t)bag * DW_MAXC + c) * 2], inv = stats[((int64_t)bag * DW_MAXC + c) * 2 + 1];
        Av = __expf(a[c] * DW_SCALE - mx) * inv;
        dav = Av * (dA[c] - delta[(int64_t)bag * DW_MAXC + c]);
      }
      a[c] = Av;
      dA[c] = dav;
    }
    if (seg == 0) {
      f32x4* oa = reinterpret_cast<f32x4*>(As + row * DW_MAXC);
      f32x4* od = reinterpret_cast<f32x4*>(das + row * DW_MAXC);
      f32x4* og = reinterpret_cast<f32x4*>(da_out + (r0 + row) * DW_MAXC);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        oa[q] = f32x4{a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]};
        const f32x4 d = f32x4{dA[4 * q], dA[4 * q + 1], dA[4 * q + 2], dA[4 * q + 3]};
        od[q] = d;
        og[q] = d;
      }
    }
  }
  __syncthreads();
  // ---- d PreV[r][e] = [V > 0] sum_c A[r][c] d B[c][e], over V in place (zero rows past the bag's N); the tile's column sums
  {
    float b0[DW_MAXC], b1[DW_MAXC];
#pragma unroll
    for (int c = 0; c < DW_MAXC; ++c) {
      b0[c] = c < C ? dB[((int64_t)bag * DW_MAXC + c) * IE + tid] : 0.f;
      b1[c] = c < C ? dB[((int64_t)bag * DW_MAXC + c) * IE + tid + DW_T] : 0.f;
    }
    float s0 = 0.f, s1 = 0.f;
#pragma unroll 4
    for (int r = 0; r < DW_ROWS; ++r) {
      float d0 = 0.f, d1 = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 p = reinterpret_cast<const f32x4*>(As + r * DW_MAXC)[q];
#pragma unroll
        for (int j = 0; j < 4; ++j) { d0 = fmaf(p[j], b0[4 * q + j], d0); d1 = fmaf(p[j], b1[4 * q + j], d1); }
      }
      if (!(r < M && Vs[r * RG_LD + tid] > 0.f)) d0 = 0.f;
      if (!(r < M && Vs[r * RG_LD + tid + DW_T] > 0.f)) d1 = 0.f;
      Vt[(int64_t)r * IE + tid] = d0;
      Vt[(int64_t)r * IE + tid + DW_T] = d1;
      s0 += d0;
      s1 += d1;
    }
    dbv_part[(int64_t)tile * IE + tid] = s0;
    dbv_part[(int64_t)tile * IE + tid + DW_T] = s1;
  }
  // ---- the tile's d q_max[c][j] = s sum_r d a[r][c] Q[r][j], rows in index order
  {
    const int j = tid & (DW_Q - 1), c0 = 8 * (tid >> 7);
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
    for (int r = 0; r < DW_ROWS; ++r) {
      const float q = Qs[r * DW_ULD + j];
      const f32x4 d0 = *reinterpret_cast<const f32x4*>(das + r * DW_MAXC + c0), d1 = *reinterpret_cast<const f32x4*>(das + r * DW_MAXC + c0 + 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) { acc[k] = fmaf(d0[k], q, acc[k]); acc[4 + k] = fmaf(d1[k], q, acc[4 + k]); }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) dqm_part[((int64_t)tile * DW_MAXC + c0 + k) * DW_Q + j] = acc[k] * DW_SCALE;
  }
}

// ------------------------------------------------------------------------------------------------ 10. d q_max of every bag
// grid (bag, 4): element i = 512 blockIdx.y + tid of [16][128]; the bag's tiles in index order
__global__ __launch_bounds__(RG_FIN_T) void dw_dqmax_kernel(InferTab tab, const float* __restrict__ dqm_part, float* __restrict__ dqmax) {
  const int bag = blockIdx.x;
  RG_BAG(bag)
  const int i = blockIdx.y * RG_FIN_T + threadIdx.x;
  const int64_t t0 = orow0 / DW_ROWS, nt = (N + DW_ROWS - 1) / DW_ROWS;
  const float* p = dqm_part + t0 * (DW_MAXC * DW_Q) + i;
  float a = 0.f;
#pragma unroll 4
  for (int64_t t = 0; t < nt; ++t) a += p[t * (DW_MAXC * DW_Q)];
  dqmax[(int64_t)bag * DW_MAXC * DW_Q + i] = a;
}

// ------------------------------------------------------------------------------------------------ 11. rows pass 2
// blockIdx.x = 32-row tile.  Wave w owns columns [32 w, 32 w + 32) of the three [32][128] tiles and column tiles 4 w .. 4 w + 3 of d h.
// PLAIN (mhimx_dsmil_mhim_window_run's token rows, which have no d out / d pre of their own): d h is written as it is, zero rows past
// the bag's N; dact and db1_part are not read or written.
template <bool PLAIN>
__global__ __launch_bounds__(DW_T) void dw_rows2_kernel(InferTab tab, const float* __restrict__ Hin, const _Float16* __restrict__ dact,
                                                      const float* __restrict__ Q, const float* __restrict__ da, const float* __restrict__ qmax,
                                                      const float* __restrict__ dqmax, const int64_t* __restrict__ crit,
                                                      const float* __restrict__ gli, const float* __restrict__ wi,
                                                      const float* __restrict__ q0_frag, const float* __restrict__ bq0,
                                                      const float* __restrict__ q2t_frag, const float* __restrict__ q0t_frag, int C,
                                                      float* __restrict__ dpre, float* __restrict__ U1out, float* __restrict__ dPQ,
                                                      float* __restrict__ dP1, float* __restrict__ db1_part, float* __restrict__ dbq0_part,
                                                      float* __restrict__ dbq2_part) {
  extern __shared__ __attribute__((aligned(16))) float dw_sm[];
  __shared__ __attribute__((aligned(16))) float das[DW_ROWS * DW_MAXC];
  __shared__ int crel[DW_MAXC];
  __shared__ float gls[DW_MAXC];
  float* Hs = dw_sm;                            // [32][516] feature rows; then the three [32][132] tiles
  float* Us = dw_sm;                            // U1
  float* Gs = Us + DW_ROWS * DW_ULD;            // d PreQ
  float* Ps = Gs + DW_ROWS * DW_ULD;            // d Pre1
  const int tile = blockIdx.x;
  const int64_t r0 = (int64_t)tile * DW_ROWS;
  RG_FIND_BAG(r0, row0)
  int64_t N = tab.N[0], orow0 = tab.row0[0];
  RG_PICK(N, tab.N, bag) RG_PICK(orow0, tab.row0, bag)
  const int64_t rin0 = r0 - orow0, left = N - rin0;
  const int M = left < DW_ROWS ? (int)left : DW_ROWS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r32 = lane & 31, kg = lane >> 5;
  const int n_col = 32 * wave + r32;
  const float* T = Hin + r0 * IE;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int f = tid + DW_T * i, r = f >> 7, c4 = f & 127;
    f32x4 v = reinterpret_cast<const f32x4*>(T + (int64_t)(r < M ? r : M - 1) * IE)[c4];
    if (r >= M) v = f32x4{0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(Hs + r * RG_LD + 4 * c4) = v;
  }
  das[tid] = da[r0 * DW_MAXC + tid];                            // [32][16] = 512 floats: two per thread
  das[tid + DW_T] = da[r0 * DW_MAXC + tid + DW_T];
  if (tid < DW_MAXC) {
    // the critical row of class tid relative to this tile (outside [0, 32): not here)
    const int64_t rel = tid < C ? crit[(int64_t)bag * C + tid] - rin0 : -1;
    crel[tid] = (rel >= 0 && rel < DW_ROWS) ? (int)rel : -1;
    gls[tid] = gli[(int64_t)bag * DW_MAXC + tid];
  }
  __syncthreads();
  // ---- d PreQ[r][j] of rows 16 (tid >> 7) .. + 16, column j = tid & 127 (kept in registers until the feature tile is dead)
  float gq[16];
  {
    const int j = tid & (DW_Q - 1), rh = 16 * (tid >> 7);
    float qm[DW_MAXC], dq[DW_MAXC];
#pragma unroll
    for (int c = 0; c < DW_MAXC; ++c) {
      qm[c] = c < C ? qmax[((int64_t)bag * DW_MAXC + c) * DW_Q + j] : 0.f;
      dq[c] = c < C ? dqmax[((int64_t)bag * DW_MAXC + c) * DW_Q + j] : 0.f;
    }
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
      const int r = rh + rr;
      float g = 0.f;
      if (r < M) {
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < DW_MAXC; ++c) d = fmaf(das[r * DW_MAXC + c], qm[c], d);
        d *= DW_SCALE;
#pragma unroll
        for (int c = 0; c < DW_MAXC; ++c)
          if (crel[c] == r) d += dq[c];
        const float q = Q[(r0 + r) * DW_Q + j];
        g = d * (1.f - q * q);
      }
      gq[rr] = g;
    }
  }
  // ---- U1 tile on the matrix cores
  const f32x16 u1 = rg_mma3<IE>(Hs + r32 * RG_LD + 8 * kg, reinterpret_cast<const f32x4*>(q0_frag + ((int64_t)wave * (IE / 16) * 64 + lane) * 8));
  __syncthreads();                              // every read of the feature tile is done
  {
    const float b0 = bq0[n_col];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = 8 * (i >> 2) + 4 * kg + (i & 3);
      const float u = u1[i] + b0;
      const float v = (row < M && u > 0.f) ? u : 0.f;
      Us[row * DW_ULD + n_col] = v;
      U1out[(r0 + row) * DW_Q + n_col] = v;
    }
    const int j = tid & (DW_Q - 1), rh = 16 * (tid >> 7);
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
      Gs[(rh + rr) * DW_ULD + j] = gq[rr];
      dPQ[(r0 + rh + rr) * DW_Q + j] = gq[rr];
    }
  }
  __syncthreads();
  if (tid < DW_Q) {
    float t = 0.f;
    for (int r = 0; r < DW_ROWS; ++r) t += Gs[r * DW_ULD + tid];
    dbq2_part[(int64_t)tile * DW_Q + tid] = t;
  }
  // ---- d Pre1 = (d PreQ Wq2) [U1 > 0], K = 128
  {
    const f32x16 p1 = rg_mma3<DW_Q>(Gs + r32 * DW_ULD + 8 * kg, reinterpret_cast<const f32x4*>(q2t_frag + ((int64_t)wave * (DW_Q / 16) * 64 + lane) * 8));
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = 8 * (i >> 2) + 4 * kg + (i & 3);
      const float v = Us[row * DW_ULD + n_col] > 0.f ? p1[i] : 0.f;
      Ps[row * DW_ULD + n_col] = v;
      dP1[(r0 + row) * DW_Q + n_col] = v;
    }
  }
  __syncthreads();
  if (tid < DW_Q) {
    float t = 0.f;
    for (int r = 0; r < DW_ROWS; ++r) t += Ps[r * DW_ULD + tid];
    dbq0_part[(int64_t)tile * DW_Q + tid] = t;
  }
  // ---- d h = d Pre1 Wq0 (K = 128) + the d PreV Wv rows + g_li Wi on the critical rows; dPRE = d h * d out / d pre; column sums
  [[maybe_unused]] const _Float16* db = dact + r0 * IE;
  float* po = dpre + r0 * IE;
#pragma unroll 1
  for (int q = 0; q < 4; ++q) {
    const int nt = 4 * wave + q, col = 32 * nt + r32;
    const f32x16 acc = rg_mma3<DW_Q>(Ps + r32 * DW_ULD + 8 * kg, reinterpret_cast<const f32x4*>(q0t_frag + ((int64_t)nt * (DW_Q / 16) * 64 + lane) * 8));
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = 8 * (i >> 2) + 4 * kg + (i & 3);
      float d = 0.f;
      if (row < M) {
        float v = acc[i] + po[(int64_t)row * IE + col];
        for (int c = 0; c < C; ++c)
          if (crel[c] == row) v = fmaf(gls[c], wi[(int64_t)c * IE + col], v);
        if constexpr (PLAIN) d = v;
        else d = v * (float)db[(int64_t)row * IE + col];
      }
      po[(int64_t)row * IE + col] = d;
      s += d;
    }
    if constexpr (!PLAIN) {
      s += __shfl_xor(s, 32, 64);
      if (kg == 0) db1_part[(int64_t)tile * IE + col] = s;
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
struct DwLay {
  int64_t w1p, vp, vtp, q0f, q2f, q2tf, q0tf, logits, losses, logits_bag, logits_ins, B, crit, qmax, stats, gli, dB, delta, dqmax, dwfcc_part,
      dbfcc_part, dwi_part, dbi_part, H, dact, V, Q, cls, da, dhv, U1, dPQ, dP1, pmax, parg, pm, pl, pB, db1_part, dbv_part, dbq0_part, dbq2_part,
      dqm_part, slab_1, slab_v, slab_q0, slab_q2, total;
  int64_t rows;
  int32_t steps, s1, s1_per, sv, sv_per, sq0, sq0_per, sq2, sq2_per;
};

int check_dw(const mhimx_dsmil_train_cfg* c, int32_t n_bags, const mhimx_pure_window_bag* bags, int32_t xdt = MHIMX_X_F32) {
  if (int r = rg_check_xdt("dsmil_window", xdt)) return r;
  MHIMX_CHECK_ARG(c && bags, "dsmil_window: null configuration / bag list");
  MHIMX_CHECK_ARG(n_bags >= 1 && n_bags <= MHIMX_DSMIL_WINDOW_MAX, "dsmil_window: 1..%d bags per window (got %d)", MHIMX_DSMIL_WINDOW_MAX, n_bags);
  MHIMX_CHECK_ARG(c->E == IE && c->C >= 1 && c->C <= DW_MAXC && c->D > 0 && c->D % 256 == 0 && c->D <= (1 << 20),
                  "dsmil_window: shapes outside the ragged DSMIL window (E = 512, q width 128, 1 <= C <= %d, D %% 256 == 0)", DW_MAXC);
  MHIMX_CHECK_ARG(c->act >= MHIMX_ACT_NONE && c->act <= MHIMX_ACT_TANH, "dsmil_window: unknown activation");
  MHIMX_CHECK_ARG(c->drop_p >= 0.f && c->drop_p < 1.f, "dsmil_window: dropout probability outside [0,1)");
  const mhimx_dsmil_params& p = c->param;
  MHIMX_CHECK_ARG(p.w1 && p.b1 && p.wi && p.bi && p.wq0 && p.bq0 && p.wq2 && p.bq2 && p.wv && p.bv && p.wfcc && p.bfcc, "dsmil_window: null parameter");
  MHIMX_CHECK_ARG(aligned16(p.w1) && aligned16(p.b1) && aligned16(p.wi) && aligned16(p.wq0) && aligned16(p.wq2) && aligned16(p.wv) && aligned16(p.bv),
                  "dsmil_window: the feature, i_classifier, q and v weights must be 16-byte aligned");
  const mhimx_dsmil_grads& g = c->grad;
  MHIMX_CHECK_ARG(g.w1 && g.b1 && g.wi && g.bi && g.wq0 && g.bq0 && g.wq2 && g.bq2 && g.wv && g.bv && g.wfcc && g.bfcc, "dsmil_window: null gradient view");
  MHIMX_CHECK_ARG(c->tick, "dsmil_window: the device dropout counter (tick) is required");
  int64_t rows = 0;
  for (int b = 0; b < n_bags; ++b) {
    if (int r = rg_check_bag("dsmil_window", b, bags[b].N, bags[b].ldx, c->D, xdt, RgRules{MHIMX_STEP_MAX_ROWS, true})) return r;
    rows += align_up(bags[b].N, DW_ROWS);
  }
  MHIMX_CHECK_ARG(rows <= MHIMX_DSMIL_WINDOW_MAX_ROWS, "dsmil_window: %lld rows in the window's row space, at most %d", (long long)rows,
                  MHIMX_DSMIL_WINDOW_MAX_ROWS);
  return 0;
}

void dw_layout(const mhimx_dsmil_train_cfg* c, int32_t n_bags, const mhimx_pure_window_bag* bags, DwLay* w, InferTab* tab, int64_t* row0_out) {
  RgCount cnt;
  for (int b = 0; b < n_bags; ++b) {
    if (row0_out) row0_out[b] = cnt.rows;
    rg_tab_add(tab, cnt, b, bags[b].X, bags[b].ldx, bags[b].N, align_up(bags[b].N, DW_ROWS));
  }
  rg_tab_close(tab, cnt, n_bags);
  const int64_t rows = cnt.rows, parts = cnt.parts;
  const int64_t E = c->E, D = c->D, C = c->C, n = n_bags;
  w->rows = rows;
  w->steps = (int32_t)(rows / DW_ROWS);
  // split-K slabs: enough workgroups to fill the part (4 D / 128 output tiles for d W1, 16 for d Wv, 4 for d Wq0, 1 for d Wq2), never an empty slab
  const int s1_room = pw_split_k(w->steps, 8, 8, &w->s1, &w->s1_per);
  const int sv_room = pw_split_k(w->steps, 16, 4, &w->sv, &w->sv_per);
  const int sq0_room = pw_split_k(w->steps, 64, 4, &w->sq0, &w->sq0_per);
  const int sq2_room = pw_split_k(w->steps, 64, 2, &w->sq2, &w->sq2_per);
  Arena ar(nullptr, 0);
  w->w1p = ar.off; ar.take<float>(E * D);
  w->vp = ar.off; ar.take<float>(E * E);
  w->vtp = ar.off; ar.take<float>(E * E);
  w->q0f = ar.off; ar.take<float>(DW_Q * E);
  w->q2f = ar.off; ar.take<float>(DW_Q * DW_Q);
  w->q2tf = ar.off; ar.take<float>(DW_Q * DW_Q);
  w->q0tf = ar.off; ar.take<float>(DW_Q * E);
  w->logits = ar.off; ar.take<float>(n * C);
  w->losses = ar.off; ar.take<float>(n * 3);
  w->logits_bag = ar.off; ar.take<float>(n * C);
  w->logits_ins = ar.off; ar.take<float>(n * C);
  w->B = ar.off; ar.take<float>(n * C * E);
  w->crit = ar.off; ar.take<int64_t>(n * C);
  w->qmax = ar.off; ar.take<float>(n * DW_MAXC * DW_Q);
  w->stats = ar.off; ar.take<float>(n * DW_MAXC * 2);
  w->gli = ar.off; ar.take<float>(n * DW_MAXC);
  w->dB = ar.off; ar.take<float>(n * DW_MAXC * E);
  w->delta = ar.off; ar.take<float>(n * DW_MAXC);
  w->dqmax = ar.off; ar.take<float>(n * DW_MAXC * DW_Q);
  w->dwfcc_part = ar.off; ar.take<float>(n * C * C * E);
  w->dbfcc_part = ar.off; ar.take<float>(n * C);
  w->dwi_part = ar.off; ar.take<float>(n * C * E);
  w->dbi_part = ar.off; ar.take<float>(n * C);
  w->H = ar.off; ar.take<float>(rows * E);
  w->dact = ar.off; ar.take<_Float16>(rows * E);
  w->V = ar.off; ar.take<float>(rows * E);
  w->Q = ar.off; ar.take<float>(rows * DW_Q);
  w->cls = ar.off; ar.take<float>(rows * DW_MAXC);
  w->da = ar.off; ar.take<float>(rows * DW_MAXC);
  w->dhv = ar.off; ar.take<float>(rows * E);
  w->U1 = ar.off; ar.take<float>(rows * DW_Q);
  w->dPQ = ar.off; ar.take<float>(rows * DW_Q);
  w->dP1 = ar.off; ar.take<float>(rows * DW_Q);
  w->pmax = ar.off; ar.take<float>(parts * DW_MAXC);
  w->parg = ar.off; ar.take<int32_t>(parts * DW_MAXC);
  w->pm = ar.off; ar.take<float>(parts * DW_MAXC);
  w->pl = ar.off; ar.take<float>(parts * DW_MAXC);
  w->pB = ar.off; ar.take<float>(parts * C * E);
  w->db1_part = ar.off; ar.take<float>((int64_t)w->steps * E);
  w->dbv_part = ar.off; ar.take<float>((int64_t)w->steps * E);
  w->dbq0_part = ar.off; ar.take<float>((int64_t)w->steps * DW_Q);
  w->dbq2_part = ar.off; ar.take<float>((int64_t)w->steps * DW_Q);
  w->dqm_part = ar.off; ar.take<float>((int64_t)w->steps * DW_MAXC * DW_Q);
  w->slab_1 = ar.off; ar.take<float>((int64_t)s1_room * E * D);
  w->slab_v = ar.off; ar.take<float>((int64_t)sv_room * E * E);
  w->slab_q0 = ar.off; ar.take<float>((int64_t)sq0_room * DW_Q * E);
  w->slab_q2 = ar.off; ar.take<float>((int64_t)sq2_room * DW_Q * DW_Q);
  w->total = ar.off;
}

}  // namespace

// launches 8, 10 and 11 as host calls (infer_tab.hpp): mhimx_dsmil_window_run below and mhimx_dsmil_mhim_window_run (dsmil_mhim.hip)
int dw_rows1(hipStream_t st, const InferTab& tab, int steps, float* V, const float* Q, const float* qmax, const float* stats, const float* dB,
             const float* delta, int C, float* da, float* dbv_part, float* dqm_part) {
  MHIMX_ONCE_PER_DEVICE(MHIMX_HIP(hipFuncSetAttribute((const void*)dw_rows1_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DW_R1_SMEM)));
  hipLaunchKernelGGL(dw_rows1_kernel, dim3((unsigned)steps), dim3(DW_T), DW_R1_SMEM, st, tab, V, Q, qmax, stats, dB, delta, C, da, dbv_part, dqm_part);
  MHIMX_LAUNCH_CHECK();
  return 0;
}

int dw_dqmax(hipStream_t st, const InferTab& tab, const float* dqm_part, float* dqmax) {
  hipLaunchKernelGGL(dw_dqmax_kernel, dim3((unsigned)tab.n, DW_MAXC * DW_Q / RG_FIN_T), dim3(RG_FIN_T), 0, st, tab, dqm_part, dqmax);
  MHIMX_LAUNCH_CHECK();
  return 0;
}

int dw_rows2_plain(hipStream_t st, const InferTab& tab, int steps, const float* Hin, const float* Q, const float* da, const float* qmax,
                   const float* dqmax, const int64_t* crit, const float* gli, const float* wi, const float* q0f, const float* bq0, const float* q2tf,
                   const float* q0tf, int C, float* dhv, float* U1, float* dPQ, float* dP1, float* dbq0_part, float* dbq2_part) {
  MHIMX_ONCE_PER_DEVICE(MHIMX_HIP(hipFuncSetAttribute((const void*)dw_rows2_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DW_R2_SMEM)));
  const _Float16* no_dact = nullptr;
  float* no_db1 = nullptr;
  hipLaunchKernelGGL(dw_rows2_kernel<true>, dim3((unsigned)steps), dim3(DW_T), DW_R2_SMEM, st, tab, Hin, no_dact, Q, da, qmax, dqmax, crit, gli, wi, q0f,
                     bq0, q2tf, q0tf, C, dhv, U1, dPQ, dP1, no_db1, dbq0_part, dbq2_part);
  MHIMX_LAUNCH_CHECK();
  return 0;
}

}  // namespace mhimx

extern "C" int mhimx_dsmil_window_layout_of(const mhimx_dsmil_train_cfg* cfg, int32_t n_bags, const mhimx_pure_window_bag* bags,
                                            mhimx_dsmil_window_layout* out) {
  using namespace mhimx;
  MHIMX_CHECK_ARG(out, "dsmil_window_layout: null output");
  if (int r = check_dw(cfg, n_bags, bags)) return r;
  DwLay w;
  memset(out, 0, sizeof(*out));
  dw_layout(cfg, n_bags, bags, &w, nullptr, out->row0);
  out->total = w.total; out->rows = w.rows; out->logits = w.logits; out->losses = w.losses; out->logits_bag = w.logits_bag;
  out->logits_ins = w.logits_ins; out->B = w.B; out->crit = w.crit; out->H = w.H; out->dact = w.dact;
  return 0;
}

extern "C" int mhimx_dsmil_window_run(void* stream, const mhimx_dsmil_train_cfg* cfg, int32_t n_bags, const mhimx_pure_window_bag* bags,
                                      int64_t host_step, void* ws, int64_t ws_bytes, int32_t update, int32_t x_dtype) {
  using namespace mhimx;
  if (int r = check_dw(cfg, n_bags, bags, x_dtype)) return r;
  for (int b = 0; b < n_bags; ++b) {
    MHIMX_CHECK_ARG(bags[b].X && aligned16(bags[b].X), "dsmil_window: bag %d: null or unaligned rows", b);
    MHIMX_CHECK_ARG(bags[b].label_dev, "dsmil_window: bag %d: null label", b);
  }
  MHIMX_CHECK_ARG(!update || (cfg->p && cfg->g && cfg->m && cfg->v && cfg->n_train > 0 && cfg->n_all >= cfg->n_train),
                  "dsmil_window: update needs the flat optimiser buffers");
  DwLay w;
  InferTab tab = {};
  dw_layout(cfg, n_bags, bags, &w, &tab, nullptr);
  tab.pad = x_dtype;                           // read by the two launches that read X: the projection (2) and d W1 (15)
  if (int r = rg_check_ws("dsmil_window", ws, ws_bytes, w.total)) return r;
  const mhimx_dsmil_train_cfg& c = *cfg;
  const mhimx_dsmil_params& P = c.param;
  hipStream_t st = (hipStream_t)stream;
  char* base = static_cast<char*>(ws);
  auto F = [&](int64_t off) { return reinterpret_cast<float*>(base + off); };
  const int D = (int)c.D, C = (int)c.C;
  float *H = F(w.H), *V = F(w.V), *Q = F(w.Q), *dhv = F(w.dhv);
  _Float16* dact = reinterpret_cast<_Float16*>(base + w.dact);
  int64_t* crit = reinterpret_cast<int64_t*>(base + w.crit);

  // ---- 1. counters and weight images
  {
    mhimx_prep_job jobs[9];
    int n = 0;
    jobs[n++] = mhimx_prep_job{3, nullptr, reinterpret_cast<float*>(c.tick), 1, 1};
    if (c.opt_step) jobs[n++] = mhimx_prep_job{3, nullptr, reinterpret_cast<float*>(c.opt_step), 1, 1};
    jobs[n++] = mhimx_prep_job{1, P.w1, F(w.w1p), c.E, c.D};
    jobs[n++] = mhimx_prep_job{1, P.wv, F(w.vp), c.E, c.E};
    jobs[n++] = mhimx_prep_job{7, P.wv, F(w.vtp), c.E, c.E};
    jobs[n++] = mhimx_prep_job{4, P.wq0, F(w.q0f), DW_Q, c.E};
    jobs[n++] = mhimx_prep_job{4, P.wq2, F(w.q2f), DW_Q, DW_Q};
    jobs[n++] = mhimx_prep_job{5, P.wq2, F(w.q2tf), DW_Q, DW_Q};
    jobs[n++] = mhimx_prep_job{5, P.wq0, F(w.q0tf), DW_Q, c.E};
    if (int r = mhimx_prep_batch(stream, jobs, n)) return r;
  }
  // ---- 2. feature rows, dropout, d out / d pre of every bag
  {
    PureWinDrop dr = {};
    for (int b = 0; b < n_bags; ++b) dr.seed[b] = bags[b].drop_seed;
    dr.tick = c.tick; dr.dact = dact; dr.drop_p = c.drop_p;
    if (int r = pure_window_project_elem(st, tab, dr, D, F(w.w1p), P.b1, c.act, H)) return r;
  }
  // ---- 3. V = relu(h Wv^T + bv): the eval projection over the feature rows as fp32 "bags" of pitch 512
  InferTab tabv = tab;
  for (int b = 0; b < n_bags; ++b) { tabv.X[b] = H + tab.row0[b] * IE; tabv.ldx[b] = IE; }
  tabv.pad = MHIMX_X_F32;
  if (int r = infer_project(st, tabv, IE, F(w.vp), P.bv, MHIMX_ACT_RELU, V)) return r;
  // ---- 4. - 6. Q, classes, critical rows, pool partials (infer_dsmil.hip)
  if (int r = dsmil_rows_crit_pool(st, tab, H, V, F(w.q0f), P.bq0, F(w.q2f), P.bq2, P.wi, P.bi, C, Q, F(w.cls), F(w.pmax),
                                   reinterpret_cast<int32_t*>(base + w.parg), F(w.qmax), F(w.logits_ins), crit, F(w.pm), F(w.pl), F(w.pB)))
    return r;
  // ---- 7. merge, fcc, mix, CE and the head gradients
  {
    DwLabels lab = {};
    for (int b = 0; b < n_bags; ++b) lab.p[b] = bags[b].label_dev;
    hipLaunchKernelGGL(dw_head_kernel, dim3((unsigned)n_bags), dim3(RG_FIN_T), 0, st, tab, lab, F(w.pm), F(w.pl), F(w.pB), H, P.wfcc, P.bfcc,
                       F(w.logits_ins), crit, C, c.main_alpha, 1.f / (float)n_bags, F(w.logits_bag), F(w.logits), F(w.losses), F(w.B), F(w.stats),
                       F(w.gli), F(w.dB), F(w.delta), F(w.dwfcc_part), F(w.dbfcc_part), F(w.dwi_part), F(w.dbi_part));
    MHIMX_LAUNCH_CHECK();
  }
  // ---- 8. rows pass 1
  if (int r = dw_rows1(st, tab, w.steps, V, Q, F(w.qmax), F(w.stats), F(w.dB), F(w.delta), C, F(w.da), F(w.dbv_part), F(w.dqm_part))) return r;
  // ---- 9. d PreV Wv: the eval projection on the d PreV rows with the paired image of Wv^T (no bias, no activation)
  for (int b = 0; b < n_bags; ++b) tabv.X[b] = V + tab.row0[b] * IE;
  if (int r = infer_project(st, tabv, IE, F(w.vtp), nullptr, MHIMX_ACT_NONE, dhv)) return r;
  // ---- 10. d q_max of every bag
  if (int r = dw_dqmax(st, tab, F(w.dqm_part), F(w.dqmax))) return r;
  // ---- 11. rows pass 2
  MHIMX_ONCE_PER_DEVICE(MHIMX_HIP(hipFuncSetAttribute((const void*)dw_rows2_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DW_R2_SMEM)));
  hipLaunchKernelGGL(dw_rows2_kernel<false>, dim3((unsigned)w.steps), dim3(DW_T), DW_R2_SMEM, st, tab, H, dact, Q, F(w.da), F(w.qmax), F(w.dqmax), crit, F(w.gli),
                     P.wi, F(w.q0f), P.bq0, F(w.q2tf), F(w.q0tf), C, dhv, F(w.U1), F(w.dPQ), F(w.dP1), F(w.db1_part), F(w.dbq0_part), F(w.dbq2_part));
  MHIMX_LAUNCH_CHECK();
  // ---- 12. - 15. the four weight gradients
  if (int r = pw_wgrad_rows(st, tab, V, IE, IE, H, IE, IE, w.steps, w.sv, w.sv_per, F(w.slab_v))) return r;
  if (int r = pw_wgrad_rows(st, tab, F(w.dPQ), DW_Q, DW_Q, F(w.U1), DW_Q, DW_Q, w.steps, w.sq2, w.sq2_per, F(w.slab_q2))) return r;
  if (int r = pw_wgrad_rows(st, tab, F(w.dP1), DW_Q, DW_Q, H, IE, IE, w.steps, w.sq0, w.sq0_per, F(w.slab_q0))) return r;
  if (int r = pw_wgrad_bagx(st, tab, dhv, D, w.steps, w.s1, w.s1_per, F(w.slab_1))) return r;
  // ---- 16., 17. the partial buffers, in index order, into the gradient views
  {
    const mhimx_dsmil_grads& G_ = c.grad;
    const float* parts[6] = {F(w.slab_1), F(w.slab_v), F(w.slab_q0), F(w.slab_q2), F(w.dwfcc_part), F(w.dwi_part)};
    const int32_t G[6] = {w.s1, w.sv, w.sq0, w.sq2, n_bags, n_bags};
    const int64_t W[6] = {(int64_t)c.E * c.D, (int64_t)c.E * c.E, (int64_t)DW_Q * c.E, (int64_t)DW_Q * DW_Q, (int64_t)C * C * c.E, (int64_t)C * c.E};
    float* out[6] = {G_.w1, G_.wv, G_.wq0, G_.wq2, G_.wfcc, G_.wi};
    if (int r = pw_reduce(st, 6, parts, G, W, out)) return r;
    const float* parts2[6] = {F(w.db1_part), F(w.dbv_part), F(w.dbq0_part), F(w.dbq2_part), F(w.dbfcc_part), F(w.dbi_part)};
    const int32_t G2[6] = {w.steps, w.steps, w.steps, w.steps, n_bags, n_bags};
    const int64_t W2[6] = {c.E, c.E, DW_Q, DW_Q, C, C};
    float* out2[6] = {G_.b1, G_.bv, G_.bq0, G_.bq2, G_.bfcc, G_.bi};
    if (int r = pw_reduce(st, 6, parts2, G2, W2, out2)) return r;
  }
  if (!update) return 0;
  // ---- 18. Adam
  mhimx_optim_args o = {};
  o.p = c.p; o.g = c.g; o.m = c.m; o.v = c.v; o.n_train = c.n_train; o.n_all = c.n_all; o.step = host_step; o.step_dev = c.opt_step;
  o.lr = c.lr; o.lr_table = c.lr_table; o.lr_len = c.lr_len; o.beta1 = c.beta1; o.beta2 = c.beta2; o.eps = c.eps; o.weight_decay = c.weight_decay;
  o.grad_scale = 1.f; o.zero_grad = 1;
  return mhimx_optim_step(stream, &o);
}
