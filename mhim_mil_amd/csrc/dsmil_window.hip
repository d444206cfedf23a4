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
//   7  ds_head_kernel<>            (dsmil_student.hpp) plane = bag: merge of the partials in index order -> B, fcc, the mix, CE; g_lb = g_li = 0.5 g_logits,
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
// The student from launch 3 on (but d W1, launch 15) is enqueued through dsmil_student.hpp's helpers, which are defined here and which
// mhimx_dsmil_mhim_window_run (dsmil_mhim.hip) enqueues over its token space.
#include <math.h>
#include <string.h>

#include "dsmil_student.hpp"

namespace mhimx {

namespace {

constexpr int DW_Q = DS_Q, DW_MAXC = DS_MAXC, DW_ROWS = RG_ROWS, DW_T = RG_T;
constexpr int DW_ULD = DW_Q + 4;                                 // pitch of a [32][128] tile in LDS
constexpr float DW_SCALE = 0.08838834764831845f;                 // 1 / sqrt(128)
constexpr size_t DW_R1_SMEM = (size_t)(DW_ROWS * RG_LD + DW_MAXC * DW_Q + DW_ROWS * DW_ULD + 2 * DW_ROWS * DW_MAXC) * sizeof(float);
constexpr size_t DW_R2_SMEM = (size_t)(DW_ROWS * RG_LD) * sizeof(float);
static_assert(3 * DW_ROWS * DW_ULD <= DW_ROWS * RG_LD, "U1, d PreQ and d Pre1 tiles reuse the feature tile's LDS");

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
  DsLay s;
  int64_t w1p, H, dact, db1_part, slab_1, total, rows;
  int32_t steps, s1, s1_per;
};

int check_dw(const mhimx_dsmil_train_cfg* c, int32_t n_bags, const mhimx_pure_window_bag* bags, int32_t xdt = MHIMX_X_F32) {
  if (int r = ds_check_base("dsmil_window", c, xdt, n_bags, MHIMX_DSMIL_WINDOW_MAX, bags, "")) return r;
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
  const int64_t rows = cnt.rows, E = c->E, D = c->D;
  w->rows = rows;
  w->steps = (int32_t)(rows / DW_ROWS);
  // d W1's split-K slabs: enough workgroups to fill the part (4 D / 128 output tiles), never an empty slab
  const int s1_room = pw_split_k(w->steps, 8, 8, &w->s1, &w->s1_per);
  Arena ar(nullptr, 0);
  w->w1p = ar.off; ar.take<float>(E * D);
  ds_take(ar, &w->s, n_bags, c->C, rows, cnt.parts, w->steps);
  w->H = ar.off; ar.take<float>(rows * E);
  w->dact = ar.off; ar.take<_Float16>(rows * E);
  w->db1_part = ar.off; ar.take<float>((int64_t)w->steps * E);
  w->slab_1 = ar.off; ar.take<float>((int64_t)s1_room * E * D);
  w->total = ar.off;
}

// the table of a launch that reads fp32 rows of pitch 512 of the row space as its "bags"
InferTab ds_rows_tab(const InferTab& tab, const float* rows) {
  InferTab t = tab;
  for (int b = 0; b < tab.n; ++b) { t.X[b] = rows + tab.row0[b] * IE; t.ldx[b] = IE; }
  t.pad = MHIMX_X_F32;
  return t;
}

// rows pass 2.  PLAIN: rows that have no d out / d pre of their own (a student's token rows): d h as it is over dhv in place, no feature-bias
// partials
template <bool PLAIN>
int dw_rows2(hipStream_t st, const InferTab& tab, char* base, const DsLay& s, const mhimx_dsmil_params& P, int C, const float* H, const _Float16* dact,
             float* db1_part) {
  auto F = [&](int64_t off) { return reinterpret_cast<float*>(base + off); };
  MHIMX_ONCE_PER_DEVICE(MHIMX_HIP(hipFuncSetAttribute((const void*)dw_rows2_kernel<PLAIN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DW_R2_SMEM)));
  hipLaunchKernelGGL(dw_rows2_kernel<PLAIN>, dim3((unsigned)s.steps), dim3(DW_T), DW_R2_SMEM, st, tab, H, dact, F(s.Q), F(s.da), F(s.qmax), F(s.dqmax),
                     reinterpret_cast<const int64_t*>(base + s.crit), F(s.gli), P.wi, F(s.q0f), P.bq0, F(s.q2tf), F(s.q0tf), C, F(s.dhv), F(s.U1), F(s.dPQ),
                     F(s.dP1), db1_part, F(s.dbq0_part), F(s.dbq2_part));
  MHIMX_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ host: dsmil_student.hpp's helpers
void ds_take(Arena& ar, DsLay* s, int64_t n, int64_t C, int64_t rows, int64_t parts, int32_t steps) {
  const int64_t E = IE;
  s->steps = steps;
  // split-K slabs: enough workgroups to fill the part (16 output tiles for d Wv, 4 for d Wq0, 1 for d Wq2), never an empty slab
  const int sv_room = pw_split_k(steps, 16, 4, &s->sv, &s->sv_per);
  const int sq0_room = pw_split_k(steps, 64, 4, &s->sq0, &s->sq0_per);
  const int sq2_room = pw_split_k(steps, 64, 2, &s->sq2, &s->sq2_per);
  s->vp = ar.off; ar.take<float>(E * E);
  s->vtp = ar.off; ar.take<float>(E * E);
  s->q0f = ar.off; ar.take<float>(DS_Q * E);
  s->q2f = ar.off; ar.take<float>(DS_Q * DS_Q);
  s->q2tf = ar.off; ar.take<float>(DS_Q * DS_Q);
  s->q0tf = ar.off; ar.take<float>(DS_Q * E);
  s->logits = ar.off; ar.take<float>(n * C);
  s->losses = ar.off; ar.take<float>(n * 3);
  s->logits_bag = ar.off; ar.take<float>(n * C);
  s->logits_ins = ar.off; ar.take<float>(n * C);
  s->B = ar.off; ar.take<float>(n * C * E);
  s->crit = ar.off; ar.take<int64_t>(n * C);
  s->qmax = ar.off; ar.take<float>(n * DS_MAXC * DS_Q);
  s->stats = ar.off; ar.take<float>(n * DS_MAXC * 2);
  s->gli = ar.off; ar.take<float>(n * DS_MAXC);
  s->dB = ar.off; ar.take<float>(n * DS_MAXC * E);
  s->delta = ar.off; ar.take<float>(n * DS_MAXC);
  s->dqmax = ar.off; ar.take<float>(n * DS_MAXC * DS_Q);
  s->dwfcc_part = ar.off; ar.take<float>(n * C * C * E);
  s->dbfcc_part = ar.off; ar.take<float>(n * C);
  s->dwi_part = ar.off; ar.take<float>(n * C * E);
  s->dbi_part = ar.off; ar.take<float>(n * C);
  s->V = ar.off; ar.take<float>(rows * E);
  s->Q = ar.off; ar.take<float>(rows * DS_Q);
  s->cls = ar.off; ar.take<float>(rows * DS_MAXC);
  s->da = ar.off; ar.take<float>(rows * DS_MAXC);
  s->dhv = ar.off; ar.take<float>(rows * E);
  s->U1 = ar.off; ar.take<float>(rows * DS_Q);
  s->dPQ = ar.off; ar.take<float>(rows * DS_Q);
  s->dP1 = ar.off; ar.take<float>(rows * DS_Q);
  s->pmax = ar.off; ar.take<float>(parts * DS_MAXC);
  s->parg = ar.off; ar.take<int32_t>(parts * DS_MAXC);
  s->pm = ar.off; ar.take<float>(parts * DS_MAXC);
  s->pl = ar.off; ar.take<float>(parts * DS_MAXC);
  s->pB = ar.off; ar.take<float>(parts * C * E);
  s->dbv_part = ar.off; ar.take<float>((int64_t)steps * E);
  s->dbq0_part = ar.off; ar.take<float>((int64_t)steps * DS_Q);
  s->dbq2_part = ar.off; ar.take<float>((int64_t)steps * DS_Q);
  s->dqm_part = ar.off; ar.take<float>((int64_t)steps * DS_MAXC * DS_Q);
  s->slab_v = ar.off; ar.take<float>((int64_t)sv_room * E * E);
  s->slab_q0 = ar.off; ar.take<float>((int64_t)sq0_room * DS_Q * E);
  s->slab_q2 = ar.off; ar.take<float>((int64_t)sq2_room * DS_Q * DS_Q);
}

int ds_prep_jobs(const mhimx_dsmil_params& P, char* base, const DsLay& s, mhimx_prep_job* j) {
  auto F = [&](int64_t off) { return reinterpret_cast<float*>(base + off); };
  int n = 0;
  j[n++] = mhimx_prep_job{1, P.wv, F(s.vp), IE, IE};
  j[n++] = mhimx_prep_job{7, P.wv, F(s.vtp), IE, IE};
  j[n++] = mhimx_prep_job{4, P.wq0, F(s.q0f), DS_Q, IE};
  j[n++] = mhimx_prep_job{4, P.wq2, F(s.q2f), DS_Q, DS_Q};
  j[n++] = mhimx_prep_job{5, P.wq2, F(s.q2tf), DS_Q, DS_Q};
  j[n++] = mhimx_prep_job{5, P.wq0, F(s.q0tf), DS_Q, IE};
  return n;
}

int ds_forward(hipStream_t st, const InferTab& tab, char* base, const DsLay& s, const mhimx_dsmil_params& P, int C, const float* H) {
  auto F = [&](int64_t off) { return reinterpret_cast<float*>(base + off); };
  // V = relu(h Wv^T + bv): the eval projection over the feature rows as fp32 "bags" of pitch 512
  if (int r = infer_project(st, ds_rows_tab(tab, H), IE, F(s.vp), P.bv, MHIMX_ACT_RELU, F(s.V))) return r;
  // Q, classes, critical rows, pool partials (infer_dsmil.hip)
  return dsmil_rows_crit_pool(st, tab, H, F(s.V), F(s.q0f), P.bq0, F(s.q2f), P.bq2, P.wi, P.bi, C, F(s.Q), F(s.cls), F(s.pmax),
                              reinterpret_cast<int32_t*>(base + s.parg), F(s.qmax), F(s.logits_ins), reinterpret_cast<int64_t*>(base + s.crit), F(s.pm),
                              F(s.pl), F(s.pB));
}

int ds_backward(hipStream_t st, const InferTab& tab, char* base, const DsLay& s, const mhimx_dsmil_params& P, int C, const float* H,
                const _Float16* dact, float* db1_part) {
  auto F = [&](int64_t off) { return reinterpret_cast<float*>(base + off); };
  float *V = F(s.V), *dhv = F(s.dhv);
  // rows pass 1
  MHIMX_ONCE_PER_DEVICE(MHIMX_HIP(hipFuncSetAttribute((const void*)dw_rows1_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DW_R1_SMEM)));
  hipLaunchKernelGGL(dw_rows1_kernel, dim3((unsigned)s.steps), dim3(DW_T), DW_R1_SMEM, st, tab, V, F(s.Q), F(s.qmax), F(s.stats), F(s.dB), F(s.delta), C,
                     F(s.da), F(s.dbv_part), F(s.dqm_part));
  MHIMX_LAUNCH_CHECK();
  // d PreV Wv: the eval projection on the d PreV rows with the paired image of Wv^T (no bias, no activation)
  if (int r = infer_project(st, ds_rows_tab(tab, V), IE, F(s.vtp), nullptr, MHIMX_ACT_NONE, dhv)) return r;
  // d q_max of every bag
  hipLaunchKernelGGL(dw_dqmax_kernel, dim3((unsigned)tab.n, DW_MAXC * DW_Q / RG_FIN_T), dim3(RG_FIN_T), 0, st, tab, F(s.dqm_part), F(s.dqmax));
  MHIMX_LAUNCH_CHECK();
  // rows pass 2
  if (int r = dact ? dw_rows2<false>(st, tab, base, s, P, C, H, dact, db1_part) : dw_rows2<true>(st, tab, base, s, P, C, H, dact, db1_part)) return r;
  // d Wv = dPreV^T h, d Wq2 = dPreQ^T U1, d Wq0 = dPre1^T h
  if (int r = pw_wgrad_rows(st, tab, V, IE, IE, H, IE, IE, s.steps, s.sv, s.sv_per, F(s.slab_v))) return r;
  if (int r = pw_wgrad_rows(st, tab, F(s.dPQ), DS_Q, DS_Q, F(s.U1), DS_Q, DS_Q, s.steps, s.sq2, s.sq2_per, F(s.slab_q2))) return r;
  return pw_wgrad_rows(st, tab, F(s.dP1), DS_Q, DS_Q, H, IE, IE, s.steps, s.sq0, s.sq0_per, F(s.slab_q0));
}

int ds_reduce(hipStream_t st, char* base, const DsLay& s, const mhimx_dsmil_grads& g, int64_t D, int C, int n_bags, const float* slab_1,
              int32_t s1, const float* db1_part, int32_t steps1) {
  auto F = [&](int64_t off) { return reinterpret_cast<float*>(base + off); };
  const float* parts[6] = {slab_1, F(s.slab_v), F(s.slab_q0), F(s.slab_q2), F(s.dwfcc_part), F(s.dwi_part)};
  const int32_t G[6] = {s1, s.sv, s.sq0, s.sq2, n_bags, n_bags};
  const int64_t W[6] = {(int64_t)IE * D, (int64_t)IE * IE, (int64_t)DS_Q * IE, (int64_t)DS_Q * DS_Q, (int64_t)C * C * IE, (int64_t)C * IE};
  float* out[6] = {g.w1, g.wv, g.wq0, g.wq2, g.wfcc, g.wi};
  if (int r = pw_reduce(st, 6, parts, G, W, out)) return r;
  const float* parts2[6] = {db1_part, F(s.dbv_part), F(s.dbq0_part), F(s.dbq2_part), F(s.dbfcc_part), F(s.dbi_part)};
  const int32_t G2[6] = {steps1, s.steps, s.steps, s.steps, n_bags, n_bags};
  const int64_t W2[6] = {IE, IE, DS_Q, DS_Q, C, C};
  float* out2[6] = {g.b1, g.bv, g.bq0, g.bq2, g.bfcc, g.bi};
  return pw_reduce(st, 6, parts2, G2, W2, out2);
}

int ds_check_base(const char* who, const mhimx_dsmil_train_cfg* c, int32_t xdt, int32_t n_bags, int32_t max_bags, const void* bags,
                  const char* student) {
  if (int r = rg_check_xdt(who, xdt)) return r;
  MHIMX_CHECK_ARG(c && bags, "%s: null configuration / bag list", who);
  MHIMX_CHECK_ARG(n_bags >= 1 && n_bags <= max_bags, "%s: 1..%d bags per window (got %d)", who, max_bags, n_bags);
  MHIMX_CHECK_ARG(c->E == IE && c->C >= 1 && c->C <= DS_MAXC && c->D > 0 && c->D % 256 == 0 && c->D <= (1 << 20),
                  "%s: shapes outside the ragged DSMIL train calls (E = 512, q width 128, 1 <= C <= %d, D %% 256 == 0, D <= 2^20)", who, DS_MAXC);
  MHIMX_CHECK_ARG(c->act >= MHIMX_ACT_NONE && c->act <= MHIMX_ACT_TANH, "%s: unknown activation", who);
  MHIMX_CHECK_ARG(c->drop_p >= 0.f && c->drop_p < 1.f, "%s: dropout probability outside [0,1)", who);
  MHIMX_CHECK_ARG(ds_params_ok(c->param), "%s: null %sparameter", who, student);
  MHIMX_CHECK_ARG(ds_params_aligned(c->param), "%s: the feature, i_classifier, q and v weights of the %smodel must be 16-byte aligned", who, student);
  const mhimx_dsmil_grads& g = c->grad;
  MHIMX_CHECK_ARG(g.w1 && g.b1 && g.wi && g.bi && g.wq0 && g.bq0 && g.wq2 && g.bq2 && g.wv && g.bv && g.wfcc && g.bfcc, "%s: null gradient view", who);
  MHIMX_CHECK_ARG(c->tick, "%s: the device dropout / draw counter (tick) is required", who);
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
  out->total = w.total; out->rows = w.rows; out->logits = w.s.logits; out->losses = w.s.losses; out->logits_bag = w.s.logits_bag;
  out->logits_ins = w.s.logits_ins; out->B = w.s.B; out->crit = w.s.crit; out->H = w.H; out->dact = w.dact;
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
  float* H = F(w.H);
  _Float16* dact = reinterpret_cast<_Float16*>(base + w.dact);

  // ---- 1. counters and weight images
  {
    mhimx_prep_job jobs[9];
    int n = 0;
    jobs[n++] = mhimx_prep_job{3, nullptr, reinterpret_cast<float*>(c.tick), 1, 1};
    if (c.opt_step) jobs[n++] = mhimx_prep_job{3, nullptr, reinterpret_cast<float*>(c.opt_step), 1, 1};
    jobs[n++] = mhimx_prep_job{1, P.w1, F(w.w1p), c.E, c.D};
    n += ds_prep_jobs(P, base, w.s, jobs + n);
    if (int r = mhimx_prep_batch(stream, jobs, n)) return r;
  }
  // ---- 2. feature rows, dropout, d out / d pre of every bag
  {
    PureWinDrop dr = {};
    for (int b = 0; b < n_bags; ++b) dr.seed[b] = bags[b].drop_seed;
    dr.tick = c.tick; dr.dact = dact; dr.drop_p = c.drop_p;
    if (int r = pure_window_project_elem(st, tab, dr, D, F(w.w1p), P.b1, c.act, H)) return r;
  }
  // ---- 3. - 6. V, Q, classes, critical rows, pool partials
  if (int r = ds_forward(st, tab, base, w.s, P, C, H)) return r;
  // ---- 7. merge, fcc, mix, CE and the head gradients
  DsLabels lab = {};
  for (int b = 0; b < n_bags; ++b) lab.p[b] = bags[b].label_dev;
  if (int r = ds_head(st, tab, base, w.s, P, C, H, lab, c.main_alpha)) return r;
  // ---- 8. - 14. the two rows passes and the student's three weight gradients; 15. d W1
  if (int r = ds_backward(st, tab, base, w.s, P, C, H, dact, F(w.db1_part))) return r;
  if (int r = pw_wgrad_bagx(st, tab, F(w.s.dhv), D, w.steps, w.s1, w.s1_per, F(w.slab_1))) return r;
  // ---- 16., 17. the partial buffers, in index order, into the gradient views
  if (int r = ds_reduce(st, base, w.s, c.grad, D, C, n_bags, F(w.slab_1), w.s1, F(w.db1_part), w.steps)) return r;
  if (!update) return 0;
  // ---- 18. Adam
  const mhimx_optim_args o = optim_args_of(c, host_step);
  return mhimx_optim_step(stream, &o);
}
