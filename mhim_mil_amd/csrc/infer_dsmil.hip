// infer_dsmil.hip — eval-mode MHIM(DSMIL) forward of up to MHIMX_INFER_MAX bags of DIFFERENT row counts in one call
// (modules/mhim.py:229-272 forward_test with baseline == 'dsmil' and merge_test off, over mhim_modules/baseline.py:112-194 BClassifier / DSMIL,
// under engines/common_mil.py:56-68 with the 0.5 * logits[0] + 0.5 * logits[1] mix of :66-67):
//
//     h = act(X W1^T + b1),  classes = h Wi^T + bi,  V = relu(h Wv^T + bv),  Q = tanh(relu(h Wq0^T + bq0) Wq2^T + bq2)
//     crit[c] = arg max_m classes[m,c],  q_max[c] = Q[crit[c]],  A = softmax_m(Q q_max^T / sqrt(128)),  B = A^T V,
//     logits_bag = fcc(B),  logits_ins = max_m classes,  logits = 0.5 logits_bag + 0.5 logits_ins,  loss = CE(logits, label)
//
// The sibling of infer.hip: the same by-value bag table (InferTab), so the call copies nothing to the device, waits for nothing and
// allocates nothing, and can be captured in a graph.  Seven launches whatever n_bags is:
//   1  mhimx_prep_batch        paired-plane images of W1 and of v.1.weight, matrix-core fragment images (kind 4) of q.0.weight [128,512]
//                              and q.2.weight [128,128] (the kind-4 job takes any K % 16 == 0: no new kind)
//   2  infer_project_kernel    (bag_project.hip) X -> h, all three element types
//   3  infer_project_kernel    again over a second table whose "bags" are the h rows in the workspace (pitch 512, fp32, D = 512): h -> V
//   4  dsmil_rows_kernel       one workgroup per CHUNK of 256 rows of one bag, 32-row tiles through LDS: U1 = relu(h q0^T + b) on the matrix
//                              cores (3-term bf16), U1 through LDS into Q = tanh(U1 q2^T + b) (K = 128), classes in fp32 FMAs; per row Q,
//                              classes[16] and max_c classes, per chunk and class the (max, arg-max) partial
//   5  dsmil_crit_kernel       grid = bags: merges the chunk partials (lowest row on equal values - colmax_kernel's rule, rows.hip) -> crit,
//                              logits_ins, and the C rows Q[crit[c]] as q_max: q(h[crit]) IS that row of Q, no second q-network pass
//   6  dsmil_pool_kernel       one workgroup per chunk: a = Q q_max^T / sqrt(128) in fp32, per class the log-sum-exp partial
//                              {max, sum, sum_m e^{a - max} V[m,:]}
//   7  dsmil_finalize_kernel   plane x = bag: block y = 0 merges the partials in index order -> B, fcc, the mix, the loss; blocks y > 0
//                              write the instance score when it is not max_c classes (they recompute a from Q and q_max)
// No workgroup waits for another and there are no floating-point atomics.  A bag's tiles, chunks and merge order depend on its own N
// alone, so its results have the same bits wherever it stands in a call.
#include <limits.h>
#include <math.h>

#include <type_traits>

#include "infer_tab.hpp"

namespace mhimx {

namespace {

constexpr int DQ = 128, DS_MAXC = 16;
constexpr int DR_ULD = DQ + 4;
constexpr size_t DR_SMEM = (size_t)(RG_ROWS * RG_LD + RG_ROWS * DS_MAXC) * sizeof(float);
constexpr int DP_THREADS = 256, DF_ATTN_BLOCKS = 8;
constexpr float DS_SCALE = 0.08838834764831845f;   // 1 / sqrt(128)
static_assert(RG_ROWS * DR_ULD <= RG_ROWS * RG_LD, "the U1 tile reuses the feature tile's LDS");

// a[c] = Q[m,:] . q_max[c,:] / sqrt(128), fp32 in a fixed order (qs: [CT][128] in LDS; classes past C hold zeros).  The pool launch
// and the attention blocks of the finalize launch share it: the same bits.
template <int CT>
MHIMX_DEV void ds_scores(const float* __restrict__ qrow, const float* qs, float (&a)[CT]) {
#pragma unroll
  for (int c = 0; c < CT; ++c) a[c] = 0.f;
#pragma unroll 4
  for (int j = 0; j < DQ / 4; ++j) {
    const f32x4 q = reinterpret_cast<const f32x4*>(qrow)[j];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const f32x4 w = reinterpret_cast<const f32x4*>(qs + c * DQ)[j];
      a[c] = fmaf(q[3], w[3], fmaf(q[2], w[2], fmaf(q[1], w[1], fmaf(q[0], w[0], a[c]))));
    }
  }
#pragma unroll
  for (int c = 0; c < CT; ++c) a[c] *= DS_SCALE;
}

// ------------------------------------------------------------------------------------------------ 4. per-row Q, classes, arg-max partials
// blockIdx.x = chunk of RG_CHUNK rows of ONE bag (the last chunk of a bag may be short).  Wave w owns columns [32 w, 32 w + 32) of U1 and of Q.
__global__ __launch_bounds__(RG_T, 2) void dsmil_rows_kernel(InferTab tab, const float* __restrict__ Hin, const float* __restrict__ q0_frag,
                                                                   const float* __restrict__ bq0, const float* __restrict__ q2_frag,
                                                                   const float* __restrict__ bq2, const float* __restrict__ wi,
                                                                   const float* __restrict__ bi, int C, float* __restrict__ Qout,
                                                                   float* __restrict__ cls, float* __restrict__ score,
                                                                   float* __restrict__ pmax, int32_t* __restrict__ parg) {
  extern __shared__ __attribute__((aligned(16))) float dr_sm[];
  float* Hs = dr_sm;                          // [32][516] feature rows; then [32][132] U1 (the feature rows are dead by then)
  float* Us = dr_sm;
  float* cs = Hs + RG_ROWS * RG_LD;           // [32][16] classes of the tile (rows past the chunk: -inf)
  const int part = blockIdx.x;
  RG_BAG_OF(part, part0)
  const int64_t c0 = (int64_t)(part - p0) * RG_CHUNK;           // first row of the chunk inside its bag
  const int64_t M = (N - c0 < RG_CHUNK) ? N - c0 : RG_CHUNK;    // rows of the chunk (>= 1)
  const float* T = Hin + (orow0 + c0) * IE;
  const int64_t grow0 = orow0 + c0;                             // first row of the chunk in the call's row space

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r32 = lane & 31, kg = lane >> 5;
  const int n_col = 32 * wave + r32;
  const float b0 = bq0[n_col], b2 = bq2[n_col];
  const f32x4* f0 = reinterpret_cast<const f32x4*>(q0_frag + ((int64_t)wave * (IE / 16) * 64 + lane) * 8);
  const f32x4* f2 = reinterpret_cast<const f32x4*>(q2_frag + ((int64_t)wave * (DQ / 16) * 64 + lane) * 8);
  const int crow = tid >> 3, seg = tid & 7;                     // classes: 8 lanes per row

  float best = -INFINITY;                                       // threads < C: running (max, arg-max) of class tid over the chunk
  int arg = (int)c0;
  const int tiles = (int)((M + RG_ROWS - 1) / RG_ROWS);
  for (int tile = 0; tile < tiles; ++tile) {
    const int64_t row0 = (int64_t)tile * RG_ROWS;
    // ---- rows -> LDS (rows past the chunk: zeros; their loads are clamped so that all 16 are in flight)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int f = tid + RG_T * i, r = f >> 7, c4 = f & 127;
      const int64_t nr = row0 + r;
      f32x4 v = reinterpret_cast<const f32x4*>(T + (nr < M ? nr : M - 1) * IE)[c4];
      if (nr >= M) v = f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(Hs + r * RG_LD + 4 * c4) = v;
    }
    __syncthreads();
    // ---- U1 tile on the matrix cores
    const f32x16 u1 = rg_mma3<IE>(Hs + r32 * RG_LD + 8 * kg, f0);
    // ---- classes = h Wi^T + bi: lane `seg` takes the 16-byte groups seg, seg + 8, .. of the row, the 8 partial sums added in a fixed xor tree
    {
      float cp[DS_MAXC];
#pragma unroll
      for (int c = 0; c < DS_MAXC; ++c) cp[c] = 0.f;
      const f32x4* hr = reinterpret_cast<const f32x4*>(Hs + crow * RG_LD);
      const f32x4* w4 = reinterpret_cast<const f32x4*>(wi);
#pragma unroll 2
      for (int g = 0; g < IE / 32; ++g) {
        const f32x4 h = hr[seg + 8 * g];
#pragma unroll
        for (int c = 0; c < DS_MAXC; ++c)
          if (c < C) {
            const f32x4 w = w4[c * (IE / 4) + seg + 8 * g];
            cp[c] = fmaf(h[3], w[3], fmaf(h[2], w[2], fmaf(h[1], w[1], fmaf(h[0], w[0], cp[c]))));
          }
      }
      const bool live = row0 + crow < M;
      float rmax = -INFINITY;
#pragma unroll
      for (int c = 0; c < DS_MAXC; ++c) {
        cp[c] += __shfl_xor(cp[c], 1);
        cp[c] += __shfl_xor(cp[c], 2);
        cp[c] += __shfl_xor(cp[c], 4);
        if (c < C) {
          cp[c] += bi[c];
          rmax = fmaxf(rmax, cp[c]);
        }
      }
      if (seg == 0) {
        if (live) {
          f32x4* o = reinterpret_cast<f32x4*>(cls + (grow0 + row0 + crow) * DS_MAXC);
#pragma unroll
          for (int q = 0; q < 4; ++q) o[q] = f32x4{cp[4 * q], cp[4 * q + 1], cp[4 * q + 2], cp[4 * q + 3]};
          if (score) score[grow0 + row0 + crow] = rmax;
        }
        f32x4* o = reinterpret_cast<f32x4*>(cs + crow * DS_MAXC);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          o[q] = live ? f32x4{cp[4 * q], cp[4 * q + 1], cp[4 * q + 2], cp[4 * q + 3]} : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      }
    }
    __syncthreads();                           // every read of the feature tile is done; the tile's classes are in LDS
    // ---- U1 = relu(. + b) -> LDS: u1[i] = U1[row = 8 (i >> 2) + 4 kg + (i & 3)][n_col]
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = 8 * (i >> 2) + 4 * kg + (i & 3);
      const float u = u1[i] + b0;
      Us[row * DR_ULD + n_col] = u > 0.f ? u : 0.f;
    }
    if (tid < C) {                             // rows in index order, strictly greater: the lowest row wins on equal values
      for (int r = 0; r < RG_ROWS; ++r) {
        const float v = cs[r * DS_MAXC + tid];
        if (v > best) { best = v; arg = (int)(c0 + row0) + r; }
      }
    }
    __syncthreads();
    // ---- Q = tanh(U1 q2^T + b), K = 128
    const f32x16 q = rg_mma3<DQ>(Us + r32 * DR_ULD + 8 * kg, f2);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = 8 * (i >> 2) + 4 * kg + (i & 3);
      if (row0 + row < M) Qout[(grow0 + row0 + row) * DQ + n_col] = tanh_fast(q[i] + b2);
    }
    __syncthreads();                           // the next tile overwrites Hs / cs
  }
  if (tid < C) {
    pmax[(int64_t)part * DS_MAXC + tid] = best;
    parg[(int64_t)part * DS_MAXC + tid] = arg;
  }
}

// ------------------------------------------------------------------------------------------------ 5. critical rows
// blockIdx.x = bag.  Wave w merges the chunk partials of classes w, w + 4, ..: the maximum, and among equal values the lowest row - the rule
// of colmax_kernel (rows.hip), so that this route and the module's name the same row.  Then the C rows Q[crit[c]] are copied as q_max.
__global__ __launch_bounds__(256) void dsmil_crit_kernel(InferTab tab, const float* __restrict__ pmax, const int32_t* __restrict__ parg,
                                                         const float* __restrict__ Q, int C, float* __restrict__ qmax,
                                                         float* __restrict__ logits_ins, int64_t* __restrict__ crit) {
  __shared__ int s_arg[DS_MAXC];
  const int bag = blockIdx.x;
  RG_BAG(bag)
  const int G = rg_parts(N);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int c = wave; c < C; c += 4) {
    float best = -INFINITY;
    int arg = INT_MAX;
    for (int g = lane; g < G; g += 64) {
      const float v = pmax[(int64_t)(p0 + g) * DS_MAXC + c];
      const int a = parg[(int64_t)(p0 + g) * DS_MAXC + c];
      if (v > best || (v == best && a < arg)) { best = v; arg = a; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(arg, o, 64);
      if (ov > best || (ov == best && oi < arg)) { best = ov; arg = oi; }
    }
    if (lane == 0) {
      s_arg[c] = arg;
      logits_ins[(int64_t)bag * C + c] = best;
      if (crit) crit[(int64_t)bag * C + c] = arg;
    }
  }
  __syncthreads();
  for (int i = tid; i < C * DQ; i += 256) {
    const int c = i >> 7, j = i & (DQ - 1);
    qmax[((int64_t)bag * DS_MAXC + c) * DQ + j] = Q[(orow0 + s_arg[c]) * DQ + j];
  }
}

// ------------------------------------------------------------------------------------------------ 6. softmax-pool partials
// blockIdx.x = chunk.  Thread t scores row t of the chunk against the C critical queries; the chunk's {max, sum} per class; then thread t owns
// columns t and t + 256 of the [C, 512] accumulator sum_m e^{a[m,c] - max_c} V[m,:], rows in index order.  CT: C rounded up to 2 / 4 / 8 / 16.
template <int CT>
__global__ __launch_bounds__(DP_THREADS) void dsmil_pool_kernel(InferTab tab, const float* __restrict__ Q, const float* __restrict__ V,
                                                                const float* __restrict__ qmax, int C, float* __restrict__ pm,
                                                                float* __restrict__ pl, float* __restrict__ pB) {
  __shared__ __attribute__((aligned(16))) float qs[CT * DQ];
  __shared__ __attribute__((aligned(16))) float ps[RG_CHUNK * CT];
  __shared__ float redm[CT][4], reds[CT][4];
  const int part = blockIdx.x;
  RG_BAG_OF(part, part0)
  const int64_t c0 = (int64_t)(part - p0) * RG_CHUNK;
  const int M = (int)((N - c0 < RG_CHUNK) ? N - c0 : RG_CHUNK);
  const int64_t grow0 = orow0 + c0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < CT * DQ; i += DP_THREADS) qs[i] = (i >> 7) < C ? qmax[(int64_t)bag * DS_MAXC * DQ + i] : 0.f;
  __syncthreads();
  const bool live = tid < M;
  float a[CT];
  ds_scores<CT>(Q + (grow0 + (live ? tid : 0)) * DQ, qs, a);
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    if (!live) a[c] = -INFINITY;
    const float m = wave_max(a[c]);
    if (lane == 0) redm[c][wave] = m;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const float mx = fmaxf(fmaxf(redm[c][0], redm[c][1]), fmaxf(redm[c][2], redm[c][3]));   // row 0 of a chunk is a real row: finite
    const float p = live ? __expf(a[c] - mx) : 0.f;
    ps[tid * CT + c] = p;
    const float s = wave_sum(p);
    if (lane == 0) reds[c][wave] = s;
  }
  __syncthreads();
  if (tid < C) {
    pm[(int64_t)part * DS_MAXC + tid] = fmaxf(fmaxf(redm[tid][0], redm[tid][1]), fmaxf(redm[tid][2], redm[tid][3]));
    pl[(int64_t)part * DS_MAXC + tid] = (reds[tid][0] + reds[tid][1]) + (reds[tid][2] + reds[tid][3]);
  }
  float acc0[CT], acc1[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) { acc0[c] = 0.f; acc1[c] = 0.f; }
  const float* Vb = V + grow0 * IE + tid;
#pragma unroll 4
  for (int m = 0; m < M; ++m) {
    const float v0 = Vb[(int64_t)m * IE], v1 = Vb[(int64_t)m * IE + DP_THREADS];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const float p = ps[m * CT + c];
      acc0[c] = fmaf(p, v0, acc0[c]);
      acc1[c] = fmaf(p, v1, acc1[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if (c < C) {
      float* o = pB + ((int64_t)part * C + c) * IE + tid;
      o[0] = acc0[c];
      o[DP_THREADS] = acc1[c];
    }
}

// ------------------------------------------------------------------------------------------------ 7. merge + fcc + mix + loss + attention
// blockIdx.x = bag.  Every block of a bag derives each class's {max, sum} from the bag's partials in the same fixed order.  blockIdx.y = 0:
// B (thread e = column e, partials in index order), the fcc head in fp32, the mix, the cross entropy.  blockIdx.y > 0: the instance score
// max_c A[m,c] (no_norm: max_c a[m,c]).
template <int CT>
__global__ __launch_bounds__(RG_FIN_T) void dsmil_finalize_kernel(InferTab tab, const float* __restrict__ pm, const float* __restrict__ pl,
                                                              const float* __restrict__ pB, const float* __restrict__ Q,
                                                              const float* __restrict__ qmax, const float* __restrict__ wfcc,
                                                              const float* __restrict__ bfcc, int C, int no_norm,
                                                              const int64_t* __restrict__ labels, const float* __restrict__ logits_ins,
                                                              float* __restrict__ logits_bag, float* __restrict__ logits,
                                                              float* __restrict__ B_out, float* __restrict__ attn, float* __restrict__ loss) {
  __shared__ float red[8];
  __shared__ float wgt[RG_FIN_T];
  __shared__ float smx[CT], sinv[CT];
  __shared__ float lg[DS_MAXC];
  __shared__ __attribute__((aligned(16))) float big[CT * IE];  // y = 0: B [C][512]; y > 0: q_max [CT][128]
  const int bag = blockIdx.x;
  RG_BAG(bag)
  const int G = rg_parts(N);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  pm += (int64_t)p0 * DS_MAXC; pl += (int64_t)p0 * DS_MAXC; pB += (int64_t)p0 * C * IE;
  for (int c = 0; c < C; ++c) {
    float mx, Ls;
    rg_merge_stats(pm + c, pl + c, G, DS_MAXC, red, mx, Ls);
    if (tid == 0) { smx[c] = mx; sinv[c] = 1.f / Ls; }
    __syncthreads();
  }
  if (blockIdx.y > 0) {
    if (!attn) return;
    for (int i = tid; i < CT * DQ; i += RG_FIN_T) big[i] = (i >> 7) < C ? qmax[(int64_t)bag * DS_MAXC * DQ + i] : 0.f;
    __syncthreads();
    float mxr[CT], ivr[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) { mxr[c] = c < C ? smx[c] : 0.f; ivr[c] = c < C ? sinv[c] : 0.f; }
    float* ab = attn + orow0;
    const int64_t step = (int64_t)(gridDim.y - 1) * RG_FIN_T;
    for (int64_t r = (int64_t)(blockIdx.y - 1) * RG_FIN_T + tid; r < N; r += step) {
      float a[CT];
      ds_scores<CT>(Q + (orow0 + r) * DQ, big, a);
      float best = -INFINITY;
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C) best = fmaxf(best, no_norm ? a[c] : __expf(a[c] - mxr[c]) * ivr[c]);
      ab[r] = best;
    }
    return;
  }
  for (int c = 0; c < C; ++c) {
    const float mx = smx[c];
    float acc = 0.f;                                          // column tid of B[c]
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
    if (B_out) B_out[((int64_t)bag * C + c) * IE + tid] = bv;
  }
  __syncthreads();
  // fcc: Conv1d(C, C, kernel = E) on [1, C, E] = a [C, C * E] dot
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
  if (!loss) return;
  __syncthreads();
  if (tid == 0) {
    // torch.nn.CrossEntropyLoss on one row: log sum_c e^{x_c} - x_label (a label outside [0, C): NaN, where torch raises)
    float cm = lg[0];
    for (int c = 1; c < C; ++c) cm = fmaxf(cm, lg[c]);
    float den = 0.f;
    for (int c = 0; c < C; ++c) den += expf(lg[c] - cm);
    const int64_t y = labels[bag];
    loss[bag] = (y >= 0 && y < C) ? (cm + logf(den)) - lg[y] : NAN;
  }
}

// ------------------------------------------------------------------------------------------------ host
struct DsmilWs { int64_t w1p, vp, q0f, q2f, H, V, Q, cls, pmax, parg, qmax, pm, pl, pB, total; };

// the checks of mhimx_infer_run_x on the bag table and the element type (infer.hip: check_infer), and this call's own shape rules
int check_dsmil(const mhimx_infer_dsmil_cfg* c, int32_t n_bags, const mhimx_infer_bag* bags, int32_t xdt) {
  if (int r = rg_check_infer_front("infer_dsmil", xdt, c, n_bags, bags, true)) return r;
  MHIMX_CHECK_ARG(c->E == IE && c->C >= 1 && c->C <= DS_MAXC && c->D > 0 && c->D % 256 == 0 && c->D <= (1 << 20),
                  "infer_dsmil: shapes outside the ragged DSMIL forward (E = 512, q width 128, 1 <= C <= %d, D %% 256 == 0)", DS_MAXC);
  MHIMX_CHECK_ARG(c->act >= MHIMX_ACT_NONE && c->act <= MHIMX_ACT_TANH, "infer_dsmil: unknown activation");
  return rg_check_infer_bags("infer_dsmil", c->D, n_bags, bags, xdt);
}

void dsmil_layout(const mhimx_infer_dsmil_cfg* c, int32_t n_bags, const mhimx_infer_bag* bags, DsmilWs* w, InferTab* tab) {
  const RgCount n = rg_tab_fill(tab, n_bags, bags);
  const int64_t rows = n.rows, parts = n.parts;
  Arena ar(nullptr, 0);
  w->w1p = ar.off; ar.take<float>(c->E * c->D);
  w->vp = ar.off; ar.take<float>(c->E * c->E);
  w->q0f = ar.off; ar.take<float>(DQ * c->E);
  w->q2f = ar.off; ar.take<float>(DQ * DQ);
  w->H = ar.off; ar.take<float>(rows * c->E);
  w->V = ar.off; ar.take<float>(rows * c->E);
  w->Q = ar.off; ar.take<float>(rows * DQ);
  w->cls = ar.off; ar.take<float>(rows * DS_MAXC);
  w->pmax = ar.off; ar.take<float>(parts * DS_MAXC);
  w->parg = ar.off; ar.take<int32_t>(parts * DS_MAXC);
  w->qmax = ar.off; ar.take<float>((int64_t)n_bags * DS_MAXC * DQ);
  w->pm = ar.off; ar.take<float>(parts * DS_MAXC);
  w->pl = ar.off; ar.take<float>(parts * DS_MAXC);
  w->pB = ar.off; ar.take<float>(parts * c->C * c->E);
  w->total = ar.off;
}

// f(std::integral_constant<int, CT>) for the instance CT of the pool and finalize kernels that holds C classes
template <class F>
void ds_for_ct(int C, F&& f) {
  if (C <= 2) f(std::integral_constant<int, 2>{});
  else if (C <= 4) f(std::integral_constant<int, 4>{});
  else if (C <= 8) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 16>{});
}

}  // namespace

// launches 4, 5, 6 of the header for mhimx_dsmil_window_run (dsmil_window.hip): the same kernels over the caller's table and buffers
int dsmil_rows_crit_pool(hipStream_t st, const InferTab& tab, const float* H, const float* V, const float* q0f, const float* bq0, const float* q2f,
                         const float* bq2, const float* wi, const float* bi, int C, float* Q, float* cls, float* pmax, int32_t* parg, float* qmax,
                         float* logits_ins, int64_t* crit, float* pm, float* pl, float* pB, float* score) {
  MHIMX_CHECK_ARG(C >= 1 && C <= DS_MAXC, "dsmil_rows_crit_pool: 1 <= C <= %d", DS_MAXC);
  MHIMX_ONCE_PER_DEVICE(MHIMX_HIP(hipFuncSetAttribute((const void*)dsmil_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DR_SMEM)));
  hipLaunchKernelGGL(dsmil_rows_kernel, dim3((unsigned)tab.parts), dim3(RG_T), DR_SMEM, st, tab, H, q0f, bq0, q2f, bq2, wi, bi, C, Q, cls, score, pmax,
                     parg);
  MHIMX_LAUNCH_CHECK();
  hipLaunchKernelGGL(dsmil_crit_kernel, dim3((unsigned)tab.n), dim3(256), 0, st, tab, pmax, parg, Q, C, qmax, logits_ins, crit);
  MHIMX_LAUNCH_CHECK();
  ds_for_ct(C, [&](auto ct) {
    hipLaunchKernelGGL(dsmil_pool_kernel<decltype(ct)::value>, dim3((unsigned)tab.parts), dim3(DP_THREADS), 0, st, tab, Q, V, qmax, C, pm, pl, pB);
  });
  MHIMX_LAUNCH_CHECK();
  return 0;
}

// launch 7; attn: the max_c A (no_norm: max_c a) blocks.  mhimx_dsmil_mhim_window_run's teacher (dsmil_mhim.hip): no labels, no loss
int dsmil_finalize(hipStream_t st, const InferTab& tab, const float* pm, const float* pl, const float* pB, const float* Q, const float* qmax,
                   const float* wfcc, const float* bfcc, int C, const float* logits_ins, float* logits_bag, float* logits, float* B, float* attn,
                   int no_norm, const int64_t* labels, float* loss) {
  MHIMX_CHECK_ARG(C >= 1 && C <= DS_MAXC, "dsmil_finalize: 1 <= C <= %d", DS_MAXC);
  ds_for_ct(C, [&](auto ct) {
    hipLaunchKernelGGL(dsmil_finalize_kernel<decltype(ct)::value>, dim3((unsigned)tab.n, attn ? 1 + DF_ATTN_BLOCKS : 1), dim3(RG_FIN_T), 0, st, tab,
                       pm, pl, pB, Q, qmax, wfcc, bfcc, C, no_norm, labels, logits_ins, logits_bag, logits, B, attn, loss);
  });
  MHIMX_LAUNCH_CHECK();
  return 0;
}

}  // namespace mhimx

extern "C" int64_t mhimx_infer_dsmil_ws_bytes(const mhimx_infer_dsmil_cfg* cfg, int32_t n_bags, const mhimx_infer_bag* bags) {
  using namespace mhimx;
  if (int r = check_dsmil(cfg, n_bags, bags, MHIMX_X_F32)) return r;
  DsmilWs w;
  dsmil_layout(cfg, n_bags, bags, &w, nullptr);
  return w.total;
}

extern "C" int mhimx_infer_dsmil_run(void* stream, const mhimx_infer_dsmil_cfg* cfg, int32_t n_bags, const mhimx_infer_bag* bags,
                                     const int64_t* labels_dev, const mhimx_infer_dsmil_out* out, void* ws, int64_t ws_bytes,
                                     int32_t x_dtype) {
  using namespace mhimx;
  if (int r = check_dsmil(cfg, n_bags, bags, x_dtype)) return r;
  MHIMX_CHECK_ARG(cfg->w1 && cfg->b1 && cfg->wi && cfg->bi && cfg->wq0 && cfg->bq0 && cfg->wq2 && cfg->bq2 && cfg->wv && cfg->bv && cfg->wfcc &&
                      cfg->bfcc,
                  "infer_dsmil: null parameter");
  MHIMX_CHECK_ARG(aligned16(cfg->w1) && aligned16(cfg->b1) && aligned16(cfg->wi) && aligned16(cfg->wq0) && aligned16(cfg->wq2) &&
                      aligned16(cfg->wv) && aligned16(cfg->bv),
                  "infer_dsmil: the feature, i_classifier, q and v weights must be 16-byte aligned");
  if (int r = rg_check_infer_io("infer_dsmil", n_bags, bags, out && out->logits_bag && out->logits_ins && out->logits,
                                "the three logits outputs are required", out ? out->loss : nullptr, labels_dev))
    return r;
  DsmilWs w;
  InferTab tab = {};
  dsmil_layout(cfg, n_bags, bags, &w, &tab);
  tab.pad = x_dtype;                           // read by the first projection launch alone: the only reader of X
  if (int r = rg_check_ws("infer_dsmil", ws, ws_bytes, w.total)) return r;
  hipStream_t st = (hipStream_t)stream;
  char* base = static_cast<char*>(ws);
  auto F = [&](int64_t off) { return reinterpret_cast<float*>(base + off); };
  float *w1p = F(w.w1p), *vp = F(w.vp), *q0f = F(w.q0f), *q2f = F(w.q2f), *H = F(w.H), *V = F(w.V), *Q = F(w.Q), *cls = F(w.cls);
  float *pmax = F(w.pmax), *qmax = F(w.qmax), *pm = F(w.pm), *pl = F(w.pl), *pB = F(w.pB);
  int32_t* parg = reinterpret_cast<int32_t*>(base + w.parg);
  const int D = (int)cfg->D, C = (int)cfg->C;

  // 1. weight images
  mhimx_prep_job jobs[4] = {mhimx_prep_job{1, cfg->w1, w1p, cfg->E, cfg->D}, mhimx_prep_job{1, cfg->wv, vp, cfg->E, cfg->E},
                            mhimx_prep_job{4, cfg->wq0, q0f, DQ, cfg->E}, mhimx_prep_job{4, cfg->wq2, q2f, DQ, DQ}};
  if (int r = mhimx_prep_batch(stream, jobs, 4)) return r;
  // 2. feature rows of every bag (bag_project.hip)
  if (int r = infer_project(st, tab, D, w1p, cfg->b1, cfg->act, H)) return r;
  // 3. V = relu(h Wv^T + bv): the same launch over the feature rows as fp32 "bags" of pitch 512
  InferTab tabv = tab;
  for (int b = 0; b < n_bags; ++b) { tabv.X[b] = H + tab.row0[b] * IE; tabv.ldx[b] = IE; }
  tabv.pad = MHIMX_X_F32;
  if (int r = infer_project(st, tabv, IE, vp, cfg->bv, MHIMX_ACT_RELU, V)) return r;
  // 4. Q, classes, arg-max partials (the instance score too when it is max_c classes); 5. critical rows, max-instance logits, q_max;
  // 6. pool partials
  if (int r = dsmil_rows_crit_pool(st, tab, H, V, q0f, cfg->bq0, q2f, cfg->bq2, cfg->wi, cfg->bi, C, Q, cls, pmax, parg, qmax, out->logits_ins,
                                   out->crit, pm, pl, pB, cfg->cls_attn ? out->attn : nullptr))
    return r;
  // 7. merge, fcc, mix, loss, attention (its blocks run only where the attention is not the instance score of launch 4)
  return dsmil_finalize(st, tab, pm, pl, pB, Q, qmax, cfg->wfcc, cfg->bfcc, C, out->logits_ins, out->logits_bag, out->logits, out->B,
                        cfg->cls_attn ? nullptr : out->attn, (int)(cfg->no_norm != 0), labels_dev, out->loss);
}
