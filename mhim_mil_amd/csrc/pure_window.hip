// pure_window.hip — ONE optimiser update over up to MHIMX_PURE_WINDOW_MAX bags of DIFFERENT row counts for the teacher-free ABMIL model
// ('mhim_pure' under --accumulation_steps) behind one C call: mhimx_pure_window_run.
// replaces: engines/base_engine.py:29-51,76-120 (the accumulation window: every bag's loss divided by the window's length, the gradients
//           added up, one optimizer.step()) around engines/common_mil.py:32-37 and modules/mhim.py `pure`, for bags b = 0 .. n-1:
//
//     h_b = dropout_b(act(X_b W1^T + b1)),  s_b = wc . da_act(h_b Wa^T),  z_b = softmax(s_b) h_b,  logits_b = z_b Wp^T + bp
//     loss_b = main_alpha CE(logits_b, label_b) / n,   g = sum_b d loss_b / d theta,   one Adam step on g (update = 1)
//
// The ragged TRAINING launches of the library: the by-value bag table is the inference call's (infer_tab.hpp), every bag starts at a multiple
// of 32 in the call's row space (a 32-row tile / k-step lies inside one bag; the rows between a bag's N and its next multiple of 32 are zero
// rows with score -inf).  Nine launches whatever n and the sizes are:
//   1  mhimx_prep_batch              counters, the W1 paired-plane image, the Wa fragment image
//   2  pure_window_project_kernel    (bag_project.hip) infer_project_kernel's tile walk in train mode: per-bag dropout, fp16 d out / d pre, zero
//                                    padding rows
//   3  infer_score_kernel<false>     (infer.hip, as it is) scores + one pool partial per 256 rows of a bag
//   4  pw_head_kernel                plane = bag: merge of the partials in index order, predictor, CE and their gradients: g_logits, g_z, z.g_z,
//                                    the bag's d Wp / d bp partial
//   5  pw_pool_bwd_kernel            one workgroup per 32-row tile of the row space: U = h Wa^T again on the matrix cores (3-term bf16), d s,
//                                    d U (kept as fp32 rows for launch 6) and the tile's d wc partial, d h = p g_z + d U Wa (fp32), the epilogue
//                                    multiplies by d out / d pre and writes fp32 dPRE rows and the tile's column sums (d b1 partial)
//   6  pw_tn_kernel<false, 0>        d Wa = dU^T H over the whole row space: 128 x 128 tiles, split-K slabs, 3-term bf16 on the matrix cores
//   7  pw_tn_kernel<true, XT>        d W1 = sum_b dPRE_b^T X_b: the same kernel, the X side read from each bag where it lies (a k-step = 32 rows
//                                    of ONE bag, found from the table)
//   8  pw_reduce_kernel              every partial buffer (slabs, per-tile and per-bag partials) summed in index order into cfg->grad
//   9  mhimx_optim_step              Adam (update = 1)
// No floating-point atomics, no workgroup waits for another, every sum has a fixed order: two runs give the same bits.  What is written per
// bag depends on that bag's N, seed and the tick alone.
#include <math.h>
#include <string.h>

#include "infer_tab.hpp"
#include "surv_dev.hpp"

namespace mhimx {

namespace {

constexpr int PW_A = 128, PW_ROWS = RG_ROWS, PW_T = RG_T, PW_LD = RG_LD, PW_DUP = PW_ROWS + 4, PW_MAXC = 4;
constexpr size_t PW_BWD_SMEM = (size_t)(PW_ROWS * PW_LD + IE + 3 * PW_ROWS + 2 * PW_A) * sizeof(float);
constexpr int TN_T = 256, TN_BM = 128, TN_BN = 128, TN_PITCH = 80;   // bytes of one column's 32 bf16 k-values (+ 16 of padding)
constexpr int RED_JOBS = 6, RED_T = 256, RED_BLOCKS = 256, RED_WIDE_G = 64;

typedef __bf16 pw_b4 __attribute__((ext_vector_type(4)));

struct PwLabels { const int64_t* p[MHIMX_INFER_MAX]; };
// the survival head of mhimx_pure_window_run_surv: every bag's censorship flag, NLLSurvLoss(alpha), the clamp, risk [n_bags] or NULL
struct PwSurv { const float* censor[MHIMX_INFER_MAX]; float alpha, eps; float* risk; };
template <class T>
MHIMX_DEV const T& pw_surv_of(const T& sv) { return sv; }

// ------------------------------------------------------------------------------------------------ 4. merge + head + CE + their gradients
// blockIdx.x = bag.  infer_finalize_kernel's merge (partials in index order) and predictor, then the backward of the head:
// g_logits = main_alpha (softmax - onehot) / n, g_z = Wp^T g_logits, zg = z . g_z, the bag's d Wp / d bp partial.
// The criterion on the logits is the trailing pack SURV.  Empty: the cross entropy - the kernel, kernel arguments and instructions of
// before.  One PwSurv: the discrete-time survival NLL of surv_dev.hpp (mhimx_pure_window_run_surv); everything around it is one text.
template <class... SURV>
__global__ __launch_bounds__(RG_FIN_T) void pw_head_kernel(InferTab tab, PwLabels lab, const float* __restrict__ pm, const float* __restrict__ pl,
                                                         const float* __restrict__ pz, const float* __restrict__ wp, const float* __restrict__ bp,
                                                         int C, float main_alpha, float inv_n, float* __restrict__ logits,
                                                         float* __restrict__ losses, float* __restrict__ z_out, float* __restrict__ stats,
                                                         float* __restrict__ g_z, float* __restrict__ zg, float* __restrict__ dwp_part,
                                                         float* __restrict__ dbp_part, SURV... surv) {
  __shared__ float red[8];
  __shared__ float wgt[RG_FIN_T];
  __shared__ float zs[IE];
  __shared__ float lg[PW_MAXC], gl[PW_MAXC];
  const int bag = blockIdx.x;
  RG_BAG(bag)
  const int64_t* label = lab.p[0];
  RG_PICK(label, lab.p, bag)
  const int G = rg_parts(N);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  pm += p0; pl += p0; pz += (int64_t)p0 * IE;
  float mx, L;
  rg_merge_stats(pm, pl, G, 1, red, mx, L);
  const float invL = 1.f / L;
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
  const float zv = acc * invL;
  zs[tid] = zv;
  z_out[(int64_t)bag * IE + tid] = zv;
  __syncthreads();
  for (int c = wave; c < C; c += RG_FIN_T / 64) {
    float d = 0.f;
#pragma unroll
    for (int q = 0; q < IE / 64; ++q) d += zs[lane + 64 * q] * wp[(int64_t)c * IE + lane + 64 * q];
    d = wave_sum(d);
    if (lane == 0) {
      const float v = d + bp[c];
      lg[c] = v;
      logits[(int64_t)bag * C + c] = v;
    }
  }
  __syncthreads();
  if constexpr (sizeof...(SURV) == 1) {
    if (tid == 0) {
      // NLLSurvLoss on one row (train_utils.py:8-37; a bin outside [0, C): NaN loss, zero gradient row), gradient scale main_alpha / n
      const PwSurv& sv = pw_surv_of(surv...);
      const float* cens = sv.censor[0];
      RG_PICK(cens, sv.censor, bag)
      float l[PW_MAXC], g[PW_MAXC], rk, nll;
#pragma unroll
      for (int c = 0; c < PW_MAXC; ++c) l[c] = c < C ? lg[c] : 0.f;
      surv_row<PW_MAXC>(l, C, label[0], cens[0], sv.alpha, sv.eps, main_alpha * inv_n, true, rk, nll, g);
      losses[3 * bag] = main_alpha * nll;
      losses[3 * bag + 1] = nll;
      losses[3 * bag + 2] = 0.f;
      if (sv.risk) sv.risk[bag] = rk;
#pragma unroll
      for (int c = 0; c < PW_MAXC; ++c) {
        gl[c] = g[c];
        if (c < C) dbp_part[C * bag + c] = g[c];
      }
    }
  } else if (tid == 0) {
    // torch.nn.CrossEntropyLoss on one row (a label outside [0, C): NaN, where torch raises)
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
    for (int c = 0; c < PW_MAXC; ++c) {
      const float g = c < C ? (ok ? main_alpha * (expf(lg[c] - cm) / den - (c == y ? 1.f : 0.f)) * inv_n : NAN) : 0.f;
      gl[c] = g;
      if (c < C) dbp_part[C * bag + c] = g;
    }
  }
  __syncthreads();
  float gz = 0.f;
  for (int c = 0; c < C; ++c) {
    gz += gl[c] * wp[(int64_t)c * IE + tid];
    dwp_part[((int64_t)bag * C + c) * IE + tid] = gl[c] * zv;
  }
  g_z[(int64_t)bag * IE + tid] = gz;
  const float d = wave_sum(__fmul_rn(zv, gz));                 // (a plain product in both kernels: pw_pool_bwd_kernel sums h . g_z alike)
  if (lane == 0) red[wave] = d;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) t += red[w];
    zg[bag] = t;
  }
}

// ------------------------------------------------------------------------------------------------ 5. ragged one-pass pool backward
// blockIdx.x = 32-row tile of the call's row space (inside ONE bag).  Wave w owns scorer columns [32 w, 32 w + 32) of U exactly as
// infer_score_kernel does; thread t owns feature columns t and t + 256 of d h.
__global__ __launch_bounds__(PW_T, 2) void pw_pool_bwd_kernel(InferTab tab, const float* __restrict__ Hin, const _Float16* __restrict__ dact,
                                                              const float* __restrict__ s, const float* __restrict__ stats,
                                                              const float* __restrict__ g_z, const float* __restrict__ zg,
                                                              const float* __restrict__ wa_frag, const float* __restrict__ wa,
                                                              const float* __restrict__ wc, int act, float* __restrict__ dU,
                                                              float* __restrict__ dpre, float* __restrict__ db1_part,
                                                              float* __restrict__ dwc_part) {
  extern __shared__ __attribute__((aligned(16))) float pw_sm[];
  float* Hs = pw_sm;                          // [32][516] the tile's feature rows; later [128][36] d U, transposed
  float* dUs = pw_sm;
  float* gzs = Hs + PW_ROWS * PW_LD;          // [512] the bag's g_z
  float* prow = gzs + IE;                     // [32] softmax weights of the rows
  float* dsr = prow + PW_ROWS;                // [32] d s
  float* spare = dsr + PW_ROWS;               // [32]
  float* wcp = spare + PW_ROWS;               // [2][128] d wc halves
  const int tile = blockIdx.x;
  const int64_t r0 = (int64_t)tile * PW_ROWS;
  RG_FIND_BAG(r0, row0)
  int64_t N = tab.N[0], orow0 = tab.row0[0];
  RG_PICK(N, tab.N, bag) RG_PICK(orow0, tab.row0, bag)       // (not RG_BAG: with the unused p0 picked too the kernel does not keep its code)
  const int64_t left = N - (r0 - orow0);
  const int M = left < PW_ROWS ? (int)left : PW_ROWS;          // real rows of the tile (>= 1)
  const float mx = stats[2 * bag], invL = 1.f / stats[2 * bag + 1], zgb = zg[bag];
  const float* T = Hin + r0 * IE;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r32 = lane & 31, kg = lane >> 5;
  const int n_col = 32 * wave + r32;
  const float wn = wc[n_col];
  const f32x4* fptr = reinterpret_cast<const f32x4*>(wa_frag + ((int64_t)wave * (IE / 16) * 64 + lane) * 8);
  const float* aptr = Hs + r32 * PW_LD + 8 * kg;

#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int f = tid + PW_T * i, r = f >> 7, c4 = f & 127;
    f32x4 v = reinterpret_cast<const f32x4*>(T + (int64_t)(r < M ? r : M - 1) * IE)[c4];
    if (r >= M) v = f32x4{0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(Hs + r * PW_LD + 4 * c4) = v;
  }
  const float gz0 = g_z[(int64_t)bag * IE + tid], gz1 = g_z[(int64_t)bag * IE + tid + PW_T];
  gzs[tid] = gz0;
  gzs[tid + PW_T] = gz1;
  if (tid < PW_ROWS) prow[tid] = tid < M ? __expf(s[r0 + tid] - mx) * invL : 0.f;
  __syncthreads();
  // ---- d s[r] = p[r] (h_r . g_z - z . g_z): wave w takes rows 8 w .. 8 w + 7
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int r = 8 * wave + j;
    // (summed in the order pw_head_kernel sums z . g_z - 64-column blocks, then the blocks in index order - so that the two dot products
    // round alike: for a bag of ONE row, where z = h, d s is exactly zero as the softmax of one score demands)
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < IE / 64; ++q) v += wave_sum(__fmul_rn(Hs[r * PW_LD + lane + 64 * q], gzs[lane + 64 * q]));   // (never contracted)
    if (lane == 0) dsr[r] = prow[r] * (v - zgb);
  }
  // ---- U tile on the matrix cores, one accumulator per bf16x3 term (infer_score_kernel's loop; own text: rg_mma3 moved this kernel's code)
  f32x16 acc, acc2, acc3;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc[i] = 0.f; acc2[i] = 0.f; acc3[i] = 0.f; }
  {
    f32x4 bh = fptr[0], bl = fptr[1];
#pragma unroll 4
    for (int ks = 0; ks < IE / 16; ++ks) {
      const int kn = ks + 1 < IE / 16 ? ks + 1 : ks;
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
  }
  __syncthreads();                             // every wave is past its reads of Hs (d U takes its place), dsr is complete
  // ---- d U[r][a] = d s[r] wc[a] da_act'(U[r][a]),  d wc[a] partial = sum_r d s[r] da_act(U[r][a]);  acc[i] = U[8 (i >> 2) + 4 kg + (i & 3)][n_col]
  {
    float wsum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = 8 * (i >> 2) + 4 * kg + (i & 3);
      const float u = acc[i] + (acc2[i] + acc3[i]);
      float y, g;
      act_fwd_grad(u, act, y, g);
      const float dsv = dsr[row];
      dUs[n_col * PW_DUP + row] = dsv * wn * g;
      wsum += dsv * y;
    }
    wcp[kg * PW_A + n_col] = wsum;
  }
  __syncthreads();
  if (tid < PW_A) dwc_part[(int64_t)tile * PW_A + tid] = wcp[tid] + wcp[PW_A + tid];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int f = tid + PW_T * i, r = f >> 7, a = f & 127;
    dU[(r0 + r) * PW_A + a] = dUs[a * PW_DUP + r];
  }
  // ---- d h[r][e] = p[r] g_z[e] + sum_a d U[r][a] Wa[a][e]   (fp32; columns e = tid, tid + 256)
  float h0[PW_ROWS], h1[PW_ROWS];
#pragma unroll
  for (int q = 0; q < PW_ROWS / 4; ++q) {
    const f32x4 p = reinterpret_cast<const f32x4*>(prow)[q];
#pragma unroll
    for (int j = 0; j < 4; ++j) { h0[4 * q + j] = p[j] * gz0; h1[4 * q + j] = p[j] * gz1; }
  }
#pragma unroll 2
  for (int a = 0; a < PW_A; ++a) {
    const float w0 = wa[(int64_t)a * IE + tid], w1 = wa[(int64_t)a * IE + tid + PW_T];
#pragma unroll
    for (int q = 0; q < PW_ROWS / 4; ++q) {
      const f32x4 d = *reinterpret_cast<const f32x4*>(dUs + a * PW_DUP + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        h0[4 * q + j] = fmaf(d[j], w0, h0[4 * q + j]);
        h1[4 * q + j] = fmaf(d[j], w1, h1[4 * q + j]);
      }
    }
  }
  // ---- epilogue: dPRE = d h * d out / d pre (zero rows past the bag's N), the tile's column sums
  float s0 = 0.f, s1 = 0.f;
  const _Float16* db = dact + r0 * IE;
  float* po = dpre + r0 * IE;
#pragma unroll
  for (int r = 0; r < PW_ROWS; ++r) {
    float d0 = 0.f, d1 = 0.f;
    if (r < M) {
      d0 = h0[r] * (float)db[(int64_t)r * IE + tid];
      d1 = h1[r] * (float)db[(int64_t)r * IE + tid + PW_T];
    }
    po[(int64_t)r * IE + tid] = d0;
    po[(int64_t)r * IE + tid + PW_T] = d1;
    s0 += d0;
    s1 += d1;
  }
  db1_part[(int64_t)tile * IE + tid] = s0;
  db1_part[(int64_t)tile * IE + tid + PW_T] = s1;
}

// ------------------------------------------------------------------------------------------------ 6, 7. C = A^T B over the row space
// slab z of C[M, Nc] = sum over the k-steps (32 rows) of slab z of A[rows, m]^T B[rows, n]; 128 x 128 output tile per workgroup, 4 waves as
// 2 x 2, 64 x 64 per wave = 2 x 2 blocks of v_mfma_f32_32x32x16_bf16 in the 3-term bf16 form.  Both operands come in as fp32 rows (16-byte
// coalesced loads one k-step ahead), are split to bf16 hi / lo and written to LDS TRANSPOSED (a column's 32 k-values contiguous), so that a
// fragment is one 16-byte LDS read.  BAGX: B = the bags' X, each where it lies: the k-step's bag from the table, rows past its N clamped
// (their A rows are zero rows).  XT (BAGX only; MHIMX_X_*): fp16 / bf16 bag rows come in as 8-byte loads of 4 elements and are widened to fp32
// (x_widen: exact) in front of the same split - the LDS image is that of the fp32 kernel on the widened rows (B / ldb: unused there).
template <bool BAGX, int XT>
__global__ __launch_bounds__(TN_T, 2) void pw_tn_kernel(InferTab tab, const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb,
                                                        int steps, int steps_per, float* __restrict__ slabs, int M, int Nc) {
  __shared__ __attribute__((aligned(16))) char lds[4][TN_BM * TN_PITCH];      // A hi, A lo, B hi, B lo
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * TN_BM, n0 = blockIdx.x * TN_BN, z = blockIdx.z;
  const int ks0 = z * steps_per, ks1 = ks0 + steps_per < steps ? ks0 + steps_per : steps;
  const int c4 = tid & 31, rg = tid >> 5;                     // this thread's 4 columns and 4 rows (4 rg .. 4 rg + 3) of a k-step
  typedef typename XRow<XT>::v4 XV4;
  f32x4 ra[4];
  XV4 rb[4];
  auto load = [&](int ks) {
    const int64_t row = (int64_t)ks * 32 + 4 * rg;
#pragma unroll
    for (int j = 0; j < 4; ++j) ra[j] = *reinterpret_cast<const f32x4*>(A + (row + j) * lda + m0 + 4 * c4);
    if constexpr (BAGX) {
      const int64_t k0 = (int64_t)ks * 32;
      RG_FIND_BAG(k0, row0)
      const float* X = tab.X[0];
      int64_t ldx = tab.ldx[0], N = tab.N[0], orow0 = tab.row0[0];
      RG_PICK(X, tab.X, bag) RG_PICK(ldx, tab.ldx, bag) RG_PICK(N, tab.N, bag) RG_PICK(orow0, tab.row0, bag)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int64_t rin = row + j - orow0;
        if (rin >= N) rin = N - 1;
        rb[j] = *reinterpret_cast<const XV4*>(reinterpret_cast<const typename XRow<XT>::elt*>(X) + rin * ldx + n0 + 4 * c4);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) rb[j] = *reinterpret_cast<const XV4*>(B + (row + j) * ldb + n0 + 4 * c4);
    }
  };
  auto store = [&](const f32x4 (&r)[4], char* hi_p, char* lo_p) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      pw_b4 hi, lo;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const __bf16 h = (__bf16)r[j][q];
        hi[j] = h;
        lo[j] = (__bf16)(r[j][q] - (float)h);
      }
      const int off = (4 * c4 + q) * TN_PITCH + 8 * rg;
      *reinterpret_cast<pw_b4*>(hi_p + off) = hi;
      *reinterpret_cast<pw_b4*>(lo_p + off) = lo;
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  const int r32 = lane & 31, kg = lane >> 5;
  if (ks0 < ks1) load(ks0);
#pragma unroll 1
  for (int ks = ks0; ks < ks1; ++ks) {
    __syncthreads();                                          // the previous k-step's fragment reads are over
    store(ra, lds[0], lds[1]);
    if constexpr (XT == 0) {
      store(rb, lds[2], lds[3]);
    } else {
      f32x4 rw[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) rw[j] = x_widen<XT>(rb[j]);
      store(rw, lds[2], lds[3]);
    }
    __syncthreads();
    if (ks + 1 < ks1) load(ks + 1);
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
      bf8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int ao = (wm * 64 + i * 32 + r32) * TN_PITCH + 32 * k2 + 16 * kg;
        const int bo = (wn * 64 + i * 32 + r32) * TN_PITCH + 32 * k2 + 16 * kg;
        ah[i] = *reinterpret_cast<const bf8*>(lds[0] + ao);
        al[i] = *reinterpret_cast<const bf8*>(lds[1] + ao);
        bh[i] = *reinterpret_cast<const bf8*>(lds[2] + bo);
        bl[i] = *reinterpret_cast<const bf8*>(lds[3] + bo);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        }
    }
  }
  float* out = slabs + (int64_t)z * M * Nc;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * 64 + i * 32 + 8 * (e >> 2) + 4 * kg + (e & 3);
        const int col = n0 + wn * 64 + j * 32 + r32;
        out[(int64_t)row * Nc + col] = acc[i][j][e];
      }
}

// ------------------------------------------------------------------------------------------------ 8. every partial buffer, in index order
// blockIdx.y = job: out[i] = sum_{g < G} parts[g W + i].  Up to RED_WIDE_G partials: one thread per element, g = 0, 1, .. in order.  More
// (the per-tile partials of a long window): 16 threads per element, thread j sums g = j, j + 16, .. in order, the 16 sums are added in
// index order - a fixed tree either way.
struct PwRed { const float* parts[RED_JOBS]; float* out[RED_JOBS]; int64_t W[RED_JOBS]; int32_t G[RED_JOBS]; };
__global__ __launch_bounds__(RED_T) void pw_reduce_kernel(PwRed r) {
  __shared__ float part[16][17];
  const int job = blockIdx.y;
  const float* parts = r.parts[0];
  float* out = r.out[0];
  int64_t W = r.W[0];
  int G = r.G[0];
#pragma unroll
  for (int q = 0; q < RED_JOBS; ++q)
    if (q == job) { parts = r.parts[q]; out = r.out[q]; W = r.W[q]; G = r.G[q]; }
  if (G <= RED_WIDE_G) {
    for (int64_t i = (int64_t)blockIdx.x * RED_T + threadIdx.x; i < W; i += (int64_t)gridDim.x * RED_T) {
      float a = 0.f;
      for (int g = 0; g < G; ++g) a += parts[(int64_t)g * W + i];
      out[i] = a;
    }
    return;
  }
  const int col = threadIdx.x & 15, gl = threadIdx.x >> 4;
  for (int64_t base = (int64_t)blockIdx.x * 16; base < W; base += (int64_t)gridDim.x * 16) {      // (uniform per block)
    const int64_t i = base + col;
    float a = 0.f;
    if (i < W) {
#pragma unroll 8
      for (int g = gl; g < G; g += 16) a += parts[(int64_t)g * W + i];
    }
    __syncthreads();
    part[gl][col] = a;
    __syncthreads();
    if (gl == 0 && i < W) {
      float t = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) t += part[j][col];
      out[i] = t;
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
struct PwLay {
  int64_t w1p, wa_frag, H, dact, s, pm, pl, pz, stats, z, logits, losses, g_z, zg, dwp_part, dbp_part, dU, dpre, db1_part, dwc_part, slab_a,
      slab_1, total;
  int64_t rows;                          // rows of the call's row space (every bag rounded up to a multiple of 32)
  int32_t steps, sa, sa_per, s1, s1_per;
};

// xdt: the element type of the bags' rows (MHIMX_X_*); the 2-byte types have their own pitch rule (16-byte rows: 8 elements)
int check_pw(const mhimx_step_cfg* c, int32_t n_bags, const mhimx_pure_window_bag* bags, int32_t xdt = MHIMX_X_F32) {
  if (int r = rg_check_xdt("pure_window", xdt)) return r;
  MHIMX_CHECK_ARG(c && bags, "pure_window: null configuration / bag list");
  MHIMX_CHECK_ARG(n_bags >= 1 && n_bags <= MHIMX_PURE_WINDOW_MAX, "pure_window: 1..%d bags per window (got %d)", MHIMX_PURE_WINDOW_MAX, n_bags);
  MHIMX_CHECK_ARG(c->E == IE && c->A == PW_A && c->C >= 1 && c->C <= PW_MAXC && c->D > 0 && c->D % 256 == 0 && c->D <= (1 << 20),
                  "pure_window: shapes outside the ragged ABMIL window (E = 512, A = 128, C <= 4, D %% 256 == 0)");
  MHIMX_CHECK_ARG(c->act >= MHIMX_ACT_NONE && c->act <= MHIMX_ACT_TANH && c->da_act >= MHIMX_ACT_NONE && c->da_act <= MHIMX_ACT_TANH,
                  "pure_window: unknown activation");
  MHIMX_CHECK_ARG(c->drop_p_student >= 0.f && c->drop_p_student < 1.f, "pure_window: dropout probability outside [0,1)");
  const mhimx_step_params& s = c->student;
  MHIMX_CHECK_ARG(s.w1 && s.b1 && s.wa && s.wc && s.wp && s.bp, "pure_window: null student parameter");
  MHIMX_CHECK_ARG(aligned16(s.w1) && aligned16(s.b1) && aligned16(s.wa), "pure_window: feature / scorer weights must be 16-byte aligned");
  const mhimx_step_grads& g = c->grad;
  MHIMX_CHECK_ARG(g.w1 && g.b1 && g.wa && g.wc && g.wp && g.bp, "pure_window: null gradient view");
  MHIMX_CHECK_ARG(c->tick, "pure_window: the device dropout counter (tick) is required");
  int64_t rows = 0;
  for (int b = 0; b < n_bags; ++b) {
    if (int r = rg_check_bag("pure_window", b, bags[b].N, bags[b].ldx, c->D, xdt, RgRules{MHIMX_STEP_MAX_ROWS, true})) return r;
    rows += align_up(bags[b].N, PW_ROWS);
  }
  MHIMX_CHECK_ARG(rows <= MHIMX_PURE_WINDOW_MAX_ROWS, "pure_window: %lld rows in the window's row space, at most %d", (long long)rows,
                  MHIMX_PURE_WINDOW_MAX_ROWS);
  return 0;
}

void pw_layout(const mhimx_step_cfg* c, int32_t n_bags, const mhimx_pure_window_bag* bags, PwLay* w, InferTab* tab, int64_t* row0_out) {
  RgCount cnt;
  for (int b = 0; b < n_bags; ++b) {
    if (row0_out) row0_out[b] = cnt.rows;
    rg_tab_add(tab, cnt, b, bags[b].X, bags[b].ldx, bags[b].N, align_up(bags[b].N, PW_ROWS));
  }
  rg_tab_close(tab, cnt, n_bags);
  const int64_t rows = cnt.rows, parts = cnt.parts;
  const int64_t E = c->E, D = c->D, A = c->A, C = c->C, n = n_bags;
  w->rows = rows;
  w->steps = (int32_t)(rows / PW_ROWS);
  // split-K slabs: enough workgroups to fill the part (4 output tiles for d Wa, 4 D / 128 for d W1), never an empty slab
  const int sa_room = pw_split_k(w->steps, 64, 4, &w->sa, &w->sa_per);
  const int s1_room = pw_split_k(w->steps, 8, 8, &w->s1, &w->s1_per);
  Arena ar(nullptr, 0);
  w->w1p = ar.off; ar.take<float>(E * D);
  w->wa_frag = ar.off; ar.take<float>(A * E);
  w->logits = ar.off; ar.take<float>(n * C);
  w->losses = ar.off; ar.take<float>(n * 3);
  w->stats = ar.off; ar.take<float>(n * 2);
  w->z = ar.off; ar.take<float>(n * E);
  w->g_z = ar.off; ar.take<float>(n * E);
  w->zg = ar.off; ar.take<float>(n);
  w->dwp_part = ar.off; ar.take<float>(n * C * E);
  w->dbp_part = ar.off; ar.take<float>(n * PW_MAXC);
  w->H = ar.off; ar.take<float>(rows * E);
  w->dact = ar.off; ar.take<_Float16>(rows * E);
  w->s = ar.off; ar.take<float>(rows);
  w->pm = ar.off; ar.take<float>(parts);
  w->pl = ar.off; ar.take<float>(parts);
  w->pz = ar.off; ar.take<float>(parts * E);
  w->dU = ar.off; ar.take<float>(rows * A);
  w->dpre = ar.off; ar.take<float>(rows * E);
  w->db1_part = ar.off; ar.take<float>((int64_t)w->steps * E);
  w->dwc_part = ar.off; ar.take<float>((int64_t)w->steps * A);
  w->slab_a = ar.off; ar.take<float>((int64_t)sa_room * A * E);
  w->slab_1 = ar.off; ar.take<float>((int64_t)s1_room * E * D);
  w->total = ar.off;
}

}  // namespace

// ---- for mhimx_ragged_window_run (ragged_window.hip) and this file's own layout / run: the split-K rule, the d W1 launch and the reduction launch as host calls
// split-K slabs for `steps` 32-row k-steps: steps / div of them, 1 .. want_max, never an empty one.  Returns the slabs to make ROOM for (a
// count that never shrinks when the window grows); *S <= room are written, *per k-steps each.
int pw_split_k(int steps, int want_max, int div, int32_t* S, int32_t* per) {
  int s = steps / div;
  s = s < 1 ? 1 : (s > want_max ? want_max : s);
  *per = (int32_t)cdiv(steps, s);
  *S = (int32_t)cdiv(steps, *per);
  return s;
}
// slabs[z][512][D] = sum over the k-steps of slab z of dpre[rows, 512]^T X_b[rows, D]: launch 7 of the header over the table's row space
int pw_wgrad_bagx(hipStream_t st, const InferTab& tab, const float* dpre, int D, int steps, int S, int per, float* slabs) {
  if (tab.pad != MHIMX_X_F32) {                                 // (tab.pad: the element type of the bags' rows; the entry points have checked it)
    const dim3 grid((unsigned)(D / TN_BN), IE / TN_BM, (unsigned)S);
    if (tab.pad == MHIMX_X_F16) hipLaunchKernelGGL((pw_tn_kernel<true, 1>), grid, dim3(TN_T), 0, st, tab, dpre, IE, nullptr, 0, steps, per, slabs, IE, D);
    else hipLaunchKernelGGL((pw_tn_kernel<true, 2>), grid, dim3(TN_T), 0, st, tab, dpre, IE, nullptr, 0, steps, per, slabs, IE, D);
    MHIMX_LAUNCH_CHECK();
    return 0;
  }
  hipLaunchKernelGGL((pw_tn_kernel<true, 0>), dim3((unsigned)(D / TN_BN), IE / TN_BM, (unsigned)S), dim3(TN_T), 0, st, tab, dpre, IE, nullptr, 0, steps, per, slabs,
                     IE, D);
  MHIMX_LAUNCH_CHECK();
  return 0;
}
// slabs[z][M][Nc] = sum over the k-steps of slab z of A[rows, M]^T B[rows, Nc], both operands fp32 rows of the row space: launch 6 of the header
int pw_wgrad_rows(hipStream_t st, const InferTab& tab, const float* A, int lda, int M, const float* B, int ldb, int Nc, int steps, int S, int per,
                  float* slabs) {
  MHIMX_CHECK_ARG(M >= TN_BM && M % TN_BM == 0 && Nc >= TN_BN && Nc % TN_BN == 0 && lda >= M && ldb >= Nc && lda % 4 == 0 && ldb % 4 == 0,
                  "pw_wgrad_rows: M and Nc must be multiples of 128 inside their pitches");
  hipLaunchKernelGGL((pw_tn_kernel<false, 0>), dim3((unsigned)(Nc / TN_BN), (unsigned)(M / TN_BM), (unsigned)S), dim3(TN_T), 0, st, tab, A, lda, B, ldb, steps,
                     per, slabs, M, Nc);
  MHIMX_LAUNCH_CHECK();
  return 0;
}
// out_j[i] = sum_{g < G_j} parts_j[g W_j + i], j < n <= 6, in index order: launch 8 of the header
int pw_reduce(hipStream_t st, int n, const float* const* parts, const int32_t* G, const int64_t* W, float* const* out) {
  MHIMX_CHECK_ARG(n >= 1 && n <= RED_JOBS, "pw_reduce: 1..%d jobs", RED_JOBS);
  PwRed r = {};
  for (int j = 0; j < n; ++j) { r.parts[j] = parts[j]; r.G[j] = G[j]; r.W[j] = W[j]; r.out[j] = out[j]; }
  hipLaunchKernelGGL(pw_reduce_kernel, dim3(RED_BLOCKS, RED_JOBS), dim3(RED_T), 0, st, r);
  MHIMX_LAUNCH_CHECK();
  return 0;
}

}  // namespace mhimx

extern "C" int mhimx_pure_window_layout_of(const mhimx_step_cfg* cfg, int32_t n_bags, const mhimx_pure_window_bag* bags,
                                           mhimx_pure_window_layout* out) {
  using namespace mhimx;
  MHIMX_CHECK_ARG(out, "pure_window_layout: null output");
  if (int r = check_pw(cfg, n_bags, bags)) return r;
  PwLay w;
  memset(out, 0, sizeof(*out));
  pw_layout(cfg, n_bags, bags, &w, nullptr, out->row0);
  out->total = w.total; out->rows = w.rows; out->logits = w.logits; out->losses = w.losses; out->H = w.H; out->dact = w.dact; out->s = w.s;
  out->stats = w.stats; out->z = w.z; out->g_z = w.g_z;
  return 0;
}

extern "C" int mhimx_pure_window_run(void* stream, const mhimx_step_cfg* cfg, int32_t n_bags, const mhimx_pure_window_bag* bags,
                                     int64_t host_step, void* ws, int64_t ws_bytes, int32_t update) {
  return mhimx_pure_window_run_x(stream, cfg, n_bags, bags, host_step, ws, ws_bytes, update, MHIMX_X_F32);
}

extern "C" int mhimx_pure_window_run_x(void* stream, const mhimx_step_cfg* cfg, int32_t n_bags, const mhimx_pure_window_bag* bags,
                                       int64_t host_step, void* ws, int64_t ws_bytes, int32_t update, int32_t x_dtype) {
  return mhimx::pure_window_run(stream, cfg, n_bags, bags, host_step, ws, ws_bytes, update, x_dtype, nullptr);
}

extern "C" int mhimx_pure_window_run_surv(void* stream, const mhimx_step_cfg* cfg, int32_t n_bags, const mhimx_pure_window_bag* bags,
                                          int64_t host_step, void* ws, int64_t ws_bytes, int32_t update, int32_t x_dtype,
                                          const mhimx_surv_spec* surv) {
  MHIMX_CHECK_ARG(surv, "pure_window: null survival description (mhimx_pure_window_run_x is the classification call)");
  return mhimx::pure_window_run(stream, cfg, n_bags, bags, host_step, ws, ws_bytes, update, x_dtype, surv);
}

// the one body of mhimx_pure_window_run(_x) (surv NULL: cross entropy) and mhimx_pure_window_run_surv
int mhimx::pure_window_run(void* stream, const mhimx_step_cfg* cfg, int32_t n_bags, const mhimx_pure_window_bag* bags, int64_t host_step, void* ws,
                           int64_t ws_bytes, int32_t update, int32_t x_dtype, const mhimx_surv_spec* surv) {
  if (int r = check_pw(cfg, n_bags, bags, x_dtype)) return r;
  if (surv)
    if (int r = surv_spec_check("pure_window", n_bags, surv)) return r;
  for (int b = 0; b < n_bags; ++b) {
    MHIMX_CHECK_ARG(bags[b].X && aligned16(bags[b].X), "pure_window: bag %d: null or unaligned rows", b);
    MHIMX_CHECK_ARG(bags[b].label_dev, "pure_window: bag %d: null label", b);
  }
  MHIMX_CHECK_ARG(!update || (cfg->p && cfg->g && cfg->m && cfg->v && cfg->n_train > 0 && cfg->n_all >= cfg->n_train),
                  "pure_window: update needs the flat optimiser buffers");
  PwLay w;
  InferTab tab = {};
  pw_layout(cfg, n_bags, bags, &w, &tab, nullptr);
  tab.pad = x_dtype;                           // read by the two launches that read X: the projection (2) and d W1 (7)
  if (int r = rg_check_ws("pure_window", ws, ws_bytes, w.total)) return r;
  const mhimx_step_cfg& c = *cfg;
  const mhimx_step_params& S = c.student;
  hipStream_t st = (hipStream_t)stream;
  char* base = static_cast<char*>(ws);
  auto F = [&](int64_t off) { return reinterpret_cast<float*>(base + off); };
  const int D = (int)c.D, C = (int)c.C;
  float *w1p = F(w.w1p), *wa_frag = F(w.wa_frag), *H = F(w.H), *s = F(w.s), *pm = F(w.pm), *pl = F(w.pl), *pz = F(w.pz);
  _Float16* dact = reinterpret_cast<_Float16*>(base + w.dact);

  // ---- 1. counters and weight images
  {
    mhimx_prep_job jobs[4];
    int n = prep_counters(c, jobs);
    jobs[n++] = mhimx_prep_job{1, S.w1, w1p, c.E, c.D};
    jobs[n++] = mhimx_prep_job{4, S.wa, wa_frag, c.A, c.E};
    if (int r = mhimx_prep_batch(stream, jobs, n)) return r;
  }
  // ---- 2. feature rows, dropout, d out / d pre of every bag
  {
    PureWinDrop dr = {};
    for (int b = 0; b < n_bags; ++b) dr.seed[b] = bags[b].drop_seed;
    dr.tick = c.tick; dr.dact = dact; dr.drop_p = c.drop_p_student;
    if (int r = pure_window_project(st, tab, dr, D, w1p, S.b1, c.act, H)) return r;
  }
  // ---- 3. scores + pool partials
  if (int r = infer_score(st, tab, H, wa_frag, S.wc, c.da_act, s, pm, pl, pz)) return r;
  // ---- 4. merge, head, CE and their gradients
  {
    PwLabels lab = {};
    for (int b = 0; b < n_bags; ++b) lab.p[b] = bags[b].label_dev;
    if (surv) {
      PwSurv sv = {};
      for (int b = 0; b < n_bags; ++b) sv.censor[b] = surv->censor_dev[b];
      sv.alpha = surv->alpha; sv.eps = surv->eps; sv.risk = surv->risk;
      hipLaunchKernelGGL(pw_head_kernel<PwSurv>, dim3((unsigned)n_bags), dim3(RG_FIN_T), 0, st, tab, lab, pm, pl, pz, S.wp, S.bp, C, c.main_alpha,
                         1.f / (float)n_bags, F(w.logits), F(w.losses), F(w.z), F(w.stats), F(w.g_z), F(w.zg), F(w.dwp_part), F(w.dbp_part), sv);
    } else {
      hipLaunchKernelGGL(pw_head_kernel<>, dim3((unsigned)n_bags), dim3(RG_FIN_T), 0, st, tab, lab, pm, pl, pz, S.wp, S.bp, C, c.main_alpha,
                         1.f / (float)n_bags, F(w.logits), F(w.losses), F(w.z), F(w.stats), F(w.g_z), F(w.zg), F(w.dwp_part), F(w.dbp_part));
    }
    MHIMX_LAUNCH_CHECK();
  }
  // ---- 5. pool backward over the row space
  MHIMX_ONCE_PER_DEVICE(MHIMX_HIP(hipFuncSetAttribute((const void*)pw_pool_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PW_BWD_SMEM)));
  hipLaunchKernelGGL(pw_pool_bwd_kernel, dim3((unsigned)w.steps), dim3(PW_T), PW_BWD_SMEM, st, tab, H, dact, s, F(w.stats), F(w.g_z), F(w.zg), wa_frag,
                     S.wa, S.wc, c.da_act, F(w.dU), F(w.dpre), F(w.db1_part), F(w.dwc_part));
  MHIMX_LAUNCH_CHECK();
  // ---- 6. d Wa = dU^T H
  hipLaunchKernelGGL((pw_tn_kernel<false, 0>), dim3(IE / TN_BN, PW_A / TN_BM, (unsigned)w.sa), dim3(TN_T), 0, st, tab, F(w.dU), PW_A, H, IE, w.steps, w.sa_per,
                     F(w.slab_a), PW_A, IE);
  MHIMX_LAUNCH_CHECK();
  // ---- 7. d W1 = sum_b dPRE_b^T X_b
  if (int r = pw_wgrad_bagx(st, tab, F(w.dpre), D, w.steps, w.s1, w.s1_per, F(w.slab_1))) return r;
  // ---- 8. the partial buffers, in index order, into the gradient views
  {
    const float* parts[RED_JOBS] = {F(w.slab_1), F(w.slab_a), F(w.db1_part), F(w.dwc_part), F(w.dwp_part), F(w.dbp_part)};
    const int32_t G[RED_JOBS] = {w.s1, w.sa, w.steps, w.steps, n_bags, n_bags};
    const int64_t W[RED_JOBS] = {(int64_t)c.E * c.D, (int64_t)c.A * c.E, c.E, c.A, (int64_t)C * c.E, C};
    float* out[RED_JOBS] = {c.grad.w1, c.grad.wa, c.grad.b1, c.grad.wc, c.grad.wp, c.grad.bp};
    if (int r = pw_reduce(st, RED_JOBS, parts, G, W, out)) return r;
  }
  if (!update) return 0;
  // ---- 9. Adam
  const mhimx_optim_args o = optim_args_of(c, host_step, false);
  return mhimx_optim_step(stream, &o);
}
