// infer.hip — eval-mode MHIM(ABMIL) forward of up to MHIMX_INFER_MAX bags of DIFFERENT row counts in one call
// (modules/mhim.py:229-272 forward_test with merge_test off, engines/common_mil.py:56-68, engines/base_engine.py:234-329):
//
//     h = act(X W1^T + b1),  s = wc . da_act(h Wa^T),  z = softmax(s) h,  logits = z Wp^T + bp,  loss = CE(logits, label)
//
// The library's first RAGGED launches; what the three later ragged calls share with them lives in infer_tab.hpp.
// Everything a kernel needs to know about a bag travels in one by-value table (InferTab: pointer,
// pitch, rows, first row tile, first pool partial, row offset), so the call copies nothing to the device, waits for nothing and allocates
// nothing: it can be captured in a graph.  Four launches whatever n_bags is:
//   1  mhimx_prep_batch        the paired-plane image of W1 and the matrix-core fragment image of Wa (weights change between epochs)
//   2  infer_project_kernel    (bag_project.hip, beside the kernel it is modelled on) 160 x 256 output tiles, row tiles numbered
//                              bag-major, a bag's last tile partial; 3-term bf16, ONE model, no dropout / d out / d pre: feature rows -> ws
//   3  infer_score_kernel<false>  one workgroup per CHUNK of 256 rows of one bag: 32-row tiles through LDS, U = h Wa^T on the matrix
//                              cores (3-term bf16), scores, the running log-sum-exp pool partial (max, sum, sum_r e^{s_r - max} h_r)
//   4  infer_finalize_kernel   plane x = bag: block y = 0 merges the bag's partials in index order -> stats, z, logits, loss;
//                              blocks y > 0 write the attention map from the same merged {max, sum}
// No workgroup waits for another: tiles and chunks are independent, merging is the next launch's work.  A bag's tiles, chunks and
// partial order depend on its own N alone, so its results have the same bits wherever it stands in a call.
#include <math.h>

#include "infer_tab.hpp"

namespace mhimx {

namespace {

constexpr int IA = 128;
constexpr size_t SC_SMEM = (size_t)(RG_ROWS * RG_LD + 4 * RG_ROWS + 2 * RG_ROWS) * sizeof(float);
constexpr int FIN_ATTN_BLOCKS = 8, FIN_MAXC = 16;

// ------------------------------------------------------------------------------------------------ 3. ragged scorer + pool partial
// sum over the 32 lanes that share (lane >> 5); valid in lanes 16..31 and 48..63
MHIMX_DEV float sc_sum32(float v) {
  v += dpp_mov<0xB1, 0xf>(0.f, v);
  v += dpp_mov<0x4E, 0xf>(0.f, v);
  v += dpp_mov<0x141, 0xf>(0.f, v);
  v += dpp_mov<0x140, 0xf>(0.f, v);
  v += dpp_mov<0x142, 0xa>(0.f, v);
  return v;
}

// blockIdx.x = pool partial = chunk of RG_CHUNK rows of ONE bag (the last chunk of a bag may be short).  Wave w owns scorer columns
// [32 w, 32 w + 32): v_mfma_f32_32x32x16_bf16, A = the tile's rows from LDS split on the fly, B = the prep kind-4 image of Wa.
// CPROJ (mhimx_ragged_window_run's teacher, ragged_window.hip): while a tile's rows are LDS-resident, the class projections h_r . Wp_c the
// pseudo score needs (scoring.py:37-58) are taken from the same copy - 8 lanes per row, lane `seg` the 16-byte groups seg, seg + 8, .. of the
// row, the 8 partial sums added in a fixed xor tree - and written as cproj[row of the row space][4] (C <= 4; columns >= C are zero).  The
// plain launch passes nulls for wp / C / cproj: the last three arguments, so that no kernarg offset depends on CPROJ.
template <bool CPROJ>
__global__ __launch_bounds__(RG_T, 2) void infer_score_kernel(InferTab tab, const float* __restrict__ Hin, const float* __restrict__ wa_frag,
                                                              const float* __restrict__ wc, int act, float* __restrict__ s_out,
                                                              float* __restrict__ pm, float* __restrict__ pl, float* __restrict__ pz,
                                                              const float* __restrict__ wp, int C, float* __restrict__ cproj) {
  extern __shared__ __attribute__((aligned(16))) float sc_sm[];
  float* Hs = sc_sm;                          // [32][516]
  float* sred = Hs + RG_ROWS * RG_LD;         // [4][32] per-wave partial scores
  float* srow = sred + 4 * RG_ROWS;           // [32] scores
  float* prow = srow + RG_ROWS;               // [32] e^{s - m}
  const int part = blockIdx.x;
  RG_BAG_OF(part, part0)
  const int64_t c0 = (int64_t)(part - p0) * RG_CHUNK;          // first row of the chunk inside its bag
  const int64_t M = (N - c0 < RG_CHUNK) ? N - c0 : RG_CHUNK;    // rows of the chunk (>= 1)
  const float* T = Hin + (orow0 + c0) * IE;
  float* so = s_out + orow0 + c0;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r32 = lane & 31, kg = lane >> 5;
  const int n_col = 32 * wave + r32;
  const float wn = wc[n_col];
  const f32x4* fptr = reinterpret_cast<const f32x4*>(wa_frag + ((int64_t)wave * (IE / 16) * 64 + lane) * 8);   // + ks * 128 (hi), + 1 (lo)
  const float* aptr = Hs + r32 * RG_LD + 8 * kg;

  float m_run = -INFINITY, l_run = 0.f, z0 = 0.f, z1 = 0.f;
  const int tiles = (int)((M + RG_ROWS - 1) / RG_ROWS);
  for (int tile = 0; tile < tiles; ++tile) {
    const int64_t row0 = (int64_t)tile * RG_ROWS;
    // ---- rows -> LDS (rows past the chunk: zeros; their loads are clamped so that all 16 are in flight).  (This loop and the k-loop below
    // are this kernel's own text: as shared functions they moved its code - profiles/ragged_shared.md)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int f = tid + RG_T * i, r = f >> 7, c4 = f & 127;
      const int64_t nr = row0 + r;
      f32x4 v = reinterpret_cast<const f32x4*>(T + (nr < M ? nr : M - 1) * IE)[c4];
      if (nr >= M) v = f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(Hs + r * RG_LD + 4 * c4) = v;
    }
    __syncthreads();
    // ---- U tile on the matrix cores (3-term bf16)
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
    // ---- scores: acc[i] = U[row = 8 (i >> 2) + 4 kg + (i & 3)][n_col]
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = 8 * (i >> 2) + 4 * kg + (i & 3);
      const float u = acc[i] + (acc2[i] + acc3[i]);
      const float v = sc_sum32(wn * act_fwd(u, act));
      if (r32 == 31) sred[wave * RG_ROWS + row] = v;
    }
    __syncthreads();
    if (tid < RG_ROWS) {
      const int64_t nr = row0 + tid;
      float s = (sred[tid] + sred[RG_ROWS + tid]) + (sred[2 * RG_ROWS + tid] + sred[3 * RG_ROWS + tid]);
      if (nr >= M) s = -INFINITY;
      else so[nr] = s;
      srow[tid] = s;
    }
    if constexpr (CPROJ) {
      const int row = tid >> 3, seg = tid & 7;
      float cp[4] = {0.f, 0.f, 0.f, 0.f};
      const f32x4* hr = reinterpret_cast<const f32x4*>(Hs + row * RG_LD);
      const f32x4* w4 = reinterpret_cast<const f32x4*>(wp);
#pragma unroll 4
      for (int g8 = 0; g8 < IE / 32; ++g8) {
        const f32x4 h = hr[seg + 8 * g8];
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < C) {
            const f32x4 w = w4[c * (IE / 4) + seg + 8 * g8];
            cp[c] += (h[0] * w[0] + h[1] * w[1]) + (h[2] * w[2] + h[3] * w[3]);
          }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        cp[c] += __shfl_xor(cp[c], 1);
        cp[c] += __shfl_xor(cp[c], 2);
        cp[c] += __shfl_xor(cp[c], 4);
      }
      if (seg == 0 && row0 + row < M) *reinterpret_cast<f32x4*>(cproj + (orow0 + c0 + row0 + row) * 4) = f32x4{cp[0], cp[1], cp[2], cp[3]};
    }
    __syncthreads();
    // ---- log-sum-exp partial, running over the chunk's tiles (row 0 of every tile is a real row: the tile maximum is finite)
    float mt = -INFINITY;
#pragma unroll
    for (int q = 0; q < RG_ROWS / 4; ++q) {
      const f32x4 v = reinterpret_cast<const f32x4*>(srow)[q];
      mt = fmaxf(fmaxf(mt, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
    }
    const float m_new = fmaxf(m_run, mt);
    const float scale = (m_run == -INFINITY) ? 0.f : __expf(m_run - m_new);
    if (tid < RG_ROWS) prow[tid] = srow[tid] == -INFINITY ? 0.f : __expf(srow[tid] - m_new);
    __syncthreads();
    float lsum = 0.f, a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int q = 0; q < RG_ROWS / 4; ++q) {
      const f32x4 p = reinterpret_cast<const f32x4*>(prow)[q];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float* hr = Hs + (4 * q + j) * RG_LD;
        lsum += p[j];
        a0 += p[j] * hr[tid];
        a1 += p[j] * hr[tid + RG_T];
      }
    }
    l_run = l_run * scale + lsum;
    z0 = z0 * scale + a0;
    z1 = z1 * scale + a1;
    m_run = m_new;
    __syncthreads();                           // the next tile overwrites Hs / srow
  }
  if (tid == 0) { pm[part] = m_run; pl[part] = l_run; }
  pz[(int64_t)part * IE + tid] = z0;
  pz[(int64_t)part * IE + tid + RG_T] = z1;
}

// ------------------------------------------------------------------------------------------------ 4. merge + head + loss + attention
// blockIdx.x = bag.  Every block of a bag derives {max, sum} from the bag's partials in the same fixed order.  blockIdx.y = 0: the pooled
// row (thread e = column e, partials in index order), the predictor in fp32, the cross entropy.  blockIdx.y > 0: the attention map.
__global__ __launch_bounds__(RG_FIN_T) void infer_finalize_kernel(InferTab tab, const float* __restrict__ pm, const float* __restrict__ pl,
                                                               const float* __restrict__ pz, const float* __restrict__ s,
                                                               const float* __restrict__ wp, const float* __restrict__ bp, int C,
                                                               const int64_t* __restrict__ labels, float* __restrict__ logits,
                                                               float* __restrict__ z_out, float* __restrict__ stats,
                                                               float* __restrict__ attn, float* __restrict__ loss) {
  __shared__ float red[8];
  __shared__ float wgt[RG_FIN_T];
  __shared__ float zs[IE];
  __shared__ float lg[FIN_MAXC];
  const int bag = blockIdx.x;
  RG_BAG(bag)
  const int G = rg_parts(N);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  pm += p0; pl += p0; pz += (int64_t)p0 * IE;
  float mx, L;
  rg_merge_stats(pm, pl, G, 1, red, mx, L);
  const float invL = 1.f / L;
  if (blockIdx.y > 0) {
    if (attn) {
      const float* sb = s + orow0;
      float* ab = attn + orow0;
      const int64_t step = (int64_t)(gridDim.y - 1) * RG_FIN_T;
      for (int64_t r = (int64_t)(blockIdx.y - 1) * RG_FIN_T + tid; r < N; r += step) ab[r] = __expf(sb[r] - mx) * invL;
    }
    return;
  }
  if (tid == 0) { stats[2 * bag] = mx; stats[2 * bag + 1] = L; }
  // (the pooled-row loop and the cross entropy below are own text in every kernel that has them: as shared functions they moved this
  // kernel's code - profiles/ragged_shared.md)
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
  if (z_out) z_out[(int64_t)bag * IE + tid] = zv;
  __syncthreads();
  for (int c = wave; c < C; c += RG_FIN_T / 64) {
    float d = 0.f;
#pragma unroll
    for (int q = 0; q < IE / 64; ++q) d += zs[lane + 64 * q] * wp[(int64_t)c * IE + lane + 64 * q];
    d = wave_sum(d);
    if (lane == 0) {
      const float v = d + (bp ? bp[c] : 0.f);
      lg[c] = v;
      logits[(int64_t)bag * C + c] = v;
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
struct InferWs { int64_t w1p, wa_frag, H, s, pm, pl, pz, total; };

// xdt: the element type of the bags' rows (MHIMX_X_*); the 2-byte types have their own pitch rule (16-byte rows: 8 elements)
int check_infer(const mhimx_infer_cfg* c, int32_t n_bags, const mhimx_infer_bag* bags, int32_t xdt = MHIMX_X_F32) {
  if (int r = rg_check_infer_front("infer", xdt, c, n_bags, bags, false)) return r;
  MHIMX_CHECK_ARG(c->E == IE && c->A == IA && c->C >= 1 && c->C <= FIN_MAXC && c->D > 0 && c->D % 256 == 0 && c->D <= (1 << 20),
                  "infer: shapes outside the ragged ABMIL forward (E = 512, A = 128, 1 <= C <= %d, D %% 256 == 0)", FIN_MAXC);
  MHIMX_CHECK_ARG(c->act >= MHIMX_ACT_NONE && c->act <= MHIMX_ACT_TANH && c->da_act >= MHIMX_ACT_NONE && c->da_act <= MHIMX_ACT_TANH,
                  "infer: unknown activation");
  return rg_check_infer_bags("infer", c->D, n_bags, bags, xdt);
}

void infer_layout(const mhimx_infer_cfg* c, int32_t n_bags, const mhimx_infer_bag* bags, InferWs* w, InferTab* tab) {
  const RgCount n = rg_tab_fill(tab, n_bags, bags);
  const int64_t rows = n.rows, parts = n.parts;
  Arena ar(nullptr, 0);
  w->w1p = ar.off; ar.take<float>(c->E * c->D);
  w->wa_frag = ar.off; ar.take<float>(c->A * c->E);
  w->H = ar.off; ar.take<float>(rows * c->E);
  w->s = ar.off; ar.take<float>(rows);
  w->pm = ar.off; ar.take<float>(parts);
  w->pl = ar.off; ar.take<float>(parts);
  w->pz = ar.off; ar.take<float>(parts * c->E);
  w->total = ar.off;
}

}  // namespace

int infer_score(hipStream_t st, const InferTab& tab, const float* H, const float* wa_frag, const float* wc, int act, float* s, float* pm, float* pl,
                float* pz) {
  MHIMX_ONCE_PER_DEVICE(MHIMX_HIP(hipFuncSetAttribute((const void*)infer_score_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SC_SMEM)));
  hipLaunchKernelGGL(infer_score_kernel<false>, dim3((unsigned)tab.parts), dim3(RG_T), SC_SMEM, st, tab, H, wa_frag, wc, act, s, pm, pl, pz,
                     (const float*)nullptr, 0, (float*)nullptr);
  MHIMX_LAUNCH_CHECK();
  return 0;
}

// the same launch + the class projections cproj [rows of the row space][4] = h . Wp_c (wp [C, 512], C <= 4, 16-byte aligned)
int infer_score_cproj(hipStream_t st, const InferTab& tab, const float* H, const float* wa_frag, const float* wc, int act, float* s, float* pm,
                      float* pl, float* pz, const float* wp, int C, float* cproj) {
  MHIMX_CHECK_ARG(wp && cproj && C >= 1 && C <= 4 && aligned16(wp) && aligned16(cproj), "infer_score_cproj: predictor weight [C <= 4, 512] / output");
  MHIMX_ONCE_PER_DEVICE(MHIMX_HIP(hipFuncSetAttribute((const void*)infer_score_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SC_SMEM)));
  hipLaunchKernelGGL(infer_score_kernel<true>, dim3((unsigned)tab.parts), dim3(RG_T), SC_SMEM, st, tab, H, wa_frag, wc, act, s, pm, pl, pz, wp, C,
                     cproj);
  MHIMX_LAUNCH_CHECK();
  return 0;
}

}  // namespace mhimx

extern "C" int64_t mhimx_infer_ws_bytes(const mhimx_infer_cfg* cfg, int32_t n_bags, const mhimx_infer_bag* bags) {
  using namespace mhimx;
  if (int r = check_infer(cfg, n_bags, bags)) return r;
  InferWs w;
  infer_layout(cfg, n_bags, bags, &w, nullptr);
  return w.total;
}

extern "C" int mhimx_infer_run(void* stream, const mhimx_infer_cfg* cfg, int32_t n_bags, const mhimx_infer_bag* bags,
                               const int64_t* labels_dev, const mhimx_infer_out* out, void* ws, int64_t ws_bytes) {
  return mhimx_infer_run_x(stream, cfg, n_bags, bags, labels_dev, out, ws, ws_bytes, MHIMX_X_F32);
}

extern "C" int mhimx_infer_run_x(void* stream, const mhimx_infer_cfg* cfg, int32_t n_bags, const mhimx_infer_bag* bags,
                                 const int64_t* labels_dev, const mhimx_infer_out* out, void* ws, int64_t ws_bytes, int32_t x_dtype) {
  using namespace mhimx;
  if (int r = check_infer(cfg, n_bags, bags, x_dtype)) return r;
  const mhimx_step_params& P = cfg->p;
  MHIMX_CHECK_ARG(P.w1 && P.b1 && P.wa && P.wc && P.wp && P.bp, "infer: null parameter");
  MHIMX_CHECK_ARG(aligned16(P.w1) && aligned16(P.b1) && aligned16(P.wa), "infer: feature / scorer weights must be 16-byte aligned");
  if (int r = rg_check_infer_io("infer", n_bags, bags, out && out->logits && out->stats, "logits and stats outputs are required",
                                out ? out->loss : nullptr, labels_dev))
    return r;
  InferWs w;
  InferTab tab = {};
  infer_layout(cfg, n_bags, bags, &w, &tab);
  tab.pad = x_dtype;                           // read by the projection launch alone: the only reader of X
  if (int r = rg_check_ws("infer", ws, ws_bytes, w.total)) return r;
  hipStream_t st = (hipStream_t)stream;
  char* base = static_cast<char*>(ws);
  float* w1p = reinterpret_cast<float*>(base + w.w1p);
  float* wa_frag = reinterpret_cast<float*>(base + w.wa_frag);
  float* H = reinterpret_cast<float*>(base + w.H);
  float* s = out->score ? out->score : reinterpret_cast<float*>(base + w.s);
  float* pm = reinterpret_cast<float*>(base + w.pm);
  float* pl = reinterpret_cast<float*>(base + w.pl);
  float* pz = reinterpret_cast<float*>(base + w.pz);
  const int D = (int)cfg->D, C = (int)cfg->C;

  // 1. weight images
  mhimx_prep_job jobs[2] = {mhimx_prep_job{1, P.w1, w1p, cfg->E, cfg->D}, mhimx_prep_job{4, P.wa, wa_frag, cfg->A, cfg->E}};
  if (int r = mhimx_prep_batch(stream, jobs, 2)) return r;
  // 2. feature rows of every bag (bag_project.hip)
  if (int r = infer_project(st, tab, D, w1p, P.b1, cfg->act, H)) return r;
  // 3. scores + pool partials
  if (int r = infer_score(st, tab, H, wa_frag, P.wc, cfg->da_act, s, pm, pl, pz)) return r;
  // 4. merge, head, loss, attention
  hipLaunchKernelGGL(infer_finalize_kernel, dim3((unsigned)n_bags, out->attn ? 1 + FIN_ATTN_BLOCKS : 1), dim3(RG_FIN_T), 0, st, tab, pm, pl, pz, s, P.wp,
                     P.bp, C, labels_dev, out->logits, out->z, out->stats, out->attn, out->loss);
  MHIMX_LAUNCH_CHECK();
  return 0;
}
