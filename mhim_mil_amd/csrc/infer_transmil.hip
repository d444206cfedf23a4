// infer_transmil.hip — eval-mode MHIM(TransMIL) forward of up to MHIMX_INFER_MAX bags of DIFFERENT row counts in one call
// (modules/mhim.py:229-272 forward_test with baseline == 'selfattn' and merge_test off, over mhim_modules/baseline.py:196-288 SAttention /
// TransLayer, modules/nystrom_attention.py:12-27,65-152, modules/emb_position.py:85-120, under engines/common_mil.py:56-68 and the per-bag
// loop + criterion call of engines/base_engine.py:234-329):
//
//     h = act(X W1^T + b1),  tok = [cls_token; h]  (n = N + 1 tokens),  per layer: front zero padding to T = 256 ceil(n / 256), l = T / 256,
//     y = x + to_out(Nystrom(to_qkv(LN(x)))),  PPEG on rows 1.. between the layers,  z = LN(cls row),  logits = z Wp^T + bp,  loss = CE.
//
// The third sibling of infer.hip / infer_dsmil.hip: the same by-value bag table, so the call copies nothing to the device, waits for nothing
// and allocates nothing, and can be captured in a graph.  All bags live in ONE padded token space (bag b: rows tok0[b] .. tok0[b] + T[b],
// its pad rows first).  96 launches whatever n_bags is:
//    1      mhimx_prep_batch            paired-plane image of W1
//    2      infer_project_kernel        (bag_project.hip) X -> h, all three element types, written at row tok0[b] + pad[b] + 1
//    3      tm_cls_kernel               the cls token into row tok0[b] + pad[b] of every bag
//   per layer (45 launches, twice):
//    1      tm_layernorm_kernel         chunk-wide: xn = LN(x) on token rows, EXACT ZEROS on pad rows (to_qkv has no bias: the pad rows of qkv
//                                       are zeros without a second pass), and y <- x (the residual the to_out launch adds to)
//    1      gemm_nt                     chunk-wide qkv = xn Wqkv^T                                        [sum T, 1536]
//    1      landmark_fwd_vec_many       bag-batched landmark means                                        [n, 256, 1024]
//    8      small_bmm (nt)              q~ k~^T: one launch PER HEAD over all bags (the head stride inside a bag differs from the bag
//                                       stride; a head's matrices across the bags are evenly spaced)      [n, 8, 256, 256]
//    1      mhimx_softmax_rows          a2, R = n 8 256
//    3      pinv_init_many              row / column sums, the two maxima PER BAG, z0 = a2^T / (c r)
//   24      mhimx_bmm_affine2 / affine  the six pseudo-inverse iterations as launches with batch = 8 n (never the persistent chain kernel)
//    2      ny_a3v_fwd_many + merge     bag-batched streamed softmax_n(q~ k^T) v, partials per bag
//    1      small_bmm (nn)              w2 = z a3v, batch = 8 n
//    1      resconv_tile_many           bag-batched residual convolution of v -> out
//    1      ny_out_fwd_tok8_many        bag-batched out += softmax_m(q k~^T) w2
//    1      gemm_nt                     chunk-wide y += out Wout^T + b
//   between the layers:
//    2      ppeg_combine, ppeg_strip_many   the 7x7 stencil of every bag on its rows 1.., the cls row copied
//   and    1 tm_tail_kernel             grid = bags: LN of the cls row, predictor, cross entropy
// No workgroup waits for another and there are no floating-point atomics.  A bag's chunks, tile walk and merge order depend on its own N
// alone and every chunk-wide kernel computes a row from that row alone, so a bag's results have the same bits wherever it stands in a call.
//
// mhimx_infer_transmil_run_attn runs the same body (ONE body: the entry above passes no attention output) and then the attention tail
// (nystrom_attention.py:143-150 under baseline.py:244-288; normalised form, eval mode), out of the operands the layers left in the workspace:
//   per layer (2 launches, twice):
//    1      tm_cls_u_kernel             grid (head, bag): a1c = softmax_m(scale q_cls k~_m), u = a1c z (the cls row of attn1 times the pseudo-inverse)
//    1      ny_cls_row8_kernel<true>    bag-batched r = u softmax_n(q~ k^T), columns pad + 1 .. of every bag packed: attn [2, 8, R], R = sum N_b
//   with pscore (get_pseudo_score_trans, scoring.py:9-34 under mhim.py:207-227,250-260; 4 launches):
//    1      tm_pscore_f_kernel          f[r] = v_r * attn_l1[head, r] over the R instance rows, v read in the token space
//    1      gemm_nt                     to_out of layer 1 + bias over the R rows
//    1      gemm_nt                     cam = f Wp^T
//    1      mhimx_pseudo_score          + bp[0], softmax over the classes, max
// 96 + 4 (+ 4) launches.  Both products run over max(R, 32) rows (the rows behind R are zeros): a call of fewer than 17 rows stays on the tiled
// kernel, so a row's bits do not depend on how many rows the call has.
#include <math.h>
#include <string.h>

#include "infer_tab.hpp"
#include "nys_args.hpp"

namespace mhimx {

int gemm_nt(hipStream_t st, const mhimx_gemm_nt_args& g);                                                                         // gemm.hip
int small_bmm(hipStream_t st, int mode, const mhimx_gemm_nt_args& a, int batch, int64_t sA, int64_t sB, int64_t sC, float alpha, float ident);

namespace {

constexpr int TM_E = 512, TM_QKV = 1536, TM_M = 256, TM_H = 8, TM_DH = 64, TM_MAXC = 16, TM_ITERS = 6;
constexpr int64_t TM_MM = (int64_t)TM_M * TM_M;                  // one 256 x 256 landmark matrix
constexpr float TM_SCALE = 0.125f;                               // dim_head ^ -0.5

// ------------------------------------------------------------------------------------------------ cls rows
// blockIdx.x = bag: the cls token (nn.Parameter [1, 1, 512]) into the bag's first token row
__global__ __launch_bounds__(128) void tm_cls_kernel(NyBags tb, const float* __restrict__ cls, float* __restrict__ x) {
  int64_t tok0 = tb.tok0[0];
  int T = tb.T[0], n = tb.n[0];
  NY_PICK(tok0, tb.tok0, blockIdx.x) NY_PICK(T, tb.T, blockIdx.x) NY_PICK(n, tb.n, blockIdx.x)
  reinterpret_cast<f32x4*>(x + (tok0 + (T - n)) * TM_E)[threadIdx.x] = reinterpret_cast<const f32x4*>(cls)[threadIdx.x];
}

// ------------------------------------------------------------------------------------------------ LayerNorm over the padded token space
// One wave per row of the token space (the arithmetic of layernorm_fwd_vec_kernel<2>, rows.hip).  A pad row - one of the first T - n rows
// of its bag - is not read: xn and y get exact zeros there.  y <- x on token rows.
__global__ __launch_bounds__(256) void tm_layernorm_kernel(NyBags tb, const float* __restrict__ x, int64_t rows, const float* __restrict__ w,
                                                           const float* __restrict__ b, float* __restrict__ xn, float* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t r = (int64_t)blockIdx.x * 4 + wave;
  if (r >= rows) return;
  int64_t tok0 = tb.tok0[0];
  int T = tb.T[0], n = tb.n[0];
#pragma unroll
  for (int q = 1; q < MHIMX_INFER_MAX; ++q)
    if (q < tb.nbags && r >= tb.tok0[q]) { tok0 = tb.tok0[q]; T = tb.T[q]; n = tb.n[q]; }
  f32x4* xo = reinterpret_cast<f32x4*>(xn + r * TM_E);
  f32x4* yo = reinterpret_cast<f32x4*>(y + r * TM_E);
  if (r - tok0 < T - n) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    xo[lane] = zero; xo[64 + lane] = zero;
    yo[lane] = zero; yo[64 + lane] = zero;
    return;
  }
  const f32x4* xi = reinterpret_cast<const f32x4*>(x + r * TM_E);
  f32x4 v[2] = {xi[lane], xi[64 + lane]};
  yo[lane] = v[0]; yo[64 + lane] = v[1];
  float sum = 0.f;
#pragma unroll
  for (int q = 0; q < 2; ++q) sum += (v[q][0] + v[q][1]) + (v[q][2] + v[q][3]);
  const float mu = wave_sum(sum) / (float)TM_E;
  float var = 0.f;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    v[q] -= mu;
    var += (v[q][0] * v[q][0] + v[q][1] * v[q][1]) + (v[q][2] * v[q][2] + v[q][3] * v[q][3]);
  }
  const float rs = rsqrtf(wave_sum(var) / (float)TM_E + 1e-5f);
#pragma unroll
  for (int q = 0; q < 2; ++q)
    xo[64 * q + lane] = v[q] * rs * reinterpret_cast<const f32x4*>(w)[64 * q + lane] + reinterpret_cast<const f32x4*>(b)[64 * q + lane];
}

// ------------------------------------------------------------------------------------------------ tail: final norm of the cls row, predictor, loss
// blockIdx.x = bag, one wave.  z = LN(y[cls row]) (only the cls row is used, baseline.py:276-278), logits[c] = z . Wp[c] + bp[c] in fp32
// with a fixed lane order and xor tree, loss = log sum_c e^{x_c} - x_label (a label outside [0, C): NaN, where torch raises).
__global__ __launch_bounds__(64) void tm_tail_kernel(NyBags tb, const float* __restrict__ y, const float* __restrict__ nw, const float* __restrict__ nb,
                                                     const float* __restrict__ wp, const float* __restrict__ bp, int C,
                                                     const int64_t* __restrict__ labels, float* __restrict__ cls_out, float* __restrict__ z_out,
                                                     float* __restrict__ logits, float* __restrict__ loss) {
  const int bag = blockIdx.x, lane = threadIdx.x;
  int64_t tok0 = tb.tok0[0];
  int T = tb.T[0], n = tb.n[0];
  NY_PICK(tok0, tb.tok0, bag) NY_PICK(T, tb.T, bag) NY_PICK(n, tb.n, bag)
  const f32x4* xi = reinterpret_cast<const f32x4*>(y + (tok0 + (T - n)) * TM_E);
  f32x4 v[2] = {xi[lane], xi[64 + lane]};
  float sum = 0.f;
#pragma unroll
  for (int q = 0; q < 2; ++q) sum += (v[q][0] + v[q][1]) + (v[q][2] + v[q][3]);
  const float mu = wave_sum(sum) / (float)TM_E;
  float var = 0.f;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    v[q] -= mu;
    var += (v[q][0] * v[q][0] + v[q][1] * v[q][1]) + (v[q][2] * v[q][2] + v[q][3] * v[q][3]);
  }
  const float rs = rsqrtf(wave_sum(var) / (float)TM_E + 1e-5f);
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    v[q] = v[q] * rs * reinterpret_cast<const f32x4*>(nw)[64 * q + lane] + reinterpret_cast<const f32x4*>(nb)[64 * q + lane];
    reinterpret_cast<f32x4*>(cls_out + (int64_t)bag * TM_E)[64 * q + lane] = v[q];
    if (z_out) reinterpret_cast<f32x4*>(z_out + (int64_t)bag * TM_E)[64 * q + lane] = v[q];
  }
  float lg[TM_MAXC];
#pragma unroll
  for (int c = 0; c < TM_MAXC; ++c) {
    lg[c] = 0.f;
    if (c < C) {
      float d = 0.f;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const f32x4 wv = reinterpret_cast<const f32x4*>(wp + (int64_t)c * TM_E)[64 * q + lane];
        d = fmaf(v[q][3], wv[3], fmaf(v[q][2], wv[2], fmaf(v[q][1], wv[1], fmaf(v[q][0], wv[0], d))));
      }
      lg[c] = wave_sum(d) + bp[c];
    }
  }
  if (lane != 0) return;
  float cm = lg[0];
#pragma unroll
  for (int c = 0; c < TM_MAXC; ++c)
    if (c < C) {
      logits[(int64_t)bag * C + c] = lg[c];
      cm = fmaxf(cm, lg[c]);
    }
  if (!loss) return;
  float den = 0.f, picked = 0.f;
  const int64_t lab = labels[bag];
#pragma unroll
  for (int c = 0; c < TM_MAXC; ++c)
    if (c < C) {
      den += expf(lg[c] - cm);
      if (c == lab) picked = lg[c];
    }
  loss[bag] = (lab >= 0 && lab < C) ? (cm + logf(den)) - picked : NAN;
}

// ------------------------------------------------------------------------------------------------ attention tail: u = attn1[cls] pinv
// grid (head, bag), 256 threads, fp32, every sum in a fixed order.  s[m] = scale q_cls . k~_m (thread m; q_cls = row tok0 + pad of qkv, k~ the
// second half of the bag's landmark means), a1c = softmax_m(s) (wave reductions, the four wave results in index order), then
// u[m'] = sum_m a1c[m] z[m, m']: thread (g, c) adds rows 64 g .. 64 g + 63 of columns 4 c .. 4 c + 3 in index order (one 16-byte load per
// row: the head's z is read once, 1 KiB rows across the workgroup), the four row groups are added in index order.
__global__ __launch_bounds__(256) void tm_cls_u_kernel(NyBags tb, const float* __restrict__ qkv, const float* __restrict__ lm, const float* __restrict__ z,
                                                       float* __restrict__ u) {
  __shared__ float qs[TM_DH];
  __shared__ float a1c[TM_M];
  __shared__ float red[4];
  __shared__ f32x4 part[4][64];
  const int h = blockIdx.x, bag = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t tok0 = tb.tok0[0];
  int T = tb.T[0], n = tb.n[0];
  NY_PICK(tok0, tb.tok0, bag) NY_PICK(T, tb.T, bag) NY_PICK(n, tb.n, bag)
  if (tid < TM_DH) qs[tid] = qkv[(tok0 + (T - n)) * TM_QKV + h * TM_DH + tid];
  __syncthreads();
  const f32x4* kr = reinterpret_cast<const f32x4*>(lm + ((int64_t)bag * TM_M + tid) * (2 * TM_E) + TM_E + h * TM_DH);
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < TM_DH / 4; ++d) {
    const f32x4 kv = kr[d];
    s = fmaf(qs[4 * d + 3], kv[3], fmaf(qs[4 * d + 2], kv[2], fmaf(qs[4 * d + 1], kv[1], fmaf(qs[4 * d], kv[0], s))));
  }
  s *= TM_SCALE;
  const float wm = wave_max(s);
  if (lane == 0) red[wave] = wm;
  __syncthreads();
  const float mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  const float e = expf(s - mx);
  const float wsum = wave_sum(e);
  if (lane == 0) red[wave] = wsum;
  __syncthreads();
  a1c[tid] = e / (((red[0] + red[1]) + red[2]) + red[3]);
  __syncthreads();
  const f32x4* zp = reinterpret_cast<const f32x4*>(z + ((int64_t)bag * TM_H + h) * TM_MM) + lane;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int i = 0; i < 64; ++i) {
    const int m = 64 * wave + i;
    const f32x4 zv = zp[m * (TM_M / 4)];
    const float am = a1c[m];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = fmaf(am, zv[j], acc[j]);
  }
  part[wave][lane] = acc;
  __syncthreads();
  if (tid < 64) reinterpret_cast<f32x4*>(u + ((int64_t)bag * TM_H + h) * TM_M)[tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
}

// ------------------------------------------------------------------------------------------------ attention tail: f = v * attn per head
// The bag-aware form of scale_heads_kernel (scoring.py:25): one wave per packed instance row r, f[r, c] = v[token(r), c] attn[c / 64, r]
// with v read where the layer left it (columns 1024.. of the token space; token(r) = the bag's row tok0 + pad + 1 + (r - the bag's first
// packed row)).  Rows R .. rows - 1 get exact zeros.
__global__ __launch_bounds__(256) void tm_pscore_f_kernel(NyBags tb, const float* __restrict__ v, const float* __restrict__ attn, int64_t R, int64_t rows,
                                                          float* __restrict__ f) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t r = (int64_t)blockIdx.x * 4 + wave;
  if (r >= rows) return;
  f32x4* fo = reinterpret_cast<f32x4*>(f + r * TM_E);
  if (r >= R) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    fo[lane] = zero; fo[64 + lane] = zero;
    return;
  }
  int64_t tok0 = tb.tok0[0], row0 = 0, o = 0;
  int T = tb.T[0], n = tb.n[0];
#pragma unroll
  for (int q = 0; q < MHIMX_INFER_MAX; ++q)
    if (q < tb.nbags) {
      if (r >= o) { tok0 = tb.tok0[q]; T = tb.T[q]; n = tb.n[q]; row0 = o; }
      o += tb.n[q] - 1;
    }
  const f32x4* vi = reinterpret_cast<const f32x4*>(v + (tok0 + (T - n) + 1 + (r - row0)) * TM_QKV);
#pragma unroll
  for (int q = 0; q < 2; ++q) fo[64 * q + lane] = vi[64 * q + lane] * attn[(int64_t)(4 * q + (lane >> 4)) * R + r];
}

// ------------------------------------------------------------------------------------------------ host
// the checks of mhimx_infer_run_x on the bag table and the element type, and this call's own shape rules
int check_transmil(const char* who, const mhimx_infer_transmil_cfg* c, int32_t n_bags, const mhimx_infer_bag* bags, int32_t xdt) {
  if (int r = rg_check_infer_front(who, xdt, c, n_bags, bags, true)) return r;
  MHIMX_CHECK_ARG(c->C >= 1 && c->C <= TM_MAXC && c->D > 0 && c->D % 256 == 0 && c->D <= (1 << 20),
                  "%s: shapes outside the ragged TransMIL forward (E = 512, 8 x 64 heads, 256 landmarks, 1 <= C <= %d, D %% 256 == 0)", who, TM_MAXC);
  MHIMX_CHECK_ARG(c->act >= MHIMX_ACT_NONE && c->act <= MHIMX_ACT_TANH, "%s: unknown activation", who);
  return rg_check_infer_bags(who, c->D, n_bags, bags, xdt);
}

// offsets that are not part of the public layout: weight image, LN rows, pseudo-inverse temporaries, PPEG stencil, partials
struct TmScratch { int64_t w1p, xn, az, t1, t2, t3, zb, stats, sums, wc, bc, nys; };

void transmil_layout(const mhimx_infer_transmil_cfg* c, int32_t n_bags, const mhimx_infer_bag* bags, mhimx_infer_transmil_layout* lo, TmScratch* sc,
                     NyBags* tb) {
  int64_t tokens = 0;
  int maxT = 0;
  for (int b = 0; b < n_bags; ++b) {
    const int64_t n = bags[b].N + 1, T = cdiv(n, TM_M) * TM_M;
    lo->tok0[b] = tokens; lo->T[b] = T; lo->pad[b] = T - n;
    if (tb) {
      int64_t wrapN = 0;
      tb->tok0[b] = tokens; tb->T[b] = (int32_t)T; tb->n[b] = (int32_t)n;
      tb->H[b] = (int32_t)mhimx_ppeg_side(bags[b].N, &wrapN);
      tb->wrapN[b] = (int32_t)wrapN;
    }
    tokens += T;
    maxT = T > maxT ? (int)T : maxT;
  }
  for (int b = n_bags; b < MHIMX_INFER_MAX; ++b) {
    lo->tok0[b] = lo->T[b] = lo->pad[b] = 0;
    if (tb) { tb->tok0[b] = 0; tb->T[b] = 0; tb->n[b] = 0; tb->H[b] = 0; tb->wrapN[b] = 0; }
  }
  if (tb) { tb->nbags = n_bags; tb->maxT = maxT; }
  lo->n_bags = n_bags;
  lo->tokens = tokens;
  const int64_t nb = n_bags;
  Arena ar(nullptr, 0);
  auto F = [&](int64_t floats) { const int64_t o = ar.off; ar.take<float>(floats); return o; };
  for (int l = 0; l < 2; ++l) lo->x[l] = F(tokens * TM_E);
  for (int l = 0; l < 2; ++l) {
    lo->qkv[l] = F(tokens * TM_QKV);
    lo->lm[l] = F(nb * TM_M * 2 * TM_E);
    lo->a2[l] = F(nb * TM_H * TM_MM);
    lo->z[l] = F(nb * TM_H * TM_MM);
    lo->a3v[l] = F(nb * TM_H * TM_M * TM_DH);
    lo->lse3[l] = F(nb * TM_H * TM_M);
    lo->w2[l] = F(nb * TM_H * TM_M * TM_DH);
    lo->out[l] = F(tokens * TM_E);
    lo->y[l] = F(tokens * TM_E);
  }
  lo->cls = F(nb * TM_E);
  TmScratch s;
  s.w1p = F((int64_t)TM_E * c->D);
  s.xn = F(tokens * TM_E);
  s.az = F(nb * TM_H * TM_MM); s.t1 = F(nb * TM_H * TM_MM); s.t2 = F(nb * TM_H * TM_MM); s.t3 = F(nb * TM_H * TM_MM);
  s.zb = F(nb * TM_H * TM_MM);
  s.stats = F(nb * 4);
  s.sums = F(2 * nb * TM_H * TM_M);
  s.wc = F(TM_E * 49); s.bc = F(TM_E);
  s.nys = F(nb * mhimx_nys_ws_floats(0));
  lo->total = ar.off;
  if (sc) *sc = s;
}

// what mhimx_infer_transmil_run_attn keeps BEHIND that layout (its prefix): u of both layers, and for the pseudo-score f, to_out(f), cam
struct TmAttnWs { int64_t R, rows, u[2], f, g, cam, total; };

void transmil_attn_layout(const mhimx_infer_transmil_cfg* c, int32_t n_bags, const mhimx_infer_bag* bags, const mhimx_infer_transmil_layout& lo,
                          bool want_pscore, TmAttnWs* a) {
  a->R = 0;
  for (int b = 0; b < n_bags; ++b) a->R += bags[b].N;
  a->rows = a->R < 32 ? 32 : a->R;
  Arena ar(nullptr, 0);
  ar.off = lo.total;
  auto F = [&](int64_t floats) { const int64_t o = ar.off; ar.take<float>(floats); return o; };
  for (int l = 0; l < 2; ++l) a->u[l] = F((int64_t)n_bags * TM_H * TM_M);
  a->f = a->g = a->cam = 0;
  if (want_pscore) { a->f = F(a->rows * TM_E); a->g = F(a->rows * TM_E); a->cam = F(a->rows * c->C); }
  a->total = ar.off;
}

struct TmAttnOut { float* attn; float* pscore; };             // the outputs of the tail (transmil_run)

}  // namespace
}  // namespace mhimx

extern "C" int64_t mhimx_infer_transmil_ws_bytes(const mhimx_infer_transmil_cfg* cfg, int32_t n_bags, const mhimx_infer_bag* bags) {
  using namespace mhimx;
  if (int r = check_transmil("infer_transmil", cfg, n_bags, bags, MHIMX_X_F32)) return r;
  mhimx_infer_transmil_layout lo;
  transmil_layout(cfg, n_bags, bags, &lo, nullptr, nullptr);
  return lo.total;
}

extern "C" int64_t mhimx_infer_transmil_attn_ws_bytes(const mhimx_infer_transmil_cfg* cfg, int32_t n_bags, const mhimx_infer_bag* bags,
                                                      int32_t want_pscore) {
  using namespace mhimx;
  if (int r = check_transmil("infer_transmil_attn", cfg, n_bags, bags, MHIMX_X_F32)) return r;
  mhimx_infer_transmil_layout lo;
  TmAttnWs aw;
  transmil_layout(cfg, n_bags, bags, &lo, nullptr, nullptr);
  transmil_attn_layout(cfg, n_bags, bags, lo, want_pscore != 0, &aw);
  return aw.total;
}

extern "C" int mhimx_infer_transmil_layout_of(const mhimx_infer_transmil_cfg* cfg, int32_t n_bags, const mhimx_infer_bag* bags,
                                              mhimx_infer_transmil_layout* out) {
  using namespace mhimx;
  if (int r = check_transmil("infer_transmil", cfg, n_bags, bags, MHIMX_X_F32)) return r;
  MHIMX_CHECK_ARG(out, "infer_transmil_layout_of: null output");
  transmil_layout(cfg, n_bags, bags, out, nullptr, nullptr);
  return 0;
}

namespace mhimx {
namespace {
// the ONE body of mhimx_infer_transmil_run (ao null: no tail) and mhimx_infer_transmil_run_attn; `who` names the entry point in the messages
int transmil_run(const char* who, void* stream, const mhimx_infer_transmil_cfg* cfg, int32_t n_bags, const mhimx_infer_bag* bags,
                 const int64_t* labels_dev, float* logits, float* loss, float* z, const TmAttnOut* ao, void* ws, int64_t ws_bytes, int32_t x_dtype) {
  if (int r = check_transmil(who, cfg, n_bags, bags, x_dtype)) return r;
  bool params = cfg->w1 && cfg->b1 && cfg->cls_token && cfg->w7 && cfg->w5 && cfg->w3 && cfg->b7 && cfg->b5 && cfg->b3 && cfg->norm_w && cfg->norm_b &&
                cfg->wp && cfg->bp;
  bool algn = aligned16(cfg->w1) && aligned16(cfg->b1) && aligned16(cfg->cls_token) && aligned16(cfg->norm_w) && aligned16(cfg->norm_b) &&
              aligned16(cfg->wp);
  for (int l = 0; l < 2; ++l) {
    const mhimx_transmil_layer& t = cfg->layer[l];
    params = params && t.ln_w && t.ln_b && t.w_qkv && t.w_out && t.b_out && t.conv_w;
    algn = algn && aligned16(t.ln_w) && aligned16(t.ln_b) && aligned16(t.w_qkv) && aligned16(t.w_out) && aligned16(t.b_out);
  }
  MHIMX_CHECK_ARG(params, "%s: null parameter", who);
  MHIMX_CHECK_ARG(algn, "%s: the feature, cls token, norm, to_qkv, to_out and predictor parameters must be 16-byte aligned", who);
  if (int r = rg_check_infer_io(who, n_bags, bags, logits, "the logits output is required", loss, labels_dev)) return r;
  if (ao) {
    MHIMX_CHECK_ARG(ao->attn, "%s: the attention output is required", who);
    MHIMX_CHECK_ARG(aligned16(ao->attn) && aligned16(ao->pscore), "%s: the attention and pseudo-score outputs must be 16-byte aligned", who);
  }
  mhimx_infer_transmil_layout lo;
  TmScratch sc;
  TmAttnWs aw = {};
  NyBags tb = {};
  transmil_layout(cfg, n_bags, bags, &lo, &sc, &tb);
  if (ao) transmil_attn_layout(cfg, n_bags, bags, lo, ao->pscore != nullptr, &aw);
  if (int r = rg_check_ws(who, ws, ws_bytes, ao ? aw.total : lo.total)) return r;
  hipStream_t st = (hipStream_t)stream;
  char* base = static_cast<char*>(ws);
  auto F = [&](int64_t off) { return reinterpret_cast<float*>(base + off); };
  const int D = (int)cfg->D, C = (int)cfg->C;
  const int64_t tokens = lo.tokens;
  const int batch = TM_H * n_bags;

  // 1. weight image; 2. feature rows of every bag behind its pad rows and cls row; 3. cls rows
  mhimx_prep_job job = {1, cfg->w1, F(sc.w1p), TM_E, cfg->D};
  if (int r = mhimx_prep_batch(stream, &job, 1)) return r;
  InferTab tab = {};
  rg_tab_fill(&tab, n_bags, bags);
  for (int b = 0; b < n_bags; ++b) tab.row0[b] = lo.tok0[b] + lo.pad[b] + 1;
  tab.pad = x_dtype;
  if (int r = infer_project(st, tab, D, F(sc.w1p), cfg->b1, cfg->act, F(lo.x[0]))) return r;
  hipLaunchKernelGGL(tm_cls_kernel, dim3((unsigned)n_bags), dim3(128), 0, st, tb, cfg->cls_token, F(lo.x[0]));
  MHIMX_LAUNCH_CHECK();

  for (int l = 0; l < 2; ++l) {
    const mhimx_transmil_layer& t = cfg->layer[l];
    float *x = F(lo.x[l]), *xn = F(sc.xn), *qkv = F(lo.qkv[l]), *lm = F(lo.lm[l]), *a2 = F(lo.a2[l]), *zz = F(lo.z[l]), *a3v = F(lo.a3v[l]);
    float *lse3 = F(lo.lse3[l]), *w2 = F(lo.w2[l]), *out = F(lo.out[l]), *y = F(lo.y[l]);
    // row-wise, chunk-wide: LayerNorm (zeros on pad rows), to_qkv
    hipLaunchKernelGGL(tm_layernorm_kernel, dim3((unsigned)cdiv(tokens, 4)), dim3(256), 0, st, tb, x, tokens, t.ln_w, t.ln_b, xn, y);
    MHIMX_LAUNCH_CHECK();
    mhimx_gemm_nt_args g = {};
    g.A = xn; g.lda = TM_E; g.B = t.w_qkv; g.ldb = TM_E; g.C = qkv; g.ldc = TM_QKV; g.M = tokens; g.N = TM_QKV; g.K = TM_E;
    g.prec = MHIMX_PREC_BF16X3;
    if (int r = gemm_nt(st, g)) return r;
    // landmark-only stage over all 8 n matrices
    if (int r = landmark_mean_many(st, tb, qkv, TM_QKV, 2 * TM_E, lm)) return r;
    for (int h = 0; h < TM_H; ++h) {
      mhimx_gemm_nt_args s = {};
      s.A = lm + h * TM_DH; s.lda = 2 * TM_E; s.B = lm + TM_E + h * TM_DH; s.ldb = 2 * TM_E; s.C = a2 + h * TM_MM; s.ldc = TM_M;
      s.M = TM_M; s.N = TM_M; s.K = TM_DH; s.prec = MHIMX_PREC_BF16X3;
      if (int r = small_bmm(st, 0, s, n_bags, (int64_t)TM_M * 2 * TM_E, (int64_t)TM_M * 2 * TM_E, TM_H * TM_MM, 1.f, 0.f)) return r;
    }
    if (int r = mhimx_softmax_rows(stream, a2, a2, (int64_t)batch * TM_M, TM_M, TM_SCALE)) return r;
    if (int r = pinv_init_many(st, n_bags, a2, zz, F(sc.stats), F(sc.sums))) return r;
    {
      float *az = F(sc.az), *t1 = F(sc.t1), *t2 = F(sc.t2), *t3 = F(sc.t3), *zs = zz, *zd = F(sc.zb);
      auto mm = [&](const float* A, const float* B, float* Cc) {
        mhimx_gemm_nt_args s = {};
        s.A = A; s.lda = TM_M; s.B = B; s.ldb = TM_M; s.C = Cc; s.ldc = TM_M; s.M = TM_M; s.N = TM_M; s.K = TM_M; s.prec = MHIMX_PREC_BF16X3;
        return s;
      };
      for (int it = 0; it < TM_ITERS; ++it) {            // z' = 0.25 z (13 I - az (15 I - az (7 I - az))), az = a2 z; the result lands in lo.z
        mhimx_gemm_nt_args s = mm(a2, zs, az);
        if (int r = mhimx_bmm_affine2(stream, 1, &s, batch, TM_MM, TM_MM, TM_MM, 1.f, 0.f, t1, -1.f, 7.f)) return r;
        s = mm(az, t1, t2);
        if (int r = mhimx_bmm_affine(stream, 1, &s, batch, TM_MM, TM_MM, TM_MM, -1.f, 15.f)) return r;
        s = mm(az, t2, t3);
        if (int r = mhimx_bmm_affine(stream, 1, &s, batch, TM_MM, TM_MM, TM_MM, -1.f, 13.f)) return r;
        s = mm(zs, t3, zd);
        if (int r = mhimx_bmm_affine(stream, 1, &s, batch, TM_MM, TM_MM, TM_MM, 0.25f, 0.f)) return r;
        float* sw = zs; zs = zd; zd = sw;
      }
    }
    // token-streaming stages, bag-batched
    NyArgs ny;
    memset(&ny, 0, sizeof(ny));
    ny.q = qkv; ny.k = qkv + TM_E; ny.v = qkv + 2 * TM_E; ny.ld = TM_QKV; ny.ql = lm; ny.kl = lm + TM_E; ny.ldl = 2 * TM_E;
    ny.scale = TM_SCALE; ny.sl2e = TM_SCALE * 1.4426950408889634f;
    if (int r = nys_a3v_fwd_many(st, tb, ny, a3v, lse3, F(sc.nys))) return r;
    {
      mhimx_gemm_nt_args s = {};
      s.A = zz; s.lda = TM_M; s.B = a3v; s.ldb = TM_DH; s.C = w2; s.ldc = TM_DH; s.M = TM_M; s.N = TM_DH; s.K = TM_M; s.prec = MHIMX_PREC_BF16X3;
      if (int r = small_bmm(st, 1, s, batch, TM_MM, TM_M * TM_DH, TM_M * TM_DH, 1.f, 0.f)) return r;
    }
    if (int r = resconv_many(st, tb, qkv + 2 * TM_E, TM_QKV, t.conv_w, out, TM_E)) return r;
    if (int r = nys_out_fwd_many(st, tb, ny, w2, out, TM_E, 1)) return r;
    // row-wise, chunk-wide: y (= x) += out Wout^T + b
    mhimx_gemm_nt_args o = {};
    o.A = out; o.lda = TM_E; o.B = t.w_out; o.ldb = TM_E; o.C = y; o.ldc = TM_E; o.M = tokens; o.N = TM_E; o.K = TM_E; o.bias = t.b_out;
    o.accumulate = 1; o.prec = MHIMX_PREC_BF16X3;
    if (int r = gemm_nt(st, o)) return r;
    if (l == 0) {
      if (int r = mhimx_ppeg_combine(stream, cfg->w7, cfg->w5, cfg->w3, cfg->b7, cfg->b5, cfg->b3, TM_E, F(sc.wc), F(sc.bc))) return r;
      if (int r = ppeg_fwd_many(st, tb, y, F(sc.wc), F(sc.bc), F(lo.x[1]))) return r;
    }
  }
  hipLaunchKernelGGL(tm_tail_kernel, dim3((unsigned)n_bags), dim3(64), 0, st, tb, F(lo.y[1]), cfg->norm_w, cfg->norm_b, cfg->wp, cfg->bp, C, labels_dev,
                     F(lo.cls), z, logits, loss);
  MHIMX_LAUNCH_CHECK();
  if (!ao) return 0;

  // the attention tail: per layer u = attn1[cls] pinv, then the cls row of the streamed attention into the packed instance rows
  const int64_t R = aw.R;
  for (int l = 0; l < 2; ++l) {
    float *qkv = F(lo.qkv[l]), *lm = F(lo.lm[l]), *u = F(aw.u[l]);
    hipLaunchKernelGGL(tm_cls_u_kernel, dim3(TM_H, (unsigned)n_bags), dim3(256), 0, st, tb, qkv, lm, F(lo.z[l]), u);
    MHIMX_LAUNCH_CHECK();
    NyArgs ny;
    memset(&ny, 0, sizeof(ny));
    ny.k = qkv + TM_E; ny.ld = TM_QKV; ny.ql = lm; ny.ldl = 2 * TM_E; ny.scale = TM_SCALE; ny.sl2e = TM_SCALE * 1.4426950408889634f;
    if (int r = nys_cls_attn_many(st, tb, ny, F(lo.lse3[l]), u, ao->attn + (int64_t)l * TM_H * R, R)) return r;
  }
  if (!ao->pscore) return 0;
  // get_pseudo_score_trans on layer 1: f = v * attn per head, to_out + bias, cam = f Wp^T, max_c softmax_c(cam + bp[0])
  float *f = F(aw.f), *fo = F(aw.g), *cam = F(aw.cam);
  hipLaunchKernelGGL(tm_pscore_f_kernel, dim3((unsigned)cdiv(aw.rows, 4)), dim3(256), 0, st, tb, F(lo.qkv[0]) + 2 * TM_E, ao->attn, R, aw.rows, f);
  MHIMX_LAUNCH_CHECK();
  const mhimx_transmil_layer& t0 = cfg->layer[0];
  mhimx_gemm_nt_args o = {};
  o.A = f; o.lda = TM_E; o.B = t0.w_out; o.ldb = TM_E; o.C = fo; o.ldc = TM_E; o.M = aw.rows; o.N = TM_E; o.K = TM_E; o.bias = t0.b_out;
  o.prec = MHIMX_PREC_BF16X3;
  if (int r = gemm_nt(st, o)) return r;
  mhimx_gemm_nt_args p = {};
  p.A = fo; p.lda = TM_E; p.B = cfg->wp; p.ldb = TM_E; p.C = cam; p.ldc = C; p.M = aw.rows; p.N = C; p.K = TM_E; p.prec = MHIMX_PREC_BF16X3;
  if (int r = gemm_nt(st, p)) return r;
  return mhimx_pseudo_score(stream, nullptr, nullptr, cam, cfg->bp, ao->pscore, nullptr, R, C);
}
}  // namespace
}  // namespace mhimx

extern "C" int mhimx_infer_transmil_run(void* stream, const mhimx_infer_transmil_cfg* cfg, int32_t n_bags, const mhimx_infer_bag* bags,
                                        const int64_t* labels_dev, float* logits, float* loss, float* z, void* ws, int64_t ws_bytes,
                                        int32_t x_dtype) {
  return mhimx::transmil_run("infer_transmil", stream, cfg, n_bags, bags, labels_dev, logits, loss, z, nullptr, ws, ws_bytes, x_dtype);
}

extern "C" int mhimx_infer_transmil_run_attn(void* stream, const mhimx_infer_transmil_cfg* cfg, int32_t n_bags, const mhimx_infer_bag* bags,
                                             const int64_t* labels_dev, float* logits, float* loss, float* z, float* attn, float* pscore, void* ws,
                                             int64_t ws_bytes, int32_t x_dtype) {
  const mhimx::TmAttnOut ao = {attn, pscore};
  return mhimx::transmil_run("infer_transmil_attn", stream, cfg, n_bags, bags, labels_dev, logits, loss, z, &ao, ws, ws_bytes, x_dtype);
}
