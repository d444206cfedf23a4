// nys_args.hpp - the kernel argument block shared by the two translation units of the streamed Nystrom attention
// (nys_flash.hip: landmark-column kernels, 8 waves; nys_flash_tok.hip: token-owning kernels, 8 waves).
#pragma once
#include "mma_tile.hpp"

namespace mhimx {

#define NY_EXP2(x) __builtin_amdgcn_exp2f(x)

constexpr int NY_H = 8, NY_D = 64, NY_M = 256, NY_TT = 64, NY_MAXCH = 32, NY_TOKCH = 32;     // token chunks per head: landmark-column kernels (= workspace bound) / token-owning kernels
constexpr int NY_IMG = 16384;                        // one fragment image of a 64 x 64 tile (hi + lo)
constexpr int NY_PART = NY_M * NY_D;                 // floats of one [256, 64] partial

struct NyArgs {
  const float* q; const float* k; const float* v;
  int64_t ld, T;
  const float* ql; const float* kl; int64_t ldl;
  float scale, sl2e;                                 // sl2e = scale * log2(e): P = exp2(s * sl2e - lse2)
  int nch;
  // per entry point
  const float* w2; const float* dout; int64_t ldd;
  const float* lse1; float* lse1_o; float* delta; const float* delta_i;
  const float* lse3; const float* delta3; const float* da3v; const float* u;
  float* out; int64_t ldo;
  float* out2; int64_t ldo2;
  float* part; float* part2;
  int accumulate;
};


// token-column kernels (nys_flash_tok.hip): enqueue only
int nytok_out_bwd_q(hipStream_t st, const NyArgs& g);
int nytok_a3v_bwd_t(hipStream_t st, const NyArgs& g, int mode);

// ---- bag-batched forms of the forward's token-streaming kernels (mhimx_infer_transmil_run: infer_transmil.hip).
// Every bag of a call owns T[b] consecutive rows of ONE padded token space (its front pad rows first) from row tok0[b] on.  The table
// travels by value; the batched entry of a kernel takes the bag from blockIdx.z, relocates the single-bag kernel's arguments to that
// bag and returns when its block index lies beyond the bag's own extent - then the single-bag kernel's body runs unchanged, so a bag's
// chunks, tile walk and merge order (hence its bits) are those of the single-bag launch on that bag alone.
struct NyBags {
  int64_t tok0[MHIMX_INFER_MAX];                     // first row of the bag in the padded token space
  int32_t T[MHIMX_INFER_MAX];                        // padded tokens: 256 * ceil(n / 256), n = N + 1 (cls token first)
  int32_t n[MHIMX_INFER_MAX];                        // tokens; pad = T - n front rows
  int32_t H[MHIMX_INFER_MAX], wrapN[MHIMX_INFER_MAX];    // PPEG grid side and wrap count of the n - 1 instance tokens (mhimx_ppeg_side)
  int32_t nbags, maxT;
};
// dst = arr[b] (constant indices only: a dynamically indexed by-value argument is copied to scratch)
#define NY_PICK(dst, arr, b)                                     \
  _Pragma("unroll") for (int q_ = 0; q_ < MHIMX_INFER_MAX; ++q_) \
    if (q_ == (int)(b)) dst = (arr)[q_];

// attn_ops.hip.  lm [nbags, 256, C]: the means of l = T / 256 consecutive rows of the first C columns of x (row pitch ldx)
int landmark_mean_many(hipStream_t st, const NyBags& tb, const float* x, int64_t ldx, int C, float* lm);
// z0 / stats of mhimx_pinv_init per bag: a, z [nbags * 8, 256, 256], stats [nbags, 4], ws 2 * nbags * 8 * 256 floats; the two maxima
// are taken over ONE bag's 8 matrices
int pinv_init_many(hipStream_t st, int nbags, const float* a, float* z, float* stats, float* ws);
// mhimx_resconv (33 taps, dim_head 64, C = 512, written not added) per bag: the stencil stops at the bag's first and last padded row
int resconv_many(hipStream_t st, const NyBags& tb, const float* v, int64_t ldv, const float* w, float* out, int64_t ldo);
// mhimx_ppeg_fwd (grid = 0) on the n - 1 rows behind every bag's cls row, y -> x2 (both [sum T, 512]); the cls row is copied
int ppeg_fwd_many(hipStream_t st, const NyBags& tb, const float* y, const float* wc, const float* bc, float* x2);
// nys_flash.hip.  base: q / k / v / ld of the whole token space, ql / kl / ldl of bag 0's landmark means (bag b: + b * 256 * ldl), scale.
// a3v [nbags, 8, 256, 64], lse3 [nbags, 8, 256]; ws: mhimx_nys_ws_floats floats PER BAG
int nys_a3v_fwd_many(hipStream_t st, const NyBags& tb, const NyArgs& base, float* a3v, float* lse3, float* ws);
// out (+)= softmax_m(q k~^T) w2, w2 [nbags, 8, 256, 64], out rows of the token space (pitch ldo)
int nys_out_fwd_many(hipStream_t st, const NyBags& tb, const NyArgs& base, const float* w2, float* out, int64_t ldo, int accumulate);
// nys_flash_tok.hip.  The cls row of every bag's streamed attention, r[token] = sum_lm u[lm] softmax_n(q~ k^T)[lm, token] (mhimx_nys_cls_attn
// per bag: min(T / 64, 64) chunks), written WITHOUT the pad columns and the cls column (r[:, pad + 1:]) into the bag's segment of the packed
// rows: attn [8, R], head pitch R = sum N_b, bag b's rows from N_0 + .. + N_{b-1} on.  base: k / ld of the whole token space, ql / ldl of
// bag 0's landmark means, scale; lse3, u [nbags, 8, 256]
int nys_cls_attn_many(hipStream_t st, const NyBags& tb, const NyArgs& base, const float* lse3, const float* u, float* attn, int64_t R);

}  // namespace mhimx
