// infer_tab.hpp — the per-bag table of the ragged inference launches (mhimx_infer_run: infer.hip; its projection kernel: bag_project.hip).
#pragma once
#include "mma_tile.hpp"

namespace mhimx {

// Everything a kernel needs to know about a bag, as ONE by-value kernel argument: no host-to-device copy, nothing to wait for.
struct InferTab {
  const float* X[MHIMX_INFER_MAX];
  int64_t ldx[MHIMX_INFER_MAX], N[MHIMX_INFER_MAX];
  int64_t row0[MHIMX_INFER_MAX];                  // first row of the bag in the call's row space (feature rows, score, attn)
  int32_t tile0[MHIMX_INFER_MAX];                 // first 160-row projection tile
  int32_t part0[MHIMX_INFER_MAX];                 // first pool partial (= first 256-row scorer chunk)
  int32_t n, tiles, parts, pad;                   // pad: the element type of the rows X points to (mhimx.h MHIMX_X_*; 0 = fp32)
};
// (constant indices only: a dynamically indexed by-value argument is copied to scratch)
#define IT_PICK(dst, field, b)                                   \
  _Pragma("unroll") for (int q_ = 0; q_ < MHIMX_INFER_MAX; ++q_) \
    if (q_ == (b)) dst = tab.field[q_];

// The element type XT (MHIMX_X_*) of the bags' rows in the two kernels that read X (infer_project_body: bag_project.hip; pw_tn_body:
// pure_window.hip): what 4 / 2 consecutive elements are loaded as, and their widening to fp32 - exact for every fp16 and bf16 value,
// subnormals included (v_cvt_f32_f16 honours fp16 denormals; a bf16 IS the upper half of an fp32).  XT = 0 is the identity.
typedef float x_f2 __attribute__((ext_vector_type(2)));
typedef unsigned x_u2 __attribute__((ext_vector_type(2)));
typedef _Float16 x_h2 __attribute__((ext_vector_type(2)));
template <int XT> struct XRow { typedef float elt; typedef f32x4 v4; typedef x_f2 v2; };
template <> struct XRow<1> { typedef _Float16 elt; typedef x_u2 v4; typedef unsigned v2; };
template <> struct XRow<2> { typedef unsigned short elt; typedef x_u2 v4; typedef unsigned v2; };
template <int XT> MHIMX_DEV x_f2 x_widen(unsigned w) {          // two 2-byte elements of one dword
  if constexpr (XT == 1) {
    const x_h2 h = __builtin_bit_cast(x_h2, w);
    return x_f2{(float)h[0], (float)h[1]};
  } else {
    return x_f2{__builtin_bit_cast(float, w << 16), __builtin_bit_cast(float, w & 0xffff0000u)};
  }
}
template <int XT> MHIMX_DEV f32x4 x_widen(const x_u2& w) {
  const x_f2 a = x_widen<XT>(w[0]), b = x_widen<XT>(w[1]);
  return f32x4{a[0], a[1], b[0], b[1]};
}
template <int XT> MHIMX_DEV const f32x4& x_widen(const f32x4& v) { return v; }
template <int XT> MHIMX_DEV const x_f2& x_widen(const x_f2& v) { return v; }

constexpr int INFER_TILE_ROWS = 160;              // rows of a projection tile (bag-major tile numbering: InferTab.tile0)
constexpr int IE = 512;                           // feature width of the ragged path

// what the TRAIN-mode ragged projection (mhimx_pure_window_run) needs beyond the table: every bag's dropout seed, the device tick the
// seeds are mixed with, the dropout probability and the fp16 d out / d pre rows (row space of the call, like the feature rows)
struct PureWinDrop {
  uint64_t seed[MHIMX_INFER_MAX];
  const uint64_t* tick;
  _Float16* dact;
  float drop_p, pad;
};
int pure_window_project(hipStream_t st, const InferTab& tab, const PureWinDrop& dr, int D, const float* w1p, const float* b1, int act, float* Hout);
// the ragged scorer + pool-partial launch of infer.hip (one workgroup per 256-row chunk of one bag; InferTab.part0 / .parts / .row0)
int infer_score(hipStream_t st, const InferTab& tab, const float* H, const float* wa_frag, const float* wc, int act, float* s, float* pm, float* pl,
                float* pz);

// the same launch + the class projections of the pseudo score, cproj [rows of the row space][4] = h . Wp_c (C <= 4), taken while the rows are
// LDS-resident (mhimx_ragged_window_run's teacher)
int infer_score_cproj(hipStream_t st, const InferTab& tab, const float* H, const float* wa_frag, const float* wc, int act, float* s, float* pm,
                      float* pl, float* pz, const float* wp, int C, float* cproj);
// pure_window.hip's split-K rule, d W1 = sum_b dPRE_b^T X_b launch (pw_tn_kernel<true>) and index-order reduction launch as host calls
int pw_split_k(int steps, int want_max, int div, int32_t* S, int32_t* per);
int pw_wgrad_bagx(hipStream_t st, const InferTab& tab, const float* dpre, int D, int steps, int S, int per, float* slabs);
int pw_reduce(hipStream_t st, int n, const float* const* parts, const int32_t* G, const int64_t* W, float* const* out);
// step.hip: the checks mhimx_step_run makes on (cfg, N, counts)
int step_check_cfg(const mhimx_step_cfg* c, int64_t N, const mhimx_step_counts* n);

// the ragged one-model projection launch (bag_project.hip): Hout[row0[b] + m, :] = act(X_b[m, :] W1^T + b1) for every bag b of the table
int infer_project(hipStream_t st, const InferTab& tab, int D, const float* w1p, const float* b1, int act, float* Hout);

}  // namespace mhimx
