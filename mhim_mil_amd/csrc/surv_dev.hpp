// surv_dev.hpp — ONE copy of the survival head's row math (train_utils.py:8-37, engines/base_engine.py:636-643) for every kernel that
// evaluates it: surv_nll_kernel (surv.hip: validation), the survival forms of head_kernel / head_fast_kernel (optim.hip:
// mhimx_head_surv_fwd_bwd, the head of mhimx_ragged_window_run_surv) and of pw_head_kernel (pure_window.hip: mhimx_pure_window_run_surv).
// Loss and gradient out of a train call are therefore, bit for bit, what mhimx_surv_nll gives on the logits that call wrote.
#pragma once
#include <math.h>
#include <stddef.h>

#include "common.hpp"

namespace mhimx {

constexpr int SURV_MAXK = 16;

MHIMX_DEV double surv_softplus(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }

// one row: K <= MAXK logits in registers, one pass for hazards / survival / risk / loss, one for the gradient row.  The head is K values
// - nothing beside the forward that made the logits - so it is evaluated in fp64 and rounded to fp32 once per output: the deviation from
// an fp64 evaluation of the reference's formulas is the rounding of the result, whatever the device's fp32 log / exp do.
// l[k >= K] is not read; g[k >= K] = 0.  y64 outside [0, K): loss NaN, gradient row 0; the risk does not depend on y.
// want_g false: g is left alone.  g = g_scale * d loss / d l.
template <int MAXK>
MHIMX_DEV void surv_row(const float (&l)[MAXK], int K, int64_t y64, float c, float alpha, float eps, float g_scale, bool want_g, float& risk,
                        float& loss, float (&g_out)[MAXK]) {
  const bool y_ok = y64 >= 0 && y64 < K;
  const int y = y_ok ? (int)y64 : -1;
  const double cr = (double)c, al = (double)alpha, ep = (double)eps;
  double h[MAXK];
  // S_pad[y] = S_{y-1} (1 at y = 0), S_pad[y + 1] = S_y: the two survival values the loss gathers, each with its log in the stable
  // form log S_k = -sum_{m <= k} softplus(l_m); log h_y = -softplus(-l_y)
  double S = 1.0, logS = 0.0, rsum = 0.0;
  double S_prev = 1.0, logS_prev = 0.0, S_at = 1.0, logS_at = 0.0, h_at = 1.0, logh_at = 0.0;
#pragma unroll
  for (int k = 0; k < MAXK; ++k) {
    if (k < K) {
      const double lk = (double)l[k];
      h[k] = 1.0 / (1.0 + exp(-lk));
      if (k == y) { S_prev = S; logS_prev = logS; h_at = h[k]; logh_at = -surv_softplus(-lk); }
      S *= 1.0 / (1.0 + exp(lk));                               // 1 - h without the cancellation
      logS -= surv_softplus(lk);
      rsum += S;
      if (k == y) { S_at = S; logS_at = logS; }
    } else {
      h[k] = 0.0;
    }
  }
  risk = (float)-rsum;
  // the reference clamps the QUANTITY (torch.clamp(min=eps) before the log): a clamped term is the constant log(eps), gradient 0
  const bool a_live = S_prev >= ep, b_live = h_at >= ep, c_live = S_at >= ep;
  const double log_eps = log(ep);
  const double unc = -(1.0 - cr) * ((a_live ? logS_prev : log_eps) + (b_live ? logh_at : log_eps));
  const double cen = -cr * (c_live ? logS_at : log_eps);
  loss = y_ok ? (float)((1.0 - al) * (cen + unc) + al * unc) : NAN;
  if (want_g) {
    // d log S_k / d l_m = -h_m (m <= k);  d log h_y / d l_y = 1 - h_y;  unc enters both terms of the loss: weight (1 - alpha) + alpha = 1
#pragma unroll
    for (int k = 0; k < MAXK; ++k) {
      double g = 0.0;
      if (k < K && y_ok) {
        double du = 0.0, dc = 0.0;                              // d (log terms) / d l_k
        if (a_live && k < y) du -= h[k];
        if (b_live && k == y) du += 1.0 - h[k];
        if (c_live && k <= y) dc -= h[k];
        g = (double)g_scale * (-(1.0 - cr) * du + (1.0 - al) * (-cr * dc));
      }
      g_out[k] = (float)g;
    }
  }
}

// the survival description a head kernel takes by value: the censorship flag's address, NLLSurvLoss(alpha), the clamp, where the risk goes
struct HeadSurv { const float* censor; float alpha, eps; float* risk; };

static_assert(sizeof(mhimx_surv_spec) == 8 + 8 * MHIMX_INFER_MAX + 8 && offsetof(mhimx_surv_spec, censor_dev) == 8 &&
                  offsetof(mhimx_surv_spec, risk) == 8 + 8 * MHIMX_INFER_MAX,
              "mhimx_surv_spec: the layout the ctypes mirror (_lib.SurvSpec) is written against");

// ---- host (surv.hip): the checks a native train call makes on its survival description before any device call, the bag named
int surv_spec_check(const char* who, int32_t n_bags, const mhimx_surv_spec* surv);
// the one body of mhimx_pure_window_run(_x) (surv NULL: cross entropy) and mhimx_pure_window_run_surv (pure_window.hip)
int pure_window_run(void* stream, const mhimx_step_cfg* cfg, int32_t n_bags, const mhimx_pure_window_bag* bags, int64_t host_step, void* ws,
                    int64_t ws_bytes, int32_t update, int32_t x_dtype, const mhimx_surv_spec* surv);
// the one body of mhimx_ragged_window_run(_x) and mhimx_ragged_window_run_surv (ragged_window.hip)
int ragged_window_run(void* stream, const mhimx_step_cfg* cfg, int32_t n_bags, const mhimx_ragged_window_bag* bags, int64_t host_step, void* ws,
                      int64_t ws_bytes, int32_t update, int32_t x_dtype, const mhimx_surv_spec* surv);

}  // namespace mhimx
