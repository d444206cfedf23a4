// surv.hip — survival validation on the device: the survival head of a pass (hazards, survival curve, risk, discrete-time NLL loss and
// its gradient; train_utils.py:8-37, engines/base_engine.py:636-643) and the censored concordance index of every bootstrap resample
// (engines/metrics.py:66-104 = sksurv.metrics.concordance_index_censored(tied_tol=1e-8), wrapped in the DeterministicBootStrapper of
// engines/metrics.py:35-64).
//
// The C-index path has the shape of metrics.hip's ROC area: all B resamples (blockIdx.y) are evaluated by the same three launches
//   1. gather : every resample's (time, event, risk) written contiguously into the workspace
//   2. pairs  : exact pair counts - one i per thread, all j swept through LDS tiles, 64-bit integer counters
//   3. final  : (concordant + 0.5 tied_risk) / comparable in fp64 from the integer counts
// Integer counts throughout: the only floating-point work is the fp32 risk difference against tied_tol and the final ratio.
#include <math.h>

#include "common.hpp"
#include "surv_dev.hpp"

namespace mhimx {

constexpr int CI_TILE = 1024;

// one thread per row: K <= 16 logits in registers, the row math of surv_dev.hpp (fp64, every output rounded to fp32 once)
__global__ __launch_bounds__(256) void surv_nll_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ Y,
                                                       const float* __restrict__ c, int64_t n, int K, float alpha, float eps, float g_scale,
                                                       float* __restrict__ risk, float* __restrict__ losses, float* __restrict__ g_logits) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  float l[SURV_MAXK], g[SURV_MAXK];
#pragma unroll
  for (int k = 0; k < SURV_MAXK; ++k) l[k] = k < K ? logits[r * ld + k] : 0.f;
  float rk, ls;
  surv_row<SURV_MAXK>(l, K, Y[r], c[r], alpha, eps, g_scale, g_logits != nullptr, rk, ls, g);
  risk[r] = rk;
  losses[r] = ls;
  if (g_logits) {
#pragma unroll
    for (int k = 0; k < SURV_MAXK; ++k)
      if (k < K) g_logits[r * K + k] = g[k];
  }
}

// time_ws / event_ws / risk_ws [B][n]: sample i of resample b is row idx[b][i] (row i without idx); an index outside [0, n) marks
// the resample bad (its five outputs become NaN) and stands in as a sample no pair rule can reach
__global__ void ci_gather_kernel(const uint8_t* __restrict__ event, const double* __restrict__ time, const float* __restrict__ risk,
                                 const int64_t* __restrict__ idx, int64_t n, double* __restrict__ time_ws, uint8_t* __restrict__ event_ws,
                                 float* __restrict__ risk_ws, int* __restrict__ bad) {
  const int b = blockIdx.y;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = idx ? idx[(int64_t)b * n + i] : i;
    const bool ok = r >= 0 && r < n;
    const int64_t o = (int64_t)b * n + i;
    time_ws[o] = ok ? time[r] : (double)NAN;
    event_ws[o] = ok ? (event[r] ? 1 : 0) : 0;
    risk_ws[o] = ok ? risk[r] : 0.f;
    if (!ok) atomicOr(&bad[b], 1);
  }
}

// counts[b][0..3] += {comparable, concordant, tied_risk, tied_time} over the pairs (i, j), i in this block's slice, j over the resample:
// comparable iff event_i and (time_j > time_i or (time_j == time_i and !event_j))
__global__ __launch_bounds__(256) void ci_pairs_kernel(const double* __restrict__ time_ws, const uint8_t* __restrict__ event_ws,
                                                       const float* __restrict__ risk_ws, int64_t n, float tied_tol,
                                                       unsigned long long* __restrict__ counts) {
  const int b = blockIdx.y;
  const double* tm = time_ws + (int64_t)b * n;
  const uint8_t* ev = event_ws + (int64_t)b * n;
  const float* rk = risk_ws + (int64_t)b * n;
  __shared__ double st[CI_TILE];
  __shared__ float sr[CI_TILE];
  __shared__ int se[CI_TILE];
  unsigned long long a_cmp = 0, a_con = 0, a_tie = 0, a_tt = 0;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool mine = i < n && ev[i] != 0;
  const double ti = mine ? tm[i] : 0.0;
  const float ri = mine ? rk[i] : 0.f;
  for (int64_t j0 = 0; j0 < n; j0 += CI_TILE) {
    __syncthreads();
    for (int t = threadIdx.x; t < CI_TILE; t += 256) {
      const int64_t j = j0 + t;
      st[t] = j < n ? tm[j] : (double)NAN;                       // padding: a time no comparison reaches
      sr[t] = j < n ? rk[j] : 0.f;
      se[t] = j < n ? (int)ev[j] : 1;
    }
    __syncthreads();
    if (mine) {
      unsigned cmp = 0, con = 0, tie = 0, tt = 0;
      for (int t = 0; t < CI_TILE; ++t) {
        const double tj = st[t];
        const bool same = tj == ti && !se[t];
        if (tj > ti || same) {
          const float rj = sr[t];
          const bool tied = fabsf(rj - ri) <= tied_tol;
          cmp += 1u;
          tt += same ? 1u : 0u;
          tie += tied ? 1u : 0u;
          con += (!tied && rj < ri) ? 1u : 0u;
        }
      }
      a_cmp += cmp; a_con += con; a_tie += tie; a_tt += tt;
    }
  }
  // wave sums -> one atomic per wave and counter
  for (int o = 32; o > 0; o >>= 1) {
    a_cmp += __shfl_down(a_cmp, o, 64);
    a_con += __shfl_down(a_con, o, 64);
    a_tie += __shfl_down(a_tie, o, 64);
    a_tt += __shfl_down(a_tt, o, 64);
  }
  if ((threadIdx.x & 63) == 0 && a_cmp) {
    unsigned long long* cb = counts + (int64_t)b * 4;
    atomicAdd(&cb[0], a_cmp);
    if (a_con) atomicAdd(&cb[1], a_con);
    if (a_tie) atomicAdd(&cb[2], a_tie);
    if (a_tt) atomicAdd(&cb[3], a_tt);
  }
}

// out [B][5]: cindex, concordant, discordant, tied_risk, tied_time
__global__ void ci_final_kernel(const unsigned long long* __restrict__ counts, const int* __restrict__ bad, int B, double* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const unsigned long long* cb = counts + (int64_t)b * 4;
  double* o = out + (int64_t)b * 5;
  if (bad[b]) {
    for (int k = 0; k < 5; ++k) o[k] = (double)NAN;
    return;
  }
  const double cmp = (double)cb[0], con = (double)cb[1], tie = (double)cb[2];
  o[0] = cb[0] ? (con + 0.5 * tie) / cmp : (double)NAN;
  o[1] = con;
  o[2] = (double)(cb[0] - cb[1] - cb[2]);
  o[3] = tie;
  o[4] = (double)cb[3];
}

// (n, B) a call takes: B rides in gridDim.y; n and B * n keep the workspace (13 bytes per gathered sample) under 2 GiB
static int ci_check(const char* who, int64_t n, int64_t B) {
  MHIMX_CHECK_ARG(n >= 1 && n <= MHIMX_CINDEX_MAX_N, "%s: n=%lld must be in 1..%d", who, (long long)n, MHIMX_CINDEX_MAX_N);
  MHIMX_CHECK_ARG(B >= 1 && B <= MHIMX_CINDEX_MAX_B, "%s: B=%lld must be in 1..%d", who, (long long)B, MHIMX_CINDEX_MAX_B);
  MHIMX_CHECK_ARG(B * n <= MHIMX_CINDEX_MAX_BN, "%s: B * n = %lld exceeds %d (evaluate the resamples in slices)", who, (long long)(B * n),
                  MHIMX_CINDEX_MAX_BN);
  return 0;
}

// alpha in [0, 1], eps in (0, 1), a censorship flag for every bag: mhimx_surv_nll's rules, per bag of a train call
int surv_spec_check(const char* who, int32_t n_bags, const mhimx_surv_spec* surv) {
  MHIMX_CHECK_ARG(surv->alpha >= 0.f && surv->alpha <= 1.f, "%s: survival alpha=%g must be in [0, 1]", who, (double)surv->alpha);
  MHIMX_CHECK_ARG(surv->eps > 0.f && surv->eps < 1.f, "%s: survival eps=%g must be in (0, 1)", who, (double)surv->eps);
  for (int b = 0; b < n_bags && b < MHIMX_INFER_MAX; ++b)
    MHIMX_CHECK_ARG(surv->censor_dev[b], "%s: bag %d: null censorship flag (surv->censor_dev)", who, b);
  return 0;
}

}  // namespace mhimx

using namespace mhimx;

extern "C" int mhimx_surv_nll(void* stream, const float* logits, int64_t ld, const int64_t* Y, const float* c, int64_t n, int64_t K,
                              float alpha, float eps, float g_scale, float* risk, float* losses, float* g_logits) {
  const char* who = "mhimx_surv_nll";
  MHIMX_CHECK_ARG(logits && Y && c && risk && losses, "%s: null logits / Y / c / risk / losses", who);
  MHIMX_CHECK_ARG(K >= 1 && K <= SURV_MAXK, "%s: K=%lld must be in 1..%d", who, (long long)K, SURV_MAXK);
  MHIMX_CHECK_ARG(n >= 1 && n <= MHIMX_SURV_MAX_N, "%s: n=%lld must be in 1..%d", who, (long long)n, MHIMX_SURV_MAX_N);
  MHIMX_CHECK_ARG(ld >= K, "%s: ld=%lld is smaller than K=%lld", who, (long long)ld, (long long)K);
  MHIMX_CHECK_ARG(eps > 0.f && eps < 1.f, "%s: eps=%g must be in (0, 1)", who, (double)eps);
  MHIMX_CHECK_ARG(alpha >= 0.f && alpha <= 1.f, "%s: alpha=%g must be in [0, 1]", who, (double)alpha);
  hipLaunchKernelGGL(surv_nll_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, logits, ld, Y, c, n, (int)K, alpha, eps,
                     g_scale, risk, losses, g_logits);
  MHIMX_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t mhimx_cindex_ws_bytes(int64_t n, int64_t B) {
  if (ci_check("mhimx_cindex_ws_bytes", n, B)) return -1;
  int64_t bytes = 0;
  bytes += align_up(B * 4 * 8, 256);                                // pair counts
  bytes += align_up(B * 4, 256);                                    // bad-index flags
  bytes += align_up(B * n * 8, 256);                                // times
  bytes += align_up(B * n * 4, 256);                                // risks
  bytes += align_up(B * n, 256);                                    // events
  return bytes;
}

extern "C" int mhimx_cindex(void* stream, const uint8_t* event, const double* time, const float* risk, int64_t n, const int64_t* sample_idx,
                            int64_t B, float tied_tol, double* out, void* ws, int64_t ws_bytes) {
  const char* who = "mhimx_cindex";
  MHIMX_CHECK_ARG(event && time && risk && out, "%s: null event / time / risk / out", who);
  if (ci_check(who, n, B)) return -1;
  MHIMX_CHECK_ARG(B == 1 || sample_idx, "%s: B=%lld resamples need sample_idx [B, n] (null)", who, (long long)B);
  MHIMX_CHECK_ARG(tied_tol >= 0.f, "%s: tied_tol=%g must be >= 0", who, (double)tied_tol);
  MHIMX_CHECK_ARG(ws, "%s: null workspace", who);
  MHIMX_CHECK_ARG(((uintptr_t)ws & 255) == 0, "%s: the workspace must be 256-byte aligned", who);
  MHIMX_CHECK_ARG(ws_bytes >= mhimx_cindex_ws_bytes(n, B), "%s: workspace too small (%lld bytes, %lld needed)", who, (long long)ws_bytes,
                  (long long)mhimx_cindex_ws_bytes(n, B));
  hipStream_t st = (hipStream_t)stream;
  char* p = (char*)ws;
  unsigned long long* counts = (unsigned long long*)p; p += align_up(B * 4 * 8, 256);
  int* bad = (int*)p; p += align_up(B * 4, 256);
  double* time_ws = (double*)p; p += align_up(B * n * 8, 256);
  float* risk_ws = (float*)p; p += align_up(B * n * 4, 256);
  uint8_t* event_ws = (uint8_t*)p;
  MHIMX_HIP(hipMemsetAsync(counts, 0, (size_t)(align_up(B * 4 * 8, 256) + B * 4), st));      // counts and flags are neighbours
  const unsigned gx = (unsigned)(cdiv(n, 256) < 1024 ? cdiv(n, 256) : 1024);
  hipLaunchKernelGGL(ci_gather_kernel, dim3(gx, (unsigned)B), dim3(256), 0, st, event, time, risk, sample_idx, n, time_ws, event_ws, risk_ws,
                     bad);
  MHIMX_LAUNCH_CHECK();
  hipLaunchKernelGGL(ci_pairs_kernel, dim3((unsigned)cdiv(n, 256), (unsigned)B), dim3(256), 0, st, time_ws, event_ws, risk_ws, n, tied_tol,
                     counts);
  MHIMX_LAUNCH_CHECK();
  hipLaunchKernelGGL(ci_final_kernel, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, st, counts, bad, (int)B, out);
  MHIMX_LAUNCH_CHECK();
  return 0;
}
