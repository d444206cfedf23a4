// nys_flash_tok.hip - the TOKEN-COLUMN kernels of the streamed Nystrom attention (see nys_flash.hip for the scheme): the token-side
// backward of out (dq), the token-side backward of a3v (dk, dv) and the cls row, all in the token-owning form: a wave owns 16 tokens and
// ALL 256 landmarks, so there is no cross-wave sum and no barrier in the loop.  (The landmark-split form these replaced - 4 waves x 64
// landmarks, the waves' partial outputs summed through LDS with 3 barriers per 32-token half - measured 281 vs 156 us for dk / dv and
// 199 vs 103 us for dq at T = 50 176.)
#include "nys_args.hpp"

namespace mhimx {
namespace nytok {

MHIMX_DEV float ny_kgsum(float v) { v += __shfl_xor(v, 16); v += __shfl_xor(v, 32); return v; }

MHIMX_DEV void ny_split8(const float (&v)[8], f32x4& hi_o, f32x4& lo_o) {
  bf8 hi, lo;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const __bf16 h = (__bf16)v[q];
    hi[q] = h;
    lo[q] = (__bf16)(v[q] - (float)h);
  }
  hi_o = __builtin_bit_cast(f32x4, hi);
  lo_o = __builtin_bit_cast(f32x4, lo);
}
MHIMX_DEV void ny_split44(const f32x4& a, const f32x4& b, f32x4& hi, f32x4& lo) {
  const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  ny_split8(v, hi, lo);
}

MHIMX_DEV void ny_chunk(const NyArgs& g, int ch, int& t_begin, int& t_end) {
  const int64_t tiles = g.T / NY_TT;
  t_begin = (int)(tiles * ch / g.nch);
  t_end = (int)(tiles * (ch + 1) / g.nch);
}

// ===========================================================================================================================
// Token-owning form of the a3v token-side backward (dk, dv): NO barrier and no cross-wave sum in the loop.  The two landmark-side
// matrices (q~ and da3v, [256, 64] of this head) sit in LDS ONCE, row-major, as bf16 hi / lo planes (128-byte rows, 16-byte chunk
// index XOR (row & 7)): an LM fragment (landmark rows, 8 consecutive head dims per lane) is a 16-byte read of a row, an LT fragment
// (head-dim rows, 8 landmarks per lane in accumulator-pair order) is TWO ds_read_b64_tr_b16 of the SAME planes - in a 16-lane group
// lane 4 r + q supplies the address of (landmark r, dims 4 q .. 4 q + 3) and lane l receives dim l of landmarks 0..3 (probed:
// tools/micro/tr_probe.hip).  Both reads are conflict-free under the XOR (b128: 16-lane groups {0-3,12-15,20-27}.. hit 16 different
// 4-bank spans; tr: 32 lanes = 8 rows x 32 bytes, even rows banks 0-31, odd rows 32-63, chunk pair db ^ (r >> 1)).  Four fragment
// images of the landmark-split form (256 KB) would not fit; the two planes pairs are 128 KB.
// A wave owns 16 tokens and ALL 256 landmarks, streamed 32 at a time: S^T, dP^T [2 lb] -> P, dS -> dv^T, dk^T [4 db]
// accumulate in registers.  k / v fragments come straight from global memory (8 consecutive head dims of the lane's token).
// 281 -> 156 us at T = 50 176 (the out backward's twin below: 199 -> 103 us).  Measured and dropped: starting waves 4..7 (the second
// wave of each SIMD) 8..48 x 64 cycles late so that the pair does not run its matrix and VALU phases in lockstep: +-1 %.
// ===========================================================================================================================
constexpr int NY8_THREADS = 512, NY8_NW = 8;
constexpr int NY_PLANE = NY_M * 128;                           // one bf16 plane of a [256, 64] matrix
constexpr int NY_SM_A3_T8 = 4 * NY_PLANE + 2 * NY_M * 4;
typedef __bf16 ny_bf4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) char* ny_lds;

MHIMX_DEV void ny_plane_fill(char* hi, char* lo, const float* M, int64_t ldm, int tid) {
#pragma unroll
  for (int u = 0; u < NY_M * 8 / NY8_THREADS; ++u) {
    const int unit = tid + NY8_THREADS * u, row = unit >> 3, oct = unit & 7;
    const float* p = M + (int64_t)row * ldm + 8 * oct;
    f32x4 h, l;
    ny_split44(*reinterpret_cast<const f32x4*>(p), *reinterpret_cast<const f32x4*>(p + 4), h, l);
    const int off = row * 128 + ((oct ^ (row & 7)) << 4);
    *reinterpret_cast<f32x4*>(hi + off) = h;
    *reinterpret_cast<f32x4*>(lo + off) = l;
  }
}
// LT fragment: landmarks 32 sx + {4 kg + i, 16 + 4 kg + i}, head dim 16 db + c; `a` = the lane's address for (sx 0, blk 0, this db)
MHIMX_DEV f32x4 ny_plane_lt(ny_lds a, int sx) {
  typedef __attribute__((address_space(3))) ny_bf4* P;
  const ny_bf4 x = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((P)(a + sx * 4096));
  const ny_bf4 y = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((P)(a + sx * 4096 + 2048));
  bf8 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) { r[j] = x[j]; r[4 + j] = y[j]; }
  return __builtin_bit_cast(f32x4, r);
}

__global__ __launch_bounds__(NY8_THREADS) void ny_a3v_bwd_t8_kernel(NyArgs g) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  char* q_hi = sm;
  char* q_lo = sm + NY_PLANE;
  char* a_hi = sm + 2 * NY_PLANE;
  char* a_lo = sm + 3 * NY_PLANE;
  float* lmst = reinterpret_cast<float*>(sm + 4 * NY_PLANE);   // lse3[256] | delta3[256]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, kg = lane >> 4;
  const int h = blockIdx.y, ch = blockIdx.x;
  int t_begin, t_end;
  ny_chunk(g, ch, t_begin, t_end);
  ny_plane_fill(q_hi, q_lo, g.ql + h * NY_D, g.ldl, tid);
  ny_plane_fill(a_hi, a_lo, g.da3v + (int64_t)h * NY_PART, NY_D, tid);
  if (tid < NY_M) {
    lmst[tid] = g.lse3[h * NY_M + tid];
    lmst[NY_M + tid] = g.delta3[h * NY_M + tid];
  }
  __syncthreads();
  // per-lane offsets inside a plane
  // (the XOR touches the chunk bits only: ks flips bit 6 of the offset, db bits 5-6 - one register each, an immediate per use)
  const int lm_off0 = c * 128 + ((kg ^ (c & 7)) << 4);         // LM fragment (lb 0, ks 0); ks 1: ^ 64
  const int lt_r = 4 * kg + (c >> 2);
  const int lt_off0 = lt_r * 128 + ((((c & 3) >> 1) ^ (lt_r & 7)) << 4) + (c & 1) * 8;   // LT fragment (sx 0, blk 0, db 0); db: ^ (db << 5)
  const ny_lds lq_hi = (ny_lds)q_hi, lq_lo = (ny_lds)q_lo, la_hi = (ny_lds)a_hi, la_lo = (ny_lds)a_lo;
  const float* kb = g.k + h * NY_D;
  const float* vb = g.v + h * NY_D;
  // 16 tokens per wave; the LDS reads of a phase are issued one phase ahead: the LT fragments of step sx before its S / dP products,
  // the LM fragments of step sx + 1 before its exp / split work (step 8 = step 0 of the wave's next group: the landmark side does not
  // depend on the tokens).  With the reads next to their use the waves sat in s_waitcnt for 47 % of their cycles (SQ_WAIT_ANY).
  const int64_t grp_end = (int64_t)t_end * 4;
  f32x4 lmf[16];                                               // [l2][ks][q~ hi, q~ lo, da hi, da lo]
  auto ld_lm = [&](int sx) {
#pragma unroll
    for (int l2 = 0; l2 < 2; ++l2)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int o = (2 * sx + l2) * 2048 + (lm_off0 ^ (ks << 6));
        lmf[(l2 * 2 + ks) * 4 + 0] = *reinterpret_cast<const f32x4*>(q_hi + o);
        lmf[(l2 * 2 + ks) * 4 + 1] = *reinterpret_cast<const f32x4*>(q_lo + o);
        lmf[(l2 * 2 + ks) * 4 + 2] = *reinterpret_cast<const f32x4*>(a_hi + o);
        lmf[(l2 * 2 + ks) * 4 + 3] = *reinterpret_cast<const f32x4*>(a_lo + o);
      }
  };
  ld_lm(0);
  // kv: [k ks0 | k ks1 | v ks0 | v ks1] x (hi, lo), or the two raw 16-byte halves before the split.  (Requesting the next group's
  // k / v into these registers as soon as the group's last S / dP products have issued measured SLOWER: 343 vs 336 us per entry.)
  f32x4 kv[8];
  auto ld_kv = [&](int64_t grp) {
    const int64_t o = (grp * 16 + c) * g.ld + 8 * kg;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      kv[2 * ks] = *reinterpret_cast<const f32x4*>(kb + o + 32 * ks);
      kv[2 * ks + 1] = *reinterpret_cast<const f32x4*>(kb + o + 32 * ks + 4);
      kv[4 + 2 * ks] = *reinterpret_cast<const f32x4*>(vb + o + 32 * ks);
      kv[5 + 2 * ks] = *reinterpret_cast<const f32x4*>(vb + o + 32 * ks + 4);
    }
  };
  const int64_t grp0 = (int64_t)t_begin * 4 + w;
  if (grp0 < grp_end) ld_kv(grp0);
  for (int64_t grp = grp0; grp < grp_end; grp += NY8_NW) {
    const int64_t tok = grp * 16 + c;
    if (grp != grp0) ld_kv(grp);
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      f32x4 hi, lo;
      ny_split44(kv[2 * x], kv[2 * x + 1], hi, lo);
      kv[2 * x] = hi;
      kv[2 * x + 1] = lo;
    }
    f32x4 ov[4], ok[4];                                        // [db]
#pragma unroll
    for (int db = 0; db < 4; ++db) { ov[db] = f32x4{0.f, 0.f, 0.f, 0.f}; ok[db] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma nounroll
    for (int sx = 0; sx < 8; ++sx) {
      f32x4 ath[4], atl[4], qth[4], qtl[4];
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        ath[db] = ny_plane_lt(la_hi + (lt_off0 ^ (db << 5)), sx); atl[db] = ny_plane_lt(la_lo + (lt_off0 ^ (db << 5)), sx);
        qth[db] = ny_plane_lt(lq_hi + (lt_off0 ^ (db << 5)), sx); qtl[db] = ny_plane_lt(lq_lo + (lt_off0 ^ (db << 5)), sx);
      }
      f32x4 ls[2], dl[2];                                      // (LDS reads return in order: these must not sit behind the LM prefetch)
#pragma unroll
      for (int l2 = 0; l2 < 2; ++l2) {
        ls[l2] = *reinterpret_cast<const f32x4*>(lmst + 32 * sx + 16 * l2 + 4 * kg);
        dl[l2] = *reinterpret_cast<const f32x4*>(lmst + NY_M + 32 * sx + 16 * l2 + 4 * kg);
      }
      __builtin_amdgcn_sched_barrier(0);
      f32x4 s[2], dp[2];                                       // [lb & 1]
#pragma unroll
      for (int l2 = 0; l2 < 2; ++l2) { s[l2] = f32x4{0.f, 0.f, 0.f, 0.f}; dp[l2] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {                         // term-major over the four (matrix, landmark block) accumulators
#pragma unroll
        for (int l2 = 0; l2 < 2; ++l2) {
          s[l2] = mt_mfma(lmf[(l2 * 2 + ks) * 4 + 1], kv[2 * ks], s[l2]);
          dp[l2] = mt_mfma(lmf[(l2 * 2 + ks) * 4 + 3], kv[4 + 2 * ks], dp[l2]);
        }
#pragma unroll
        for (int l2 = 0; l2 < 2; ++l2) {
          s[l2] = mt_mfma(lmf[(l2 * 2 + ks) * 4 + 0], kv[2 * ks + 1], s[l2]);
          dp[l2] = mt_mfma(lmf[(l2 * 2 + ks) * 4 + 2], kv[5 + 2 * ks], dp[l2]);
        }
#pragma unroll
        for (int l2 = 0; l2 < 2; ++l2) {
          s[l2] = mt_mfma(lmf[(l2 * 2 + ks) * 4 + 0], kv[2 * ks], s[l2]);
          dp[l2] = mt_mfma(lmf[(l2 * 2 + ks) * 4 + 2], kv[4 + 2 * ks], dp[l2]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      ld_lm((sx + 1) & 7);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int l2 = 0; l2 < 2; ++l2)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float pr = NY_EXP2(s[l2][i] * g.sl2e - ls[l2][i]);
          s[l2][i] = pr;
          dp[l2][i] = g.scale * pr * (dp[l2][i] - dl[l2][i]);
        }
      f32x4 ph, pl, sh, sl;
      ny_split44(s[0], s[1], ph, pl);
      ny_split44(dp[0], dp[1], sh, sl);
#pragma unroll
      for (int db = 0; db < 4; ++db) { ov[db] = mt_mfma(atl[db], ph, ov[db]); ok[db] = mt_mfma(qtl[db], sh, ok[db]); }
#pragma unroll
      for (int db = 0; db < 4; ++db) { ov[db] = mt_mfma(ath[db], pl, ov[db]); ok[db] = mt_mfma(qth[db], sl, ok[db]); }
#pragma unroll
      for (int db = 0; db < 4; ++db) { ov[db] = mt_mfma(ath[db], ph, ov[db]); ok[db] = mt_mfma(qth[db], sh, ok[db]); }
    }
    float* okp = g.out + tok * g.ldo + h * NY_D + 4 * kg;
    float* ovp = g.out2 + tok * g.ldo2 + h * NY_D + 4 * kg;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      *reinterpret_cast<f32x4*>(okp + 16 * db) = ok[db];
      f32x4 bv = ov[db];
      if (g.accumulate) bv += *reinterpret_cast<const f32x4*>(ovp + 16 * db);
      *reinterpret_cast<f32x4*>(ovp + 16 * db) = bv;
    }
  }
}

// ===========================================================================================================================
// Token-owning form of the out token-side backward (dq, delta): k~ (LM for S, LT for dq) and w2 (LM for dP) as row-major planes;
// a wave owns 16 tokens and holds S^T and dP^T of ALL 256 landmarks ([16 lb] accumulators each), because delta = sum_m P dP of a
// token must be complete before any dS: the softmax row is the lane's own accumulators + its three k-octet lanes, no cross-wave
// step, no barrier.  q / dout fragments straight from global memory.
// ===========================================================================================================================
__global__ __launch_bounds__(NY8_THREADS) void ny_out_bwd_q8_kernel(NyArgs g) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  char* k_hi = sm;
  char* k_lo = sm + NY_PLANE;
  char* w_hi = sm + 2 * NY_PLANE;
  char* w_lo = sm + 3 * NY_PLANE;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, kg = lane >> 4;
  const int h = blockIdx.y, ch = blockIdx.x;
  int t_begin, t_end;
  ny_chunk(g, ch, t_begin, t_end);
  ny_plane_fill(k_hi, k_lo, g.kl + h * NY_D, g.ldl, tid);
  ny_plane_fill(w_hi, w_lo, g.w2 + (int64_t)h * NY_PART, NY_D, tid);
  __syncthreads();
  int lm_off[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) lm_off[ks] = c * 128 + (((4 * ks + kg) ^ (c & 7)) << 4);
  int lt_off[4];
  {
    const int r = 4 * kg + (c >> 2), r7 = r & 7;
#pragma unroll
    for (int db = 0; db < 4; ++db) lt_off[db] = r * 128 + (((2 * db + ((c & 3) >> 1)) ^ r7) << 4) + (c & 1) * 8;
  }
  const ny_lds lk_hi = (ny_lds)k_hi, lk_lo = (ny_lds)k_lo;
  const float* qb = g.q + h * NY_D;
  const float* gb = g.dout + h * NY_D;
  const float* lse = g.lse1 + (int64_t)h * g.T;
  const int64_t grp_end = (int64_t)t_end * 4;
  for (int64_t grp = (int64_t)t_begin * 4 + w; grp < grp_end; grp += NY8_NW) {
    const int64_t tok = grp * 16 + c;
    f32x4 qh[2], ql[2], gh[2], gl[2];                          // [ks]
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const float* pq = qb + tok * g.ld + 32 * ks + 8 * kg;
      const float* pg = gb + tok * g.ldd + 32 * ks + 8 * kg;
      ny_split44(*reinterpret_cast<const f32x4*>(pq), *reinterpret_cast<const f32x4*>(pq + 4), qh[ks], ql[ks]);
      ny_split44(*reinterpret_cast<const f32x4*>(pg), *reinterpret_cast<const f32x4*>(pg + 4), gh[ks], gl[ks]);
    }
    const float ls = lse[tok];
    f32x4 s[16], dp[16];                                       // [lb]
#pragma unroll
    for (int lb = 0; lb < 16; ++lb) { s[lb] = f32x4{0.f, 0.f, 0.f, 0.f}; dp[lb] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    // fragments of block lb + 1 are requested before the products of block lb (the scheduling barriers keep the 128 reads from
    // being hoisted to the top)
    f32x4 fa[8], fb[8];                                        // k~ (ks0 hi, lo, ks1 hi, lo), w2 (the same)
    auto ld_lm = [&](int lb, f32x4 (&f)[8]) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int o = lb * 2048 + lm_off[ks];
        f[2 * ks] = *reinterpret_cast<const f32x4*>(k_hi + o);
        f[2 * ks + 1] = *reinterpret_cast<const f32x4*>(k_lo + o);
        f[4 + 2 * ks] = *reinterpret_cast<const f32x4*>(w_hi + o);
        f[5 + 2 * ks] = *reinterpret_cast<const f32x4*>(w_lo + o);
      }
    };
    auto mm = [&](int lb, const f32x4 (&f)[8]) {                // term-major over the four (matrix, ks) products
      s[lb] = mt_mfma(f[1], qh[0], s[lb]);
      dp[lb] = mt_mfma(f[5], gh[0], dp[lb]);
      s[lb] = mt_mfma(f[0], ql[0], s[lb]);
      dp[lb] = mt_mfma(f[4], gl[0], dp[lb]);
      s[lb] = mt_mfma(f[0], qh[0], s[lb]);
      dp[lb] = mt_mfma(f[4], gh[0], dp[lb]);
      s[lb] = mt_mfma(f[3], qh[1], s[lb]);
      dp[lb] = mt_mfma(f[7], gh[1], dp[lb]);
      s[lb] = mt_mfma(f[2], ql[1], s[lb]);
      dp[lb] = mt_mfma(f[6], gl[1], dp[lb]);
      s[lb] = mt_mfma(f[2], qh[1], s[lb]);
      dp[lb] = mt_mfma(f[6], gh[1], dp[lb]);
    };
    ld_lm(0, fa);
#pragma unroll
    for (int lb = 0; lb < 16; lb += 2) {
      ld_lm(lb + 1, fb);
      mm(lb, fa);
      __builtin_amdgcn_sched_barrier(0);
      if (lb + 2 < 16) ld_lm(lb + 2, fa);
      mm(lb + 1, fb);
      __builtin_amdgcn_sched_barrier(0);
    }
    float dl = 0.f;
#pragma unroll
    for (int lb = 0; lb < 16; ++lb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float pr = NY_EXP2(s[lb][i] * g.sl2e - ls);
        s[lb][i] = pr;
        dl += pr * dp[lb][i];
      }
    dl = ny_kgsum(dl);
    if (kg == 0) g.delta[(int64_t)h * g.T + tok] = dl;
    f32x4 o[4];                                                // [db]
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int sx = 0; sx < 8; ++sx) {
      f32x4 dh, dlo, th[4], tl[4];
#pragma unroll
      for (int db = 0; db < 4; ++db) { th[db] = ny_plane_lt(lk_hi + lt_off[db], sx); tl[db] = ny_plane_lt(lk_lo + lt_off[db], sx); }
#pragma unroll
      for (int l2 = 0; l2 < 2; ++l2)
#pragma unroll
        for (int i = 0; i < 4; ++i) s[2 * sx + l2][i] = g.scale * s[2 * sx + l2][i] * (dp[2 * sx + l2][i] - dl);
      ny_split44(s[2 * sx], s[2 * sx + 1], dh, dlo);
#pragma unroll
      for (int db = 0; db < 4; ++db) o[db] = mt_mfma(tl[db], dh, o[db]);
#pragma unroll
      for (int db = 0; db < 4; ++db) o[db] = mt_mfma(th[db], dlo, o[db]);
#pragma unroll
      for (int db = 0; db < 4; ++db) o[db] = mt_mfma(th[db], dh, o[db]);
      __builtin_amdgcn_sched_barrier(0);
    }
    float* op = g.out + tok * g.ldo + h * NY_D + 4 * kg;
#pragma unroll
    for (int db = 0; db < 4; ++db) *reinterpret_cast<f32x4*>(op + 16 * db) = o[db];
  }
}

// ===========================================================================================================================
// The cls row r[token] = sum_lm u[lm] softmax_n(q~ k^T)[lm, token] (nystrom:143-150) in the token-owning form: q~ as row-major planes,
// a wave owns 16 tokens and all 256 landmarks (S^T[16 lb] in registers), no barrier in the loop.
// MANY: the bag-batched entry (NyBags, nys_args.hpp; one kernel template for the reason given at ny_out_fwd_tok8_kernel) - blockIdx.z = bag,
// min(T / 64, NY_CLSCH) chunks of its own tokens, blocks beyond return; the argument block is relocated to the bag and the single-bag code
// runs as it is up to the store: the bag's row lands in its segment of the packed instance rows (head pitch g.ldo), token pad + 1 + i at
// entry i - the pad columns and the cls column are not written.
// ===========================================================================================================================
constexpr int NY_CLSCH = 64;                                   // 66 KB of LDS, 84 VGPRs: two workgroups per CU
constexpr int NY_SM_CLS = 2 * NY_PLANE + 2 * NY_M * 4;
template <bool MANY>
__global__ __launch_bounds__(NY8_THREADS) void ny_cls_row8_kernel(NyArgs g, NyBags tb) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  [[maybe_unused]] int first = 0;                              // MANY: the bag's first instance token (pad + 1)
  if constexpr (MANY) {
    int64_t tok0 = tb.tok0[0];
    int T = tb.T[0], n = tb.n[0];
    NY_PICK(tok0, tb.tok0, blockIdx.z) NY_PICK(T, tb.T, blockIdx.z) NY_PICK(n, tb.n, blockIdx.z)
    const int nch = T / NY_TT < NY_CLSCH ? T / NY_TT : NY_CLSCH;
    if ((int)blockIdx.x >= nch) return;
    int64_t row0 = 0;                                          // instance rows of the bags in front
#pragma unroll
    for (int q = 0; q < MHIMX_INFER_MAX; ++q)
      if (q < (int)blockIdx.z) row0 += tb.n[q] - 1;
    g.T = T;
    g.nch = nch;
    g.k += tok0 * g.ld;
    g.ql += (int64_t)blockIdx.z * NY_M * g.ldl;
    g.lse3 += (int64_t)blockIdx.z * NY_H * NY_M;
    g.u += (int64_t)blockIdx.z * NY_H * NY_M;
    g.out += row0;
    first = T - n + 1;
  }
  char* q_hi = sm;
  char* q_lo = sm + NY_PLANE;
  float* lmst = reinterpret_cast<float*>(sm + 2 * NY_PLANE);   // lse3[256] | u[256]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, kg = lane >> 4;
  const int h = blockIdx.y, ch = blockIdx.x;
  int t_begin, t_end;
  ny_chunk(g, ch, t_begin, t_end);
  ny_plane_fill(q_hi, q_lo, g.ql + h * NY_D, g.ldl, tid);
  if (tid < NY_M) {
    lmst[tid] = g.lse3[h * NY_M + tid];
    lmst[NY_M + tid] = g.u[h * NY_M + tid];
  }
  __syncthreads();
  int lm_off[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) lm_off[ks] = c * 128 + (((4 * ks + kg) ^ (c & 7)) << 4);
  const float* kb = g.k + h * NY_D;
  const int64_t grp_end = (int64_t)t_end * 4;
  for (int64_t grp = (int64_t)t_begin * 4 + w; grp < grp_end; grp += NY8_NW) {
    const int64_t tok = grp * 16 + c;
    f32x4 kh[2], kl[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const float* pk = kb + tok * g.ld + 32 * ks + 8 * kg;
      ny_split44(*reinterpret_cast<const f32x4*>(pk), *reinterpret_cast<const f32x4*>(pk + 4), kh[ks], kl[ks]);
    }
    float r = 0.f;
    f32x4 fa[4], fb[4];                                        // (ks0 hi, lo, ks1 hi, lo) of one landmark block
    auto ld_lm = [&](int lb, f32x4 (&f)[4]) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int o = lb * 2048 + lm_off[ks];
        f[2 * ks] = *reinterpret_cast<const f32x4*>(q_hi + o);
        f[2 * ks + 1] = *reinterpret_cast<const f32x4*>(q_lo + o);
      }
    };
    auto blk = [&](int lb, const f32x4 (&f)[4]) {
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
      s = mt_mfma(f[1], kh[0], s);
      s = mt_mfma(f[0], kl[0], s);
      s = mt_mfma(f[0], kh[0], s);
      s = mt_mfma(f[3], kh[1], s);
      s = mt_mfma(f[2], kl[1], s);
      s = mt_mfma(f[2], kh[1], s);
      const f32x4 ls = *reinterpret_cast<const f32x4*>(lmst + 16 * lb + 4 * kg);
      const f32x4 uu = *reinterpret_cast<const f32x4*>(lmst + NY_M + 16 * lb + 4 * kg);
#pragma unroll
      for (int i = 0; i < 4; ++i) r += uu[i] * NY_EXP2(s[i] * g.sl2e - ls[i]);
    };
    ld_lm(0, fa);
#pragma unroll
    for (int lb = 0; lb < 16; lb += 2) {
      ld_lm(lb + 1, fb);
      blk(lb, fa);
      __builtin_amdgcn_sched_barrier(0);
      if (lb + 2 < 16) ld_lm(lb + 2, fa);
      blk(lb + 1, fb);
      __builtin_amdgcn_sched_barrier(0);
    }
    r = ny_kgsum(r);
    if constexpr (MANY) {
      if (kg == 0 && tok >= first) g.out[(int64_t)h * g.ldo + (tok - first)] = r;
    } else {
      if (kg == 0) g.out[(int64_t)h * g.T + tok] = r;
    }
  }
}

}  // namespace nytok

// The two backward kernels write per-token outputs only (no per-chunk partials), so their chunking is free.  One workgroup per CU
// (128 KB of LDS): 64 chunks measured 9.48 vs 9.43 ms per c3 step.
static NyArgs ny_tok_chunks(const NyArgs& g0) {
  NyArgs g = g0;
  const int64_t tiles = g.T / NY_TT;
  g.nch = (int)(tiles < NY_TOKCH ? tiles : NY_TOKCH);
  return g;
}
int nytok_out_bwd_q(hipStream_t st, const NyArgs& g0) {
  using namespace nytok;
  const NyArgs g = ny_tok_chunks(g0);
  MHIMX_ONCE_PER_DEVICE(MHIMX_HIP(hipFuncSetAttribute((const void*)ny_out_bwd_q8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * NY_PLANE)));
  hipLaunchKernelGGL(ny_out_bwd_q8_kernel, dim3(g.nch, NY_H), dim3(NY8_THREADS), 4 * NY_PLANE, st, g);
  MHIMX_LAUNCH_CHECK();
  return 0;
}
int nytok_a3v_bwd_t(hipStream_t st, const NyArgs& g0, int mode) {
  using namespace nytok;
  if (mode == 0) {
    const NyArgs g = ny_tok_chunks(g0);
    MHIMX_ONCE_PER_DEVICE(MHIMX_HIP(hipFuncSetAttribute((const void*)ny_a3v_bwd_t8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, NY_SM_A3_T8)));
    hipLaunchKernelGGL(ny_a3v_bwd_t8_kernel, dim3(g.nch, NY_H), dim3(NY8_THREADS), NY_SM_A3_T8, st, g);
    MHIMX_LAUNCH_CHECK();
    return 0;
  }
  NyArgs gc = g0;
  const int64_t tiles = gc.T / NY_TT;
  gc.nch = (int)(tiles < NY_CLSCH ? tiles : NY_CLSCH);
  MHIMX_ONCE_PER_DEVICE(MHIMX_HIP(hipFuncSetAttribute((const void*)ny_cls_row8_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, NY_SM_CLS)));
  hipLaunchKernelGGL(ny_cls_row8_kernel<false>, dim3(gc.nch, NY_H), dim3(NY8_THREADS), NY_SM_CLS, st, gc, NyBags{});
  MHIMX_LAUNCH_CHECK();
  return 0;
}
int nys_cls_attn_many(hipStream_t st, const NyBags& tb, const NyArgs& base, const float* lse3, const float* u, float* attn, int64_t R) {
  using namespace nytok;
  MHIMX_CHECK_ARG(base.k && base.ql && lse3 && u && attn && aligned16(base.k) && aligned16(base.ql) && base.ld % 4 == 0 && base.ldl % 4 == 0 && R >= 1,
                  "nys_cls_attn_many: null / unaligned operands");
  NyArgs g = base;
  g.lse3 = lse3; g.u = u; g.out = attn; g.ldo = R;
  MHIMX_ONCE_PER_DEVICE(MHIMX_HIP(hipFuncSetAttribute((const void*)ny_cls_row8_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, NY_SM_CLS)));
  hipLaunchKernelGGL(ny_cls_row8_kernel<true>, dim3(NY_CLSCH, NY_H, (unsigned)tb.nbags), dim3(NY8_THREADS), NY_SM_CLS, st, g, tb);
  MHIMX_LAUNCH_CHECK();
  return 0;
}

}  // namespace mhimx
