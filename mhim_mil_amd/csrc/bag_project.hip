// bag_project.hip — the entry points of the bag projection and the RAGGED one-model projection kernels.
//
//     H_g[N,E] = dropout_g( act( X[N,D] . W_g[E,D]^T + b_g ) ),  g = 0 (teacher), 1 (student)      (mhim.py:69-76,84)
//
// The reference's student computes the feature on ALL N rows before it masks (modules/mhim.py:335-336) and its teacher
// does the same on the same bag (mhim.py:186): the two projections are one GEMM with B = [W_teacher; W_student]
// (2E = 1024 output columns).  X is read from HBM once per step instead of twice, there is no separate "pair planes"
// pass over the bag (the fp32 -> bf16 hi/lo split happens on the way into LDS, once per workgroup), and the per-CU
// operand ingest per output halves against the 160 x 128 tiling of feat_gemm.hip.
//
// mhimx_bag_project / mhimx_bag_project_multi check their arguments here and launch the specialised-wave kernel of bag_project_ws.hip
// (8 ping-pong consumer waves + 4 producer waves).  The kernels of THIS file are the ragged one-model projections of mhimx_infer_run
// and mhimx_pure_window_run (infer_project_body below): same tiles, same arithmetic, as a uniform 8-wave lock-step loop.
//
// Shape on MI355X: N = 10 000 rows x 1024 columns = 10.24 M outputs over 256 CUs = 40 000 per CU, so the workgroup
// tile is 160 x 256 (40 960 outputs): ceil(10000/160) x 4 = 252 tiles — one balanced round over the chip.
//   * 8 waves as 2 (M) x 4 (N), 80 x 64 outputs per wave = 5 x 4 blocks of v_mfma_f32_16x16x32_bf16 in the 3-term
//     bf16 form (hi*hi + hi*lo + lo*hi, ~2^-16: the instance scores feed a top-k), 60 MFMAs per 32-deep k-step per wave;
//     two waves per SIMD cover each other's LDS latency.
//   * B (the weights, already paired planes made by the step's prep launch) goes L2 -> LDS by direct DMA
//     (global_load_lds_dwordx4); A (raw fp32 X) goes through registers: 16-byte coalesced loads one k-step ahead,
//     split into bf16 hi / lo (v_cvt_pk_bf16_f32) and written as the same paired 128-byte row image the DMA path uses,
//     so the fragment reads (and their bank swizzle) are those of feat_gemm.hip.
//   * 3-stage LDS ring of [160 + 256 rows][128 B] = 156 KB, one s_barrier per k-step: B is issued two tiles ahead, A one tile
//     ahead; the MFMAs are software-pipelined across the barrier (the last term of tile t-1 runs under the first fragment reads
//     of tile t), so the matrix pipe has work while LDS reads are in flight.
//   * epilogue through LDS in two 80-row halves (one compact loop: bias, GELU and its derivative from one erf, counter
//     dropout with one hash per two elements, 512-byte row stores).  The student's d out / d pre goes out as fp16.
//   * XCD-aware tile order: the column tiles of one row tile run on the same XCD (X rows shared through its L2).
//   MEASURED (lock-step against a ping-pong of the two waves of every SIMD, same box, p = 0.25, us): lock-step 72.4-73.8 | ping-pong
//   71.0-75.4 by where the split / stores / DMA sit.  The k-step moves 144 KB of fragment reads + 52 KB of operand writes through the LDS
//   against 2 x 1020 MFMA cycles: ~80 % LDS occupancy whatever the phase structure - the lever is fewer fragment bytes per MFMA, which
//   is what the specialised-wave form of bag_project_ws.hip buys.
#include "mma_tile.hpp"
#include "infer_tab.hpp"

namespace mhimx {

constexpr int PBN = 256, PBK = 32;        // column tile and k-step of mhimx_bag_project (the argument checks below)

typedef _Float16 pj_h4 __attribute__((ext_vector_type(4)));

// one hash per TWO elements: 16-bit fields against a 16-bit threshold (p quantised to 1/65536; the keep scale uses the
// quantised probability, so the mask is exactly unbiased)
MHIMX_DEV uint32_t pj_pair_hash(uint32_t row_key, uint32_t pair) { return mix32(row_key + pair * 0x85EBCA77u); }

// ------------------------------------------------------------------------------------------------------------------------
// The RAGGED one-model projection of mhimx_infer_run (infer.hip; modules/mhim.py:229-272 forward_test, eval mode): the feature rows of up to
// MHIMX_INFER_MAX bags of different row counts in one launch.  Row tiles are numbered bag-major from the by-value table (infer_tab.hpp), a
// bag's last tile is partial; a tile lies inside ONE bag.  The tiling, the LDS image and the k loop are the lock-step form the file header
// describes; eval mode needs no second model, no dropout, no d out / d pre and no residual rows.
// ------------------------------------------------------------------------------------------------------------------------
constexpr int IBM = INFER_TILE_ROWS, IBN = 256, IBK = 32, ITHREADS = 512;
constexpr int IA_BYTES = IBM * 128, IB_BYTES = IBN * 128, ISTAGE = IA_BYTES + IB_BYTES, INST = 3;      // 3 x 52 KiB
constexpr int ITP = IBN + 4;                                                                          // epilogue tile pitch (floats)
typedef __bf16 in_bf4 __attribute__((ext_vector_type(4)));
typedef __bf16 in_bf2 __attribute__((ext_vector_type(2)));
typedef float in_f2 __attribute__((ext_vector_type(2)));

// TRAIN (mhimx_pure_window_run, pure_window.hip): the same tile walk and k loop; the epilogue is that of mhimx_bag_project - per-bag counter
// dropout (row key = row INSIDE the bag: a bag's mask is the one mhimx_bag_project draws for it alone with the same seed and tick) and the
// fp16 d out / d pre rows - and the rows between a bag's N and the next multiple of 32 (the call's row space starts every bag at a
// multiple of 32) are written as zero rows, so that no later launch of the window reads workspace memory nobody wrote.
//
// XT: the element type of the bags' rows (mhimx.h MHIMX_X_*: 0 fp32, 1 fp16, 2 bf16; tab.X then points to 2-byte elements and ldx counts
// them).  A half row is loaded as half the bytes per unit (8 / 8 / 4 instead of 16 / 16 / 8: still three VMEM operations per k-step, so the
// waits and the DMA ring are the fp32 form's), widened to fp32 in registers - exact for every fp16 and bf16 value, subnormals included - and
// handed to the same split (XRow / x_widen: infer_tab.hpp): the LDS image, and with it every bit behind it, is that of the fp32 kernel on
// the widened rows.
// ELEM (TRAIN only; mhimx_dsmil_window_run): the keep-mask is the per-element law of the gemm epilogues (drop_keep_k: one 24-bit hash per
// element, keep scale 1 / (1 - p)) - the mask ops.gemm_nt draws for the same seed, tick, row and column - instead of mhimx_bag_project's.
template <bool TRAIN, int XT, bool ELEM = false>
MHIMX_DEV void infer_project_body(const InferTab& tab, int D, const float* __restrict__ w1p, const float* __restrict__ b1, int act,
                                  float* __restrict__ Hout, const PureWinDrop& dr) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  constexpr int nN = IE / IBN;
  // XCD-aware order: the two column tiles of a row tile run on the same XCD (its X rows are shared through that L2)
  const int xcd = blockIdx.x & 7, sidx = blockIdx.x >> 3;
  const int m_tile = (sidx / nN) * 8 + xcd, n_tile = sidx % nN;
  if (m_tile >= tab.tiles) return;
  int bag = 0;
#pragma unroll
  for (int b = 1; b < MHIMX_INFER_MAX; ++b)
    if (b < tab.n && m_tile >= tab.tile0[b]) bag = b;
  const float* X = tab.X[0];
  int64_t ldx = tab.ldx[0], N = tab.N[0], orow0 = tab.row0[0];
  int t0 = tab.tile0[0];
  RG_PICK(X, tab.X, bag) RG_PICK(ldx, tab.ldx, bag) RG_PICK(N, tab.N, bag) RG_PICK(orow0, tab.row0, bag) RG_PICK(t0, tab.tile0, bag)
  const int64_t m0 = (int64_t)(m_tile - t0) * IBM;             // first row of the tile inside its bag
  const int64_t n0 = (int64_t)n_tile * IBN;
  typedef typename XRow<XT>::elt XE;
  const XE* Xt = reinterpret_cast<const XE*>(X) + m0 * ldx;    // uniform: the tile's first row

  // ---- A (raw rows): two units of 4 elements u = tid + 512 j (row u >> 3, slot u & 7; rows 0..127) and one unit of 2 elements of rows
  // 128..159 - 16 / 16 / 8 bytes of fp32, 8 / 8 / 4 bytes of fp16 / bf16
  unsigned aoff[3];                                           // byte offsets from Xt (< 160 rows)
  unsigned a_hi[3], a_lo[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int row = j < 2 ? (tid >> 3) + 64 * j : 128 + (tid >> 4);
    const int slot = j < 2 ? (tid & 7) : ((tid & 15) >> 1);
    const int sub = j < 2 ? 0 : (tid & 1) * 4;
    int64_t mr = row;
    if (m0 + mr >= N) mr = N - 1 - m0;                         // clamped rows feed accumulators that are never stored
    aoff[j] = (unsigned)((mr * ldx + slot * 4 + (sub >> 1)) * (int)sizeof(XE));
    const int sw = mt_swz(row), kg2 = (slot >> 1) * 2;
    a_hi[j] = (unsigned)(row * 128 + ((kg2 ^ sw) << 4) + (slot & 1) * 8 + sub);
    a_lo[j] = (unsigned)(row * 128 + (((kg2 + 1) ^ sw) << 4) + (slot & 1) * 8 + sub);
  }
  // ---- B (paired weights) by DMA: slot p = tid + 512 j of a [256 rows][8 x 16 B] tile, SOURCE slot swizzled
  const unsigned boff = (unsigned)(((tid >> 3) * D + ((tid & 7) ^ mt_swz(tid >> 3)) * 4) * 4);
  const char* bbase = reinterpret_cast<const char*>(w1p + n0 * D);
  // `live` false (past the last k-step): the same four pieces are issued from ONE address into a stage nobody reads any more, so that every
  // iteration has the same VMEM count and the hand-written vmcnt waits need no branch
  auto issue_b = [&](int t, bool live) {
    char* sb = smem + (t % INST) * ISTAGE + IA_BYTES + wave * 1024;
    const int64_t k0 = (int64_t)t * IBK;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const char* bj = bbase + ((int64_t)j * 64 * D + k0) * 4;      // uniform
      __builtin_amdgcn_global_load_lds((gptr_f)(live ? bj + boff : reinterpret_cast<const char*>(Xt)), (lptr_f)(sb + j * 8192), 16, 0, 0);
    }
  };
  // the A loads of the loop are inline asm, waited for by hand (the compiler's wait-count pass would drain the DMA pieces issued behind them)
  struct ARegs { typename XRow<XT>::v4 v0, v1; typename XRow<XT>::v2 v2; };
  auto load_a_async = [&](int t, ARegs& r) {
    const XE* xk = Xt + (int64_t)t * IBK;                      // uniform: an SGPR pair
    if constexpr (XT == 0)
      asm volatile("global_load_dwordx4 %0, %3, %6\n\tglobal_load_dwordx4 %1, %4, %6\n\tglobal_load_dwordx2 %2, %5, %6"
                   : "=&v"(r.v0), "=&v"(r.v1), "=&v"(r.v2)
                   : "v"(aoff[0]), "v"(aoff[1]), "v"(aoff[2]), "s"(xk)
                   : "memory");
    else
      asm volatile("global_load_dwordx2 %0, %3, %6\n\tglobal_load_dwordx2 %1, %4, %6\n\tglobal_load_dword %2, %5, %6"
                   : "=&v"(r.v0), "=&v"(r.v1), "=&v"(r.v2)
                   : "v"(aoff[0]), "v"(aoff[1]), "v"(aoff[2]), "s"(xk)
                   : "memory");
  };
  auto split4 = [&](const f32x4& v, char* hi_p, char* lo_p) {
    in_bf4 hi, lo;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const __bf16 h = (__bf16)v[q];
      hi[q] = h;
      lo[q] = (__bf16)(v[q] - (float)h);
    }
    *reinterpret_cast<in_bf4*>(hi_p) = hi;
    *reinterpret_cast<in_bf4*>(lo_p) = lo;
  };
  auto store_a = [&](int t, const ARegs& r) {                 // registers -> bf16 hi / lo -> the paired row image of stage t % 3
    char* sa = smem + (t % INST) * ISTAGE;
    split4(x_widen<XT>(r.v0), sa + a_hi[0], sa + a_lo[0]);
    split4(x_widen<XT>(r.v1), sa + a_hi[1], sa + a_lo[1]);
    const in_f2 v2 = x_widen<XT>(r.v2);
    in_bf2 hi, lo;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const __bf16 h = (__bf16)v2[q];
      hi[q] = h;
      lo[q] = (__bf16)(v2[q] - (float)h);
    }
    *reinterpret_cast<in_bf2*>(sa + a_hi[2]) = hi;
    *reinterpret_cast<in_bf2*>(sa + a_lo[2]) = lo;
  };

  // fragment addresses (stage 0): row r = lane & 15 of a 16-row block, k-group kg = lane >> 4 -> slots 2kg (hi), 2kg+1 (lo)
  const int r16 = lane & 15, kg = lane >> 4;
  const unsigned lds0 = (unsigned)(uintptr_t)(lptr_f)smem;
  const int ra = wm * 80 + r16, rb = wn * 64 + r16;
  const unsigned fa_hi = lds0 + ra * 128 + (((2 * kg) ^ mt_swz(ra)) << 4);
  const unsigned fa_lo = lds0 + ra * 128 + (((2 * kg + 1) ^ mt_swz(ra)) << 4);
  const unsigned fb_hi = lds0 + IA_BYTES + rb * 128 + (((2 * kg) ^ mt_swz(rb)) << 4);
  const unsigned fb_lo = lds0 + IA_BYTES + rb * 128 + (((2 * kg + 1) ^ mt_swz(rb)) << 4);

  f32x4 acc[NRA][NRB];
#pragma unroll
  for (int i = 0; i < NRA; ++i)
#pragma unroll
    for (int j = 0; j < NRB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = D / IBK;
  ARegs rga, rgb;
  // prologue: B(0), B(1) in flight, A(0) -> stage 0 (the compiler's wait in front of the conversion drains all three), A(1) in flight
  issue_b(0, true);
  issue_b(1, nk > 1);
  {
    ARegs r0;
    const char* xb = reinterpret_cast<const char*>(Xt);
    r0.v0 = *reinterpret_cast<const typename XRow<XT>::v4*>(xb + aoff[0]);
    r0.v1 = *reinterpret_cast<const typename XRow<XT>::v4*>(xb + aoff[1]);
    r0.v2 = *reinterpret_cast<const typename XRow<XT>::v2*>(xb + aoff[2]);
    store_a(0, r0);
  }
  load_a_async(nk > 1 ? 1 : 0, rga);

  // Iteration t (3-stage ring):  [barrier: tile t complete in stage t % 3]
  //   reads g1(t) = {A lo, B hi};  A(t+2) loads -> the free register set;  B(t+2) DMA -> stage (t+2) % 3 (= (t-1) % 3: every wave is past its
  //   reads);  20 MFMAs hi*lo of tile t-1 (operands still in registers);  reads g2(t) = {A hi, B lo};  20 MFMAs lo*hi of tile t;  wait until
  //   only this iteration's 7 VMEM operations are in flight (A(t+1) is in its registers, B(t+1) has landed);  20 MFMAs hi*hi of tile t with
  //   the split of A(t+1) and its LDS stores into stage (t+1) % 3 in their shadow.
  f32x4 x[NFR];
  auto body = [&](int t, ARegs& r_load, ARegs& r_use) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // my A(t) stores to LDS are done
    __builtin_amdgcn_s_barrier();
    const unsigned so = (unsigned)((t % INST) * ISTAGE);
    MT_READ9(x, 5, 10, fa_lo + so, fb_hi + so);
    load_a_async(t + 2 < nk ? t + 2 : nk - 1, r_load);
    issue_b(t + 2, t + 2 < nk);
    __builtin_amdgcn_sched_barrier(0);
    if (t > 0) mt_term(x, 0, 14, acc);                        // hi*lo of tile t-1
    __builtin_amdgcn_sched_barrier(0);
    MT_WAIT9(0, x, 5, 10);
    MT_READ9(x, 0, 14, fa_hi + so, fb_lo + so);
    __builtin_amdgcn_sched_barrier(0);
    mt_term(x, 5, 10, acc);                                   // lo*hi
    __builtin_amdgcn_sched_barrier(0);
    MT_WAIT9(0, x, 0, 14);
    asm volatile("s_waitcnt vmcnt(7)" : "+v"(r_use.v0), "+v"(r_use.v1), "+v"(r_use.v2) : : "memory");
    __builtin_amdgcn_sched_barrier(0);
    mt_term(x, 0, 10, acc);                                   // hi*hi
    if (t + 1 < nk) store_a(t + 1, r_use);
#pragma unroll
    for (int q = 0; q < 20; ++q) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // one MFMA
      __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);      // three VALU
      if (q % 3 == 2) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);   // a DS write
    }
  };
  int t = 0;
#pragma unroll 1
  for (; t + 1 < nk; t += 2) {
    body(t, rgb, rga);
    body(t + 1, rga, rgb);
  }
  if (t < nk) body(t, rgb, rga);
  mt_term(x, 0, 14, acc);                                     // hi*lo of the last tile
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(rga.v0), "+v"(rga.v1), "+v"(rga.v2), "+v"(rgb.v0), "+v"(rgb.v1), "+v"(rgb.v2) : : "memory");

  // ---- epilogue, two 80-row halves through LDS (the ring is free): bias, activation, 1 KiB row stores
  float* tile = reinterpret_cast<float*>(smem);
  const int c4 = (tid & 63) * 4, r0 = tid >> 6;               // this thread's 4 columns are fixed
  const int64_t n = n0 + c4;
  const f32x4 bias = b1 ? *reinterpret_cast<const f32x4*>(b1 + n) : f32x4{0.f, 0.f, 0.f, 0.f};
  float* Hb = Hout + (orow0 + m0) * IE + n;
  const int64_t rows_left = N - m0;
  if constexpr (TRAIN) {
    uint64_t seed = dr.seed[0];
#pragma unroll
    for (int q_ = 0; q_ < MHIMX_INFER_MAX; ++q_)
      if (q_ == bag) seed = dr.seed[q_];
    uint32_t* rkeys = reinterpret_cast<uint32_t*>(smem + 80 * ITP * 4);
    const bool hashed = dr.drop_p > 0.f;
    const uint64_t dseed = hashed ? eff_seed(seed, dr.tick) : 0;
    [[maybe_unused]] const uint32_t thr16 = (uint32_t)(dr.drop_p * 65536.f + 0.5f);                       // mhimx_bag_project's pair law
    [[maybe_unused]] const float inv_keep = 65536.f / (float)(65536u - thr16);
    [[maybe_unused]] const float inv_keep_elem = 1.f / (1.f - dr.drop_p);                                 // ELEM: the gemm epilogues' law
    _Float16* db = dr.dact + (orow0 + m0) * IE + n;
    const int64_t rows_pad = ((N + 31) & ~(int64_t)31) - m0;   // the bag's rows up to the next multiple of 32: zero rows
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
      __syncthreads();
      if (wm == half) {
        const int cl = lane & 15, rq = lane >> 4;
#pragma unroll
        for (int i = 0; i < NRA; ++i)
#pragma unroll
          for (int j = 0; j < NRB; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[(i * 16 + rq * 4 + e) * ITP + wn * 64 + j * 16 + cl] = acc[i][j][e];
      }
      if (hashed && tid < 80) rkeys[tid] = drop_row_key(dseed, (uint64_t)(m0 + half * 80 + tid));
      __syncthreads();
      for (int r = r0; r < 80; r += 8) {
        const int m = half * 80 + r;
        if (m >= rows_pad) break;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        pj_h4 d = pj_h4{(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
        if (m < rows_left) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(tile + r * ITP + c4);
          float ks[4] = {1.f, 1.f, 1.f, 1.f};
          if constexpr (ELEM) {
            if (hashed) {
              const uint32_t rk = rkeys[r];
#pragma unroll
              for (int q = 0; q < 4; ++q) ks[q] = drop_keep_k(rk, (uint32_t)(n + q), dr.drop_p) ? inv_keep_elem : 0.f;
            }
          } else if (hashed) {
            const uint32_t rk = rkeys[r];
            const uint32_t h0 = pj_pair_hash(rk, (uint32_t)(n >> 1)), h1 = pj_pair_hash(rk, (uint32_t)(n >> 1) + 1u);
            ks[0] = (h0 & 0xffffu) >= thr16 ? inv_keep : 0.f;
            ks[1] = (h0 >> 16) >= thr16 ? inv_keep : 0.f;
            ks[2] = (h1 & 0xffffu) >= thr16 ? inv_keep : 0.f;
            ks[3] = (h1 >> 16) >= thr16 ? inv_keep : 0.f;
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            float y, gq;
            act_fwd_grad(a[q] + bias[q], act, y, gq);
            v[q] = y * ks[q];
            d[q] = (_Float16)(gq * ks[q]);
          }
        }
        *reinterpret_cast<pj_h4*>(db + (int64_t)m * IE) = d;
        *reinterpret_cast<f32x4*>(Hb + (int64_t)m * IE) = v;
      }
    }
    return;
  }
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    __syncthreads();                                          // fragment reads / the previous half's tile reads are over
    if (wm == half) {
      const int cl = lane & 15, rq = lane >> 4;
#pragma unroll
      for (int i = 0; i < NRA; ++i)
#pragma unroll
        for (int j = 0; j < NRB; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) tile[(i * 16 + rq * 4 + e) * ITP + wn * 64 + j * 16 + cl] = acc[i][j][e];
    }
    __syncthreads();
    for (int r = r0; r < 80; r += 8) {
      const int m = half * 80 + r;
      if (m >= rows_left) break;
      const f32x4 a = *reinterpret_cast<const f32x4*>(tile + r * ITP + c4);
      f32x4 v;
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = act_fwd(a[q] + bias[q], act);
      *reinterpret_cast<f32x4*>(Hb + (int64_t)m * IE) = v;
    }
  }
}

__global__ __launch_bounds__(ITHREADS, 2) void infer_project_kernel(InferTab tab, int D, const float* __restrict__ w1p,
                                                                    const float* __restrict__ b1, int act, float* __restrict__ Hout) {
  infer_project_body<false, 0>(tab, D, w1p, b1, act, Hout, PureWinDrop{});
}
__global__ __launch_bounds__(ITHREADS, 2) void pure_window_project_kernel(InferTab tab, PureWinDrop dr, int D, const float* __restrict__ w1p,
                                                                          const float* __restrict__ b1, int act, float* __restrict__ Hout) {
  infer_project_body<true, 0>(tab, D, w1p, b1, act, Hout, dr);
}
// the same two kernels over fp16 (XT = 1) / bf16 (XT = 2) rows: mhimx_infer_run_x, mhimx_pure_window_run_x, mhimx_ragged_window_run_x
template <int XT>
__global__ __launch_bounds__(ITHREADS, 2) void infer_project_x_kernel(InferTab tab, int D, const float* __restrict__ w1p,
                                                                      const float* __restrict__ b1, int act, float* __restrict__ Hout) {
  infer_project_body<false, XT>(tab, D, w1p, b1, act, Hout, PureWinDrop{});
}
template <int XT>
__global__ __launch_bounds__(ITHREADS, 2) void pure_window_project_x_kernel(InferTab tab, PureWinDrop dr, int D, const float* __restrict__ w1p,
                                                                            const float* __restrict__ b1, int act, float* __restrict__ Hout) {
  infer_project_body<true, XT>(tab, D, w1p, b1, act, Hout, dr);
}
// the train projection with the gemm epilogues' per-element dropout law, all three element types (mhimx_dsmil_window_run)
template <int XT>
__global__ __launch_bounds__(ITHREADS, 2) void pure_window_project_elem_kernel(InferTab tab, PureWinDrop dr, int D, const float* __restrict__ w1p,
                                                                               const float* __restrict__ b1, int act, float* __restrict__ Hout) {
  infer_project_body<true, XT, true>(tab, D, w1p, b1, act, Hout, dr);
}
template <int XT>
static int pure_window_project_elem_x(hipStream_t st, const InferTab& tab, const PureWinDrop& dr, int D, const float* w1p, const float* b1, int act,
                                      float* Hout) {
  MHIMX_ONCE_PER_DEVICE(MHIMX_HIP(hipFuncSetAttribute((const void*)pure_window_project_elem_kernel<XT>, hipFuncAttributeMaxDynamicSharedMemorySize, INST * ISTAGE)));
  hipLaunchKernelGGL(pure_window_project_elem_kernel<XT>, dim3((unsigned)(8 * (IE / IBN) * cdiv(tab.tiles, 8))), dim3(ITHREADS), INST * ISTAGE, st, tab,
                     dr, D, w1p, b1, act, Hout);
  MHIMX_LAUNCH_CHECK();
  return 0;
}
int pure_window_project_elem(hipStream_t st, const InferTab& tab, const PureWinDrop& dr, int D, const float* w1p, const float* b1, int act, float* Hout) {
  if (tab.pad == MHIMX_X_F16) return pure_window_project_elem_x<1>(st, tab, dr, D, w1p, b1, act, Hout);
  if (tab.pad == MHIMX_X_BF16) return pure_window_project_elem_x<2>(st, tab, dr, D, w1p, b1, act, Hout);
  return pure_window_project_elem_x<0>(st, tab, dr, D, w1p, b1, act, Hout);
}
template <int XT>
static int pure_window_project_x(hipStream_t st, const InferTab& tab, const PureWinDrop& dr, int D, const float* w1p, const float* b1, int act,
                                 float* Hout) {
  MHIMX_ONCE_PER_DEVICE(MHIMX_HIP(hipFuncSetAttribute((const void*)pure_window_project_x_kernel<XT>, hipFuncAttributeMaxDynamicSharedMemorySize, INST * ISTAGE)));
  hipLaunchKernelGGL(pure_window_project_x_kernel<XT>, dim3((unsigned)(8 * (IE / IBN) * cdiv(tab.tiles, 8))), dim3(ITHREADS), INST * ISTAGE, st, tab, dr,
                     D, w1p, b1, act, Hout);
  MHIMX_LAUNCH_CHECK();
  return 0;
}
template <int XT>
static int infer_project_x(hipStream_t st, const InferTab& tab, int D, const float* w1p, const float* b1, int act, float* Hout) {
  MHIMX_ONCE_PER_DEVICE(MHIMX_HIP(hipFuncSetAttribute((const void*)infer_project_x_kernel<XT>, hipFuncAttributeMaxDynamicSharedMemorySize, INST * ISTAGE)));
  hipLaunchKernelGGL(infer_project_x_kernel<XT>, dim3((unsigned)(8 * (IE / IBN) * cdiv(tab.tiles, 8))), dim3(ITHREADS), INST * ISTAGE, st, tab, D, w1p,
                     b1, act, Hout);
  MHIMX_LAUNCH_CHECK();
  return 0;
}

// (tab.pad: the element type of the bags' rows, MHIMX_X_*; the entry points have checked it)
int pure_window_project(hipStream_t st, const InferTab& tab, const PureWinDrop& dr, int D, const float* w1p, const float* b1, int act, float* Hout) {
  if (tab.pad == MHIMX_X_F16) return pure_window_project_x<1>(st, tab, dr, D, w1p, b1, act, Hout);
  if (tab.pad == MHIMX_X_BF16) return pure_window_project_x<2>(st, tab, dr, D, w1p, b1, act, Hout);
  MHIMX_ONCE_PER_DEVICE(MHIMX_HIP(hipFuncSetAttribute((const void*)pure_window_project_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, INST * ISTAGE)));
  hipLaunchKernelGGL(pure_window_project_kernel, dim3((unsigned)(8 * (IE / IBN) * cdiv(tab.tiles, 8))), dim3(ITHREADS), INST * ISTAGE, st, tab, dr, D,
                     w1p, b1, act, Hout);
  MHIMX_LAUNCH_CHECK();
  return 0;
}

int infer_project(hipStream_t st, const InferTab& tab, int D, const float* w1p, const float* b1, int act, float* Hout) {
  if (tab.pad == MHIMX_X_F16) return infer_project_x<1>(st, tab, D, w1p, b1, act, Hout);
  if (tab.pad == MHIMX_X_BF16) return infer_project_x<2>(st, tab, D, w1p, b1, act, Hout);
  MHIMX_ONCE_PER_DEVICE(MHIMX_HIP(hipFuncSetAttribute((const void*)infer_project_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, INST * ISTAGE)));
  hipLaunchKernelGGL(infer_project_kernel, dim3((unsigned)(8 * (IE / IBN) * cdiv(tab.tiles, 8))), dim3(ITHREADS), INST * ISTAGE, st, tab, D, w1p, b1,
                     act, Hout);
  MHIMX_LAUNCH_CHECK();
  return 0;
}

int bag_project_ws(hipStream_t st, const mhimx_bag_project_args* bags, int n_bags);       // bag_project_ws.hip

static int bag_project_check(const mhimx_bag_project_args& g) {
  MHIMX_CHECK_ARG(g.X && g.N >= 1 && g.D >= PBK && g.D % PBK == 0, "bag_project: X [N,D] with D a multiple of 32");
  MHIMX_CHECK_ARG(g.E >= PBN && g.E % PBN == 0, "bag_project: E must be a multiple of 256");
  MHIMX_CHECK_ARG(g.n_heads >= 1 && g.n_heads <= MHIMX_PROJ_MAX_HEADS, "bag_project: 1..%d models", MHIMX_PROJ_MAX_HEADS);
  MHIMX_CHECK_ARG(g.ldx % 4 == 0 && g.ldx >= g.D && aligned16(g.X), "bag_project: X rows must be 16-byte aligned");
  for (int h = 0; h < g.n_heads; ++h) {
    const mhimx_proj_head& H = g.head[h];
    const bool scored = h == 0 && g.score0 != nullptr;          // (the scored model 0 may leave its feature rows unwritten)
    MHIMX_CHECK_ARG(H.wp && (H.H || scored) && aligned16(H.wp) && aligned16(H.H) && (!H.H || (H.ldh % 4 == 0 && H.ldh >= g.E)),
                    "bag_project: model %d: null / unaligned weight image or output", h);
    MHIMX_CHECK_ARG(!H.resid || (aligned16(H.resid) && H.ldr % 4 == 0 && H.ldr >= g.E && H.resid != H.H), "bag_project: model %d: unaligned residual rows / the output itself", h);
    MHIMX_CHECK_ARG(!H.bias || aligned16(H.bias), "bag_project: model %d: unaligned bias", h);
    MHIMX_CHECK_ARG(!H.dact || (reinterpret_cast<uintptr_t>(H.dact) & 7) == 0, "bag_project: model %d: unaligned dact", h);
    MHIMX_CHECK_ARG(H.drop_p >= 0.f && H.drop_p < 1.f, "bag_project: model %d: dropout probability outside [0,1)", h);
    MHIMX_CHECK_ARG(!H.drop_mask || (reinterpret_cast<uintptr_t>(H.drop_mask) & 3) == 0, "bag_project: model %d: unaligned mask", h);
  }
  return 0;
}

int bag_project(hipStream_t st, const mhimx_bag_project_args* bags, int n_bags) {
  const mhimx_bag_project_args& g = bags[0];
  for (int b = 0; b < n_bags; ++b) {
    if (int rc = bag_project_check(bags[b])) return rc;
    if (b == 0) continue;
    const mhimx_bag_project_args& q = bags[b];
    bool same = q.N == g.N && q.D == g.D && q.E == g.E && q.ldx == g.ldx && q.act == g.act && q.n_heads == g.n_heads && q.drop_tick == g.drop_tick;
    for (int h = 0; same && h < g.n_heads; ++h)
      same = q.head[h].wp == g.head[h].wp && q.head[h].bias == g.head[h].bias && q.head[h].ldh == g.head[h].ldh && q.head[h].drop_p == g.head[h].drop_p &&
             !q.head[h].drop_mask && !g.head[h].drop_mask && !q.head[h].resid && !g.head[h].resid && (q.head[h].dact != nullptr) == (g.head[h].dact != nullptr);
    MHIMX_CHECK_ARG(same, "bag_project_multi: bag %d: the bags of one launch share shapes, weights, activation and dropout law (no masks, no residual rows)", b);
  }
  return bag_project_ws(st, bags, n_bags);       // the specialised-wave kernel (8 ping-pong consumer waves + 4 producer waves)
}

}  // namespace mhimx

extern "C" int mhimx_bag_project(void* stream, const mhimx_bag_project_args* a) {
  if (!a) return mhimx::fail(-1, "bag_project: null argument block");
  return mhimx::bag_project((hipStream_t)stream, a, 1);
}
extern "C" int mhimx_bag_project_multi(void* stream, const mhimx_bag_project_args* bags, int32_t n_bags) {
  using namespace mhimx;
  MHIMX_CHECK_ARG(bags && n_bags >= 1 && n_bags <= 8, "bag_project_multi: 1..8 bags");
  return bag_project((hipStream_t)stream, bags, n_bags);
}
