// pw_tn_body.hpp — the BODY of pure_window.hip's C = A^T B kernels, included as text inside each of them (not a function: the fp32 kernels
// pw_tn_kernel<BAGX> have to keep their code, instruction for instruction, and an inlined helper did not give that).  The including kernel
// provides: BAGX (B = the bags' X), XT (MHIMX_X_*: the element type of the bags' rows), tab, A, lda, B, ldb, steps, steps_per, slabs, M, Nc.
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
      int bag = 0;
#pragma unroll
      for (int b = 1; b < MHIMX_INFER_MAX; ++b)
        if (b < tab.n && k0 >= tab.row0[b]) bag = b;
      const float* X = tab.X[0];
      int64_t ldx = tab.ldx[0], N = tab.N[0], orow0 = tab.row0[0];
      IT_PICK(X, X, bag) IT_PICK(ldx, ldx, bag) IT_PICK(N, N, bag) IT_PICK(orow0, row0, bag)
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
  pw_f16 acc[2][2];
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
      pw_b8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int ao = (wm * 64 + i * 32 + r32) * TN_PITCH + 32 * k2 + 16 * kg;
        const int bo = (wn * 64 + i * 32 + r32) * TN_PITCH + 32 * k2 + 16 * kg;
        ah[i] = *reinterpret_cast<const pw_b8*>(lds[0] + ao);
        al[i] = *reinterpret_cast<const pw_b8*>(lds[1] + ao);
        bh[i] = *reinterpret_cast<const pw_b8*>(lds[2] + bo);
        bl[i] = *reinterpret_cast<const pw_b8*>(lds[3] + bo);
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
