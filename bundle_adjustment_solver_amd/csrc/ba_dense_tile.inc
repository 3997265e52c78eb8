// ba_dense_tile.inc — the NB-dependent kernels of ba_dense.hip.  Included once
// per supported tile order inside a namespace that defines `constexpr int NB`
// (32 or 64); everything here is generic in NB.
constexpr int NP = NB / 16;                    // 16-column panels per tile
constexpr int WS = NB * NB + NP * 256;         // workspace doubles per diagonal tile
static_assert(NB == 32 || NB == 64, "tile order");

// Cholesky of the NB x NB tile held in LDS (Lb[c*LS + r], lower triangle) by
// left-looking 16-column panels; leaves L in Lb and the tile inverses
// E_pp = L_pp^-T in Eb.  All 256 threads of the workgroup call it.
constexpr int LS = NB + 1;
constexpr int ES = 17;
__device__ __forceinline__ void factor_tile_lds(double *Lb, double (*Eb)[16 * ES], int tid,
                                                int *bad) {
  const int lane = tid & 63, wv = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    // (1) left-looking update of panel p: tile (ti,p) -= sum_kt L(ti,kt) L(p,kt)^T
    if (p > 0) {
      const int ti = p + wv;
      if (ti < NP) {
        v4f64 acc;
#pragma unroll
        for (int g = 0; g < 4; ++g)
          acc[g] = Lb[(16 * p + lk + 4 * g) * LS + 16 * ti + lr];
        for (int kc = 0; kc < 16 * p; kc += 4) {
          const double a = -Lb[(kc + lk) * LS + 16 * p + lr];
          const double b = Lb[(kc + lk) * LS + 16 * ti + lr];
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g)
          Lb[(16 * p + lk + 4 * g) * LS + 16 * ti + lr] = acc[g];
      }
      __syncthreads();
    }
    // (2) factor the diagonal tile (wave 0)
    if (wv == 0) {
      const int r = lr, q = lk;
      double g[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = 4 * j + q;
        g[j] = (r >= c) ? Lb[(16 * p + c) * LS + 16 * p + r] : 0.0;
      }
      double dinv;
      count_bad_pivots(bad, tile16::tile16_potrf_inv2(g, lane, dinv), lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = 4 * j + q;
        if (r >= c) Lb[(16 * p + c) * LS + 16 * p + r] = g[j];
        if (r < c) Eb[p][r * ES + c] = g[j];
        if (r == c) Eb[p][r * ES + c] = dinv;
      }
    }
    __syncthreads();
    // (3) TRSM of the tiles below: X = T * E_pp   (waves 1..3)
    if (p < NP - 1) {
      const int ti = p + wv;
      if (wv >= 1 && ti < NP) {
        v4f64 acc = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const double a = Eb[p][(lk + 4 * g) * ES + lr];
          const double b = Lb[(16 * p + lk + 4 * g) * LS + 16 * ti + lr];
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
        // all reads of this tile precede the writes within the wave
#pragma unroll
        for (int g = 0; g < 4; ++g)
          Lb[(16 * p + lk + 4 * g) * LS + 16 * ti + lr] = acc[g];
      }
      __syncthreads();
    }
  }
}

template <int FLOW>
__device__ __forceinline__ void st_tile(double *p, double v) {
  if (FLOW)
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else
    *p = v;
}
template <int FLOW>
__device__ __forceinline__ double ld_tile(const double *p) {
  return FLOW ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p;
}
// (FLOW 2 — k_chol_dag, every level of the three-kernel path in one dataflow launch: the
//  tile was updated by workgroups of the same launch: wait until the column's counter of
//  finished updates has reached `need`, read it with sc1 loads; the factor and its tile
//  inverses leave with sc1 stores for the TRSM workgroups that wait for this tile's flag)
template <int FLOW>
__device__ __forceinline__ void diag_body(const double *L, int ld, const int p, double *ws_all,
                                          const int *done, int *bad, double *Lb, double (*Eb)[16 * ES],
                                          const int *cnt = nullptr, int need = 0) {
#ifdef BA_DENSE_DBG
  int dd_n = 0;
  const int t0 = p;  // (DD_STAMP: the first tile)
#endif
  DD_STAMP()
  const int k0 = p * NB;
  double *ws = ws_all + (size_t)p * WS;
  const int tid = threadIdx.x;
  const int dn = done ? *done : 0;
  if (FLOW == 2 && need > 0 && !dn) {
    int spins = 0;
    while (__hip_atomic_load(&cnt[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < need) {
      __builtin_amdgcn_s_sleep(1);
      if (++spins > (1 << 22)) {
        if (bad && tid == 0) atomicAdd(bad, ::ba::kFlowTimeout);
        break;
      }
    }
  }
  // the block is requested before the `done` word is examined: one memory
  // latency for both instead of two in a row
  double lv[NB * NB / 256];
#pragma unroll
  for (int k = 0; k < NB * NB / 256; ++k) {
    const int e = tid + 256 * k;
    const int c = e / NB, r = e % NB;
    lv[k] = (r >= c) ? ld_tile<(FLOW == 2)>(&L[(size_t)(k0 + c) * ld + k0 + r]) : 0.0;
  }
  if (dn) return;
#pragma unroll
  for (int k = 0; k < NB * NB / 256; ++k) {
    const int e = tid + 256 * k;
    Lb[(e / NB) * LS + e % NB] = lv[k];
  }
  for (int e = tid; e < NP * 16 * ES; e += 256) (&Eb[0][0])[e] = 0.0;
  __syncthreads();
  DD_STAMP()
  factor_tile_lds(Lb, Eb, tid, bad);
  DD_STAMP()
  for (int e = tid; e < NB * NB; e += 256) {
    const int c = e / NB, r = e % NB;
    st_tile<(FLOW == 2)>(&ws[e], (r >= c) ? Lb[c * LS + r] : 0.0);
  }
  for (int e = tid; e < NP * 256; e += 256) {
    const int pp = e >> 8, k = (e >> 4) & 15, c = e & 15;
    st_tile<(FLOW == 2)>(&ws[NB * NB + e], Eb[pp][k * ES + c]);
  }
  DD_STAMP()
}

__global__ __launch_bounds__(256) void k_chol_diag(const double *L, int ld,
                                                   int t0, double *ws_all,
                                                   const int *done, int *bad) {
  // one workgroup per diagonal tile of the level (independent tiles)
  __shared__ double Lb[NB * LS];      // Lb[c*LS + r]
  __shared__ double Eb[NP][16 * ES];  // Eb[p][k*ES + c] = E_pp[k][c]
  diag_body<0>(L, ld, t0 + blockIdx.x, ws_all, done, bad, Lb, Eb);
}


// ---- steps 1+2 in one launch: diagonal factorisation, then the TRSM of the
// tile's own row tiles by the same workgroup (wave group wv / NP: row tile,
// wave wv % NP: 16 of its rows).  The row tiles belong to this column only, so
// nothing is shared with another workgroup; their values are requested
// together with the diagonal tile, before the factorisation starts, and are
// waiting in registers when it ends.  Saves one dependent launch per level.
constexpr int RGD = 4 / NP;   // row tiles per pass of the four waves
constexpr int PPRE = 4;       // passes whose operands are prefetched
// (FLOW: the row tiles this workgroup solves are read by update workgroups of the SAME
//  launch — k_chol_level_flow —: they leave with sc1 stores, like x in k_chol_back_flow)
template <int FLOW>
__device__ __forceinline__ void diag_trsm_body(double *L, int ld, int npad, const int p,
                                               const int *__restrict__ row_desc,
                                               const int *__restrict__ rows,
                                               double *ws_all, const int *done,
                                               int *bad, double *Lb, double (*Eb)[16 * ES]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int k0 = p * NB;
  const int4 *dq = (const int4 *)(row_desc + 16 * (size_t)p);
  const int4 d0 = dq[0];              // nrow, row_begin
  const int4 d2 = dq[2], d3 = dq[3];  // first eight row tiles
  const int dn = done ? *done : 0;
  const int nrow = d0.x;
  double lv[NB * NB / 256];
#pragma unroll
  for (int k = 0; k < NB * NB / 256; ++k) {
    const int e = tid + 256 * k;
    const int c = e / NB, r = e % NB;
    lv[k] = (r >= c) ? L[(size_t)(k0 + c) * ld + k0 + r] : 0.0;
  }
  // this wave's rows of the first PPRE passes
  const int w = wv % NP, grp = wv / NP;
  v4f64 A0[PPRE][NP];
  int r0s[PPRE];
#pragma unroll
  for (int ps = 0; ps < PPRE; ++ps) {
    const int a = ps * RGD + grp;
    const int I = a >= nrow ? -1
                : a == 0 ? d2.x : a == 1 ? d2.y : a == 2 ? d2.z : a == 3 ? d2.w
                : a == 4 ? d3.x : a == 5 ? d3.y : a == 6 ? d3.z : a == 7 ? d3.w
                : rows[d0.y + a];
    const int r0 = I * NB + 16 * w;
    r0s[ps] = (I >= 0 && r0 < npad + 16) ? r0 : -1;
#pragma unroll
    for (int pp = 0; pp < NP; ++pp)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        A0[ps][pp][g] = r0s[ps] >= 0 ? L[(size_t)(k0 + 16 * pp + lk + 4 * g) * ld + r0s[ps] + lr] : 0.0;
  }
  if (dn) return;
#pragma unroll
  for (int k = 0; k < NB * NB / 256; ++k) {
    const int e = tid + 256 * k;
    Lb[(e / NB) * LS + e % NB] = lv[k];
  }
  for (int e = tid; e < NP * 16 * ES; e += 256) (&Eb[0][0])[e] = 0.0;
  __syncthreads();
  factor_tile_lds(Lb, Eb, tid, bad);
  {
    double *ws = ws_all + (size_t)p * WS;
    for (int e = tid; e < NB * NB; e += 256) {
      const int c = e / NB, r = e % NB;
      ws[e] = (r >= c) ? Lb[c * LS + r] : 0.0;
    }
    for (int e = tid; e < NP * 256; e += 256) {
      const int pp = e >> 8, k = (e >> 4) & 15, c = e & 15;
      ws[NB * NB + e] = Eb[pp][k * ES + c];
    }
  }
  // TRSM passes: X_pp = (A_pp - sum_{kq<pp} X_kq L(pp,kq)^T) E_pp, operands from LDS
  const int npass = (nrow + RGD - 1) / RGD;
  for (int ps = 0; ps < npass; ++ps) {
    v4f64 Ain[NP];
    int r0;
    if (ps < PPRE) {
      r0 = ps == 0 ? r0s[0] : ps == 1 ? r0s[1 < PPRE ? 1 : 0] : ps == 2 ? r0s[2 < PPRE ? 2 : 0] : r0s[3 < PPRE ? 3 : 0];
#pragma unroll
      for (int pp = 0; pp < NP; ++pp)
        Ain[pp] = ps == 0 ? A0[0][pp] : ps == 1 ? A0[1 < PPRE ? 1 : 0][pp]
                : ps == 2 ? A0[2 < PPRE ? 2 : 0][pp] : A0[3 < PPRE ? 3 : 0][pp];
    } else {
      const int a = ps * RGD + grp;
      const int I = a < nrow ? rows[d0.y + a] : -1;
      r0 = I * NB + 16 * w;
      if (I < 0 || r0 >= npad + 16) r0 = -1;
#pragma unroll
      for (int pp = 0; pp < NP; ++pp)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          Ain[pp][g] = r0 >= 0 ? L[(size_t)(k0 + 16 * pp + lk + 4 * g) * ld + r0 + lr] : 0.0;
    }
    if (r0 < 0) continue;  // wave-uniform
    v4f64 X[NP];
#pragma unroll
    for (int pp = 0; pp < NP; ++pp) {
      v4f64 acc = Ain[pp];
#pragma unroll
      for (int kq = 0; kq < pp; ++kq)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const double lo = -Lb[(16 * kq + lk + 4 * g) * LS + 16 * pp + lr];
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(lo, X[kq][g], acc, 0, 0, 0);
        }
      v4f64 out = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const double eo = Eb[pp][(lk + 4 * g) * ES + lr];
        out = __builtin_amdgcn_mfma_f64_16x16x4f64(eo, acc[g], out, 0, 0, 0);
      }
      X[pp] = out;
#pragma unroll
      for (int g = 0; g < 4; ++g)
        st_tile<FLOW>(&L[(size_t)(k0 + 16 * pp + lk + 4 * g) * ld + r0 + lr], out[g]);
    }
  }
}

__global__ __launch_bounds__(256, NB == 32 ? 2 : 1) void k_chol_diag_trsm(double *L, int ld, int npad, int t0,
                                                        const int *__restrict__ row_desc,
                                                        const int *__restrict__ rows,
                                                        double *ws_all, const int *done,
                                                        int *bad) {
  __shared__ double Lb[NB * LS];
  __shared__ double Eb[NP][16 * ES];
  diag_trsm_body<0>(L, ld, npad, t0 + blockIdx.x, row_desc, rows, ws_all, done, bad, Lb, Eb);
}

// ---- step 2: TRSM of the rows below the diagonal block --------------------
// X = A21 * L11^-T by block forward substitution over the four 16-column
// panels, entirely on the matrix cores: one wave per 16 rows,
//   X_p = (A_p - sum_{k<p} X_k L_pk^T) * E_pp.
// Orientation D[m = column][n = row]: an accumulator register is 16
// consecutive rows of one column (128 contiguous bytes), and — because the
// f64 C/D map is row = (lane>>4) + 4*reg — the accumulator of one product is
// already the B operand of the next (k-step g <-> k = (lane>>4) + 4g).
// (FLOW 2 — k_chol_dag: the item waits for its diagonal tile's flag, reads the row tile —
//  updated by workgroups of the same launch; the column's updates are complete, the
//  diagonal tile waited for them — and the factor with sc1 loads and stores X with sc1
//  stores.  Called by all threads of the workgroup; waves beyond NP have no rows.)
template <int FLOW>
__device__ __forceinline__ void trsm_body(double *L, int ld, int row_limit, const int t, const int I,
                                          const double *__restrict__ ws_all, const int *done,
                                          const int *dflags = nullptr, int gen = 0, int *bad = nullptr) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int k0 = t * NB;
  const int r0 = I * NB + 16 * wv;
  const int dn = done ? *done : 0;
  if (FLOW == 2) {
    if (threadIdx.x == 0 && !dn) {
      int spins = 0;
      while (__hip_atomic_load(&dflags[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != gen) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > (1 << 22)) {
          if (bad) atomicAdd(bad, ::ba::kFlowTimeout);
          break;
        }
      }
    }
    __syncthreads();
  }
  if (wv >= NP || r0 >= row_limit) return;
  const double *ws = ws_all + (size_t)t * WS;
  const double *Ld = ws;
  const double *Et = ws + NB * NB;
  // every operand is requested up front (addresses depend only on the item),
  // then the `done` word is examined: one memory latency for the whole kernel
  v4f64 A0[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      A0[p][g] = ld_tile<(FLOW == 2)>(&L[(size_t)(k0 + 16 * p + lk + 4 * g) * ld + r0 + lr]);
  double ld_op[NP * (NP - 1) / 2][4], et_op[NP][4];
  {
    int q = 0;
#pragma unroll
    for (int p = 1; p < NP; ++p)
#pragma unroll
      for (int kq = 0; kq < p; ++kq) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
          ld_op[q][g] = -ld_tile<(FLOW == 2)>(&Ld[(16 * kq + lk + 4 * g) * NB + 16 * p + lr]);
        ++q;
      }
  }
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int g = 0; g < 4; ++g) et_op[p][g] = ld_tile<(FLOW == 2)>(&Et[p * 256 + (lk + 4 * g) * 16 + lr]);
  if (dn) return;
  v4f64 X[NP];
  int q = 0;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    v4f64 acc = A0[p];
#pragma unroll
    for (int kq = 0; kq < p; ++kq) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ld_op[q][g], X[kq][g], acc, 0, 0, 0);
      ++q;
    }
    v4f64 out = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int g = 0; g < 4; ++g)
      out = __builtin_amdgcn_mfma_f64_16x16x4f64(et_op[p][g], acc[g], out, 0, 0, 0);
    X[p] = out;
#pragma unroll
    for (int g = 0; g < 4; ++g)
      st_tile<(FLOW == 2)>(&L[(size_t)(k0 + 16 * p + lk + 4 * g) * ld + r0 + lr], out[g]);
  }
}

__global__ __launch_bounds__(NP * 64) void k_chol_trsm(double *L, int ld,
                                                   int row_limit, int it0,
                                                   const int *__restrict__ item_t,
                                                   const int *__restrict__ item_I,
                                                   const double *__restrict__ ws_all,
                                                   const int *done) {
  // one workgroup per structurally non-zero NB-row tile (t, I) of the level
  trsm_body<0>(L, ld, row_limit, item_t[it0 + blockIdx.x], item_I[it0 + blockIdx.x], ws_all, done);
}

// ---- step 3: trailing update on the fp64 matrix cores ---------------------
// TARGET-centric: one workgroup per 64x64 tile (I,J) touched in this level;
// it sums the contributions P_I P_J^T of every source panel of the level that
// reaches it (ascending position: deterministic) and applies them with ONE
// read-modify-write.  4 waves of 32x32 (2x2 MFMA 16x16x4 tiles).
// MFMA orientation: the MFMA "row" index runs over C's COLUMN j and the MFMA
// "column" index (lane&15) over C's ROW i, so that each accumulator register
// is 16 consecutive rows of one column = 128 contiguous bytes in memory.
constexpr int MT = NB / 32;  // 16x16 MFMA tiles per wave and dimension
// (FLOW: the source panels come from diag / TRSM workgroups of the same launch: the
//  workgroup requests its target tile, then waits for the flags of its sources — bounded
//  polls, like k_chol_back_flow — and reads the panels with sc1 loads)
// (FLOW 2, all levels in one launch: the target tile itself may still be waiting for an
//  update of an EARLIER level: the workgroup also waits until the counter of finished
//  updates of the target's column has reached `pre` — the updates of earlier levels on that
//  column —, reads the target with sc1 loads after the waits, stores it with sc1 stores and
//  raises the counter)
// (FLOW 3, k_chol_look: sources and target are complete — earlier launches —, nothing to
//  wait for; the target leaves with sc1 stores and raises its column's counter for the
//  tile workgroups of the same launch)
template <int FLOW>
__device__ __forceinline__ void update_body(double *L, int ld, const int tg,
                                            const int *__restrict__ tgt_desc,
                                            const int *__restrict__ src_t,
                                            const int *done, const int *flags, int gen, int *bad,
                                            int *cnt = nullptr, int pre = 0) {
  // inline record: I, J, nsrc, src_begin | first four sources
  const int4 d0 = ((const int4 *)tgt_desc)[2 * tg];
  const int4 d1 = ((const int4 *)tgt_desc)[2 * tg + 1];
  const int dn = done ? *done : 0;
  if (dn) return;
  const int I = d0.x, J = d0.y, nsrc = d0.z;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wi = wv & 1, wj = wv >> 1;
  // four waves, each a (NB/2) x (NB/2) quadrant of the target tile
  const int i0 = I * NB + (NB / 2) * wi, j0 = J * NB + (NB / 2) * wj;
  const int lr = lane & 15, lk = lane >> 4;
  // the target tile is requested together with the first source panel (FLOW 2: after the waits)
  v4f64 tv[MT][MT];
  if (FLOW != 2) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int n = 0; n < MT; ++n)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          tv[m][n][g] = L[(size_t)(j0 + 16 * m + lk + 4 * g) * ld + i0 + 16 * n + lr];
  }
  v4f64 acc[MT][MT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < MT; ++n) acc[m][n] = (v4f64){0.0, 0.0, 0.0, 0.0};
  if (FLOW == 1 || FLOW == 2) {
    for (int k = threadIdx.x; k < nsrc; k += 256) {
      const int st = k == 0 ? d1.x : k == 1 ? d1.y : k == 2 ? d1.z : k == 3 ? d1.w : src_t[d0.w + k];
      int spins = 0;
      while (__hip_atomic_load(&flags[st], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != gen) {
        __builtin_amdgcn_s_sleep(2);
        if (++spins > (1 << 22)) {  // ~ a second: give up, flag the solve as failed
          if (bad) atomicAdd(bad, ::ba::kFlowTimeout);
          break;
        }
      }
    }
    if (FLOW == 2 && pre > 0 && threadIdx.x == 255) {
      int spins = 0;
      while (__hip_atomic_load(&cnt[J], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < pre) {
        __builtin_amdgcn_s_sleep(2);
        if (++spins > (1 << 22)) {
          if (bad) atomicAdd(bad, ::ba::kFlowTimeout);
          break;
        }
      }
    }
    __syncthreads();
    if (FLOW == 2) {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < MT; ++n)
#pragma unroll
          for (int g = 0; g < 4; ++g)
            tv[m][n][g] = ld_tile<1>(&L[(size_t)(j0 + 16 * m + lk + 4 * g) * ld + i0 + 16 * n + lr]);
    }
  }
  for (int k = 0; k < nsrc; ++k) {
    const int st = k == 0 ? d1.x : k == 1 ? d1.y : k == 2 ? d1.z : k == 3 ? d1.w : src_t[d0.w + k];
    const double *P = L + (size_t)st * NB * ld;
#pragma unroll 4
    for (int kk = 0; kk < NB / 4; ++kk) {
      const double *col = P + (size_t)(kk * 4 + lk) * ld;
      double av[MT], bv[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        av[m] = ld_tile<(FLOW == 1 || FLOW == 2)>(&col[j0 + 16 * m + lr]);
        bv[m] = ld_tile<(FLOW == 1 || FLOW == 2)>(&col[i0 + 16 * m + lr]);
      }
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < MT; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[m], bv[n], acc[m][n], 0, 0, 0);
    }
  }
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < MT; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int j = j0 + 16 * m + lk + 4 * g;
        const int i = i0 + 16 * n + lr;
        st_tile<(FLOW >= 2)>(&L[(size_t)j * ld + i], tv[m][n][g] - acc[m][n][g]);
      }
  if (FLOW >= 2) {  // publish: the target's stores drained, then the column's counter
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(&cnt[J], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(256) void k_chol_update(double *L, int ld, int tg0,
                                                     const int *__restrict__ tgt_desc,
                                                     const int *__restrict__ src_t,
                                                     const int *done) {
  update_body<0>(L, ld, tg0 + blockIdx.x, tgt_desc, src_t, done, nullptr, 0, nullptr);
}

// ---- one launch per level: factorisation + TRSM workgroups AND the update workgroups
// that consume their row tiles, as a dataflow.  A workgroup takes its role from a ticket
// (the first nt tickets are the level's tiles, which wait for nothing; the others are
// update targets, which only wait for tiles, i.e. for earlier tickets: no deadlock
// whatever the dispatch order); a tile raises its flag (= the generation number of this
// solve) after its row tiles have left with sc1 stores and drained.  Saves the launch
// boundary between k_chol_diag_trsm and k_chol_update and lets an update workgroup fetch
// its target tile while the factorisation it depends on is still running.
__global__ __launch_bounds__(256, NB == 32 ? 2 : 1) void k_chol_level_flow(double *L, int ld, int npad, int t0, int nt,
                                                         int tg0, int ng,
                                                         const int *__restrict__ row_desc,
                                                         const int *__restrict__ rows,
                                                         double *ws_all,
                                                         const int *__restrict__ tgt_desc,
                                                         const int *__restrict__ src_t,
                                                         const int *done, int *bad, int *flags,
                                                         int *ticket, int gen) {
  __shared__ double Lb[NB * LS];
  __shared__ double Eb[NP][16 * ES];
  __shared__ int s_k;
  // ticket == nullptr: the whole grid is resident at once (the host checked: at most
  // kFlowResident workgroups), every workgroup runs whatever the dispatch order and the
  // role is the block index — one global atomic round trip (~1 us) less on every level's
  // critical path.  Larger grids take tickets.
  int k = blockIdx.x;
  if (ticket) {
    if (threadIdx.x == 0) {
      const int kt = atomicAdd(ticket, 1);
      if (kt == nt + ng - 1) *ticket = 0;  // every ticket of this launch is taken
      s_k = kt;
    }
    __syncthreads();
    k = s_k;
  }
  if (k < nt) {
    diag_trsm_body<1>(L, ld, npad, t0 + k, row_desc, rows, ws_all, done, bad, Lb, Eb);
    // publish: every wave's (write-through) stores drained, then the flag
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0 && !(done && *done))
      __hip_atomic_store(&flags[t0 + k], gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    update_body<1>(L, ld, tg0 + (k - nt), tgt_desc, src_t, done, flags, gen, bad);
  }
}

// ---- the forward sweep of the THREE-KERNEL path (dense patterns: many row tiles per
// column) as one dataflow launch over all levels, with lookahead ----
// Items {kind, index}: 0 = diagonal tile (position), 1 = TRSM item, 2 = update target, in
// the order  D_0 T_0 | U_0' D_1 T_1 U_0'' | U_1' D_2 T_2 U_1'' | ...  where U_l' are the
// targets of level l in a column of level l + 1 (sorted first by the schedule): the next
// level's tiles and row tiles take their tickets BEFORE the bulk of level l's update and
// run beside it.  Every wait is for an earlier item: a tile for its column's counter of
// finished updates (need), a TRSM item for its tile's flag, an update for the "row tiles
// solved" flags of its source columns — raised by the LAST TRSM item of a column (its
// counter of finished items; tiles without row tiles raise it themselves) — and for the
// earlier levels' updates on its target's column (pre).  sc1 stores / loads for
// everything handed over, bounded polls, tickets.  Bit-identical to the three launches
// per level (BA_DENSE_DAG=0): same arithmetic in the same order.
__global__ __launch_bounds__(256) void k_chol_dag(double *L, int ld, int row_limit,
                                                  const int2 *__restrict__ items, int n_items,
                                                  const int *__restrict__ item_t,
                                                  const int *__restrict__ item_I,
                                                  const int *__restrict__ n_trsm, double *ws_all,
                                                  const int *__restrict__ tgt_desc,
                                                  const int *__restrict__ src_t,
                                                  const int *__restrict__ upd_pre,
                                                  const int *__restrict__ col_need,
                                                  const int *done, int *bad, int *flags, int *dflags,
                                                  int *tcnt, int *cnt, int *ticket, int gen) {
  __shared__ double Lb[NB * LS];
  __shared__ double Eb[NP][16 * ES];
  __shared__ int s_k;
  if (threadIdx.x == 0) {
    const int kt = atomicAdd(ticket, 1);
    if (kt == n_items - 1) *ticket = 0;
    s_k = kt;
  }
  __syncthreads();
  const int2 it = items[s_k];
  const int dn = done ? *done : 0;
  if (it.x == 0) {
    const int p = it.y;
    diag_body<2>(L, ld, p, ws_all, done, bad, Lb, Eb, cnt, col_need[p]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0 && !dn) {
      __hip_atomic_store(&dflags[p], gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (n_trsm[p] == 0) __hip_atomic_store(&flags[p], gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  } else if (it.x == 1) {
    const int t = item_t[it.y];
    trsm_body<2>(L, ld, row_limit, t, item_I[it.y], ws_all, done, dflags, gen, bad);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0 && !dn) {
      const int c = __hip_atomic_fetch_add(&tcnt[t], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (c == n_trsm[t] - 1) {  // the column's last row tile: reset the counter, raise the flag
        __hip_atomic_store(&tcnt[t], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&flags[t], gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  } else {
    update_body<2>(L, ld, it.y, tgt_desc, src_t, done, flags, gen, bad, cnt, upd_pre[it.y]);
  }
}

// ---- dense patterns (more items than k_chol_dag takes): LOOKAHEAD inside one launch ----
// ONE launch per level l.  Roles from the block index, in this order:
//   [0, nf)           the targets of level l in a column of level l + 1 (the schedule sorts
//                     them first): plain updates — level l's row tiles are complete, the
//                     previous launch solved them — that raise their column's counter;
//   [nf, nf + nt1)    the tiles of level l + 1: wait until their column's counter has reached
//                     the number of those targets (need), factorise, raise their flag;
//   [.., + ni1)       the TRSM items of level l + 1: wait for their tile's flag;
//   the rest          the bulk of level l's update: plain workgroups, no ticket, no poll.
// The factorisation + TRSM of the next column (26 of a level's 59 us at n = 5 970) run
// BESIDE the update instead of in front of it, and a level is one launch instead of three.
// A workgroup only waits for blocks with a smaller index (dispatched earlier).
__global__ __launch_bounds__(256, 3) void k_chol_look(double *L, int ld, int row_limit, int nf, int t1,
                                                      int nt1, int it1, int ni1, int tg0,
                                                      const int *__restrict__ item_t,
                                                      const int *__restrict__ item_I, double *ws_all,
                                                      const int *__restrict__ tgt_desc,
                                                      const int *__restrict__ src_t,
                                                      const int *__restrict__ look_need,
                                                      const int *done, int *bad, int *dflags, int *cnt,
                                                      int gen) {
  __shared__ double Lb[NB * LS];
  __shared__ double Eb[NP][16 * ES];
  const int k = blockIdx.x;
  if (k < nf) {
    update_body<3>(L, ld, tg0 + k, tgt_desc, src_t, done, nullptr, 0, bad, cnt, 0);
  } else if (k < nf + nt1) {
    const int p = t1 + (k - nf);
    diag_body<2>(L, ld, p, ws_all, done, bad, Lb, Eb, cnt, look_need[p]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0 && !(done && *done))
      __hip_atomic_store(&dflags[p], gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else if (k < nf + nt1 + ni1) {
    const int q = it1 + (k - nf - nt1);
    trsm_body<2>(L, ld, row_limit, item_t[q], item_I[q], ws_all, done, dflags, gen, bad);
  } else {
    update_body<0>(L, ld, tg0 + (k - nt1 - ni1), tgt_desc, src_t, done, nullptr, 0, nullptr);
  }
}

// ---- backward sweep L^T x = z, one launch per level (reverse order) --------
// Left-looking: the workgroup of tile t gathers  w = z_t - sum_I L(I,t)^T x_I
// over the non-zero row tiles I below t (all solved in earlier launches), then
// wave 0 solves the 64x64 diagonal system by block back substitution with the
// tile inverses:  x_p = E_pp (w_p - sum_{u>p} L_up^T x_u),  p = 3..0.
constexpr int BG = 256 / NB;  // row groups of the gather (each NB/BG rows)
constexpr int BR = NB / BG;
__global__ __launch_bounds__(256) void k_chol_back(const double *L, int ld,
                                                   int npad, int t0,
                                                   const int *__restrict__ back_desc,
                                                   const int *__restrict__ rows,
                                                   const double *__restrict__ ws_all,
                                                   double *xc, double *x,
                                                   const int *__restrict__ col_x,
                                                   const int *done) {
  __shared__ double xs[NB];
  __shared__ double part[BG][NB];
  const int tid = threadIdx.x;
  const int t = t0 + blockIdx.x;
  const int k0 = t * NB;
  // inline record: nrow, row_begin | first six row tiles
  const int4 d0 = ((const int4 *)back_desc)[2 * t];
  const int4 d1 = ((const int4 *)back_desc)[2 * t + 1];
  const int dn = done ? *done : 0;
  const double *Ld = ws_all + (size_t)t * WS;
  const double *Et = Ld + NB * NB;
  // wave 0 needs, much later, operands whose addresses depend on nothing but t:
  // they are requested now so that their latency hides behind the gather
  const int i = tid & 15, q = (tid >> 4) & 3;
  double lop[NP][NP][4];  // [p][u][rr], u > p
  double eop[NP][4], zv[NP];
  int xidx = -1;
  if (tid < 64) {
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int u = p + 1; u < NP; ++u)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          lop[p][u][rr] = Ld[(16 * p + i) * NB + 16 * u + 4 * q + rr];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) eop[p][cc] = Et[p * 256 + i * 16 + 4 * q + cc];
      zv[p] = L[(size_t)(k0 + 16 * p + i) * ld + npad];
    }
    if (tid < NB) xidx = col_x[k0 + tid];
  }
  if (dn) return;
  {
    // gather  below[c] = sum_I sum_r L(I*NB + r, k0 + c) x(I*NB + r):  lane = ROW r of
    // the row tile (a wave instruction reads 64 consecutive rows of one column:
    // contiguous), thread group cg = its share of BR columns; the row sums are
    // folded across the lanes once, after the last tile.  The tile index of the
    // next iteration is requested one iteration ahead (dense patterns have up to
    // ncb row tiles per column: a dependent index load per iteration was the
    // whole cost of the sweep there).
    const int r = tid % NB, cg = tid / NB;
    const int nrow = d0.x;
    double s[BR];
#pragma unroll
    for (int u = 0; u < BR; ++u) s[u] = 0.0;
    auto tile_of = [&](int a) {
      return a == 0 ? d0.z : a == 1 ? d0.w : a == 2 ? d1.x : a == 3 ? d1.y
           : a == 4 ? d1.z : a == 5 ? d1.w : rows[d0.y + (a < nrow ? a : nrow - 1)];
    };
    int I = nrow > 0 ? tile_of(0) : 0;
    for (int a = 0; a < nrow; ++a) {
      const int In = tile_of(a + 1 < nrow ? a + 1 : a);
      const double *src = L + (size_t)(k0 + BR * cg) * ld + I * NB + r;
      const double xv = xc[I * NB + r];
      double lv[BR];
#pragma unroll
      for (int u = 0; u < BR; ++u) lv[u] = src[(size_t)u * ld];
#pragma unroll
      for (int u = 0; u < BR; ++u) s[u] = fma(lv[u], xv, s[u]);
      I = In;
    }
    // fold the NB row lanes of a group (xor butterfly: fixed order), lane r == 0 keeps the sum
#pragma unroll
    for (int u = 0; u < BR; ++u) {
      double v = s[u];
#pragma unroll
      for (int off = NB / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
      if (r == 0) part[0][BR * cg + u] = v;
    }
  }
  __syncthreads();
  if (tid < 64) {
#pragma unroll
    for (int p = NP - 1; p >= 0; --p) {
      double acc = 0.0;
#pragma unroll
      for (int u = p + 1; u < NP; ++u)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int row = 16 * u + 4 * q + rr;
          acc += lop[p][u][rr] * xs[row];
        }
      acc += __shfl_xor(acc, 16, 64);
      acc += __shfl_xor(acc, 32, 64);
      const int c = 16 * p + i;
      const double below = part[0][c];
      const double wv = (zv[p] - below) - acc;
      double px = 0.0;
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        const int c2 = 4 * q + cc;
        px += eop[p][cc] * __shfl(wv, c2, 64);
      }
      px += __shfl_xor(px, 16, 64);
      px += __shfl_xor(px, 32, 64);
      if (q == 0) xs[16 * p + i] = px;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (tid < NB) {
      xc[k0 + tid] = xs[tid];
      if (xidx >= 0) x[xidx] = xs[tid];
    }
  }
}

// ---- backward sweep as ONE launch: dataflow over the tiles ------------------
// The per-level launches above cost a launch boundary plus two memory round trips
// each (4.8 us per level at C4) for a 32-vector per tile.  Here every non-tail tile
// has its own workgroup in one launch; a workgroup takes its logical position from
// a TICKET counter (positions are ordered top level first, so a workgroup only ever
// waits for workgroups that took an earlier ticket and are therefore running or
// finished: no deadlock whatever the dispatch order), waits for the flags of its row
// tiles (relaxed polls with s_sleep, BOUNDED: a poll limit sets the error word
// and lets the workgroup finish), acquires, runs the same gather + block back
// substitution as k_chol_back, publishes x, releases and raises its own flag
// (= the generation number of this solve: flags are never reset).
// The hand-off below is NOT expressed in the memory model (that costs a cache
// write-back / invalidate per hop): it relies on gfx9-family behaviour — agent-scope
// relaxed atomics compile to sc1 accesses that bypass the non-coherent cache levels,
// and `s_waitcnt vmcnt(0)` also drains the wave's stores.  Other targets must take the
// per-level launches (BA_DENSE_FLOW=0); tests/test_abi.py checks the sc1 bits in the
// generated code.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__) && !defined(__gfx90a__)
#error "k_chol_back_flow relies on gfx9-family cache behaviour (sc1 hand-offs): build for gfx950"
#endif
// ORDERED (dense patterns: up to ncb row tiles per column): the row tiles are consumed ONE
// BY ONE in descending position, each as soon as its flag is up, so that only the LAST
// tile's 32 KB — not the whole 3 MB panel — sits between the hand-off and the tile solve;
// the factor tile of a step is requested before its flag is polled.
template <bool ORDERED>
__global__ __launch_bounds__(256) void k_chol_back_flow(const double *L, int ld, int npad,
                                                        const int *__restrict__ order, int n_order,
                                                        int tail_t0,
                                                        const int *__restrict__ back_desc,
                                                        const int *__restrict__ rows,
                                                        const double *__restrict__ ws_all,
                                                        double *xc, double *x,
                                                        const int *__restrict__ col_x,
                                                        const int *done, int *flags, int *ticket,
                                                        int gen, int *bad, int *fwd_cnt, int n_cnt) {
  __shared__ double xs[NB];
  __shared__ double part[BG][NB];
  __shared__ int s_t;
  const int tid = threadIdx.x;
  const int dn = done ? *done : 0;
  // (the forward sweep's column counters, k_chol_dag / k_chol_look: zero again for the next solve;
  //  that launch has completed — stream order — and a solve skipped by `done` leaves them zero)
  if (fwd_cnt && blockIdx.x == 0 && !dn)
    for (int e = tid; e < n_cnt; e += 256) fwd_cnt[e] = 0;
  int t;
  if (ticket) {
    if (tid == 0) {
      const int k = atomicAdd(ticket, 1);
      if (k == n_order - 1) *ticket = 0;  // every ticket of this launch is taken
      s_t = order[k];
    }
    __syncthreads();
    t = s_t;
  } else {
    t = order[blockIdx.x];  // (the whole grid is resident: see k_chol_level_flow)
  }
  const int k0 = t * NB;
  const int4 d0 = ((const int4 *)back_desc)[2 * t];
  const int4 d1 = ((const int4 *)back_desc)[2 * t + 1];
  const double *Ld = ws_all + (size_t)t * WS;
  const double *Et = Ld + NB * NB;
  const int i = tid & 15, q = (tid >> 4) & 3;
  double lop[NP][NP][4];
  double eop[NP][4], zv[NP];
  int xidx = -1;
  if (tid < 64) {
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int u = p + 1; u < NP; ++u)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          lop[p][u][rr] = Ld[(16 * p + i) * NB + 16 * u + 4 * q + rr];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) eop[p][cc] = Et[p * 256 + i * 16 + 4 * q + cc];
      zv[p] = L[(size_t)(k0 + 16 * p + i) * ld + npad];
    }
    if (tid < NB) xidx = col_x[k0 + tid];
  }
  const int nrow = d0.x;
  auto tile_of = [&](int a) {
    return a == 0 ? d0.z : a == 1 ? d0.w : a == 2 ? d1.x : a == 3 ? d1.y
         : a == 4 ? d1.z : a == 5 ? d1.w : rows[d0.y + (a < nrow ? a : nrow - 1)];
  };
  if (ORDERED) {
    if (dn) return;
    const int r = tid % NB, cg = tid / NB;
    double s[BR];
#pragma unroll
    for (int u = 0; u < BR; ++u) s[u] = 0.0;
    int I = nrow > 0 ? tile_of(nrow - 1) : 0;
    for (int a = nrow - 1; a >= 0; --a) {
      const int In = tile_of(a > 0 ? a - 1 : 0);  // (index of the next step one step ahead)
      const double *src = L + (size_t)(k0 + BR * cg) * ld + I * NB + r;
      double lv[BR];
#pragma unroll
      for (int u = 0; u < BR; ++u) lv[u] = src[(size_t)u * ld];
      if (I < tail_t0) {
        int spins = 0;
        while (__hip_atomic_load(&flags[I], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != gen) {
          __builtin_amdgcn_s_sleep(1);
          if (++spins > (1 << 22)) {
            if (bad && tid == 0) atomicAdd(bad, ::ba::kFlowTimeout);
            break;
          }
        }
      }
      const double xv = __hip_atomic_load(&xc[I * NB + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int u = 0; u < BR; ++u) s[u] = fma(lv[u], xv, s[u]);
      I = In;
    }
#pragma unroll
    for (int u = 0; u < BR; ++u) {
      double v = s[u];
#pragma unroll
      for (int off = NB / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
      if (r == 0) part[0][BR * cg + u] = v;
    }
    __syncthreads();
  }
  // the factor tiles of the first four row tiles do not depend on x: requested before the wait
  constexpr int PF = 4;
  double lpre[PF][BR];
  if (!ORDERED) {
    const int r = tid % NB, cg = tid / NB;
#pragma unroll
    for (int a = 0; a < PF; ++a) {
      const int I = tile_of(a < nrow ? a : (nrow > 0 ? nrow - 1 : 0));
      const double *src = L + (size_t)(k0 + BR * cg) * ld + (nrow > 0 ? I : t) * NB + r;
#pragma unroll
      for (int u = 0; u < BR; ++u) lpre[a][u] = src[(size_t)u * ld];
    }
  }
  if (!ORDERED && !dn) {
    // wait for the row tiles (tiles of the tail block were solved by k_chol_tail, a launch ago)
    for (int a = tid; a < nrow; a += 256) {
      const int I = tile_of(a);
      if (I < tail_t0) {
        int spins = 0;
        while (__hip_atomic_load(&flags[I], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != gen) {
          __builtin_amdgcn_s_sleep(2);
          if (++spins > (1 << 22)) {  // ~ a second: give up, flag the solve as failed
            if (bad) atomicAdd(bad, ::ba::kFlowTimeout);
            break;
          }
        }
      }
    }
    // (no acquire fence: the handed-off bytes — the 32 entries of x per tile — are written
    //  and read with agent-scope atomics, i.e. sc1 accesses that bypass the non-coherent
    //  cache levels; a fence writes back / invalidates whole caches: 4.8 us per hop)
  }
  __syncthreads();
  if (dn) return;
  if (!ORDERED) {
    const int r = tid % NB, cg = tid / NB;
    double s[BR];
#pragma unroll
    for (int u = 0; u < BR; ++u) s[u] = 0.0;
    {  // the prefetched row tiles: only x is still to come
      double xv[PF];
#pragma unroll
      for (int a = 0; a < PF; ++a) {
        const int I = tile_of(a < nrow ? a : (nrow > 0 ? nrow - 1 : 0));
        xv[a] = __hip_atomic_load(&xc[(nrow > 0 ? I : t) * NB + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int a = 0; a < PF; ++a)
        if (a < nrow) {
#pragma unroll
          for (int u = 0; u < BR; ++u) s[u] = fma(lpre[a][u], xv[a], s[u]);
        }
    }
    int I = nrow > PF ? tile_of(PF) : 0;
    for (int a = PF; a < nrow; ++a) {
      const int In = tile_of(a + 1 < nrow ? a + 1 : a);
      const double *src = L + (size_t)(k0 + BR * cg) * ld + I * NB + r;
      const double xv = __hip_atomic_load(&xc[I * NB + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      double lv[BR];
#pragma unroll
      for (int u = 0; u < BR; ++u) lv[u] = src[(size_t)u * ld];
#pragma unroll
      for (int u = 0; u < BR; ++u) s[u] = fma(lv[u], xv, s[u]);
      I = In;
    }
#pragma unroll
    for (int u = 0; u < BR; ++u) {
      double v = s[u];
#pragma unroll
      for (int off = NB / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
      if (r == 0) part[0][BR * cg + u] = v;
    }
  }
  __syncthreads();
  if (tid < 64) {
#pragma unroll
    for (int p = NP - 1; p >= 0; --p) {
      double acc = 0.0;
#pragma unroll
      for (int u = p + 1; u < NP; ++u)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int row = 16 * u + 4 * q + rr;
          acc += lop[p][u][rr] * xs[row];
        }
      acc += __shfl_xor(acc, 16, 64);
      acc += __shfl_xor(acc, 32, 64);
      const int c = 16 * p + i;
      const double below = part[0][c];
      const double wv = (zv[p] - below) - acc;
      double px = 0.0;
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        const int c2 = 4 * q + cc;
        px += eop[p][cc] * __shfl(wv, c2, 64);
      }
      px += __shfl_xor(px, 16, 64);
      px += __shfl_xor(px, 32, 64);
      if (q == 0) xs[16 * p + i] = px;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (tid < NB) {
      __hip_atomic_store(&xc[k0 + tid], xs[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (xidx >= 0) x[xidx] = xs[tid];
    }
    // publish: this wave's (write-through) stores drained, then the flag
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tid == 0) __hip_atomic_store(&flags[t], gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- backward sweep without hand-offs: one workgroup per LEAF --------------------------
// On narrow patterns the dataflow sweep above is a chain of hops between workgroups (store,
// drain, flag, poll, load: ~3.8 us each at C4) around a few hundred flops.  Here the
// workgroup of a leaf solves its whole CONE itself (ba_dense_sched.h: DenseCone), top
// ancestor first, starting from the x that k_chol_tail left a launch ago: ancestors shared
// by several leaves are solved redundantly, x between steps stays in LDS, and nothing waits
// for another workgroup — no flags, no tickets, no polls, no generation number.  A step is
// the gather and the wave-0 block back substitution of k_chol_back, operation by operation
// (row tiles in list order, the same fma chain, the same butterfly per value, the same panel
// loop): x is bit-identical to the other sweeps.
// Everything a step reads besides x is factor data of earlier launches, written on other
// CUs: a load of it takes ~3 us, three times the arithmetic of a step.  The leaf's records
// go to LDS first; the operands of the first kConeDepth steps are requested before the
// first step, those of step k + kConeDepth as soon as step k has released its registers.
// A request is unconditional (every thread loads the wave-0 operands, the first PF row tiles
// are always loaded: the records repeat the last one; past the last step the last step is
// requested once more): under a branch the compiler waits for ALL loads in flight at the
// next use, i.e. for the request it has just issued.  Exactly one leaf stores a position's x
// (plain stores, after the loop).
// (registers: a step in flight holds 60 VGPRs at order 32 and 120 at order 64; two steps with two row tiles spill at order 64)
constexpr int kConeDepth = NB == 32 ? 4 : 2;  // steps in flight
constexpr int kConePF = NB == 32 ? 4 : 1;     // row tiles of a step that are requested with it
struct ConeOps {
  double lop[NP][NP][4];  // [p][u][rr], u > p
  double eop[NP][4], zv[NP];
  double lpre[kConePF][BR];
};
__global__ __launch_bounds__(256) void k_chol_back_cone(const double *L, int ld, int npad,
                                                        const int *__restrict__ cone_rec, int stride,
                                                        int tail_t0, int n_tail_cols,
                                                        const double *__restrict__ ws_all,
                                                        double *xc, double *x,
                                                        const int *__restrict__ col_x,
                                                        const int *done, int *fwd_cnt, int n_cnt) {
  using ::ba::kConeMaxLen;
  using ::ba::kConeRec;
  using ::ba::kConeSlotShift;
  using ::ba::kConeTailSlots;
  constexpr int PF = kConePF, D = kConeDepth;
  constexpr int kSlotMask = (1 << kConeSlotShift) - 1;
  static_assert(kConeMaxLen * kConeRec <= 256, "one pass of the workgroup fetches a leaf's records");
  __shared__ double xsl[(kConeTailSlots + kConeMaxLen) * NB];  // x per slot: tail tiles, then the steps
  __shared__ double part[NB];
  __shared__ int s_rec[kConeMaxLen * kConeRec];    // the records of this leaf's steps
  const int tid = threadIdx.x;
  const int i = tid & 15, q = (tid >> 4) & 3;      // (wave 0's operand lanes; the other waves load the same)
  const int r = tid % NB, cg = tid / NB;
  const int dn = done ? *done : 0;
  if (tid < stride * kConeRec) s_rec[tid] = cone_rec[(size_t)blockIdx.x * stride * kConeRec + tid];
  if (tid < n_tail_cols) xsl[tid] = xc[tail_t0 * NB + tid];  // x of the tail block (k_chol_tail)
  if (dn) return;
  // (the forward sweep's column counters: zero again for the next solve, as in k_chol_back_flow)
  if (fwd_cnt && blockIdx.x == 0)
    for (int e = tid; e < n_cnt; e += 256) fwd_cnt[e] = 0;
  __syncthreads();
  const int nstep = s_rec[3];
  auto request = [&](ConeOps &o, int k) {
    const int *rk = s_rec + kConeRec * k;
    const int t = rk[0], k0 = t * NB;
    const double *Ld = ws_all + (size_t)t * WS;
    const double *Et = Ld + NB * NB;
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int u = p + 1; u < NP; ++u)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          o.lop[p][u][rr] = Ld[(16 * p + i) * NB + 16 * u + 4 * q + rr];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) o.eop[p][cc] = Et[p * 256 + i * 16 + 4 * q + cc];
      o.zv[p] = L[(size_t)(k0 + 16 * p + i) * ld + npad];
    }
#pragma unroll
    for (int a = 0; a < PF; ++a) {
      const double *src = L + (size_t)(k0 + BR * cg) * ld + (rk[4 + a] & kSlotMask) * NB + r;
#pragma unroll
      for (int u = 0; u < BR; ++u) o.lpre[a][u] = src[(size_t)u * ld];
    }
  };
  // (where the stores after the loop go in x: asked for now, not between the last step and the
  //  stores — at order 32; at order 64 the registers are all taken)
  constexpr int kOut = (kConeMaxLen * NB + 255) / 256;
  constexpr bool kOutAhead = NB == 32;
  int xi[kOut];
#pragma unroll
  for (int j = 0; j < kOut; ++j) {
    const int e = tid + 256 * j, k = e / NB < nstep ? e / NB : nstep - 1;
    xi[j] = kOutAhead ? col_x[s_rec[kConeRec * k] * NB + e % NB] : -1;
  }
  ConeOps ring[D];
#pragma unroll
  for (int d = 0; d < D; ++d) request(ring[d], d < nstep ? d : nstep - 1);
  // (straight-line code, one exit per step: across a loop's back edge the compiler's count of the
  //  loads in flight is a worst case, and every D-th step waited for the request just issued)
  static_assert(kConeMaxLen % D == 0, "whole turns of the ring");
#pragma unroll
  for (int kb = 0; kb < kConeMaxLen; kb += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int k = kb + d;
      if (k >= nstep) break;
      ConeOps &o = ring[d];
      const int *rk = s_rec + kConeRec * k;
      const int t = rk[0], nrow = rk[1], k0 = t * NB;
      double *xs = xsl + (kConeTailSlots + k) * NB;
      {
        double s[BR];
#pragma unroll
        for (int u = 0; u < BR; ++u) s[u] = 0.0;
        double xv[PF];
#pragma unroll
        for (int a = 0; a < PF; ++a) xv[a] = xsl[(rk[4 + a] >> kConeSlotShift) * NB + r];
#pragma unroll
        for (int a = 0; a < PF; ++a)
          if (a < nrow) {
#pragma unroll
            for (int u = 0; u < BR; ++u) s[u] = fma(o.lpre[a][u], xv[a], s[u]);
          }
        for (int a = PF; a < nrow; ++a) {
          const int cd = rk[4 + a];
          const double *src = L + (size_t)(k0 + BR * cg) * ld + (cd & kSlotMask) * NB + r;
          const double xa = xsl[(cd >> kConeSlotShift) * NB + r];
          double lv[BR];
#pragma unroll
          for (int u = 0; u < BR; ++u) lv[u] = src[(size_t)u * ld];
#pragma unroll
          for (int u = 0; u < BR; ++u) s[u] = fma(lv[u], xa, s[u]);
        }
        // fold the NB row lanes of a group (xor butterfly: fixed order per value; the BR values of a
        // thread go through it side by side), lane r == 0 keeps the sums
#pragma unroll
        for (int off = NB / 2; off >= 1; off >>= 1)
#pragma unroll
          for (int u = 0; u < BR; ++u) s[u] += __shfl_xor(s[u], off, 64);
        if (r == 0) {
#pragma unroll
          for (int u = 0; u < BR; ++u) part[BR * cg + u] = s[u];
        }
      }
      __syncthreads();
      if (tid < 64) {
#pragma unroll
        for (int p = NP - 1; p >= 0; --p) {
          double acc = 0.0;
#pragma unroll
          for (int u = p + 1; u < NP; ++u)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
              const int row = 16 * u + 4 * q + rr;
              acc += o.lop[p][u][rr] * xs[row];
            }
          acc += __shfl_xor(acc, 16, 64);
          acc += __shfl_xor(acc, 32, 64);
          const int col = 16 * p + i;
          const double below = part[col];
          const double wv = (o.zv[p] - below) - acc;
          double px = 0.0;
#pragma unroll
          for (int cc = 0; cc < 4; ++cc) {
            const int c2 = 4 * q + cc;
            px += o.eop[p][cc] * __shfl(wv, c2, 64);
          }
          px += __shfl_xor(px, 16, 64);
          px += __shfl_xor(px, 32, 64);
          if (q == 0) xs[16 * p + i] = px;
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
      }
      request(o, k + D < nstep ? k + D : nstep - 1);  // (past the end: the last step's once more, not a branch)
      __syncthreads();
    }
  }
  // the x this leaf is the writer of, in column order and in pose order
#pragma unroll
  for (int j = 0; j < kOut; ++j) {
    const int e = tid + 256 * j, k = e / NB, col = e % NB;
    if (e < nstep * NB && s_rec[kConeRec * k + 2]) {
      const int t = s_rec[kConeRec * k];
      const double v = xsl[(kConeTailSlots + k) * NB + col];
      xc[t * NB + col] = v;
      const int xo = kOutAhead ? xi[j] : col_x[t * NB + col];
      if (xo >= 0) x[xo] = v;
    }
  }
}
