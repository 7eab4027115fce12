// Body of gemm_rows_kernel and gemm_rows_gram_kernel (mx_rows_v4.inc includes it into both, so
// that neither kernel's code depends on how the other is built).  In scope: the kernel argument
// `a`, the template parameters MT, NT, EPI, NORM, SUB, F8, PW, NSM, and GRAM.
  constexpr int NP = MX_ROWS_NP, ST = 4;    // activation parts; k-steps per sub-chunk
  constexpr int MQ = NT <= 2 ? 8 : 4;       // K ranges whose partials are loaded per merge round
  constexpr int DX = PW, NBX = DX + 1, NBW = PW + 1;  // prefetch distances, buffers
  constexpr int ITEMS = (NT * 16 * 16) / 512 > 0 ? (NT * 16 * 16) / 512 : 1;  // X pieces/thread
  constexpr int WSLAB = MT * NT * 4 * 64;   // floats per wave partial
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  // Block -> (weight tile bx, K range kc, batch tile bz), K range fastest: blocks are dealt
  // round-robin over the 8 XCDs, so with nkc | 8 every block of one K range lands on the same
  // nkc-th of the XCDs, and that range's activation slice is fetched into fewer L2s (with
  // x fastest every XCD fetched every slice: the activation part of FETCH_SIZE in
  // profiles/r03_pmc_rows32.json)
  const int nkc = gridDim.y;
  const int lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  const int kc = lin % nkc, rest = lin / nkc;
  const int bx = rest % gridDim.x, bz = rest / gridDim.x;
  const int n0 = bx * (8 * 16 * MT) + w * 16 * MT;
  const int r0 = bz * (16 * NT);
  const int kr0 = kc * SUB * 128;
  // diagnostic phase stamps (mx_llm_bench_gemv_trace), thread 0, vector stores; compiled in
  // only by the MX_ROWS_TRACE build (build.py, MORPHEUS_MX_ROWS_TRACE=1)
  auto stamp = [&](int k) {
#if MX_ROWS_TRACE
    if (a.trace && tid == 0 && lin < a.trace_cap) a.trace[(size_t)lin * 8 + k] = __builtin_amdgcn_s_memrealtime();
#else
    (void)k;
#endif
  };
  stamp(0);

  __shared__ uint4 xs[2][NP][NT][ST][64];
  __shared__ float ssh[2][16 * NT];  // per-row sums of squares, two halves of the K pieces
  __shared__ int last_s;
  // the RMSNorm weights of this K range, staged once (every batch row reads the same k's; kept
  // out of the per-thread prefetch registers)
  __shared__ __attribute__((aligned(16))) float nws[NORM ? SUB * 128 : 4];
  static_assert(NSM == 0 || (NT == 1 && !NORM && EPI == EPI_RESID), "merge: o-projection, 16-row tile");
  __shared__ __attribute__((aligned(16))) float4 xmg[NSM > 0 ? 16 * SUB * 32 : 1];  // merged rows [16][SUB * 128]

  // X piece of thread q = t + 512 it: batch row b = bits 0-2 and 7.. of q, 8 k at 8 j with
  // j = bits 3-6.  Consecutive lanes take consecutive rows, so the 8 lanes of one LDS write
  // group store 8 distinct 16-byte slots of a fragment plane (with j fastest they all hit the
  // same 4 banks: the SQ_LDS_BANK_CONFLICT cycles of profiles/r02_pmc_rows32.json), and a wave
  // still reads X as 8 rows x 256-byte runs.
  const bool xact = tid < NT * 16 * 16;
  int xb[ITEMS], xj[ITEMS];
  const float* xrow[ITEMS];
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const int q = tid + 512 * it;
    xb[it] = min((q & 7) | ((q >> 7) << 3), 16 * NT - 1);
    xj[it] = (q >> 3) & 15;
    xrow[it] = a.X + (size_t)min(r0 + xb[it], a.R - 1) * a.xstride + 8 * xj[it];
  }
  // weight load (sub-chunk s, piece l, tile mt) = wbase[mt] + s * wss + l * wls (16-byte units).
  // Row-major W: lane (c, g) reads row c at 64-byte runs, i.e. 16 rows x 64 B per instruction,
  // which streams at ~4.7 TB/s; the fragment-major copy Wf (launch_frag_major) stores each
  // instruction's 1 KB contiguously: 6.4 TB/s for the same bytes (scripts/micro/stream_pattern.hip).
  constexpr int WL = F8 ? ST / 2 : ST;      // 16-byte weight loads per row per sub-chunk
  const uint4* wbase[MT];
  int wss, wls;
  if (a.Wf) {
    const int S = a.K / 128;
    wls = 64;
    if constexpr (!F8) {
      // bf16: [sub-chunk][tile][WL][64] (launch_frag_major): at each k step the whole grid
      // reads one contiguous region; against tile-major 1-2 % per 8 / 32-row step, e4m3 1.4 %
      // slower at 8 rows, so e4m3 stays tile-major (profiles/r05_frag_submajor_ab.log)
      // (a row window of the lm_head: tiles wf_t0 .. of the whole matrix's wf_T)
      const int T = GRAM && a.wf_T ? a.wf_T : (a.N + 15) / 16;
      wss = T * WL * 64;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int t = (GRAM ? a.wf_t0 : 0) + (min(n0 + 16 * mt, a.N - 1) >> 4);
        wbase[mt] = static_cast<const uint4*>(a.Wf) + ((size_t)kc * SUB * T + t) * WL * 64 + lane;
      }
    } else {  // e4m3: [tile][sub-chunk][WL][64]
      wss = WL * 64;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int t = (GRAM ? a.wf_t0 : 0) + (min(n0 + 16 * mt, a.N - 1) >> 4);
        wbase[mt] = static_cast<const uint4*>(a.Wf) + ((size_t)t * S + (size_t)kc * SUB) * WL * 64 + lane;
      }
    }
  } else {
    wss = F8 ? 8 : 16;
    wls = 4;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int n = min(n0 + 16 * mt + c, a.N - 1);
      wbase[mt] = (F8 ? reinterpret_cast<const uint4*>(static_cast<const uint8_t*>(a.W) + (size_t)n * a.K)
                      : reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(a.W) + (size_t)n * a.K)) +
                  g + kr0 / (F8 ? 16 : 8);
    }
  }
  float ssp[ITEMS];
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) ssp[it] = 0.f;

  float4 xr[NBX][ITEMS][2];
  uint4 wv[NBW][WL][MT];
  if (NORM) {
    for (int i = tid; i < SUB * 32; i += 512)
      reinterpret_cast<float4*>(nws)[i] = reinterpret_cast<const float4*>(a.norm_w + kr0)[i];
  }
  auto load_x = [&](int sub, int buf) {
    const int k = kr0 + 128 * sub;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      if constexpr (NSM > 0) {  // the merged rows staged in LDS
        const int m = xb[it] * (SUB * 32) + 32 * sub + 2 * xj[it];
        xr[buf][it][0] = xmg[m];
        xr[buf][it][1] = xmg[m + 1];
      } else {
        xr[buf][it][0] = *reinterpret_cast<const float4*>(xrow[it] + k);
        xr[buf][it][1] = *reinterpret_cast<const float4*>(xrow[it] + k + 4);
      }
    }
  };
  auto load_w = [&](int sub, int buf) {
#pragma unroll
    for (int l = 0; l < WL; ++l)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        wv[buf][l][mt] = MX_ROWS_WLOAD_PLAIN ? wbase[mt][sub * wss + l * wls] : load_nt(wbase[mt] + sub * wss + l * wls);
  };
  // A fragment of k-step st for weight tile mt
  auto afrag = [&](int buf, int st, int mt) -> bf16x8 {
    if (!F8) return __builtin_bit_cast(bf16x8, wv[buf][st][mt]);
    const uint4 q = wv[buf][st >> 1][mt];
    const uint32_t d0 = (st & 1) ? q.z : q.x, d1 = (st & 1) ? q.w : q.y;
    const bf16x2_t e0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, 1.0f, false);
    const bf16x2_t e1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, 1.0f, true);
    const bf16x2_t e2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, 1.0f, false);
    const bf16x2_t e3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, 1.0f, true);
    return __builtin_bit_cast(bf16x8, make_uint4(__builtin_bit_cast(uint32_t, e0),
                                                 __builtin_bit_cast(uint32_t, e1),
                                                 __builtin_bit_cast(uint32_t, e2),
                                                 __builtin_bit_cast(uint32_t, e3)));
  };
  auto stage_x2 = [&](int buf, int lb, int sub) {
    if (!xact) return;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      float x[8] = {xr[buf][it][0].x, xr[buf][it][0].y, xr[buf][it][0].z, xr[buf][it][0].w,
                    xr[buf][it][1].x, xr[buf][it][1].y, xr[buf][it][1].z, xr[buf][it][1].w};
      if (NORM) {
        const float4 n0 = reinterpret_cast<const float4*>(nws + 128 * sub + 8 * xj[it])[0];
        const float4 n1 = reinterpret_cast<const float4*>(nws + 128 * sub + 8 * xj[it])[1];
#pragma unroll
        for (int j = 0; j < 8; ++j) ssp[it] = fmaf(x[j], x[j], ssp[it]);
        x[0] *= n0.x; x[1] *= n0.y; x[2] *= n0.z; x[3] *= n0.w;
        x[4] *= n1.x; x[5] *= n1.y; x[6] *= n1.z; x[7] *= n1.w;
      }
      bf16x8 pf[NP];
      split_parts<NP>(x, pf);
      const int b = xb[it], j = xj[it];  // 8 activations at k = 8 j of the sub-chunk
      const int st = F8 ? 2 * (j >> 3) + (j & 1) : j >> 2;
      const int gq = F8 ? (j & 7) >> 1 : j & 3;
#pragma unroll
      for (int p = 0; p < NP; ++p)
        xs[lb][p][b >> 4][st][gq * 16 + (b & 15)] = __builtin_bit_cast(uint4, pf[p]);
    }
  };
  auto stage_x = [&](int buf) { stage_x2(buf, 0, 0); };

  // one accumulator per activation part: NP x NT x MT independent MFMA chains, so consecutive
  // MFMAs never wait on each other's result (SQ_WAIT_INST_ANY was 38 % of wave cycles)
  f32x4 pacc[NP][MT][NT];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) pacc[p][mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  if constexpr (NSM > 0) {
    // the block's K range for its 16 rows: 16 x SUB x 16 groups of 8 dims, the partial loads
    // first, the first weight sub-chunks behind them, then the merge into LDS
    constexpr int MI = (16 * SUB * 16 + 511) / 512;
    MergeIn<NSM> mi[MI];
    int mns[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int q = min(tid + 512 * i, 16 * SUB * 16 - 1);
      mns[i] = row_merge_load<NSM>(a, min(r0 + (q / (SUB * 16)), a.R - 1), kr0 + 8 * (q % (SUB * 16)), mi[i]);
    }
#pragma unroll
    for (int d = 0; d < PW; ++d)
      if (d < SUB) load_w(d, d % NBW);
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int q = tid + 512 * i;
      if (q < 16 * SUB * 16) {
        float4 lo, hi;
        row_merge_apply<NSM>(mi[i], mns[i], lo, hi);
        xmg[2 * q] = lo;  // row q / (16 SUB), dims 8 (q % (16 SUB)) of the K range
        xmg[2 * q + 1] = hi;
      }
    }
    __syncthreads();
#pragma unroll
    for (int d = 0; d < DX; ++d)
      if (d < SUB) load_x(d, d % NBX);
  } else {
#pragma unroll
    for (int d = 0; d < DX; ++d)
      if (d < SUB) load_x(d, d % NBX);
#pragma unroll
    for (int d = 0; d < PW; ++d)
      if (d < SUB) load_w(d, d % NBW);
  }
  EpiPre<MT, NT, EPI, GRAM> pre;
  float wsa[4] = {1.f, 1.f, 1.f, 1.f};  // e4m3 row scales of the atomic residual epilogue
  if (NORM) __syncthreads();  // nws staged
  stage_x(0);
  __syncthreads();
  stamp(1);
#pragma unroll
  for (int sub = 0; sub < SUB; ++sub) {
    const int cur = sub & 1, nxt = cur ^ 1;  // LDS buffers
    if (sub + DX < SUB) load_x(sub + DX, (sub + DX) % NBX);
    if (sub + PW < SUB) load_w(sub + PW, (sub + PW) % NBW);
    if constexpr (EPI == EPI_ARGMAX) {
      if (sub == (SUB >= 2 ? SUB - 2 : 0)) argmax_slots<MT, NT, EPI, GRAM>(a, pre, r0, c);
      if (sub == SUB - 1) argmax_operands<MT, NT, EPI, GRAM>(a, pre, n0, g);
    }
    if constexpr ((EPI == EPI_RESID || EPI == EPI_QKV) && F8) {  // the atomic / partial
      if (sub == SUB - 1) {  // epilogues' row scales, behind the last weight loads (vmcnt exact)
#pragma unroll
        for (int i = 0; i < 4; ++i) wsa[i] = a.wscale[min(n0 + 4 * g + i, a.N - 1)];
      }
    }
    // keep the prefetch at the top of the sub-chunk: under the 128-VGPR cap the scheduler
    // otherwise sinks these loads behind the MFMAs to hold more LDS fragments live
    __builtin_amdgcn_sched_barrier(0);
    const int wb = sub % NBW;
    // the k-step's activation fragments are read from LDS as one group ahead of its MFMAs
    // (one LDS round trip per k-step, not one per MFMA)
#pragma unroll
    for (int st = 0; st < ST; ++st) {
      bf16x8 xb8[NP][NT];
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) xb8[p][nt] = __builtin_bit_cast(bf16x8, xs[cur][p][nt][st][lane]);
      __builtin_amdgcn_sched_barrier(0);  // (the scheduler would pair each read with its MFMA)
      bf16x8 af[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) af[mt] = afrag(wb, st, mt);
#pragma unroll
      for (int p = 0; p < NP; ++p) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            pacc[p][mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[mt], xb8[p][nt],
                                                                      pacc[p][mt][nt], 0, 0, 0);
        }
      }
    }
    if (sub + 1 < SUB) stage_x2((sub + 1) % NBX, nxt, sub + 1);
    __syncthreads();
    if (sub == 0) stamp(2);
  }
  stamp(3);
  f32x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      acc[mt][nt] = pacc[0][mt][nt] + pacc[1][mt][nt];
      if (NP > 2) acc[mt][nt] += pacc[NP - 1][mt][nt];
    }
  // per-row sum of squares of this K range: a row's 16 pieces are lanes 8 apart in two
  // adjacent waves (j bit 3 = wave bit 0); each wave sums its 8, the halves add in LDS
  if (NORM) {
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      float t = ssp[it];
      t += __shfl_xor(t, 8, 64);
      t += __shfl_xor(t, 16, 64);
      t += __shfl_xor(t, 32, 64);
      if (xact && (xj[it] & 7) == 0) ssh[xj[it] >> 3][xb[it]] = t;
    }
    __syncthreads();
  }
  float ss[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) ss[nt] = NORM ? ssh[0][16 * nt + c] + ssh[1][16 * nt + c] : 0.f;

  if constexpr (EPI == EPI_RESID && MT == 1) {
    if (nkc > 1 && a.rows_atomic) {
      // Seam-free split-K for the residual projections (option rows_atomic): y = h + W x is
      // linear in the K ranges, so every range adds its partial tile straight into the
      // residual stream -- no write-through partials, no drain, no ticket, no last-arriver
      // merge.  The tile goes through LDS first so that each atomic wave-instruction covers
      // 64 consecutive floats of one row (256 B: the full-rate shape, MI355X_MICROARCH.md
      // "Global float atomics"); the MFMA layout would give 16 rows x 4 scattered dwords.
      // The adds land in any order (fp32 rounding of the sum is not fixed run to run).
      constexpr int OTS = 132;  // floats per staged row (16-byte aligned, 2-way banks at most)
      static_assert(16 * NT * OTS * 4 <= (int)sizeof(xs), "staging fits the activation buffer");
      float* ot = reinterpret_cast<float*>(&xs[0][0][0][0][0]);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        f32x4 v = acc[0][nt];
        if constexpr (F8) {
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] *= wsa[i];
        }
        *reinterpret_cast<f32x4*>(ot + (16 * nt + c) * OTS + 16 * w + 4 * g) = v;
      }
      __syncthreads();
      const int nb0 = bx * 128;
#pragma unroll
      for (int it = 0; it < NT * 4; ++it) {
        const int idx = it * 512 + tid, row = idx >> 7, col = idx & 127;
        const int b = r0 + row, n = nb0 + col;
        if (b < a.R && n < a.N) atomicAdd(a.Y + (size_t)b * a.ystride + n, ot[row * OTS + col]);
      }
      stamp(6);
      return;
    }
  }
  if constexpr (EPI == EPI_QKV && MT == 1) {
    if (a.qkv_parts) {
      // Decode without the split-K seam (option rows_qkv_parts): this K range stores its raw
      // partial tile (and its rows' partial sums of squares) with plain stores and exits; the
      // attention launch that follows sums the ranges in range order, applies the RMS scale
      // and RoPE, and appends the new position's K / V (attn_kernel, AttnArgs::qkv_parts).
      float* dst = a.qkv_parts + (size_t)kc * a.R * a.N;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int b = r0 + 16 * nt + c;
        f32x4 v = acc[0][nt];
        if constexpr (F8) {
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] *= wsa[i];
        }
        if (b < a.R && n0 + 4 * g < a.N) *reinterpret_cast<f32x4*>(dst + (size_t)b * a.N + n0 + 4 * g) = v;
      }
      if (NORM && bx == 0 && tid < 16 * NT && r0 + tid < a.R)
        a.qkv_ss[(size_t)kc * a.R + r0 + tid] = ssh[0][tid] + ssh[1][tid];
      stamp(6);
      return;
    }
  }
  // in flight across the hand-off (measured against loading them after the merge: 32 rows
  // 2.84 -> 2.83 ms, 8 rows fp8 1.73 -> 1.69-1.70 ms per step, profiles/r03_rows_epilogue_prefetch.log)
  rows_epilogue_pre<MT, NT, EPI, GRAM>(a, pre, n0, r0, c, g);
  if (nkc > 1) {  // publish this K range's partial, last arriver merges in range order
    const size_t tile = (size_t)bz * gridDim.x + bx;
    const size_t slab_floats = 8 * (size_t)WSLAB + 16 * NT;
    float* base = a.ws + tile * nkc * slab_floats;
    float* mine = base + (size_t)kc * slab_floats;
    // lane-major partial: a lane's MT x NT quads are contiguous (16-byte sc1 accesses); the
    // buffer descriptor stays block-uniform (a per-lane base would be a waterfall loop)
    const int wu = __builtin_amdgcn_readfirstlane(w);
    const size_t lofs = (size_t)wu * WSLAB + (size_t)lane * (4 * MT * NT);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) st4_wt(mine, lofs + (mt * NT + nt) * 4, acc[mt][nt]);
    if (NORM && tid < 16 * NT) st_wt(mine + 8 * (size_t)WSLAB + tid, ssh[0][tid] + ssh[1][tid]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      const int t = __hip_atomic_fetch_add(a.tickets + tile, 1, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
      const int last = t == nkc - 1;
      if (last) __hip_atomic_store(a.tickets + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last_s = last;
    }
    __syncthreads();
    stamp(4);
    if (!last_s) return;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) ss[nt] = 0.f;
    // the K ranges' partials, four ranges' loads in flight at a time, summed in range order
    for (int q0 = 0; q0 < nkc; q0 += MQ) {
      f32x4 t[MQ][MT][NT];
      float sq[MQ][NT];
#pragma unroll
      for (int j = 0; j < MQ; ++j) {
        if (q0 + j >= nkc) break;  // block-uniform: no duplicate loads of the last range
        const float* src = base + (size_t)(q0 + j) * slab_floats;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) t[j][mt][nt] = ld4_wt(src, lofs + (mt * NT + nt) * 4);
        if (NORM) {
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) sq[j][nt] = ld_wt(src + 8 * (size_t)WSLAB + 16 * nt + c);
        }
      }
#pragma unroll
      for (int j = 0; j < MQ; ++j) {
        if (q0 + j >= nkc) break;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[mt][nt][i] += t[j][mt][nt][i];
        if (NORM) {
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) ss[nt] += sq[j][nt];
        }
      }
    }
  }
  if (nkc > 1) stamp(5);
  float scale[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
    scale[nt] = NORM ? rms_scale(ss[nt], a.K, a.eps) : 1.f;
  rows_epilogue<MT, NT, EPI, GRAM>(a, acc, scale, n0, r0, c, g, pre);
#if MX_ROWS_TRACE
  if (a.trace) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    stamp(6);
  }
#endif
