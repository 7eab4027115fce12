#pragma once
// Multi-row decode GEMM, generation 4 (the only multi-row generation built; generations 5
// and 7 were measured 3.6-5 % and 13-60 % slower and were retired, DESIGN.md §5).
// Multi-row decode / prefill projections on bf16 MFMA (gfx950) — the B = 2..64 path.
//
// Replaces the batched decode GEMMs of vLLM's engine (continuous batching of concurrent
// requests, Orpheus-TTS/orpheus_tts_pypi/orpheus_tts/engine_class.py:117) for BASELINE
// configs 3 and 5 (B = 32 / 8 streams per GPU).  Every weight byte is still streamed ONCE
// per step (the step stays HBM-bound up to B ~ 300), so the kernel is a weight-streaming
// skinny GEMM:
//   * D[16 weight rows][16 batch rows] tiles of v_mfma_f32_16x16x32_bf16; A = weights
//     straight from HBM (16 B per lane, non-temporal), B = activation rows.
//   * Precision contract (DESIGN.md §3): activations are fp32.  They enter the MFMA as
//     NPART bf16 parts x = x0 + x1 (+ x2) split in registers, so products are the fp32
//     products of the oracle (bf16 weights are exact) up to summation order.
//   * RMSNorm is folded: y = (W (x . nw)) * rsqrt(mean(x^2) + eps); the sum of squares is
//     accumulated from the same activation loads.
//   * A block of WK waves splits K; partial tiles are summed in LDS in a fixed order
//     (deterministic), then wave 0 runs the epilogue (RoPE + KV append, SiLU*up, residual,
//     penalty + argmax) with the same lane layout as the MFMA result.
#include "mx_common.h"
#include "mx_llm_kernels.h"
#include "mx_rows_common.h"

#include <algorithm>

// Activation parts fed to the bf16 MFMA: 3 reproduces the fp32 products exactly; 2 keeps
// 16 mantissa bits (|dropped| < 2^-16 |x|).  Build-time experiment knob.
#ifndef MX_ROWS_NP
#define MX_ROWS_NP 3
#endif
#ifndef MX_ROWS_TRACE
#define MX_ROWS_TRACE 0
#endif
// weight loads non-temporal (1, the product) or default cache policy (experiment knob)
#ifndef MX_ROWS_WLOAD_PLAIN
#define MX_ROWS_WLOAD_PLAIN 0
#endif

namespace mx {
namespace v4 {

using namespace rows;

// One block = 8 waves; wave w owns weight rows n0 + 16 MT w .. (+16 MT) of the block's tile
// and the tile's 16 NT batch rows, over the block's K range of SUB sub-chunks of 128.
// Activations are shared, not re-read per wave: each sub-chunk of X is loaded ONCE per block
// (one 32-byte piece per thread), RMS-norm-weighted, split into three bf16 parts and written
// to LDS in MFMA B-fragment order (ds_read_b128, lane-linear, conflict-free); the weights
// stream straight to registers one sub-chunk ahead.  Issue order per sub-chunk: X(s+1)
// then W(s+1), so staging X(s+1) never waits behind the weight stream (vmcnt is in order).
// K ranges (gridDim.y of them) give the grid its parallelism; each publishes its partial
// tiles with write-through (sc1) stores, and the last arriving range sums them in range
// order (deterministic) and runs the epilogue (MI355X_MICROARCH.md "Valid forms", row 1).
// F8: weights are OCP e4m3 (16 per 16-byte load = two MFMA k-steps; converted to bf16 in
// registers by v_cvt_scalef32_pk_bf16_fp8, exact) with a per-row scale in the epilogue.  A
// lane's 16 bytes hold k = 64 P + 16 g .. +15, so k-step 2P + h contracts k = 64 P + 16 g +
// 8 h + j, and the activation fragments are staged in that (consistent) k order.
// PW: weight prefetch distance in sub-chunks (1 = the original double buffer); the activation
// pieces run DX = PW sub-chunks ahead and are issued BEFORE each sub-chunk's weights.  vmcnt
// counts in order: staging X(s+1) waits for every load issued before it, i.e. the weights up
// to w(s + PW - DX); DX >= PW keeps that at w(s), which the MFMAs of s needed anyway (with
// DX = 2 < PW = 3 the wait drained a prefetched sub-chunk: why distance 3 once measured
// slower than 2).
// Occupancy: up to 32 batch rows the kernel is capped at 128 VGPRs (4 waves per SIMD, two
// 8-wave blocks per CU): twice the weight bytes in flight per CU of the 134-VGPR build.
// NSM > 0 (o-projection, 16-row batch tile): the activation is the attention output, merged
// here from its split partials (attn_kernel no_merge mode, as the one-row o-projection does):
// before the main loop the block merges its K range for its 16 rows into LDS -- the partial
// loads go out first, the first weight sub-chunks behind them -- and the activation pieces are
// then read from there.  The attention takes no ticket and runs no last-arriver merge.
// (MergeIn, row_merge_load and row_merge_apply: mx_epilogue.h.)
// The body is mx_rows_v4_body.inc.  GRAM (gemm_rows_gram_kernel): the lm_head of a context that
// carries a code grammar -- a row window of the weights and the per-row mask; every other launch
// runs gemm_rows_kernel, which has neither.
template <int MT, int NT, int EPI, bool NORM, int SUB, bool F8, int PW = 1, int NSM = 0>
__global__ __launch_bounds__(512, (MT == 1 && NT <= 2) ? 4 : 2) void gemm_rows_kernel(GemvArgs a) {
  constexpr bool GRAM = false;
#include "mx_rows_v4_body.inc"
}
template <int MT, int NT, bool NORM, int SUB, bool F8, int PW>
__global__ __launch_bounds__(512, (MT == 1 && NT <= 2) ? 4 : 2) void gemm_rows_gram_kernel(GemvArgs a) {
  constexpr bool GRAM = true;
  constexpr int EPI = EPI_ARGMAX, NSM = 0;
#include "mx_rows_v4_body.inc"
}

// K ranges per launch: enough blocks to fill the chip without inflating the partial-tile
// traffic (each range adds R x N x 4 bytes of write-through partials).
inline int rows_nkc(int N, int K, int R, int MT, int NT, int target = 384) {
  const int subs = K / 128;
  const int tiles = ((N + 128 * MT - 1) / (128 * MT)) * ((R + 16 * NT - 1) / (16 * NT));
  int nkc = 1;
  while (tiles * nkc < target && subs % (2 * nkc) == 0 && subs / (2 * nkc) >= 2) nkc *= 2;
  while (tiles * nkc < target && subs % (3 * nkc) == 0 && subs / (3 * nkc) >= 2) nkc *= 3;
  // the kernel is instantiated for these sub-chunk counts only (launch_rows_k); K = 8192 at
  // two ranges (32 sub-chunks) fell back to the grid-stride GEMV: 726 us per prefill launch
  auto ok = [](int s) {
    return s == 1 || s == 2 || s == 3 || s == 4 || s == 6 || s == 8 || s == 12 || s == 16 || s == 24;
  };
  while (!ok(subs / nkc) && subs % (2 * nkc) == 0) nkc *= 2;
  return nkc;
}

template <int MT, int NT, int EPI, bool NORM, int SUB, int PW, int NSM = 0>
inline hipError_t launch_rows_pw(const GemvArgs& a, int nkc, hipStream_t st) {
  if (a.wdtype == WT_FP8 && a.K % 128) return hipErrorNotSupported;
  const int tiles_n = (a.N + 128 * MT - 1) / (128 * MT), tiles_r = (a.R + 16 * NT - 1) / (16 * NT);
  if (nkc > 1) {
    const size_t need = (size_t)tiles_n * tiles_r * nkc * (8 * MT * NT * 4 * 64 + 16 * NT);
    if (!a.ws || !a.tickets || need > a.ws_floats || (size_t)tiles_n * tiles_r > a.tickets_n)
      return hipErrorInvalidValue;
  }
  const dim3 grid(tiles_n, nkc, tiles_r);
  if constexpr (EPI == EPI_ARGMAX && NSM == 0) {
    if (a.gram.origin) {
      if (a.wdtype == WT_FP8) {
        hipLaunchKernelGGL((gemm_rows_gram_kernel<MT, NT, NORM, SUB, true, PW>), grid, dim3(512), a.rows_lds_pad * 1024, st, a);
      } else {
        // the 64-row bf16 tile at prefetch distance 2 over 12 or more sub-chunks sits at 256
        // VGPRs without the spans (they would spill): the grammar kernel takes distance 1 there
        constexpr int GPW = (NT == 4 && PW == 2 && SUB >= 12) ? 1 : PW;
        hipLaunchKernelGGL((gemm_rows_gram_kernel<MT, NT, NORM, SUB, false, GPW>), grid, dim3(512), a.rows_lds_pad * 1024, st, a);
      }
      return hipGetLastError();
    }
  }
  // (a row window exists only under a grammar)
  if (EPI == EPI_ARGMAX && (a.id0 || a.V != a.N || a.wf_t0 || a.wf_T)) return hipErrorInvalidValue;
  if (a.wdtype == WT_FP8) {
    hipLaunchKernelGGL((gemm_rows_kernel<MT, NT, EPI, NORM, SUB, true, PW, NSM>), grid, dim3(512), a.rows_lds_pad * 1024, st, a);
  } else {
    hipLaunchKernelGGL((gemm_rows_kernel<MT, NT, EPI, NORM, SUB, false, PW, NSM>), grid, dim3(512), a.rows_lds_pad * 1024, st, a);
  }
  return hipGetLastError();
}

// Prefetch distance 2 (bf16): measured 97.3 vs 103.5 us per layer of projections at 32 rows,
// neutral at 8 rows; distance 3 was slower (scripts/gpu_pw.sh).  e4m3 weights (half the bytes
// per sub-chunk): distance 2 measured 53.6 vs 66.3 us per layer at 8 rows, 3 no better
// (scripts/gpu_f8pw.sh).
template <int MT, int NT, int EPI, bool NORM, int SUB, int NSM = 0>
inline hipError_t launch_rows_sub(const GemvArgs& a, int nkc, hipStream_t st) {
  // distances 3 and 4 measured slower again at 8 / 32 / 64 rows (profiles/r02_rows_gen4_pw*.log)
  const int pw = std::min(a.wdtype == WT_FP8 ? a.rows_pw_f8 : a.rows_pw, SUB);
  if (pw >= 2) return launch_rows_pw<MT, NT, EPI, NORM, SUB, 2, NSM>(a, nkc, st);
  return launch_rows_pw<MT, NT, EPI, NORM, SUB, 1, NSM>(a, nkc, st);
}

template <int EPI>
inline int rows_target_of(const GemvArgs& a) {
  // K-range split target (blocks): measured at 8 and 32 rows (scripts/gpu_target.sh) the qkv
  // projection is fastest aiming at 128 blocks, the others at 192 (384 was the old default)
  return (EPI == EPI_ARGMAX && a.rows_head_target > 0) ? a.rows_head_target
         : a.rows_target > 0 ? a.rows_target : (EPI == EPI_QKV ? 128 : 192);
}

template <int MT, int NT, int EPI, bool NORM>
inline hipError_t launch_rows_k(const GemvArgs& a, hipStream_t st) {
  if (a.K % 128) return hipErrorNotSupported;
  const int nkc = rows_nkc(a.N, a.K, a.R, MT, NT, rows_target_of<EPI>(a));
  if constexpr (EPI == EPI_RESID && !NORM && MT == 1 && NT == 1) {
    if (a.att_ml) {  // the merging o-projection (rows_merge_ok): 3 sub-chunks per K range
      if (a.K / 128 / nkc != 3 || a.att_nsm > 4) return hipErrorInvalidValue;
      return a.att_nsm <= 2 ? launch_rows_sub<1, 1, EPI_RESID, false, 3, 2>(a, nkc, st)
                            : launch_rows_sub<1, 1, EPI_RESID, false, 3, 4>(a, nkc, st);
    }
  }
  if (a.att_ml) return hipErrorInvalidValue;  // (no other shape merges)
  switch (a.K / 128 / nkc) {
    case 1: return launch_rows_sub<MT, NT, EPI, NORM, 1>(a, nkc, st);
    case 2: return launch_rows_sub<MT, NT, EPI, NORM, 2>(a, nkc, st);
    case 3: return launch_rows_sub<MT, NT, EPI, NORM, 3>(a, nkc, st);
    case 4: return launch_rows_sub<MT, NT, EPI, NORM, 4>(a, nkc, st);
    case 6: return launch_rows_sub<MT, NT, EPI, NORM, 6>(a, nkc, st);
    case 8: return launch_rows_sub<MT, NT, EPI, NORM, 8>(a, nkc, st);
    case 12: return launch_rows_sub<MT, NT, EPI, NORM, 12>(a, nkc, st);
    case 16: return launch_rows_sub<MT, NT, EPI, NORM, 16>(a, nkc, st);
    case 24: return launch_rows_sub<MT, NT, EPI, NORM, 24>(a, nkc, st);
    default: return hipErrorNotSupported;
  }
}

// Batch tile: 16 NT rows (nt_max caps it: option rows_nt_max).  Measured at 32 rows: a 16-row
// cap is slower (102.7 vs 87.9 us per layer of projections), and 32 weight rows per wave
// (one staged activation sub-chunk feeding twice the weights) far slower (141.7 us: half the
// tiles leave CUs idle), so the weight tile stays 16 rows per wave.
inline void rows_tiles(int epi, int R, int* mt, int* nt, int nt_max = 4) {
  *nt = R <= 16 ? 1 : R <= 32 ? 2 : 4;
  if (nt_max > 0 && *nt > nt_max) *nt = nt_max;
  *mt = 1;
}

// The o-projection merges the attention splits itself (attn no_merge) when its launch is a
// 16-row batch tile over K ranges of 3 sub-chunks (3 heads) and a row has at most 4 splits.
inline bool rows_merge_ok(const GemvArgs& o) {
  int mt, nt;
  rows_tiles(EPI_RESID, o.R, &mt, &nt, o.rows_nt_max);
  if (o.R < 2 || nt != 1 || o.K % 128 || o.att_nsm < 1 || o.att_nsm > 4) return false;
  const int nkc = rows_nkc(o.N, o.K, o.R, mt, nt, rows_target_of<EPI_RESID>(o));
  return o.K / 128 / nkc == 3;
}


// One entry per epilogue class, each compiled in its own translation unit (rows_v4_*.hip)
// so the instantiations build in parallel.
hipError_t launch_rows_qkv(const GemvArgs& a, int nt, hipStream_t st);
hipError_t launch_rows_resid(const GemvArgs& a, int nt, hipStream_t st);
hipError_t launch_rows_silu(const GemvArgs& a, int nt, hipStream_t st);
hipError_t launch_rows_head(const GemvArgs& a, int epi, bool norm, int nt, hipStream_t st);

}  // namespace v4
}  // namespace mx
