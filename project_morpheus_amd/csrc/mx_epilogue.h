// The decode projections' epilogues, once: the packed-QKV pair (RoPE + Q store + K / V append),
// the lm_head candidate (grammar, penalty, logit, argmax key) and the attention split merge.
// Used by gemv_kernel, gemv1_kernel and attn_kernel (llm_kernels.hip), head_b1_kernel
// (head_b1.hip) and the multi-row rows_epilogue (mx_rows_common.h).  The persistent engine
// (engine_b1.hip) publishes granules beside the cache entries: it shares the rotation only.
#pragma once
#include "mx_common.h"
#include "mx_llm_kernels.h"

namespace mx {

// ---- packed wqkv rows -----------------------------------------------------------------------
// Row n of the packed wqkv is head hh = n / 128 (q heads, then k heads, then v heads), element
// `within` of it.  q and k rows are pair-interleaved: rows (n, n + 1), n even, are dims
// (p, p + 64) of the head, the pair RoPE rotates; v rows are in natural order.
// RoPE of the pair (x1, x2) = dims (p, p + 64): the rotated dim p and dim p + 64
__device__ __forceinline__ float rope_lo(float x1, float x2, float cs, float sn) {
  return x1 * cs - x2 * sn;
}
__device__ __forceinline__ float rope_hi(float x1, float x2, float cs, float sn) {
  return x2 * cs + x1 * sn;
}
// the bf16 append of dim d at position pos of one (slot, kv head)'s K / V block (mx_common.h
// layout): attn_kernel's qkv_parts path
__device__ __forceinline__ void kv_put_k(uint16_t* k, int pos, int d, float x) {
  k[kv_k_off(pos, d)] = f32_to_bf16(x);
}
__device__ __forceinline__ void kv_put_v(uint16_t* v, int pos, int d, float x) {
  v[kv_v_off(pos, d)] = f32_to_bf16(x);
}

// One pair (X1, X2) = rows (N, N + 1) of the packed projection for batch row QROW, bound to
// (SLOT, POS): q -> RoPE -> Q[QROW], k -> RoPE -> K cache, v -> V cache.  COS and SIN are
// expressions in `p` (the pair's index within its head) and are evaluated for q and k pairs
// only, inside the branch: each kernel keeps its RoPE loads where it issues them (after the
// reduction in the one-row kernels, preloaded in the multi-row one).
// A macro, not a function: a function of this size is optimised on its own before it is inlined
// (its address arithmetic is folded without the caller's known bits), and gemv_kernel,
// gemv1_kernel and gemm_rows_kernel all came out with different code (scripts/isa_parity.py);
// the text below expands to exactly the statements each of them held (for the same reason it
// indexes the cache itself and does not go through kv_put_k / kv_put_v).
#define MX_QKV_PAIR(A, N, X1, X2, SLOT, POS, QROW, COS, SIN)                                    \
  {                                                                                             \
    const int n_ = (N);                                                                         \
    const int hh_ = n_ >> 7, within_ = n_ & 127, p = within_ >> 1;                              \
    const float x1_ = (X1), x2_ = (X2);                                                         \
    if (hh_ < (A).heads + (A).kv_heads) {                                                       \
      const float cs_ = (COS);                                                                  \
      const float sn_ = (SIN);                                                                  \
      const float o1_ = ::mx::rope_lo(x1_, x2_, cs_, sn_);                                      \
      const float o2_ = ::mx::rope_hi(x1_, x2_, cs_, sn_);                                      \
      if (hh_ < (A).heads) {                                                                    \
        float* q_ = (A).Q + ((size_t)(QROW) * (A).heads + hh_) * 128;                           \
        q_[p] = o1_;                                                                            \
        q_[p + 64] = o2_;                                                                       \
      } else {                                                                                  \
        uint16_t* k_ = (A).kcache +                                                             \
            ((size_t)(SLOT) * (A).kv_heads + (hh_ - (A).heads)) * (A).max_pos * 128;            \
        k_[::mx::kv_k_off(POS, p)] = ::mx::f32_to_bf16(o1_);                                    \
        k_[::mx::kv_k_off(POS, p + 64)] = ::mx::f32_to_bf16(o2_);                               \
      }                                                                                         \
    } else { /* fragment-major chunks (mx_common.h kv_v_off, see attn_kernel) */                \
      uint16_t* v_ = (A).vcache +                                                               \
          ((size_t)(SLOT) * (A).kv_heads + (hh_ - (A).heads - (A).kv_heads)) * 128 * (A).max_pos; \
      v_[::mx::kv_v_off(POS, within_)] = ::mx::f32_to_bf16(x1_);                                \
      v_[::mx::kv_v_off(POS, within_ + 1)] = ::mx::f32_to_bf16(x2_);                            \
    }                                                                                           \
  }

// ---- lm_head ----------------------------------------------------------------------------------
// the penalised logits of a slot's row are kept for the sampler (or for every row: parity reads)
__device__ __forceinline__ bool head_keep(const GemvArgs& a, int slot) {
  return a.logits && (a.logits_all || a.samp_temp[slot] > 0.f);
}
// One candidate: logit v of token `id` for decode row `row` (logits stride V).  Ids outside a
// constrained slot's allowed set count as -inf: no key, no logit.  `seen` (the id is under the
// repetition penalty) is fetched by the caller: a byte, a preloaded dword, a register.  Where
// several lanes hold the same candidate, `writer` picks the one that stores the kept logit.
__device__ __forceinline__ void head_candidate(const GemvArgs& a, const GrammarSpan& sp, int id,
                                               float v, bool seen, float pen, bool keep,
                                               bool writer, size_t row, int V,
                                               unsigned long long& best) {
  if (!grammar_allows(a.gram, sp, id)) return;
  if (seen) v = v > 0.f ? v / pen : v * pen;
  if (keep && writer) a.logits[row * V + id] = v;
  const unsigned long long key = argmax_key(v, (uint32_t)id);
  best = key > best ? key : best;
}

// ---- attention split merge --------------------------------------------------------------------
// att = sum_s e^(m_s - M) acc_s / sum_s e^(m_s - M) l_s over a row's live splits (attn_kernel
// no_merge mode), for one 8-dim group of one head.
template <int NSM>
struct MergeIn {  // one 8-dim group's split partials, loaded
  float2 ml[NSM];
  float4 lo[NSM], hi[NSM];
};
// One-row o-projection (gemv1_kernel): group j of row 0; slot s is read at an address fixed by
// the kernel arguments (clamped to nb), whatever the row's live count.
template <int NSM>
__device__ __forceinline__ void merge_load(const GemvArgs& a, int stride, int nb, int j, MergeIn<NSM>& in) {
  const int GRP = a.heads / a.kv_heads;
  const int hh = j >> 4, d0 = (j & 15) * 8;
  const int kvh = hh / GRP, hin = hh - kvh * GRP;
  // slot s of this kv head sits s * GRP (m, l) pairs / accumulator rows past slot 0: the lane's
  // part of the address is formed once, the slot's part is wave-uniform
  const size_t p0 = (size_t)kvh * stride * GRP + hin;
  const float* ml0 = a.att_ml + p0 * 2;
  const float* ac0 = a.att_acc + p0 * 128 + d0;
#pragma unroll
  for (int s = 0; s < NSM; ++s) {
    const size_t so = (size_t)(min(s, nb - 1) * GRP);
    in.ml[s] = *reinterpret_cast<const float2*>(ml0 + so * 2);
    const float4* ac = reinterpret_cast<const float4*>(ac0 + so * 128);
    in.lo[s] = ac[0];
    in.hi[s] = ac[1];
  }
}
// Multi-row o-projection (gemm_rows_kernel): dims k .. k + 7 of row b; the addresses wait for
// the row's live count ns (returned), slots past it re-read the last live one.
template <int NSM>
__device__ __forceinline__ int row_merge_load(const GemvArgs& a, int b, int k, MergeIn<NSM>& in) {
  const int GRP = a.heads / a.kv_heads;
  const int hh = k >> 7, d0 = k & 127;
  const int kvh = hh / GRP, hin = hh - kvh * GRP;
  const int ns = (a.row_pos[b] + a.att_S) / a.att_S;  // splits of this row's L = pos + 1
  const size_t pb = ((size_t)b * a.kv_heads + kvh) * a.att_stride;
#pragma unroll
  for (int s = 0; s < NSM; ++s) {
    const size_t sp = pb + min(s, ns - 1);
    in.ml[s] = *reinterpret_cast<const float2*>(a.att_ml + (sp * GRP + hin) * 2);
    const float4* ac = reinterpret_cast<const float4*>(a.att_acc + (sp * GRP + hin) * 128 + d0);
    in.lo[s] = ac[0];
    in.hi[s] = ac[1];
  }
  return ns;
}
// EARLY: the loads did not wait for ns, so a slot at or past it may hold anything (never
// written, a stale partial, NaN, Inf) and is dropped with selects on the loaded values; else a
// dead slot is a copy of the last live one and only its factor is zeroed.
template <int NSM, bool EARLY>
__device__ __forceinline__ void merge_apply(const MergeIn<NSM>& in, int ns, float* x) {
  float M = -INFINITY;
#pragma unroll
  for (int s = 0; s < NSM; ++s)
    if (s < ns) M = fmaxf(M, in.ml[s].x);
  float den = 0.f;
  float num[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < NSM; ++s) {
    // a dead slot enters as f = 0 times zeros (selects, not 0 * x: x may be NaN / Inf)
    const bool live = !EARLY || s < ns;  // (!EARLY: a dead slot is a copy of the last live one)
    const float f = s < ns ? expf(in.ml[s].x - M) : 0.f;
    const float l = live ? in.ml[s].y : 0.f;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 lo = live ? in.lo[s] : z, hi = live ? in.hi[s] : z;
    den = fmaf(f, l, den);
    num[0] = fmaf(f, lo.x, num[0]); num[1] = fmaf(f, lo.y, num[1]);
    num[2] = fmaf(f, lo.z, num[2]); num[3] = fmaf(f, lo.w, num[3]);
    num[4] = fmaf(f, hi.x, num[4]); num[5] = fmaf(f, hi.y, num[5]);
    num[6] = fmaf(f, hi.z, num[6]); num[7] = fmaf(f, hi.w, num[7]);
  }
  const float inv = 1.0f / den;
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = num[i] * inv;
}

// The multi-row o-projection's merge: merge_apply<NSM, false>'s arithmetic written float4-wise.
// It stays a text of its own: through merge_apply the eight merging gemm_rows_kernel
// instantiations come out with two packed multiplies' operands swapped.
template <int NSM>
__device__ __forceinline__ void row_merge_apply(const MergeIn<NSM>& in, int ns, float4& lo, float4& hi) {
  float M = -INFINITY;
#pragma unroll
  for (int s = 0; s < NSM; ++s)
    if (s < ns) M = fmaxf(M, in.ml[s].x);
  float den = 0.f;
  float4 nl = make_float4(0.f, 0.f, 0.f, 0.f), nh = nl;
#pragma unroll
  for (int s = 0; s < NSM; ++s) {
    const float f = s < ns ? expf(in.ml[s].x - M) : 0.f;
    den = fmaf(f, in.ml[s].y, den);
    nl.x = fmaf(f, in.lo[s].x, nl.x); nl.y = fmaf(f, in.lo[s].y, nl.y);
    nl.z = fmaf(f, in.lo[s].z, nl.z); nl.w = fmaf(f, in.lo[s].w, nl.w);
    nh.x = fmaf(f, in.hi[s].x, nh.x); nh.y = fmaf(f, in.hi[s].y, nh.y);
    nh.z = fmaf(f, in.hi[s].z, nh.z); nh.w = fmaf(f, in.hi[s].w, nh.w);
  }
  const float inv = 1.0f / den;
  lo = make_float4(nl.x * inv, nl.y * inv, nl.z * inv, nl.w * inv);
  hi = make_float4(nh.x * inv, nh.y * inv, nh.z * inv, nh.w * inv);
}

}  // namespace mx
