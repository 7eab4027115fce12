// Temperature + top-p sampling of the next token (BASELINE P2).
//
// Replaces the sampler behind vLLM SamplingParams(temperature, top_p, repetition_penalty)
// (Orpheus-TTS/orpheus_tts_pypi/orpheus_tts/engine_class.py:106-112) and the llama.cpp
// sampler the reference drives with the same three knobs (Morpheus_Client/tts_engine/
// inference.py:75-105, llama_local.py:77).  Greedy decoding stays the parity mode: rows whose
// KV slot has temperature <= 0 keep the argmax key of the lm_head epilogue and this kernel
// returns at once.
//
// Definition (restated by oracle/sampling_ref.py, which the GPU tests compare against):
//   l_i   penalised logits (the lm_head epilogue keeps them for sampling rows)
//   e_i   = exp((l_i - max l) / T)                        in (0, 1]
//   f_i   = floor(e_i * 2^40)                             integer mass (uint64, exact sums)
//   Z     = sum f_i;   thr = max(1, floor(top_p * Z)) in float64 (top_p >= 1: thr = Z)
//   keep i  iff  sum_{j : e_j > e_i} f_j < thr            (nucleus; ties kept together)
//   u_i   = ((philox(seed, (i, pos)).x >> 9) + 0.5) * 2^-23,   q_i = -log(u_i)
//           (23 bits: u + 0.5 is exact in fp32, so u is strictly inside (0, 1))
//   token = argmax_{kept i} e_i / q_i  (smallest index on ties)   -- the exponential race,
//           an exact draw from the renormalised kept distribution.
// A slot under the context's code grammar (Code grammar) has l_i = -inf outside
// its allowed set A(k): e_i = 0 there, so such ids carry no mass and are never kept.  The
// kernels below therefore sweep A(k) alone -- one span of ids plus at most one stop id -- and
// compute the same sums, counts and race as a sweep over the masked vocabulary.
// Integer masses make the nucleus cut order-independent (deterministic under atomics); the
// cut is found by a 3-pass radix select over the bit pattern of e_i (12 + 12 + 8 bits) with
// per-bin masses in LDS, one 1024-thread block per row.
#include "mx_common.h"
#include "mx_llm_kernels.h"

namespace mx {

// Philox4x32-10 (Salmon et al., SC'11): word 0 of the block for counter (c0, c1, 0, 0).
__device__ __forceinline__ uint32_t philox_x0(uint32_t c0, uint32_t c1, uint32_t k0,
                                              uint32_t k1) {
  uint32_t x0 = c0, x1 = c1, x2 = 0u, x3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, x0), lo0 = 0xD2511F53u * x0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, x2), lo1 = 0xCD9E8D57u * x2;
    x0 = hi1 ^ x1 ^ k0;
    x1 = lo1;
    x2 = hi0 ^ x3 ^ k1;
    x3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return x0;
}

constexpr int SMP_T = 1024;  // threads per row block
constexpr float SMP_FX = 1099511627776.0f;  // 2^40

__device__ __forceinline__ unsigned long long u64_wave_sum(unsigned long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, MX_WAVE);
  return v;
}

// Bins [0, 1024*PER) of `hist` hold integer masses; `base` is the mass of everything above
// bin NB-1.  Finds the unique bin b with C_b < thr <= C_b + hist[b], where C_b = base + mass
// of bins above b, and publishes (b, C_b) to *cut_bin / *cut_base.
template <int PER>
__device__ void find_cut(const unsigned long long* hist, unsigned long long base,
                         unsigned long long thr, int* cut_bin, unsigned long long* cut_base,
                         unsigned long long* wsum) {
  constexpr int NB = SMP_T * PER;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (t == 0) {  // (always overwritten: thr <= base + the mass of these bins)
    *cut_bin = 0;
    *cut_base = base;
  }
  unsigned long long v[PER], tot = 0ull;
#pragma unroll
  for (int k = 0; k < PER; ++k) {  // thread t owns bins NB-1-t*PER .. NB-PER-t*PER (descending)
    v[k] = hist[NB - 1 - (t * PER + k)];
    tot += v[k];
  }
  unsigned long long inc = tot;  // inclusive scan over the descending order
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = __shfl_up(inc, d, MX_WAVE);
    if (lane >= d) inc += o;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  unsigned long long c = base + inc - tot;
  for (int i = 0; i < w; ++i) c += wsum[i];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (c < thr && c + v[k] >= thr) {
      *cut_bin = NB - 1 - (t * PER + k);
      *cut_base = c;
    }
    c += v[k];
  }
  __syncthreads();
}

__global__ __launch_bounds__(SMP_T) void sample_kernel(SampleArgs a) {
  const int r = blockIdx.x;
  const int slot = a.row_slot[r];
  const float T = a.temp[slot];
  if (!(T > 0.f)) return;  // greedy row: the epilogue's argmax key stands
  const float top_p = a.top_p[slot];
  const uint32_t k0 = a.seed[2 * slot], k1 = a.seed[2 * slot + 1];
  const uint32_t ctr1 = (uint32_t)a.row_pos[r];
  const float* lg = a.logits + (size_t)r * a.V;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  // the ids the row may pick: every id, or a constrained slot's span [lo, lo + span_n) plus its
  // stop id.  Sweep element j is id id_of(j); everything below is a sum, a histogram or a
  // maximum over the swept ids, and the Philox counter is the id, so the order does not matter.
  const GrammarSpan sp = grammar_span(a.gram, grammar_origin(a.gram, slot), a.row_pos[r]);
  const int span_lo = sp.lo < 0 ? 0 : sp.lo;
  const int span_n = sp.lo < 0 ? a.V : a.gram.codes - a.gram.cmin;
  const int n_it = span_n + (sp.stop >= 0 ? 1 : 0);
  auto id_of = [&](int j) { return j < span_n ? span_lo + j : sp.stop; };

  __shared__ unsigned long long hist[4096];
  __shared__ unsigned long long wsum[SMP_T / 64];
  __shared__ float fred[SMP_T / 64];
  __shared__ int cut_bin;
  __shared__ unsigned long long cut_base;

  // pass 1: max logit
  float m = -INFINITY;
  for (int j = t; j < n_it; j += SMP_T) m = fmaxf(m, lg[id_of(j)]);
  m = wave_max(m);
  if (lane == 0) fred[w] = m;
  for (int i = t; i < 4096; i += SMP_T) hist[i] = 0ull;
  __syncthreads();
  m = fred[0];
  for (int i = 1; i < SMP_T / 64; ++i) m = fmaxf(m, fred[i]);
  auto e_of = [&](int i) { return expf((lg[i] - m) / T); };
  auto f_of = [&](float e) { return (unsigned long long)(e * SMP_FX); };

  // pass 2: total integer mass Z and the first radix histogram (bits 31..20 of e)
  unsigned long long z = 0ull;
  for (int j = t; j < n_it; j += SMP_T) {
    const int i = id_of(j);
    const float e = e_of(i);
    const unsigned long long f = f_of(e);
    z += f;
    if (f) atomicAdd(&hist[__float_as_uint(e) >> 20], f);
  }
  z = u64_wave_sum(z);
  if (lane == 0) wsum[w] = z;
  __syncthreads();
  unsigned long long Z = 0ull;
  for (int i = 0; i < SMP_T / 64; ++i) Z += wsum[i];
  unsigned long long thr = Z;
  if (top_p < 1.f) {
    thr = (unsigned long long)((double)Z * (double)top_p);
    if (thr < 1ull) thr = 1ull;
  }
  __syncthreads();  // every thread has read wsum
  find_cut<1>(hist, 0ull, thr, &cut_bin, &cut_base, wsum);
  const uint32_t b1 = (uint32_t)cut_bin;
  const unsigned long long c1 = cut_base;

  // pass 3: bits 19..8 inside bin b1
  for (int i = t; i < 4096; i += SMP_T) hist[i] = 0ull;
  __syncthreads();
  for (int j = t; j < n_it; j += SMP_T) {
    const int i = id_of(j);
    const float e = e_of(i);
    const uint32_t bits = __float_as_uint(e);
    if ((bits >> 20) == b1) {
      const unsigned long long f = f_of(e);
      if (f) atomicAdd(&hist[(bits >> 8) & 0xFFFu], f);
    }
  }
  __syncthreads();
  find_cut<4>(hist, c1, thr, &cut_bin, &cut_base, wsum);
  const uint32_t b12 = (b1 << 12) | (uint32_t)cut_bin;
  const unsigned long long c2 = cut_base;

  // pass 4: bits 7..0 inside (b1, b2)
  for (int i = t; i < 4096; i += SMP_T) hist[i] = 0ull;
  __syncthreads();
  for (int j = t; j < n_it; j += SMP_T) {
    const int i = id_of(j);
    const float e = e_of(i);
    const uint32_t bits = __float_as_uint(e);
    if ((bits >> 8) == b12) {
      const unsigned long long f = f_of(e);
      if (f) atomicAdd(&hist[bits & 0xFFu], f);
    }
  }
  __syncthreads();
  find_cut<1>(hist, c2, thr, &cut_bin, &cut_base, wsum);
  const uint32_t tcut = (b12 << 8) | (uint32_t)cut_bin;

  // pass 5: exponential race over the kept tokens
  unsigned long long best = 0ull;
  for (int j = t; j < n_it; j += SMP_T) {
    const int i = id_of(j);
    const float e = e_of(i);
    if (__float_as_uint(e) >= tcut) {
      const uint32_t x = philox_x0((uint32_t)i, ctr1, k0, k1);
      const float u = ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f;  // 2^-23, u < 1 exactly
      const float s = e / -logf(u);
      const unsigned long long key = argmax_key(s, (uint32_t)i);
      best = key > best ? key : best;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(best, d, MX_WAVE);
    best = o > best ? o : best;
  }
  if (lane == 0) wsum[w] = best;
  __syncthreads();
  if (t == 0) {
    unsigned long long k = wsum[0];
    for (int i = 1; i < SMP_T / 64; ++i) k = wsum[i] > k ? wsum[i] : k;
    a.best[r] = k;
  }
}

// The sampler with two filters in front of the nucleus (temperature, then top-k and min-p,
// then top-p: vLLM's order).  Token i is in the filter set F iff f_i > 0, e_i >= min_p and
// #{j : e_j > e_i} < top_k (0: no limit; ties at the k-th value kept together).  F is an upper
// set in e-order, so both filters are ONE threshold `fbits` on the bit pattern of e: min_p
// gives its bits directly, top-k the same 12 + 12 + 8 radix select run over counts (find_cut
// unchanged, thr = k).  The mass select and the race of sample_kernel then run with everything
// below fbits masked out, so Z is the mass of F.  A row whose slot has neutral extras does no
// extra sweep and computes exactly what sample_kernel computes (fbits = 0); a row with top-k
// takes three more sweeps, one with min-p alone none.
__global__ __launch_bounds__(SMP_T) void sample_chain_kernel(SampleChainArgs c) {
  const SampleArgs& a = c.s;
  const int r = blockIdx.x;
  const int slot = a.row_slot[r];
  const float T = a.temp[slot];
  if (!(T > 0.f)) return;  // greedy row: the epilogue's argmax key stands
  const float top_p = a.top_p[slot];
  const int top_k = c.top_k[slot];
  const float min_p = c.min_p[slot];
  const uint32_t k0 = a.seed[2 * slot], k1 = a.seed[2 * slot + 1];
  const uint32_t ctr1 = (uint32_t)a.row_pos[r];
  const float* lg = a.logits + (size_t)r * a.V;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  // the ids the row may pick: every id, or a constrained slot's span [lo, lo + span_n) plus its
  // stop id.  Sweep element j is id id_of(j); everything below is a sum, a histogram or a
  // maximum over the swept ids, and the Philox counter is the id, so the order does not matter.
  const GrammarSpan sp = grammar_span(a.gram, grammar_origin(a.gram, slot), a.row_pos[r]);
  const int span_lo = sp.lo < 0 ? 0 : sp.lo;
  const int span_n = sp.lo < 0 ? a.V : a.gram.codes - a.gram.cmin;
  const int n_it = span_n + (sp.stop >= 0 ? 1 : 0);
  auto id_of = [&](int j) { return j < span_n ? span_lo + j : sp.stop; };

  __shared__ unsigned long long hist[4096];
  __shared__ unsigned long long wsum[SMP_T / 64];
  __shared__ float fred[SMP_T / 64];
  __shared__ int cut_bin;
  __shared__ unsigned long long cut_base;

  // pass 1: max logit
  float m = -INFINITY;
  for (int j = t; j < n_it; j += SMP_T) m = fmaxf(m, lg[id_of(j)]);
  m = wave_max(m);
  if (lane == 0) fred[w] = m;
  for (int i = t; i < 4096; i += SMP_T) hist[i] = 0ull;
  __syncthreads();
  m = fred[0];
  for (int i = 1; i < SMP_T / 64; ++i) m = fmaxf(m, fred[i]);
  auto e_of = [&](int i) { return expf((lg[i] - m) / T); };
  auto f_of = [&](float e) { return (unsigned long long)(e * SMP_FX); };

  // the filter threshold: min_p's bits (positive floats order as their bit patterns) ...
  uint32_t fbits = min_p > 0.f ? __float_as_uint(min_p) : 0u;
  // ... and, for 0 < top_k < the ids swept, the k-th largest e among the tokens with f > 0
  if (top_k > 0 && top_k < n_it) {
    // count pass 1: how many tokens have f > 0, and their histogram over bits 31..20 of e
    unsigned long long n = 0ull;
    for (int j = t; j < n_it; j += SMP_T) {
      const int i = id_of(j);
      const float e = e_of(i);
      if (f_of(e)) {
        ++n;
        atomicAdd(&hist[__float_as_uint(e) >> 20], 1ull);
      }
    }
    n = u64_wave_sum(n);
    if (lane == 0) wsum[w] = n;
    __syncthreads();
    unsigned long long npos = 0ull;
    for (int i = 0; i < SMP_T / 64; ++i) npos += wsum[i];
    // (npos >= 1: the maximum has e = 1.)  k past the last such token keeps them all.
    const unsigned long long kthr = (unsigned long long)top_k < npos ? (unsigned long long)top_k : npos;
    __syncthreads();  // every thread has read wsum
    find_cut<1>(hist, 0ull, kthr, &cut_bin, &cut_base, wsum);
    const uint32_t kb1 = (uint32_t)cut_bin;
    const unsigned long long kc1 = cut_base;

    // count pass 2: bits 19..8 inside bin kb1
    for (int i = t; i < 4096; i += SMP_T) hist[i] = 0ull;
    __syncthreads();
    for (int j = t; j < n_it; j += SMP_T) {
      const int i = id_of(j);
      const float e = e_of(i);
      const uint32_t bits = __float_as_uint(e);
      if ((bits >> 20) == kb1 && f_of(e)) atomicAdd(&hist[(bits >> 8) & 0xFFFu], 1ull);
    }
    __syncthreads();
    find_cut<4>(hist, kc1, kthr, &cut_bin, &cut_base, wsum);
    const uint32_t kb12 = (kb1 << 12) | (uint32_t)cut_bin;
    const unsigned long long kc2 = cut_base;

    // count pass 3: bits 7..0 inside (kb1, kb2)
    for (int i = t; i < 4096; i += SMP_T) hist[i] = 0ull;
    __syncthreads();
    for (int j = t; j < n_it; j += SMP_T) {
      const int i = id_of(j);
      const float e = e_of(i);
      const uint32_t bits = __float_as_uint(e);
      if ((bits >> 8) == kb12 && f_of(e)) atomicAdd(&hist[bits & 0xFFu], 1ull);
    }
    __syncthreads();
    find_cut<1>(hist, kc2, kthr, &cut_bin, &cut_base, wsum);
    const uint32_t kcut = (kb12 << 8) | (uint32_t)cut_bin;
    fbits = kcut > fbits ? kcut : fbits;
    __syncthreads();  // every thread has read cut_bin
    for (int i = t; i < 4096; i += SMP_T) hist[i] = 0ull;
    __syncthreads();
  }

  // mass pass 1: Z over F and the first radix histogram (bits 31..20 of e)
  unsigned long long z = 0ull;
  for (int j = t; j < n_it; j += SMP_T) {
    const int i = id_of(j);
    const float e = e_of(i);
    const uint32_t bits = __float_as_uint(e);
    const unsigned long long f = bits >= fbits ? f_of(e) : 0ull;
    z += f;
    if (f) atomicAdd(&hist[bits >> 20], f);
  }
  z = u64_wave_sum(z);
  if (lane == 0) wsum[w] = z;
  __syncthreads();
  unsigned long long Z = 0ull;
  for (int i = 0; i < SMP_T / 64; ++i) Z += wsum[i];
  unsigned long long thr = Z;
  if (top_p < 1.f) {
    thr = (unsigned long long)((double)Z * (double)top_p);
    if (thr < 1ull) thr = 1ull;
  }
  __syncthreads();  // every thread has read wsum
  find_cut<1>(hist, 0ull, thr, &cut_bin, &cut_base, wsum);
  const uint32_t b1 = (uint32_t)cut_bin;
  const unsigned long long c1 = cut_base;

  // mass pass 2: bits 19..8 inside bin b1
  for (int i = t; i < 4096; i += SMP_T) hist[i] = 0ull;
  __syncthreads();
  for (int j = t; j < n_it; j += SMP_T) {
    const int i = id_of(j);
    const float e = e_of(i);
    const uint32_t bits = __float_as_uint(e);
    if ((bits >> 20) == b1 && bits >= fbits) {
      const unsigned long long f = f_of(e);
      if (f) atomicAdd(&hist[(bits >> 8) & 0xFFFu], f);
    }
  }
  __syncthreads();
  find_cut<4>(hist, c1, thr, &cut_bin, &cut_base, wsum);
  const uint32_t b12 = (b1 << 12) | (uint32_t)cut_bin;
  const unsigned long long c2 = cut_base;

  // mass pass 3: bits 7..0 inside (b1, b2)
  for (int i = t; i < 4096; i += SMP_T) hist[i] = 0ull;
  __syncthreads();
  for (int j = t; j < n_it; j += SMP_T) {
    const int i = id_of(j);
    const float e = e_of(i);
    const uint32_t bits = __float_as_uint(e);
    if ((bits >> 8) == b12 && bits >= fbits) {
      const unsigned long long f = f_of(e);
      if (f) atomicAdd(&hist[bits & 0xFFu], f);
    }
  }
  __syncthreads();
  find_cut<1>(hist, c2, thr, &cut_bin, &cut_base, wsum);
  // (the cut bin holds mass, so tcut is the e of a token in F: tcut >= fbits)
  const uint32_t tcut = (b12 << 8) | (uint32_t)cut_bin;

  // race pass: exponential race over the kept tokens
  unsigned long long best = 0ull;
  for (int j = t; j < n_it; j += SMP_T) {
    const int i = id_of(j);
    const float e = e_of(i);
    if (__float_as_uint(e) >= tcut) {
      const uint32_t x = philox_x0((uint32_t)i, ctr1, k0, k1);
      const float u = ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f;  // 2^-23, u < 1 exactly
      const float s = e / -logf(u);
      const unsigned long long key = argmax_key(s, (uint32_t)i);
      best = key > best ? key : best;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(best, d, MX_WAVE);
    best = o > best ? o : best;
  }
  if (lane == 0) wsum[w] = best;
  __syncthreads();
  if (t == 0) {
    unsigned long long k = wsum[0];
    for (int i = 1; i < SMP_T / 64; ++i) k = wsum[i] > k ? wsum[i] : k;
    a.best[r] = k;
  }
}

// Argmax key of one row of caller logits (the greedy branch of mx_llm_debug_sample).
__global__ __launch_bounds__(SMP_T) void argmax_row_kernel(const float* lg, int lo, int n, int stop,
                                                          unsigned long long* out) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  __shared__ unsigned long long wbest[SMP_T / 64];
  unsigned long long best = 0ull;
  for (int j = t; j < n + (stop >= 0 ? 1 : 0); j += SMP_T) {
    const int i = j < n ? lo + j : stop;
    const unsigned long long key = argmax_key(lg[i], (uint32_t)i);
    best = key > best ? key : best;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(best, d, MX_WAVE);
    best = o > best ? o : best;
  }
  if (lane == 0) wbest[w] = best;
  __syncthreads();
  if (t == 0) {
    unsigned long long k = wbest[0];
    for (int i = 1; i < SMP_T / 64; ++i) k = wbest[i] > k ? wbest[i] : k;
    out[0] = k;
  }
}

__global__ void set_slot_ext_kernel(int32_t* top_k, float* min_p, int32_t* last_n, int slot,
                                    int k, float mp, int n) {
  top_k[slot] = k;
  min_p[slot] = mp;
  last_n[slot] = n;
}

__global__ void set_slot_origin_kernel(int32_t* origin, int slot, int value) { origin[slot] = value; }

__global__ void set_slot_params_kernel(float* penalty, float* temp, float* top_p,
                                       uint32_t* seed, int slot, float pen, float t, float p,
                                       uint32_t s0, uint32_t s1) {
  penalty[slot] = pen;
  temp[slot] = t;
  top_p[slot] = p;
  seed[2 * slot] = s0;
  seed[2 * slot + 1] = s1;
}

hipError_t launch_sample(const SampleArgs& a, int R, hipStream_t st) {
  hipLaunchKernelGGL(sample_kernel, dim3(R), dim3(SMP_T), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_sample_chain(const SampleChainArgs& a, int R, hipStream_t st) {
  hipLaunchKernelGGL(sample_chain_kernel, dim3(R), dim3(SMP_T), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_argmax_row(const float* logits, int lo, int n, int stop,
                             unsigned long long* best, hipStream_t st) {
  hipLaunchKernelGGL(argmax_row_kernel, dim3(1), dim3(SMP_T), 0, st, logits, lo, n, stop, best);
  return hipGetLastError();
}

hipError_t launch_set_slot_origin(int32_t* origin, int slot, int value, hipStream_t st) {
  hipLaunchKernelGGL(set_slot_origin_kernel, dim3(1), dim3(1), 0, st, origin, slot, value);
  return hipGetLastError();
}

hipError_t launch_set_slot_ext(int32_t* top_k, float* min_p, int32_t* last_n, int slot, int k,
                               float mp, int n, hipStream_t st) {
  hipLaunchKernelGGL(set_slot_ext_kernel, dim3(1), dim3(1), 0, st, top_k, min_p, last_n, slot,
                     k, mp, n);
  return hipGetLastError();
}

hipError_t launch_set_slot_params(float* penalty, float* temp, float* top_p, uint32_t* seed,
                                  int slot, float pen, float t, float p, uint64_t s,
                                  hipStream_t st) {
  hipLaunchKernelGGL(set_slot_params_kernel, dim3(1), dim3(1), 0, st, penalty, temp, top_p,
                     seed, slot, pen, t, p, (uint32_t)s, (uint32_t)(s >> 32));
  return hipGetLastError();
}

}  // namespace mx
