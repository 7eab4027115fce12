// SNAC 24 kHz codec encoder and residual vector quantiser on MI355X (gfx950), fp32 arithmetic.
//
// Replaces snac.SNAC.encode (third-party snac 1.2.x): the mirror image of snac_kernels.hip.
// Dense contractions (the residual units' 1x1 convs and the strided down-convs) run as one
// "run" conv-GEMM on the bf16 MFMA with both fp32 operands split into three bf16 parts, the
// decoder's precision contract; the depthwise dilated k7 convs stage a haloed, Snake-activated
// tile in LDS, in a 48-channel-block variant for the two full-rate levels (C = 48, 96); the
// quantiser's nearest-codebook search is exact fp32 FMA on the VALU.  No atomics anywhere: two
// encodes of one recording are bit-identical.
#include "mx_common.h"
#include "mx_snac_kernels.h"
#include "mx_snac_enc_kernels.h"
#include "mx_rows_common.h"

namespace mx {


// ---------------------------------------------------------------------------------
// Stem: conv k7 pad 3, 1 -> 48.  Block = 64 samples x 48 channels (12 channel quads x 16 row
// groups); the 70 input samples are staged in LDS, each lane keeps its quad's 28 weights.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(192) void enc_stem_kernel(const float* audio, int64_t n_samples,
                                                       const float* w, const float* b, float* out,
                                                       int T) {
  __shared__ float xs[64 + 6];
  const int t0 = blockIdx.x * 64;
  for (int i = threadIdx.x; i < 70; i += 192) {
    const int64_t t = (int64_t)t0 - 3 + i;
    xs[i] = (t >= 0 && t < n_samples) ? audio[t] : 0.f;
  }
  const int cq = threadIdx.x % 12, tr = threadIdx.x / 12;
  float wk[7][4];
#pragma unroll
  for (int k = 0; k < 7; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) wk[k][e] = w[(4 * cq + e) * 7 + k];
  const float4 bias = *reinterpret_cast<const float4*>(b + 4 * cq);
  __syncthreads();
  for (int i = tr; i < 64; i += 16) {
    const int t = t0 + i;
    if (t >= T) break;
    float4 acc = bias;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const float x = xs[i + k];
      acc.x = fmaf(wk[k][0], x, acc.x);
      acc.y = fmaf(wk[k][1], x, acc.y);
      acc.z = fmaf(wk[k][2], x, acc.z);
      acc.w = fmaf(wk[k][3], x, acc.w);
    }
    *reinterpret_cast<float4*>(out + (size_t)t * 48 + 4 * cq) = acc;
  }
}

// ---------------------------------------------------------------------------------
// Depthwise k7 dilated conv, the 48-channel-block variant of dwconv_kernel (snac_kernels.hip,
// which tiles 64 channels): block = 48 channels x 16 time rows on 192 threads, 4 channels (one
// 16-byte piece) per lane.  At C = 48 a row is 192 contiguous bytes and consecutive rows are
// adjacent, so a wave's load or store instruction still moves 64 x 16 B = 1 KB of consecutive
// addresses; at C = 96 it moves 192-byte pieces of 5-6 rows.  Grid (ceil(T / 64), C / 48).
// ---------------------------------------------------------------------------------
constexpr int ENC_DW_TT = 64;
__global__ __launch_bounds__(192) void enc_dwconv_kernel(const float* x, float* y, const float* w,
                                                         const float* b, const float* ain,
                                                         const float* aout, int C, int T, int dil) {
  constexpr int TT = ENC_DW_TT;
  const int cq = threadIdx.x % 12, tr = threadIdx.x / 12;  // channel quad, row group (16)
  const int c = blockIdx.y * 48 + 4 * cq, t0 = blockIdx.x * TT;
  const int halo = 3 * dil;
  __shared__ float4 tile[TT + 54][12];
  const float* xb = x + c;
  const float4 a_in = ain ? *reinterpret_cast<const float4*>(ain + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  // every global load of the haloed tile is issued before any is consumed
  constexpr int NI = (TT + 54 + 15) / 16;
  const int rows = TT + 2 * halo;
  float4 v[NI];
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int i = tr + 16 * j, t = t0 - halo + i;
    v[j] = (i < rows && t >= 0 && t < T) ? *reinterpret_cast<const float4*>(xb + (size_t)t * C)
                                         : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int i = tr + 16 * j;
    if (i < rows) {
      float4 u = v[j];
      if (ain) {
        u.x = snake(u.x, a_in.x); u.y = snake(u.y, a_in.y);
        u.z = snake(u.z, a_in.z); u.w = snake(u.w, a_in.w);
      }
      tile[i][cq] = u;
    }
  }
  __syncthreads();
  float wk[7][4];
#pragma unroll
  for (int k = 0; k < 7; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) wk[k][e] = w[(c + e) * 7 + k];
  const float4 bias = *reinterpret_cast<const float4*>(b + c);
  const float4 a_out = aout ? *reinterpret_cast<const float4*>(aout + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  float* yb = y + c;
  for (int i = tr; i < TT; i += 16) {
    const int t = t0 + i;
    if (t >= T) break;
    float4 acc = bias;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const float4 u = tile[i + k * dil][cq];
      acc.x = fmaf(wk[k][0], u.x, acc.x);
      acc.y = fmaf(wk[k][1], u.y, acc.y);
      acc.z = fmaf(wk[k][2], u.z, acc.z);
      acc.w = fmaf(wk[k][3], u.w, acc.w);
    }
    if (aout) {
      acc.x = snake(acc.x, a_out.x); acc.y = snake(acc.y, a_out.y);
      acc.z = snake(acc.z, a_out.z); acc.w = snake(acc.w, a_out.w);
    }
    *reinterpret_cast<float4*>(yb + (size_t)t * C) = acc;
  }
}

// ---------------------------------------------------------------------------------
// Run conv-GEMM (EncGemmArgs): the decoder's split-bf16 scheme (three parts per operand, the
// six products whose part indices sum to <= 2, smallest first) on v_mfma_f32_16x16x32_bf16.
// One block = one 48 x 32 output tile (every encoder M is a multiple of 48); its WK waves split
// K and their partial tiles are summed in LDS in a fixed order.  A lane's B fragment (column n,
// k = 8g .. 8g+7) is two 16-byte loads at float offset (stride n - pad) C + k of the
// channels-last input: C and K are multiples of 8, so an 8-run is wholly inside the input and
// below K, or wholly zero.  Grid (ceil(Tout / 32), M / 48).
// ---------------------------------------------------------------------------------
struct EncOps4 {
  f32x4 bias, r, a2;
};
__device__ __forceinline__ EncOps4 enc_gemm_ops4(const EncGemmArgs& a, int m, int n) {
  EncOps4 p;
  const size_t o = (size_t)n * a.M + m;
  p.bias = *reinterpret_cast<const f32x4*>(a.bias + m);
  p.r = a.R ? *reinterpret_cast<const f32x4*>(a.R + o) : f32x4{0.f, 0.f, 0.f, 0.f};
  p.a2 = a.out2 ? *reinterpret_cast<const f32x4*>(a.alpha2 + m) : f32x4{0.f, 0.f, 0.f, 0.f};
  return p;
}
__device__ __forceinline__ void enc_gemm_store4(const EncGemmArgs& a, f32x4 v, int m, int n,
                                                const EncOps4& p) {
  const size_t o = (size_t)n * a.M + m;
  v += p.bias;
  if (a.R) v = p.r + v;
  *reinterpret_cast<f32x4*>(a.out + o) = v;
  if (a.out2) {
    f32x4 s2;
#pragma unroll
    for (int r = 0; r < 4; ++r) s2[r] = snake(v[r], p.a2[r]);
    *reinterpret_cast<f32x4*>(a.out2 + o) = s2;
  }
}

template <int WK>
__global__ __launch_bounds__(WK * 64) void enc_gemm_kernel(EncGemmArgs a) {
  constexpr int MT = 3, NS = 2, BM = 16 * MT, BN = 16 * NS;
  const int lane = threadIdx.x & 63, wk = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM;
  const size_t plane = (size_t)a.M * a.Kp;
  const int steps = a.Kp / 32 / WK, s0 = wk * steps, s1 = s0 + steps;
  const int64_t xlen = (int64_t)a.Tin * a.C;
  int64_t xoff[NS];
  bool nok[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int n = n0 + 16 * j + c;
    nok[j] = n < a.Tout;
    xoff[j] = ((int64_t)a.stride * n - a.pad) * a.C;
  }
  const uint16_t* Ar[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) Ar[i] = a.A + (size_t)(m0 + 16 * i + c) * a.Kp + 8 * g;
  f32x4 acc[MT][NS];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NS; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // two-stage pipeline: the next 32-deep step's A planes and X pieces are in flight while this
  // step splits X and runs its MFMAs
  uint4 ab[2][MT][3];
  float4 xb[2][NS][2];
  auto xvalid = [&](int s, int j) __attribute__((always_inline)) {
    const int k0 = 32 * s + 8 * g;
    const int64_t e = xoff[j] + k0;
    return nok[j] && k0 < a.K && e >= 0 && e + 8 <= xlen;
  };
  auto load = [&](int s, int buf) __attribute__((always_inline)) {
    const int kc = 32 * s;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int p = 0; p < 3; ++p)
        ab[buf][i][p] = *reinterpret_cast<const uint4*>(Ar[i] + p * plane + kc);
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      // unconditional loads from an address clamped in range, zeroed in step()
      const int64_t e = xvalid(s, j) ? xoff[j] + kc + 8 * g : 0;
      const float4* xp = reinterpret_cast<const float4*>(a.X + e);
      xb[buf][j][0] = xp[0];
      xb[buf][j][1] = xp[1];
    }
  };
  auto step = [&](int s, int buf) __attribute__((always_inline)) {
    bf16x8 xf[NS][3];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const bool ok = xvalid(s, j);
      const float4 lo = xb[buf][j][0], hi = xb[buf][j][1];
      float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = ok ? x[e] : 0.f;
      rows::split_parts<3>(x, xf[j]);
    }
    constexpr int PA[6] = {1, 0, 2, 0, 1, 0}, PB[6] = {1, 2, 0, 1, 0, 0};
#pragma unroll
    for (int q = 0; q < 6; ++q)
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NS; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              __builtin_bit_cast(bf16x8, ab[buf][i][PA[q]]), xf[j][PB[q]], acc[i][j], 0, 0, 0);
  };
  load(s0, 0);
  for (int s = s0; s < s1; s += 2) {
    if (s + 1 < s1) load(s + 1, 1);
    step(s, 0);
    if (s + 1 < s1) {
      if (s + 2 < s1) load(s + 2, 0);
      step(s + 1, 1);
    }
  }
  if constexpr (WK == 1) {
    // operands of every element first, then the stores (R and out are one buffer in the
    // residual units: a load behind a store would wait for it)
    EncOps4 ops[MT][NS];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NS; ++j)
        ops[i][j] = enc_gemm_ops4(a, m0 + 16 * i + 4 * g, min(n0 + 16 * j + c, a.Tout - 1));
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        const int n = n0 + 16 * j + c;
        if (n < a.Tout) enc_gemm_store4(a, acc[i][j], m0 + 16 * i + 4 * g, n, ops[i][j]);
      }
  } else {
    // deterministic cross-wave K reduction through LDS: tile [BN][BM] per wave, 4 consecutive
    // channels per 16-byte piece
    __shared__ f32x4 red[WK][BN * BM / 4];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NS; ++j) red[wk][(16 * j + c) * (BM / 4) + 4 * i + g] = acc[i][j];
    __syncthreads();
    for (int e = threadIdx.x; e < BN * BM / 4; e += WK * 64) {
      const int nn = e / (BM / 4), mq = e - nn * (BM / 4);
      const int n = n0 + nn;
      if (n >= a.Tout) continue;
      f32x4 v = red[0][e];
#pragma unroll
      for (int w = 1; w < WK; ++w) v += red[w][e];
      const int m = m0 + 4 * mq;
      enc_gemm_store4(a, v, m, n, enc_gemm_ops4(a, m, n));
    }
  }
}

// ---------------------------------------------------------------------------------
// Residual vector quantiser, one launch per level (the levels are sequential: each works on
// the residual the coarser one left).  Level i has stride st = 4 >> i and n_frames << i
// positions; one 256-thread block per position:
//   r = mean of the residual over the position's st latents; e = in_proj(r) (768 -> 8);
//   en = e / max(|e|, 1e-12); code = argmax_r -( |en|^2 - 2 en . cn_r + |cn_r|^2 ), smallest
//   index on ties (cn: the codebook normalised once at finalize; 128 KB, read from L2);
//   zq = out_proj(codebook[code]); the st latents -= zq; the code goes to its slot of the
//   speechpipe frame (the inverse of snac_embed_kernel's de-interleave).
// ---------------------------------------------------------------------------------
template <int ST>
__global__ __launch_bounds__(256) void enc_quant_kernel(EncQuantArgs a) {
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  float* res = a.res + (size_t)p * ST * 768;
  __shared__ float part[4][8];
  __shared__ unsigned long long best_s[4];
  float r[3], acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int ch = tid + 256 * q;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < ST; ++j) s += res[j * 768 + ch];
    r[q] = s * (1.0f / ST);
  }
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = fmaf(a.in_w[k * 768 + tid + 256 * q], r[q], acc[k]);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float s = wave_sum(acc[k]);
    if (lane == 0) part[wid][k] = s;
  }
  __syncthreads();
  float en[8], n2 = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    en[k] = a.in_b[k] + (((part[0][k] + part[1][k]) + part[2][k]) + part[3][k]);
    n2 = fmaf(en[k], en[k], n2);
  }
  const float inv = 1.0f / fmaxf(sqrtf(n2), 1e-12f);
  float e2 = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    en[k] *= inv;
    e2 = fmaf(en[k], en[k], e2);
  }
  unsigned long long best = 0ull;
  for (int row = tid; row < 4096; row += 256) {
    const float4 lo = *reinterpret_cast<const float4*>(a.cn + row * 8);
    const float4 hi = *reinterpret_cast<const float4*>(a.cn + row * 8 + 4);
    float d = en[0] * lo.x;
    d = fmaf(en[1], lo.y, d); d = fmaf(en[2], lo.z, d); d = fmaf(en[3], lo.w, d);
    d = fmaf(en[4], hi.x, d); d = fmaf(en[5], hi.y, d); d = fmaf(en[6], hi.z, d);
    d = fmaf(en[7], hi.w, d);
    const float dist = (e2 - 2.0f * d) + a.cn2[row];
    const unsigned long long key = argmax_key(-dist, (uint32_t)row);
    best = key > best ? key : best;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(best, m, MX_WAVE);
    best = o > best ? o : best;
  }
  if (lane == 0) best_s[wid] = best;
  __syncthreads();
  best = best_s[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) best = best_s[w] > best ? best_s[w] : best;
  const int code = min(max((int)argmax_index(best), 0), 4095);  // (a NaN latent leaves no key)
  float cbv[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) cbv[k] = a.cb[code * 8 + k];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int ch = tid + 256 * q;
    const float4 lo = *reinterpret_cast<const float4*>(a.out_w + ch * 8);
    const float4 hi = *reinterpret_cast<const float4*>(a.out_w + ch * 8 + 4);
    float z = a.out_b[ch];
    z = fmaf(lo.x, cbv[0], z); z = fmaf(lo.y, cbv[1], z); z = fmaf(lo.z, cbv[2], z);
    z = fmaf(lo.w, cbv[3], z); z = fmaf(hi.x, cbv[4], z); z = fmaf(hi.y, cbv[5], z);
    z = fmaf(hi.z, cbv[6], z); z = fmaf(hi.w, cbv[7], z);
#pragma unroll
    for (int j = 0; j < ST; ++j) res[j * 768 + ch] -= z;
  }
  if (tid == 0) {
    int f, slot;
    if (ST == 4) {
      f = p; slot = 0;
    } else if (ST == 2) {
      f = p >> 1; slot = (p & 1) ? 4 : 1;
    } else {
      const int off[4] = {2, 3, 5, 6};
      f = p >> 2; slot = off[p & 3];
    }
    a.frames[7 * f + slot] = code;
  }
}

__global__ __launch_bounds__(256) void enc_codebook_norm_kernel(const float* cb, float* cn,
                                                                float* cn2) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= 4096) return;
  float v[8], n2 = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    v[k] = cb[row * 8 + k];
    n2 = fmaf(v[k], v[k], n2);
  }
  const float inv = 1.0f / fmaxf(sqrtf(n2), 1e-12f);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    v[k] *= inv;
    cn[row * 8 + k] = v[k];
    s = fmaf(v[k], v[k], s);
  }
  cn2[row] = s;
}

// ---------------------------------------------------------------------------------
hipError_t launch_enc_stem(const float* audio, int64_t n_samples, const float* w, const float* b,
                           float* out, int T, hipStream_t st) {
  if (T < 1 || n_samples < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(enc_stem_kernel, dim3((T + 63) / 64), dim3(192), 0, st, audio, n_samples, w,
                     b, out, T);
  return hipGetLastError();
}

hipError_t launch_enc_dwconv(const float* x, float* y, const float* w, const float* b,
                             const float* alpha_in, const float* alpha_out, int C, int T, int dil,
                             hipStream_t st) {
  if (dil < 1 || dil > 9 || C % 48 || T < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(enc_dwconv_kernel, dim3((T + ENC_DW_TT - 1) / ENC_DW_TT, C / 48), dim3(192),
                     0, st, x, y, w, b, alpha_in, alpha_out, C, T, dil);
  return hipGetLastError();
}

hipError_t launch_enc_gemm(const EncGemmArgs& a, hipStream_t st) {
  if (a.M % 48 || a.Kp % 32 || a.K % 8 || a.C % 8 || a.K > a.Kp || a.Tin < 1 || a.Tout < 1 ||
      a.stride < 1 || a.pad < 0 || (a.Kp / 32) % a.wk)
    return hipErrorInvalidValue;
  const dim3 grid((a.Tout + 31) / 32, a.M / 48);
  switch (a.wk) {
    case 1: hipLaunchKernelGGL(enc_gemm_kernel<1>, grid, dim3(64), 0, st, a); break;
    case 2: hipLaunchKernelGGL(enc_gemm_kernel<2>, grid, dim3(128), 0, st, a); break;
    case 4: hipLaunchKernelGGL(enc_gemm_kernel<4>, grid, dim3(256), 0, st, a); break;
    case 8: hipLaunchKernelGGL(enc_gemm_kernel<8>, grid, dim3(512), 0, st, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_enc_codebook_norm(const float* cb, float* cn, float* cn2, hipStream_t st) {
  hipLaunchKernelGGL(enc_codebook_norm_kernel, dim3(16), dim3(256), 0, st, cb, cn, cn2);
  return hipGetLastError();
}

hipError_t launch_enc_quant(const EncQuantArgs& a, hipStream_t st) {
  if (a.n_frames < 1 || a.level < 0 || a.level > 2) return hipErrorInvalidValue;
  const dim3 grid(a.n_frames << a.level);
  if (a.level == 0) hipLaunchKernelGGL(enc_quant_kernel<4>, grid, dim3(256), 0, st, a);
  else if (a.level == 1) hipLaunchKernelGGL(enc_quant_kernel<2>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(enc_quant_kernel<1>, grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace mx
