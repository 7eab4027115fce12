// SNAC 24 kHz encoder + residual vector quantiser kernels (snac_enc_kernels.hip).  fp32
// arithmetic, one recording per call, activations channels-last [time][channels] like the
// decoder's (mx_snac_kernels.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mx {

// "Run" conv-GEMM: on channels-last input the K operands of one output column are one contiguous
// run of floats, out[n][m] = epi( sum_{k < K} A[m][k] Xflat[(stride n - pad) C + k] ), with
// zeros where the run leaves [0, Tin C).  A 1x1 conv is stride 1, pad 0, K = C; the strided
// down-conv Conv1d(C -> 2C, k = 2s, stride s, pad ceil(s/2)) is stride s, K = 2s C with the
// weight repacked [M][tap][C].  A is three bf16 planes [3][M][Kp], Kp = K rounded up to 32
// with zero columns.
struct EncGemmArgs {
  const uint16_t* A;
  const float* X;      // [Tin][C]
  const float* bias;   // [M]
  const float* R;      // residual [Tout][M] added to the result, or null (may be `out`)
  float* out;          // [Tout][M]
  float* out2;         // optional: Snake(out, alpha2) for the next consumer
  const float* alpha2;
  int M, K, Kp, C, Tin, Tout, stride, pad;
  int wk;              // waves splitting K (1, 2, 4, 8; Kp / 32 is a multiple of it)
};
hipError_t launch_enc_gemm(const EncGemmArgs& a, hipStream_t st);

// conv k7 pad 3, 1 -> 48 on audio[n_samples] read as zeros past its end; out [T][48]
hipError_t launch_enc_stem(const float* audio, int64_t n_samples, const float* w, const float* b,
                           float* out, int T, hipStream_t st);
// depthwise k7 dilated conv with Snake on input and output (either alpha may be null), for
// channel counts that are multiples of 48 (the decoder's launch_dwconv takes multiples of 64)
hipError_t launch_enc_dwconv(const float* x, float* y, const float* w, const float* b,
                             const float* alpha_in, const float* alpha_out, int C, int T, int dil,
                             hipStream_t st);

// codebook [4096][8] -> rows scaled to unit length (F.normalize) and their squared lengths
hipError_t launch_enc_codebook_norm(const float* cb, float* cn, float* cn2, hipStream_t st);

struct EncQuantArgs {
  float* res;             // residual [4 n_frames][768], updated in place
  const float* in_w;      // [8][768]
  const float* in_b;      // [8]
  const float* cn;        // normalised codebook [4096][8]
  const float* cn2;       // [4096]
  const float* cb;        // codebook [4096][8]
  const float* out_w;     // [768][8]
  const float* out_b;     // [768]
  int32_t* frames;        // [n_frames][7]
  int n_frames;
  int level;              // 0, 1, 2: stride 4, 2, 1
};
hipError_t launch_enc_quant(const EncQuantArgs& a, hipStream_t st);

}  // namespace mx
