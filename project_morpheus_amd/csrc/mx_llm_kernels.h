// Argument blocks and launchers for the decode-step kernels (llm_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mx {

enum { EPI_STORE = 0, EPI_RESID = 1, EPI_SILU = 2, EPI_QKV = 3, EPI_ARGMAX = 4 };
enum { WT_BF16 = 0, WT_FP8 = 1 };  // weight storage: bf16, or OCP e4m3 + fp32 scale per row

constexpr int ATT_S_MIN = 128;      // smallest split (positions) = 4 waves x 32 x 1 chunk
constexpr int ATT_MAX_SPLITS = 256; // splits one launch may merge
constexpr int ATT_MAXG = 4;         // max q-heads per kv-head
constexpr int ATT_MERGE_CHUNK = 16; // splits whose partials the merging block prefetches
constexpr int ATT_QKV_NKC_MAX = 8;  // qkv K ranges the attention sums (AttnArgs::qkv_parts)

// Code grammar (DESIGN.md §3 "Code grammar"): the token a constrained slot puts at position p
// has phase k = (p - origin[slot]) mod phases and may only be an id of
//   A(k) = [base + k * codes + cmin, base + (k + 1) * codes)  plus {stop} when k == 0.
// origin[slot] < 0 (or origin == null: no grammar on the context) leaves the slot unconstrained.
struct GrammarArgs {
  const int32_t* origin;   // per KV slot: the prefill's length, or -1; null = no grammar
  int base, codes, phases, cmin, stop;
};
#ifdef __HIPCC__
// A row's allowed set as (lo, stop): ids [lo, lo + codes - cmin) and `stop` (-1: none);
// lo < 0 = unconstrained.  `pos` is the position of the row's input token: the token picked
// takes pos + 1.
struct GrammarSpan {
  int lo, stop;
};
__device__ __forceinline__ GrammarSpan grammar_span(const GrammarArgs& g, int origin, int pos) {
  GrammarSpan s{-1, -1};
  if (origin >= 0) {
    int k = (pos + 1 - origin) % g.phases;
    k += k < 0 ? g.phases : 0;
    s.lo = g.base + k * g.codes + g.cmin;
    s.stop = k == 0 ? g.stop : -1;
  }
  return s;
}
// the span back from its first id alone (phase 0 is the only one that starts at base + cmin)
__device__ __forceinline__ GrammarSpan grammar_span_of(const GrammarArgs& g, int lo) {
  return GrammarSpan{lo, lo == g.base + g.cmin ? g.stop : -1};
}
__device__ __forceinline__ int grammar_origin(const GrammarArgs& g, int slot) {
  return g.origin ? g.origin[slot] : -1;
}
__device__ __forceinline__ bool grammar_allows(const GrammarArgs& g, const GrammarSpan& s, int id) {
  return s.lo < 0 || (unsigned)(id - s.lo) < (unsigned)(g.codes - g.cmin) || id == s.stop;
}
#endif

struct GemvArgs {
  const void* W;           // [N][K] bf16 (WT_BF16) or e4m3 bytes (WT_FP8), packed row order
  const void* Wf;          // null, or the same matrix fragment-major (launch_frag_major) for R >= 2
  int wf_t0, wf_T;         // Wf of a row window: its first 16-row tile and the tile count of the
                           // whole matrix (the bf16 copy is sub-chunk-major over all tiles); 0, 0 = all
  const float* wscale;     // WT_FP8: dequant scale per row [N]
  int wdtype;
  int N, K;
  const float* X;          // activations, row r at X + r * xstride
  int xstride;
  int R;                   // activation rows
  const float* norm_w;     // RMSNorm weight [K] (NORM prologue)
  float eps;
  float* Y;                // STORE [R][N]; RESID [R][ystride] += ; SILU [R][N/2]
  int ystride;
  int max_blocks;          // grid cap (0 = default)
  int force_legacy;        // 1: use the grid-stride kernel even for R = 1 (A/B timing)
  int wpb;                 // R = 1 kernel: waves per block (4 or 8; 0 = 8)
  int gemv_cus;            // R = 1 kernel, option gemv_balance: CU count to balance the qkv /
                           // merging o-proj grids over (0 = off)
  int rpw;                 // R = 1 kernel: weight rows per wave (0 = default per epilogue)
  float* ws;               // R >= 2 kernel: split-K partial tiles (gemm_rows_workspace)
  size_t ws_floats;
  int* tickets;            // R >= 2 kernel: per-tile arrival counters (zero between launches)
  size_t tickets_n;
  int rows_lds_pad;        // R >= 2 kernel: extra dynamic LDS KB per block (occupancy probe; 0 = none)
  int rows_pw;             // generation 4: weight prefetch distance in sub-chunks (1, 2; 0 = 1)
  int rows_pw_f8;          // the same for e4m3 weights
  int rows_target;         // generation 4: blocks the K-range split aims for (0 = per shape)
  int rows_nt_max;         // generation 4: largest batch tile in 16-row units (0 = 4)
  int rows_head_target;    // generation 4: K-range target of the lm_head (0 = the default 192)
  int rows_head_mt;        // R >= 2 lm_head: weight rows per wave in 16-row units (1 or 2)
  int rows_atomic;         // generation 4, residual projections split over K: every K range
                           // adds its partial tile into Y with float atomics (no seam)
  float* qkv_parts;        // generation 4 EPI_QKV, decode: null, or [nkc][R][N] -- every K range
  float* qkv_ss;           // stores its raw partial (and [nkc][R] partial sums of squares);
                           // the attention launch sums them, scales, RoPEs and appends K / V
  unsigned long long* trace;  // generation 4 diagnostic: [block][8] phase stamps (null = off)
  int trace_cap;           // blocks the trace buffer holds (stamps of later blocks are dropped)
  int head_b1;             // R = 1 lm_head on the persistent kernel (head_b1.hip; 0 = gemv_kernel)
  // EPI_QKV
  const float* rope_cos;   // [max_pos][64]
  const float* rope_sin;
  const int32_t* row_slot;
  const int32_t* row_pos;
  uint16_t* kcache;        // this layer: [slots][kv_heads][max_pos * 128], 32-position chunks (kv_k_off)
  uint16_t* vcache;
  int heads, kv_heads, max_pos;
  float* Q;                // [R][heads][128]
  // R = 1 o-proj: merge the attention split partials in the prologue (attn no_merge mode)
  const float* att_ml;     // [kv_heads][att_stride][grp][2]  (m, l) per split, row 0
  const float* att_acc;    // [kv_heads][att_stride][grp][128]
  int att_S, att_stride;   // split length (positions) and partial slots per kv head
  int att_nsm;             // splits the launch may have to merge (host bound, <= 8)
  // EPI_ARGMAX.  The launch may cover a row window of the lm_head: weight row n is id id0 + n,
  // and `seen`, `logits` and the argmax key are indexed by id with the vocabulary V as stride
  // (launch_gemv sets V = N when it is 0).  Rows of constrained slots skip ids outside their
  // allowed set (`gram`; row_pos gives the phase).
  int id0, V;
  GrammarArgs gram;
  const uint8_t* seen;     // [slots][V]
  const float* penalty;    // repetition penalty per KV slot [slots]
  const float* samp_temp;  // sampling temperature per KV slot (> 0: the row samples)
  unsigned long long* best;  // [R]
  float* logits;           // penalised logits [R][V], kept for sampling rows (or every row)
  int logits_all;          // 1: keep every row's logits (parity / debug reads)
};

struct AttnArgs {
  const float* Q;          // [R][heads][128]
  const uint16_t* kcache;  // this layer
  const uint16_t* vcache;  // the same, V chunks in P.V fragment order (kv_v_off)
  const int32_t* row_slot;
  const int32_t* row_pos;
  int heads, kv_heads, max_pos;
  int cpw;                 // 32-position chunks per wave: split = 32 * nw * cpw positions
  int nw;                  // waves per block (4 or 8; 0 = 4)
  int split_stride;        // partial slots per (row, kv-head) >= max_pos / split
  float scale;
  float* part_ml;          // [R][kv_heads][nsplit_max][grp][2]  (m, l) per split
  float* part_acc;         // [R][kv_heads][nsplit_max][grp][128]
  int* counter;            // [R][kv_heads] split arrival tickets (zero between launches)
  float* out;              // [R][heads*128]
  int debug;               // timing experiments only (0 in the product path)
  int no_merge;            // 1: every split stores its partial, the consumer merges (R = 1)
  // multi-row decode with the qkv GEMM's K-range partials (GemvArgs::qkv_parts): q / k / v of
  // the new position = RoPE(rsqrt(mean x^2 + eps) x sum of the partials), K / V appended here
  const float* qkv_parts;  // [nkc][R][qkv_n] raw partial sums, packed wqkv row order (null: off)
  const float* qkv_ss;     // [nkc][R] partial sums of squares of the qkv input
  int qkv_nkc, qkv_n, hidden;
  float eps;
  const float* rope_cos;   // [max_pos][64]
  const float* rope_sin;
};

struct CommitArgs {
  unsigned long long* best;  // [R]
  const int32_t* dst_row;    // optional remap
  int32_t* row_slot;
  int32_t* row_pos;
  int32_t* row_token;
  uint8_t* seen;
  int32_t* hist;             // host-mapped [slots][max_pos]
  const uint16_t* embed;
  float* h;
  int hidden, vocab, max_pos, pos_advance;
  int scratch_slot;          // rows bound to this slot are parked: no advance, no history
  const int* abort_word;     // null, or the persistent engine's host-mapped status: when set,
                             // nothing is committed and the history entry reads -1
  // penalty window (last_n[slot] = N > 0): the slot's seen bytes are counts of the ids at the
  // last N positions, recent[slot] is the ring of those ids (cell = position & 255)
  const int32_t* last_n;     // [slots]
  int32_t* recent;           // [slots][PEN_RING]
};
constexpr int PEN_RING = 256;  // ring cells per slot: the window is at most PEN_RING - 1 ids


hipError_t gemv_prepare(int kmax);
hipError_t launch_gemv(const GemvArgs& a, int epi, bool norm, hipStream_t st);
// R = 1 lm_head + penalty + argmax, persistent (head_b1.hip); hipErrorNotSupported off K = 3072
hipError_t launch_head_b1(const GemvArgs& a, hipStream_t st);
namespace v4 {  // multi-row GEMM generation 4 (mx_rows_v4.inc)
hipError_t launch_gemm_rows_v4(const GemvArgs& a, int epi, bool norm, hipStream_t st);
void gemm_rows_workspace_v4(int N, int K, int R, int epi, size_t* ws_floats, size_t* tickets);
// the multi-row o-projection can merge the attention splits itself (attn no_merge)
bool rows_merge_ok_v4(const GemvArgs& o);
// K ranges the qkv launch (EPI_QKV, NORM) of these arguments splits into
int rows_qkv_nkc_v4(const GemvArgs& a);
}  // namespace v4
struct SampleArgs {
  const float* logits;     // [R][V] penalised logits (kept by the lm_head epilogue)
  const int32_t* row_slot; // [R]
  const int32_t* row_pos;  // [R] position of the row's input token (RNG counter)
  const float* temp;       // per KV slot: temperature (<= 0: greedy, kernel returns)
  const float* top_p;      // per KV slot
  const uint32_t* seed;    // per KV slot: Philox key (lo, hi)
  unsigned long long* best;  // [R] argmax-key encoded token (read by commit)
  int V;
  GrammarArgs gram;        // constrained rows sweep their allowed span only
};
hipError_t launch_sample(const SampleArgs& a, int R, hipStream_t st);
// the sampler with the top-k / min-p filters in front of the nucleus (sample_chain_kernel)
struct SampleChainArgs {
  SampleArgs s;
  const int32_t* top_k;    // per KV slot: 0 = no limit
  const float* min_p;      // per KV slot: 0 = off
};
hipError_t launch_sample_chain(const SampleChainArgs& a, int R, hipStream_t st);
// best[0] = argmax key of logits over the ids [lo, lo + n) and `stop` (-1: none): the smallest
// index among equal maxima
hipError_t launch_argmax_row(const float* logits, int lo, int n, int stop,
                             unsigned long long* best, hipStream_t st);
hipError_t launch_set_slot_origin(int32_t* origin, int slot, int value, hipStream_t st);
hipError_t launch_set_slot_params(float* penalty, float* temp, float* top_p, uint32_t* seed,
                                  int slot, float pen, float t, float p, uint64_t s,
                                  hipStream_t st);
hipError_t launch_set_slot_ext(int32_t* top_k, float* min_p, int32_t* last_n, int slot, int k,
                               float mp, int n, hipStream_t st);
// window mode prefill: counts and ring of the last min(n, N) prompt ids (one block, serial)
hipError_t launch_window_prefill(const int32_t* ids, int n, int N, int slot, int vocab,
                                 uint8_t* seen, int32_t* recent, hipStream_t st);
hipError_t launch_set_rows(int32_t* slot, int32_t* pos, int n, int slot_val, int pos0,
                           hipStream_t st);
hipError_t launch_set_scalar(float* p, float v, hipStream_t st);
hipError_t launch_move_row(int32_t* slot, int32_t* pos, int32_t* token, float* h, int hidden,
                           int dst, int src, int scratch, hipStream_t st);
hipError_t launch_attention(const AttnArgs& a, int R, int max_len, hipStream_t st);
hipError_t launch_commit(const CommitArgs& a, int R, hipStream_t st);
hipError_t launch_embed_rows(const int32_t* ids, int n, int slot, const uint16_t* embed,
                             int hidden, int vocab, uint8_t* seen, float* h, hipStream_t st);
hipError_t launch_scatter_rows(void* dst, const void* src, const int32_t* dmap, int rows,
                               int cols, int mode, hipStream_t st);

// ---- packed prefill (mx_llm_prefill_batch): several prompts as one row set -----------
// The host uploads one table per call: a PackSeg per segment, then a PackRow per prompt row
// (segment after segment).  Every kernel below reads it from device memory.
struct PackSeg {
  int32_t slot, row;       // KV slot, decode row the stream is bound to
  int32_t first, n;        // the segment's rows: [first, first + n) of the row set
  int32_t origin;          // grammar origin of the slot (pos0 + n, or -1: unconstrained)
  int32_t top_k, last_n;   // extras (0 = neutral)
  float pen, temp, top_p, min_p;
  uint32_t seed_lo, seed_hi;
  int32_t pos0;            // positions the slot holds in front of the rows (mx_llm_prefill_pack)
  int32_t hist;            // ... whose ids [0, pos0) start here in the staged histories
  int32_t pad;
};
static_assert(sizeof(PackSeg) == 64, "PackSeg is uploaded as 16 words");
struct PackRow {
  int32_t id, slot, pos;
  int32_t mark;            // 1: whole-sequence penalty, the row marks seen[slot][id]
};
static_assert(sizeof(PackRow) == 16, "PackRow is uploaded as 4 words");
struct PackSetupArgs {
  const PackRow* rows;
  const PackSeg* segs;
  int R, n_segs;
  const uint16_t* embed;
  int hidden, vocab;
  uint8_t* seen;           // [slots][vocab]
  float* h;                // [R][hidden] prompt rows (h_pre)
  int32_t *pre_slot, *pre_pos;
  // per KV slot generation state, written for every segment's slot
  float *penalty, *temp, *top_p;
  uint32_t* seed;
  int32_t* top_k;
  float* min_p;
  int32_t* last_n;
  int32_t* origin;         // null: the context has no grammar
};
struct PackTailArgs {
  const PackSeg* segs;
  const float* h;          // [R][hidden] prompt rows after the layers
  int hidden;
  float* head_h;           // [n_segs][hidden] the segments' last rows, contiguous
  int32_t *head_slot, *head_pos, *head_row;  // [n_segs] (head_row: the commit's dst_row)
  unsigned long long* head_best;             // [n_segs], zeroed
  int32_t *row_slot, *row_pos;               // decode rows: bound to (slot, n - 1)
};
// zero the seen bytes and the penalty ring of every segment's slot (one launch)
hipError_t launch_pack_clear(const PackSeg* segs, int n_segs, int vocab, uint8_t* seen,
                             int32_t* recent, hipStream_t st);
// per row: pre_slot / pre_pos, the embedding gather and the seen mark; per segment: the slot's
// generation parameters, extras and grammar origin (one launch, grid R + n_segs)
hipError_t launch_pack_setup(const PackSetupArgs& a, hipStream_t st);
// window counts and ring of every windowed segment (last_n > 0; one block each, serial) over
// positions max(0, pos0 + n - last_n) .. pos0 + n - 1: below pos0 from `hist` (the staged
// histories; null when no segment has one), from there on from the rows
hipError_t launch_pack_window(const PackRow* rows, const PackSeg* segs, const int32_t* hist,
                              int n_segs, int vocab, uint8_t* seen, int32_t* recent,
                              hipStream_t st);
// seen[slot][hist[seg.hist + i]] = 1, i < pos0, for every whole-sequence segment (last_n = 0)
// behind a history (one launch; max_pos0 sizes the grid)
hipError_t launch_pack_hist_marks(const PackSeg* segs, const int32_t* hist, int n_segs,
                                  int max_pos0, int vocab, uint8_t* seen, hipStream_t st);
hipError_t launch_pack_tail(const PackTailArgs& a, int n_segs, hipStream_t st);
// dst[rows[k]][0, V) = src[k][0, V): the kept logits to the decode rows' own lines
hipError_t launch_pack_logits(float* dst, const float* src, const int32_t* rows, int n_segs,
                              int V, hipStream_t st);
// ---- prompt continuation (mx_llm_prefill_chunk / mx_llm_fork_slot) --------------------
struct KvForkArgs {
  uint16_t* kcache;        // all layers: [layers][slots][kv_heads][max_pos * 128]
  uint16_t* vcache;
  size_t kv_layer_elems;   // elements of one layer
  int layers, kv_heads, max_pos;
  int src, dst;            // KV slots
  int chunks;              // 32-position chunks copied per block: ceil(n_pos / 32)
  int runs;                // 2 * layers * kv_heads
};
// dst's first `chunks` chunks of every (K | V, layer, kv head) block = src's (one launch; the
// grid is sized from `cus`).  hipErrorInvalidValue on chunks outside [1, max_pos / 32] or
// src == dst.
hipError_t launch_kv_fork(const KvForkArgs& a, int cus, hipStream_t st);
// n forks in one launch (mx_llm_fork_slots): the fork table is read from device memory
struct KvFork {
  int32_t dst, src;        // KV slots
  int32_t chunks;          // ceil(n_pos / 32)
  int32_t pad;
};
static_assert(sizeof(KvFork) == 16, "KvFork is uploaded as 4 words");
struct KvForkManyArgs {
  uint16_t* kcache;
  uint16_t* vcache;
  size_t kv_layer_elems;
  int layers, kv_heads, max_pos;
  int runs;                // 2 * layers * kv_heads
  const KvFork* forks;     // device, [n]
  int n;
  int max_chunks;          // the largest `chunks` of the table
};
// hipErrorInvalidValue on n < 1 or max_chunks outside [1, max_pos / 32]; the caller has checked
// the table (slots in range, every dst distinct and no src)
hipError_t launch_kv_fork_many(const KvForkManyArgs& a, int cus, hipStream_t st);
// seen[slot][ids[i]] = 1, i < n (the whole-sequence penalty state from an id history)
hipError_t launch_mark_seen(const int32_t* ids, int n, int slot, int vocab, uint8_t* seen,
                            hipStream_t st);
hipError_t launch_to_f32(float* dst, const void* src, int64_t n, int src_bf16, hipStream_t st);
// [N][K] (esz bytes per element) -> fragment-major copy for the multi-row GEMM (mx_rows_v4.inc)
hipError_t launch_frag_major(const void* src, void* dst, int N, int K, int esz, hipStream_t st);
inline size_t frag_major_bytes(int N, int K, int esz) { return (size_t)((N + 15) / 16) * 16 * K * esz; }

}  // namespace mx
