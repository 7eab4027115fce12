/*
 * morpheus_mx.h — C ABI of libmorpheus_mx.so, the MI355X-native Orpheus TTS hot path.
 *
 * Drop-in boundary for the reference's L0 arithmetic.  The reference has
 * no native code of its own; these entry points replace the third-party engines it binds:
 *
 *   mx_llm_*   replaces the Orpheus decoder loop's LLM engine:
 *                vLLM AsyncLLMEngine.generate  Orpheus-TTS/orpheus_tts_pypi/orpheus_tts/engine_class.py:117
 *                (SamplingParams engine_class.py:106-112), llama.cpp Llama(...)/text_to_speech
 *                Morpheus_Client/tts_engine/llama_local.py:42-52,77, and the remote
 *                /v1/completions stream Morpheus_Client/tts_engine/remote_backend.py:64-117.
 *   mx_snac_enc_*  replaces snac.SNAC.encode(audio) (third-party snac 1.2.x): reference audio
 *                -> the speech codes of a voice prompt.
 *   mx_snac_*  replaces snac.SNAC.decode(codes) + slice + PCM16 in convert_to_audio
 *                Morpheus_Client/tts_engine/speechpipe.py:76-129 (model load :41-49).
 *
 * Conventions: return 0 on success, a negative code on error (message via *_last_error);
 * no exceptions cross the ABI.  All device I/O pointers are caller-owned device memory (or
 * host-mapped memory from mx_host_alloc); weights passed to *_set_weight are copied and
 * packed into context-owned storage.  Streams are hipStream_t passed as void*.  One context
 * per (GPU, host thread); contexts are not re-entrant.  The host engine calls these from
 * its own thread (never from the asyncio event loop), mirroring llama_local.py:79.
 */
#ifndef MORPHEUS_MX_H
#define MORPHEUS_MX_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MX_OK 0
#define MX_ERR_ARG (-1)
#define MX_ERR_HIP (-2)
#define MX_ERR_STATE (-3)
#define MX_ERR_OOM (-4)

#define MX_DTYPE_F32 0
#define MX_DTYPE_BF16 1
#define MX_DTYPE_FP8 2   /* OCP e4m3 (e4m3fn) bytes */

#define MX_WEIGHTS_BF16 0
#define MX_WEIGHTS_FP8 1 /* e4m3 matrices + one fp32 dequant scale per output row */

typedef struct mx_llm mx_llm;
typedef struct mx_snac mx_snac;
typedef struct mx_snac_enc mx_snac_enc;

/* Llama-3 decoder shape (Orpheus-3B: 3072/28/24/8/128/8192/156940), limits and eps. */
typedef struct mx_llm_config {
  int32_t hidden, layers, heads, kv_heads, head_dim, ffn, vocab;
  int32_t max_slots;    /* concurrent utterance streams (KV slots) */
  int32_t max_pos;      /* positions per slot (n_ctx, llama_local.py:45) */
  int32_t max_batch;    /* decode rows per step */
  int32_t max_prefill;  /* prompt tokens per prefill call */
  float eps;            /* RMSNorm eps (1e-5) */
  int32_t tied;         /* lm_head shares the embedding table */
  int32_t wdtype;       /* MX_WEIGHTS_BF16 | MX_WEIGHTS_FP8 (BASELINE configs[4]) */
} mx_llm_config;

/* Per-stream generation parameters (engine_class.py:106-112 SamplingParams; inference.py:75-105).
 * temperature <= 0 selects greedy decoding (argmax after the penalty; the parity mode).
 * Otherwise: logits / temperature -> nucleus of mass top_p -> one draw from a Philox4x32-10
 * stream keyed by `seed` and counted by position (definition in csrc/sample_kernels.hip). */
typedef struct mx_sampling {
  float temperature;
  float top_p;
  float repetition_penalty; /* HF/vLLM rule on the prompt + generated set (1.1 in Orpheus) */
  uint64_t seed;
} mx_sampling;

/* Optional extras of a stream (mx_llm_prefill_ex); all zero = neutral = mx_llm_prefill.
 * Order: temperature, then top_k and min_p, then top_p (vLLM's order).  top_k keeps the k most
 * probable ids (ties at the k-th kept together), min_p the ids with probability >= min_p x the
 * top probability; the nucleus mass is taken over what they leave.  penalty_last_n = N > 0
 * applies the repetition penalty to the ids at the last N positions only (prompt included);
 * 0 = the whole sequence.  N <= 255: the window is kept as byte counts. */
typedef struct mx_sampling_ext {
  int32_t top_k;
  float min_p;
  int32_t penalty_last_n;
} mx_sampling_ext;

/* Code grammar of a context (mx_llm_set_grammar; DESIGN.md §3 "Code grammar").  The token a
 * constrained slot puts at position p has phase k = (p - origin) mod phases, origin = the length
 * of the slot's prefill, and may only be an id of
 *   A(k) = [code_base + k*codes + code_min, code_base + (k+1)*codes), plus stop_id when k == 0
 * (stop_id < 0: no stop id).  Every other id behaves as a logit of -inf, in front of the
 * repetition penalty, temperature, top-k / min-p, top-p and the draw.  Orpheus:
 * (128266, 4096, 7, 1, 128258) -- seven SNAC code ranges, code 0 excluded (the reference
 * pipeline drops it, speechpipe.py:146-189), end-of-speech on frame boundaries only. */
typedef struct mx_code_grammar {
  int32_t code_base, codes, phases, code_min, stop_id;
} mx_code_grammar;

/* ---- library / memory -------------------------------------------------------------- */
const char* mx_version(void);
int mx_host_alloc(size_t bytes, void** host_ptr, void** dev_ptr); /* pinned, device-mapped */
int mx_host_free(void* host_ptr);

/* ---- LLM decoder (replaces vLLM / llama.cpp decode) -------------------------------- */
int mx_llm_create(int device, const mx_llm_config* cfg, mx_llm** out);
/* names: embed, norm, lm_head (untied), l{i}.{attn_norm,wq,wk,wv,wo,mlp_norm,wg,wu,wd}.
 * MX_WEIGHTS_FP8 engines: every matrix but embed comes as MX_DTYPE_FP8 bytes plus
 * "<name>.scale" (fp32, one per output row: W = scale[row] * e4m3); lm_head is always given
 * (the tied embedding stays bf16 for the token lookup). */
int mx_llm_set_weight(mx_llm* ctx, const char* name, const void* dev_data, int64_t numel,
                      int dtype);
/* RoPE tables [n_pos][head_dim/2] fp32 (host memory), llama3-scaled frequencies. */
int mx_llm_set_rope(mx_llm* ctx, const float* cos_host, const float* sin_host, int n_pos);
/* Checks every weight is present and builds the fragment-major copies the multi-row GEMM
 * streams (2x the matrix bytes in HBM).  Weights are frozen afterwards: mx_llm_set_weight
 * then returns MX_ERR_STATE. */
int mx_llm_finalize(mx_llm* ctx);
/* Prefill prompt ids (host) into `slot`, bind the slot to decode row `row`, set the slot's
 * generation parameters, pick the first token.  Enqueued on `stream`. */
int mx_llm_prefill(mx_llm* ctx, int slot, int row, const int32_t* ids_host, int n_ids,
                   const mx_sampling* params, void* stream);
/* The same with the extras (`ext` NULL = neutral).  MX_ERR_ARG on top_k < 0, min_p outside
 * [0, 1] or NaN, penalty_last_n outside [0, 255].  Every prefill resets the slot's penalty
 * state, so whole-sequence and windowed requests may follow each other on one slot. */
int mx_llm_prefill_ex(mx_llm* ctx, int slot, int row, const int32_t* ids_host, int n_ids,
                      const mx_sampling* params, const mx_sampling_ext* ext, void* stream);
/* Packed prefill: admit n_segs streams in ONE pass over the weights.  The prompts' rows run
 * the layers as one row set (R = sum of n_ids), one lm_head launch covers the n_segs last rows,
 * one sampler node picks every first token.  Afterwards the context is in the state n_segs
 * calls of mx_llm_prefill_ex in segment order would leave, up to fp32 summation order: KV,
 * penalty state, slot parameters and extras, grammar origins (per mx_llm_set_slot_grammar), row
 * bindings, first tokens, history, next inputs, and mx_llm_read_logits(row).  Every check runs
 * before anything is enqueued, so a refused call leaves the context as it was: MX_ERR_ARG on
 * n_segs outside [1, max_batch], sum n_ids > max_prefill, an n_ids < 1 or >= max_pos, a slot or
 * row out of range or named twice, an id out of vocab, or sampling values mx_llm_prefill_ex
 * refuses; MX_ERR_STATE before finalize.
 * Layout (64-bit ABI; checked by the static_assert below and by the ctypes binding):
 *   offset 0 slot, 4 row, 8 ids_host, 16 n_ids, 24 params (24 bytes), 48 ext (12 bytes);
 *   sizeof 64. */
typedef struct mx_prefill_seg {
  int32_t slot, row;          /* KV slot, decode row the stream is bound to */
  const int32_t* ids_host;    /* prompt ids (host) */
  int32_t n_ids;
  mx_sampling params;
  mx_sampling_ext ext;        /* all zero = neutral */
} mx_prefill_seg;
#ifdef __cplusplus
static_assert(sizeof(void*) != 8 ||
                  (sizeof(mx_prefill_seg) == 64 && offsetof(mx_prefill_seg, row) == 4 &&
                   offsetof(mx_prefill_seg, ids_host) == 8 && offsetof(mx_prefill_seg, n_ids) == 16 &&
                   offsetof(mx_prefill_seg, params) == 24 && offsetof(mx_prefill_seg, ext) == 48),
              "mx_prefill_seg layout");
#endif
int mx_llm_prefill_batch(mx_llm* ctx, const mx_prefill_seg* segs, int n_segs, void* stream);
/* Prompt continuation (DESIGN.md §3 "Prompt continuation"): a prompt given as chunks
 * c_0 .. c_m, chunk c_j at pos0 = |c_0| + .. + |c_{j-1}| and the last one marked `last`, leaves
 * the slot, the row, the penalty state, the grammar origin and the sampler counters as ONE
 * prefill of the concatenated ids would, up to float summation order inside the layer kernels
 * and the bf16 KV rounding that follows from it.  A chunk with last = 0 records its ids in the
 * slot's id history, runs the layers and appends K / V: no head, sampler or commit, no row bound,
 * `row`, `params` and `ext` not read.  The chunk with last = 1 builds the penalty state from the
 * history over [0, pos0 + n_ids) (whole sequence, or the window of the last N positions, which may
 * straddle a seam), sets the grammar origin to pos0 + n_ids, picks the first token (Philox
 * counter of position pos0 + n_ids) and binds `row` there.  pos0 = 0 with last = 1 is
 * mx_llm_prefill_ex; pos0 = 0 starts the slot over.
 * The library mirrors on the host how many prompt positions every slot holds (mx_llm_slot_len;
 * set by every prefill entry point and by mx_llm_fork_slot).  Every check runs before anything
 * is enqueued, so a refused call leaves the context as it was: MX_ERR_ARG on a slot (or, last,
 * a row) out of range, n_ids outside [1, max_prefill], pos0 < 0 or pos0 + n_ids >= max_pos, an id
 * out of vocab, sampling values mx_llm_prefill_ex refuses (last only), or a context one attention
 * launch cannot merge; MX_ERR_STATE on pos0 > 0 that is not the slot's length, on a slot bound to
 * an active row, and before finalize.
 * Layout (64-bit ABI): offset 0 slot, 4 row, 8 ids_host, 16 n_ids, 20 pos0, 24 last,
 *   32 params (24 bytes), 56 ext (12 bytes); sizeof 72. */
typedef struct mx_prefill_chunk {
  int32_t slot, row;          /* row is read only when last != 0 */
  const int32_t* ids_host;
  int32_t n_ids;
  int32_t pos0;               /* positions the slot already holds */
  int32_t last;               /* 0: layers + KV only; 1: ends the prompt */
  mx_sampling params;         /* read only when last != 0 */
  mx_sampling_ext ext;
} mx_prefill_chunk;
#ifdef __cplusplus
static_assert(sizeof(void*) != 8 ||
                  (sizeof(mx_prefill_chunk) == 72 && offsetof(mx_prefill_chunk, ids_host) == 8 &&
                   offsetof(mx_prefill_chunk, n_ids) == 16 && offsetof(mx_prefill_chunk, pos0) == 20 &&
                   offsetof(mx_prefill_chunk, last) == 24 && offsetof(mx_prefill_chunk, params) == 32 &&
                   offsetof(mx_prefill_chunk, ext) == 56),
              "mx_prefill_chunk layout");
#endif
int mx_llm_prefill_chunk(mx_llm* ctx, const mx_prefill_chunk* chunk, void* stream);
/* Fork: `dst_slot` holds `src_slot`'s first n_pos positions afterwards -- K / V of every layer
 * (one device copy, ordered on `stream`) and the id history; no penalty state (the request's
 * final chunk builds it).  `src_slot` may be an unbound template slot or bound to a live row:
 * its first n_pos <= mx_llm_slot_len positions are immutable.  MX_ERR_STATE (nothing enqueued,
 * nothing changed) on a slot out of range, dst == src, n_pos < 1 or above the source's length,
 * or a dst bound to an active row. */
int mx_llm_fork_slot(mx_llm* ctx, int dst_slot, int src_slot, int n_pos, void* stream);
/* Packed continuation (DESIGN.md §3 "Packed continuation"): a pack of FINAL chunks.  Entry j puts
 * n_ids ids onto `slot` behind the pos0 positions it holds (pos0 = 0 starts the slot over) and
 * binds `row`; the layers run once over the sum of the entries' rows.  Afterwards the context
 * is in the state n_chunks calls of mx_llm_prefill_chunk(last = 1) in entry order would leave,
 * up to fp32 summation order: K / V, the penalty state over the whole prompt [0, pos0 + n_ids),
 * slot parameters, grammar origin and sampler counter pos0 + n_ids, the row, the host mirrors.
 * Every check runs before anything is enqueued.  MX_ERR_ARG on what mx_llm_prefill_batch
 * refuses (n_chunks outside [1, max_batch], more than max_prefill rows in all, a slot or row
 * out of range or named twice, an id out of vocab, bad sampling values), on last = 0 (packing
 * non-final chunks is not offered), pos0 < 0, pos0 + n_ids >= max_pos, or a context (rows in
 * all, longest pos0 + n_ids) one attention launch cannot merge; MX_ERR_STATE on pos0 > 0 that is
 * not the slot's mx_llm_slot_len or whose slot is bound to an active row, and before finalize. */
int mx_llm_prefill_pack(mx_llm* ctx, const mx_prefill_chunk* chunks, int n_chunks, void* stream);
/* n forks in one device launch: dst[i] holds src[i]'s first n_pos[i] positions afterwards,
 * exactly as n calls of mx_llm_fork_slot leave them (sources may repeat).  MX_ERR_ARG on n < 1,
 * n > max_slots or a null pointer; MX_ERR_STATE (nothing enqueued, nothing changed) on what
 * mx_llm_fork_slot refuses for any triple, a dst named twice, or a dst that is also a src of
 * the call. */
int mx_llm_fork_slots(mx_llm* ctx, const int32_t* dst, const int32_t* src, const int32_t* n_pos,
                      int n, void* stream);
/* The host mirror: prompt positions `slot` holds (its last prefill's length, the chunks so far,
 * or a fork's n_pos; tokens decoded behind the prompt are not counted). */
int mx_llm_slot_len(const mx_llm* ctx, int slot, int* n_pos);
/* One decode step for rows [0, n_rows), each under its slot's parameters (hipGraph-captured
 * per row count and attention grid; replayed). */
int mx_llm_decode(mx_llm* ctx, int n_rows, void* stream);
/* After the host has waited for a step: MX_ERR_HIP if a persistent-engine launch (option
 * b1_engine) gave up on a bounded wait since the last check.  Such a step commits nothing (its
 * history entry reads -1, the row does not advance); this call waits for `stream`, clears the
 * engine's attention tickets and re-reads the row positions, so the next mx_llm_decode
 * recomputes the step.  mx_llm_decode performs the same check before it enqueues. */
int mx_llm_check(mx_llm* ctx, void* stream);
/* Same step launched eagerly (no graph) with HIP events around every launch; adds the
 * elapsed milliseconds per launch class to ms_by_class[k] (k < n_classes; classes:
 * 0 qkv, 1 attention, 2 o-proj, 3 gate/up, 4 down, 5 lm_head+argmax, 6 commit, 7 the
 * persistent engine launch when option b1_engine is on).
 * Synchronises the stream.  Used by bench.py for the roofline of individual kernels. */
int mx_llm_decode_profiled(mx_llm* ctx, int n_rows, void* stream, double* ms_by_class,
                           int n_classes);
/* Tuning knobs (capi.hip mx_llm_set_option; unknown keys and out-of-range values fail with
 * MX_ERR_ARG): "legacy_gemv", "gemv_wpb", "rpw_o", "rpw_gu", "rpw_down", "head_b1",
 * "o_merge", "att_cpw", "att_nw", "att_cpw_batch", "att_nw_batch", "att_b1_short" (one-row
 * attention may split the context into 64- / 96-position pieces: 2 / 1), "att_b1_nw6" (one-row
 * attention may take 192-position splits on 6-wave blocks past L 1,024), "att_nw6" (multi-row
 * attention may pick 6-wave blocks: the shortest split covering the context), "gemv_balance"
 * (one-row qkv / merging o-proj: the waves per block that load the most loaded CU least), "rows_frag",
 * "rows_merge", "rows_head_mt", "rows_head_target", "grammar_head" (steps whose active rows are
 * all constrained run the lm_head over the grammar's row window only: 1, the default; 0 = always
 * the whole vocabulary with the mask), "rows_target", "rows_target_qkv", "rows_target_o",
 * "rows_target_gu", "rows_target_down" (the target for one kind of layer launch), "rows_nt_max", "rows_nt1",
 * "rows_pw", "rows_pw_f8", "rows_lds_pad", "rows_atomic" (o-proj / down at >= 2 rows: K ranges
 * add into the residual with float atomics, no split-K seam), "rows_qkv_parts" (decode at >= 2
 * rows: the qkv K ranges' raw partials summed, scaled, RoPE'd and appended by the attention
 * launch, no split-K seam), "b1_engine" (one-row steps as ONE persistent
 * launch, engine_b1.hip), "engine_slots" (its LDS ring slots), "engine_depth" (ring slots in
 * flight per loader wave, 2 or 3), "engine_loaders" (loader waves, 1 or 2), "engine_trace" (record the engine's phase timeline),
 * "engine_timeout" (bound of every engine wait, 100 MHz ticks; 0 = 50 ms), "engine_dbg" (timing
 * experiments: 1 = no hand-off waits, 2 = no weight stream; outputs invalid), "bench_one_layer"
 * (diagnostic: the GEMV probes below sweep layer 0 only, its weights resident on die).  Drops
 * the captured graphs so the next mx_llm_decode re-captures with the new choice.
 * One key is a test hook rather than a knob: "debug_poison_att_partials" = 1 fills the attention
 * split partials (m, l, accumulators) with 0xFF bytes -- quiet NaNs -- once, on the call (it
 * waits for the device before and after, keeps the captured graphs, and is part of no step):
 * the steps after it must not let a split slot past the row's live count into their result. */
int mx_llm_set_option(mx_llm* ctx, const char* key, int value);
/* Diagnostic (option engine_trace on): after a device sync, copy the last engine launch's
 * timeline, 12 stamps of the 100 MHz clock per (CU, layer) -- consumer: layer start, input
 * ready, qkv done, attention done, o input ready, o done, gate/up input ready, gate/up done,
 * down input ready, down done; loader: layer start, layer streamed -- into host_out
 * ([grid][layers][12], n entries available); *grid_out = the engine's grid. */
int mx_llm_engine_trace(mx_llm* ctx, uint64_t* host_out, int n, int* grid_out);
/* Roofline probe: mean microseconds per launch of the decode GEMV/GEMM `which` (0 qkv,
 * 1 o-proj, 2 gate/up, 3 down, 4 the one-row o-proj merging 8 attention splits, 5 lm_head +
 * penalty + argmax) for `n_rows` rows (1..max_batch), timed over one hipGraph of
 * `reps` sweeps across all layers' weights (as in a decode step); *bytes_out = weight
 * bytes per launch.  Clobbers decode-row state and KV position 0 of the first n_rows
 * slots: only on an idle context. */
int mx_llm_bench_gemv(mx_llm* ctx, int which, int n_rows, int reps, float* us_out,
                      double* bytes_out);
/* Diagnostic: per-block phase stamps (s_memrealtime, 100 MHz) of the multi-row GEMM launch of
 * mx_llm_bench_gemv's last layer, replayed inside its sweep: host_out[block * 8 + k], k = 0
 * entry, 1 first activation staged, 2 first weight sub-chunk consumed, 3 main loop done,
 * 4 split-K partial published + ticket, 5 K ranges merged, 6 epilogue done (0 = not
 * reached).  n_rows >= 2; *blocks_out = grid size (<= cap_blocks).  The stamps exist only in
 * the diagnostic build (MORPHEUS_MX_ROWS_TRACE=1, libmorpheus_mx_trace.so); the product
 * library returns MX_ERR_STATE. */
int mx_llm_bench_gemv_trace(mx_llm* ctx, int which, int n_rows, uint64_t* host_out,
                            int cap_blocks, int* blocks_out);
/* Diagnostic: mx_llm_bench_gemv's all-layer multi-row sweep (n_rows >= 2; which 0-3, 5)
 * replayed on nstreams (1..4) streams at once, each with its own split-K workspace (values
 * meaningless): wall microseconds per launch of one stream's sweep. */
int mx_llm_bench_gemv_streams(mx_llm* ctx, int which, int n_rows, int reps, int nstreams,
                              float* us_out);
/* Diagnostic: mean microseconds of one eager attention launch (layer 0) for n_rows rows of
 * length L, `cpw` 32-position chunks per wave (split = 128*cpw), experiment flags `debug`
 * (0 = product kernel).  Clobbers decode-row state: only on an idle context. */
int mx_llm_bench_attention(mx_llm* ctx, int L, int n_rows, int cpw, int debug, int reps,
                           float* us_out);
/* Set (or, with NULL, clear) the context's code grammar.  After finalize, on an idle context:
 * MX_ERR_STATE while any row is active.  MX_ERR_ARG on phases < 1, codes < 1, code_min outside
 * [0, codes), code_base < 0, code_base + phases*codes > vocab, a stop_id inside a code range or
 * >= vocab.  Clears every slot's flag and drops the captured graphs. */
int mx_llm_set_grammar(mx_llm* ctx, const mx_code_grammar* grammar);
/* Debug view of the grammar's row window: the lm_head of a step whose active rows are all
 * constrained covers ids [*lo, *lo + *n) only (*n = 0: no grammar, or no window fits this
 * vocabulary and every step runs the whole head with the mask).  *heads = lm_head launches
 * issued over the window since mx_llm_set_grammar; a launch captured into a step graph counts
 * once, at capture, not per replay. */
int mx_llm_grammar_window(const mx_llm* ctx, int* lo, int* n, long long* heads);
/* Constrain (on != 0) or free the streams `slot` starts from its next prefill on; holds until
 * changed.  Host state only.  MX_ERR_STATE if turned on without a context grammar.  A step whose
 * active rows are all constrained computes only the lm_head rows a grammar can allow (option
 * grammar_head); mx_llm_read_logits of a constrained row returns -inf outside its allowed set,
 * and mx_llm_debug_sample uses the allowed set of the token that would take position pos + 1. */
int mx_llm_set_slot_grammar(mx_llm* ctx, int slot, int on);
/* Park decode row `row` on the scratch slot (stream ended / barge-in reset). */
int mx_llm_release_row(mx_llm* ctx, int row, void* stream);
/* Row compaction (stream-ordered on `stream`, between steps): the stream bound to row `src`
 * continues in the parked row `dst` -- same KV slot, position, token and next input; `src`
 * is parked.  Lets a step run the row class of the live stream count instead of the highest
 * row index in use (replaces nothing in the reference: vLLM's scheduler compacts its batch
 * internally, engine_class.py:114-134).  MX_ERR_STATE if `dst` is live. */
int mx_llm_move_row(mx_llm* ctx, int dst, int src, void* stream);
/* Host view of decode row `row`: *active = 1 while a stream is bound to it (prefill until
 * release), *next_pos = the position its next token takes. */
int mx_llm_row_state(const mx_llm* ctx, int row, int* active, int* next_pos);
/* Host-mapped token history [max_slots][max_pos] int32 written by the device. */
int32_t* mx_llm_history(mx_llm* ctx);
/* Parity/debug: keep a copy of the penalised logits of each decode row (enable before the
 * first mx_llm_decode; costs one extra write per vocab entry) and read one row back. */
int mx_llm_debug_logits(mx_llm* ctx, int enable);
int mx_llm_read_logits(mx_llm* ctx, int row, float* host_out, void* stream);
/* Parity/debug, idle context, after a wait: run the sampler of `row`'s slot on caller logits
 * [vocab] (host) at RNG counter `pos`; nothing is committed (the row's kept logits are
 * overwritten).  A greedy slot returns the smallest-index maximum. */
int mx_llm_debug_sample(mx_llm* ctx, int row, const float* logits_host, int pos,
                        int32_t* token_out, void* stream);
const char* mx_llm_last_error(const mx_llm* ctx);
void mx_llm_destroy(mx_llm* ctx);

/* ---- SNAC 24 kHz decoder (replaces SNAC.decode + slice + int16) --------------------- */
int mx_snac_create(int device, int max_frames, int max_batch, mx_snac** out);
/* names: q{i}.codebook [4096*8], q{i}.out_proj.w [768*8], q{i}.out_proj.b, in.dw.w [768*7],
 * in.dw.b, in.pw.w [1024*768], in.pw.b, b{k}.alpha, b{k}.up.w [Cin*Cout*2s], b{k}.up.b,
 * b{k}.noise.w, b{k}.r{j}.{alpha1,dw.w,dw.b,alpha2,pw.w,pw.b}, out.alpha, out.conv.w, out.conv.b
 * (weight norm already folded; layouts as torch Conv1d / ConvTranspose1d weights). */
int mx_snac_set_weight(mx_snac* ctx, const char* name, const void* dev_data, int64_t numel,
                       int dtype);
int mx_snac_finalize(mx_snac* ctx);
/* Decode `batch` windows of n_frames frames each.  frames: [batch][7*n_frames] SNAC codes in
 * speechpipe token order (0..4095; the caller applies the range check of speechpipe.py:108-111).
 * noise: [batch][sum of the 4 NoiseBlock lengths] or NULL: fresh N(0,1) drawn from `seeds[b]`
 * per window (device-accessible [batch], e.g. host-mapped; a window's noise then depends on
 * its own seed only) or, with seeds NULL, from `seed` over the whole batch.
 * pcm: [batch][hi-lo] int16 of samples [lo,hi) (NULL to skip); audio: [batch][2048*n_frames]
 * fp32 full window (NULL to skip).  With audio NULL only the positions [lo,hi) depend on are
 * computed past the first DecoderBlock (the same PCM within fp32 summation order). */
int mx_snac_decode(mx_snac* ctx, const int32_t* frames, int n_frames, int batch,
                   const float* noise, uint64_t seed, const uint64_t* seeds, int16_t* pcm,
                   float* audio, int lo, int hi, void* stream);
const char* mx_snac_last_error(const mx_snac* ctx);
void mx_snac_destroy(mx_snac* ctx);

/* ---- SNAC 24 kHz encoder + residual vector quantiser (replaces SNAC.encode) ---------- */
/* A context of its own (nothing is shared with mx_snac).  Buffers are sized by max_frames
 * (1 .. 4096) at finalize: 3 x 393,216 bytes per frame. */
int mx_snac_enc_create(int device, int max_frames, mx_snac_enc** out);
/* names: enc.in.{w,b} [48*7], enc.b{k}.r{j}.{alpha1,dw.w,dw.b,alpha2,pw.w,pw.b},
 * enc.b{k}.alpha, enc.b{k}.down.{w,b} ([2C][C][2s], C = 48 << k, s = 2, 4, 8, 8),
 * enc.out.dw.{w,b} [768*7], q{i}.in_proj.{w,b} ([8][768]), q{i}.codebook [4096*8],
 * q{i}.out_proj.{w,b} (weight norm already folded; layouts as torch Conv1d weights).
 * MX_ERR_STATE after finalize. */
int mx_snac_enc_set_weight(mx_snac_enc* ctx, const char* name, const void* dev_data,
                           int64_t numel, int dtype);
int mx_snac_enc_finalize(mx_snac_enc* ctx);
/* audio: device-accessible fp32 mono 24 kHz [n_samples], read as zeros past its end up to the
 * next multiple of 2048; frames_out: device-accessible int32 [7 * ceil(n_samples / 2048)] in
 * speechpipe order (frame f = c0[f], c1[2f], c2[4f], c2[4f+1], c1[2f+1], c2[4f+2], c2[4f+3]).
 * Enqueued on `stream`; deterministic (no atomics).  Every check runs before anything is
 * enqueued: MX_ERR_ARG on a null pointer, n_samples < 1 or more than max_frames frames,
 * MX_ERR_STATE before finalize. */
int mx_snac_enc_encode(mx_snac_enc* ctx, const float* audio, int64_t n_samples,
                       int32_t* frames_out, void* stream);
/* parity/debug: the latent z, channels-last [4 * n_frames][768] */
int mx_snac_enc_latent(mx_snac_enc* ctx, const float* audio, int64_t n_samples, float* z_out,
                       void* stream);
/* parity/debug: the quantiser alone on a caller's z [4 * n_frames][768] */
int mx_snac_enc_quantize(mx_snac_enc* ctx, const float* z, int n_frames, int32_t* frames_out,
                         void* stream);
const char* mx_snac_enc_last_error(const mx_snac_enc* ctx);
void mx_snac_enc_destroy(mx_snac_enc* ctx);

#ifdef __cplusplus
}
#endif
#endif /* MORPHEUS_MX_H */
