// C ABI of libmorpheus_mx.so (include/morpheus_mx.h): context lifetime, weight packing,
// the decode-step schedule, hipGraph capture/replay, and the SNAC window pipeline.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdio>
#include <algorithm>
#include <array>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/morpheus_mx.h"
#include "mx_engine.h"
#include "mx_llm_kernels.h"
#include "mx_snac_kernels.h"
#include "mx_snac_enc_kernels.h"

using namespace mx;

#define MX_TRY(ctx, expr)                                                              \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess) {                                                            \
      (void)hipGetLastError(); /* do not leave the error for the caller's runtime */  \
      (ctx)->err = std::string(#expr) + " -> " + hipGetErrorString(e_);               \
      return MX_ERR_HIP;                                                               \
    }                                                                                  \
  } while (0)

#define MX_FAIL(ctx, code, msg) \
  do {                          \
    (ctx)->err = (msg);         \
    return (code);              \
  } while (0)

static thread_local std::string g_err;

extern "C" const char* mx_version(void) { return "morpheus_mx 0.1 gfx950"; }

extern "C" int mx_host_alloc(size_t bytes, void** host_ptr, void** dev_ptr) {
  void* h = nullptr;
  if (hipHostMalloc(&h, bytes, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess)
    return MX_ERR_OOM;
  std::memset(h, 0, bytes);
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
    (void)hipHostFree(h);
    return MX_ERR_HIP;
  }
  *host_ptr = h;
  *dev_ptr = d;
  return MX_OK;
}

extern "C" int mx_host_free(void* host_ptr) {
  return hipHostFree(host_ptr) == hipSuccess ? MX_OK : MX_ERR_HIP;
}

// =====================================================================================
// LLM context
// =====================================================================================
// Weight matrices are bf16, or OCP e4m3 bytes + one fp32 dequant scale per packed row
// (mx_llm_config.wdtype); the packed row order serves the kernels' epilogues.
struct LayerW {
  float* attn_norm = nullptr;
  float* mlp_norm = nullptr;
  void* wqkv = nullptr;  // [(H + 2*kvh*128)][H], q/k rows pair-interleaved for RoPE
  void* wo = nullptr;    // [H][heads*128]
  void* wgu = nullptr;   // [2F][H], rows (gate_i, up_i) interleaved
  void* wd = nullptr;    // [H][F]
  float *sqkv = nullptr, *so = nullptr, *sgu = nullptr, *sd = nullptr;  // fp8 row scales
  // fragment-major copies for the multi-row GEMM (built at finalize)
  void *wqkv_f = nullptr, *wo_f = nullptr, *wgu_f = nullptr, *wd_f = nullptr;
  unsigned loaded = 0, scaled = 0;
};

struct mx_llm {
  int device = 0;
  mx_llm_config c{};
  std::string err;
  std::vector<void*> allocs;
  uint16_t* embed = nullptr;   // bf16 always (token embedding gather)
  void* lm = nullptr;          // lm_head: the embedding (tied bf16) or its own matrix
  float* slm = nullptr;        // fp8 lm_head row scales
  bool lm_loaded = false, lm_scaled = false;
  void* lm_f = nullptr;        // fragment-major lm_head for the multi-row GEMM
  int rows_frag = 1;           // option: multi-row GEMMs read the fragment-major copies
  int esz = 2;                 // bytes per matrix element (2 bf16, 1 fp8)
  float* norm = nullptr;
  std::vector<LayerW> L;
  float* rope_cos = nullptr;
  float* rope_sin = nullptr;
  int rope_rows = 0;
  uint16_t* kcache = nullptr;  // [layers][slots+1][kvh][max_pos/32][4096] (mx_common.h kv_k_off)
  uint16_t* vcache = nullptr;
  size_t kv_layer_elems = 0;
  float *h_dec = nullptr, *h_pre = nullptr, *q = nullptr, *att = nullptr, *act = nullptr;
  float *part_ml = nullptr, *part_acc = nullptr;
  int* att_cnt = nullptr;
  float* rows_ws = nullptr;     // split-K partial tiles of the multi-row GEMM
  size_t rows_ws_floats = 0;
  int* rows_tickets = nullptr;
  size_t rows_tickets_n = 0;
  int nsplit_max = 0;
  int32_t *row_slot = nullptr, *row_pos = nullptr, *row_token = nullptr;
  int32_t *pre_slot = nullptr, *pre_pos = nullptr, *pre_ids = nullptr;
  unsigned long long* best = nullptr;
  uint8_t* seen = nullptr;
  // per KV slot sampling state (set at prefill; the scratch slot stays greedy)
  float *penalty = nullptr, *samp_temp = nullptr, *samp_top_p = nullptr;
  uint32_t* samp_seed = nullptr;
  int32_t* samp_top_k = nullptr;  // per KV slot: 0 = no limit
  float* samp_min_p = nullptr;    // per KV slot: 0 = off
  int32_t* last_n = nullptr;      // per KV slot penalty window (0: the whole sequence)
  int32_t* recent = nullptr;      // [slots][PEN_RING] ids at the window's positions
  unsigned long long* dbg_best = nullptr;  // mx_llm_debug_sample: its own key and counter
  int32_t* dbg_pos = nullptr;              // (slot word, position word)
  float* logits = nullptr;      // [max_rows_head][vocab] penalised logits (sampling / parity)
  int logits_all = 0;           // option via mx_llm_debug_logits: keep every row's logits
  int32_t* hist_host = nullptr;
  int32_t* hist_dev = nullptr;
  hipStream_t cap = nullptr;
  std::map<int, hipGraphExec_t> graphs;   // key: n_rows * 4096 + attention splits
  std::vector<int> pos_mirror;            // host copy of row_pos (position of next token)
  std::vector<char> row_active;
  std::vector<char> row_samples;          // row's slot samples (temperature > 0): head runs the sampler
  std::vector<char> row_chain;            // ... with a non-neutral top-k or min-p (sample_chain_kernel)
  std::map<int, hipGraph_t> graph_defs;
  // code grammar (mx_llm_set_grammar): constrained slots pick from their phase's ids only
  bool gram_on = false;
  mx_code_grammar gram{};
  int32_t* gram_origin = nullptr;         // device, per KV slot: the prefill's length, or -1
  std::vector<char> slot_grammar;         // mx_llm_set_slot_grammar: read by the slot's next prefill
  std::vector<int> row_origin;            // per decode row: its stream's origin, -1 = unconstrained
  int grammar_head = 1;                   // option: steps of constrained rows only run the lm_head
  int win_lo = 0, win_n = 0;              //   over ids [win_lo, win_lo + win_n) (win_n 0: no window fits)
  long long win_heads = 0;                //   lm_head launches issued over it (mx_llm_grammar_window)
  // packed prefill (mx_llm_prefill_batch): allocated by its first call, behind every other
  // buffer, so a context that never packs keeps its allocations
  int32_t* pk_tab = nullptr;              // the call's table: [max_batch] PackSeg, [max_prefill] PackRow
  int32_t* pk_idx = nullptr;              // [3][max_batch] head rows' slot, position, decode row
  unsigned long long* pk_best = nullptr;  // [max_batch] argmax keys of the head rows
  float* pk_h = nullptr;                  // [max_batch][hidden] the segments' last rows
  float* pk_logits = nullptr;             // [max_batch][vocab] their penalised logits
  std::vector<int32_t> pk_host;           // host copy of the table (one upload per call)
  // packed continuation (mx_llm_prefill_pack): the id histories [0, pos0) of a call's entries,
  // back to back (allocated by the first pack behind a history, behind every other buffer)
  int32_t* pk_hist = nullptr;             // device [max_batch][max_pos]
  std::vector<int32_t> pk_hist_host;      // its staging copy (one upload per call)
  int32_t* fork_tab = nullptr;            // device [max_slots] KvFork: mx_llm_fork_slots' table
                                          // (allocated by its first call, as above)
  // prompt continuation (mx_llm_prefill_chunk / mx_llm_fork_slot): the id history of every slot's
  // prompt lives in plain host memory, written at call time by every prefill entry point and
  // copied by a fork; a final chunk uploads it once (DESIGN.md §3 "Prompt continuation")
  std::vector<int32_t> slot_ids;          // [max_slots][max_pos] prompt ids the slot holds
  std::vector<int> slot_len;              // ... and how many (tokens decoded behind them not counted)
  std::vector<int> row_slot_h;            // per decode row: the KV slot it is bound to, -1 = parked
  int32_t* cont_ids = nullptr;            // device [max_pos]: a final chunk's history upload
                                          // (allocated by the first one, behind every other buffer)
  bool final = false;
  int max_rows = 0;
  int legacy_gemv = 0;          // option: grid-stride GEMV for R = 1 too (A/B timing)
  int att_cpw_b1 = 0;           // option: chunks per wave, single-row attention (0 = auto)
  int att_cpw_batch = 0;        // option: same for multi-row (batched decode / prefill); 0 =
                                // auto (att_shape): measured -14 % attention at 32 rows
  int att_nw_b1 = 4, att_nw_batch = 8;  // options: attention waves per block (4 or 8; measured)
  int att_b1_short = 1;                 // option: one-row attention may take 64 / 96-position
                                        // splits (2: both, 1: 96 only; 0: from 128). 1 measured
                                        // -1.8 % bf16 / -2.6 % e4m3 per step at L 600, 2 slower
                                        // at L 300 (profiles/r06_att_b1_short.log)
  int att_b1_nw6 = 1;                   // option: one-row attention may take 192-position
                                        // splits (6-wave blocks) past L 1,024: measured -0.6 to
                                        // -0.8 % bf16, -1.1 % e4m3 per step at L 1,100..1,400
  int att_nw6 = 1;                      // option: multi-row attention may take 6-wave blocks
                                        // (8 rows, L 300-1100: -0.3..-0.7 % per step, bf16 and
                                        // e4m3; profiles/r06_att_nw6_gemv_balance.log)
  int gemv_balance = 1;                 // option: one-row qkv / merging o-proj grids balanced
  int cus = 0;                          //   over the CUs (this many; mx_llm_finalize); bf16 step
                                        //   -1.0 %, e4m3 -0.3 % (the same log)
  int o_merge = 1;     // option: one-row o-proj merges the attention splits (0 = ticket merge)
  int rows_merge = 1;  // option: the same at 2-16 rows (generation-4 o-proj, rows_merge_ok):
                       // 8 e4m3 rows 1.654 -> 1.637 ms, bf16 8 / 4 / 16 rows unchanged (+-0.1 %)
  int gemv_wpb = 4;
  int rows_lds_pad = 0;              // option: extra LDS KB per multi-row block (occupancy probe)
  int rows_pw = 2;                   // option: generation-4 weight prefetch distance (2 measured best)
  int rows_pw_f8 = 2;                // option: the same for e4m3 weights (1, 2)
  int rows_target = 0;               // option: generation-4 K-range split target (0 = per shape)
  int rows_target_k[4] = {0, 0, 0, 0};  // options rows_target_{qkv,o,gu,down}: the same for
                                        // one kind of the layer's launches (0 = rows_target)
  int rows_nt_max = 0;               // option: generation-4 batch-tile cap in 16-row units (0 = 4)
  int rows_nt1 = 2;                  // option: kinds whose 17-32-row launches take 16-row batch
                                     // tiles (bit 0 qkv, 1 o-proj, 2 gate/up, 3 down, 4 lm_head;
                                     // round 5: 11; with the seam-free qkv / down of round 6 the
                                     // o-proj alone is best: profiles/r06_rows_nt1.log)
  int rows_head_target = 0;          // option: lm_head K-range target (0 = default)
  int rows_head_mt = 1;              // option: multi-row lm_head weight rows per wave / 16
                                     // (1 since round 5: with one argmax atomic per block the
                                     // 128-VGPR 16-row tiles stream faster: 8 bf16 rows 172.6
                                     // -> 149.7 us, 8 e4m3 rows -> 79.6 us, 32 rows -> 154 us;
                                     // profiles/r05_head_options.log)
  int rows_atomic = 1;               // option: residual projections (o-proj, down) at >= 2 rows
                                     // add each K range's partial into h with float atomics
                                     // instead of the split-K seam (mx_rows_v4.inc)
  int rows_qkv_parts = 1;            // option: decode at >= 2 rows, the qkv GEMM's K ranges
                                     // store raw partials and the attention launch sums them
                                     // (scale, RoPE, K / V append): no split-K seam
  float* qkv_parts = nullptr;        // [qkv_nkc_cap][max_batch][qkv rows]
  float* qkv_ss = nullptr;           // [qkv_nkc_cap][max_batch]
  static constexpr int qkv_nkc_cap = ATT_QKV_NKC_MAX;  // more ranges: the seam qkv
  int bench_one_layer = 0;           // diagnostic option: the GEMV probes sweep layer 0 only
                                     // (weights resident in the Infinity Cache: the on-die bound)
  int head_b1 = 1;                  // option: one-row lm_head on the persistent kernel
                                     // (measured -24 us bf16 / -45 us e4m3 per step, round 4)
  int rpw_o = 0, rpw_gu = 0, rpw_down = 0;  // options: rows per wave (0 = default)
  // persistent one-row engine (engine_b1.hip): option b1_engine runs the layers of a
  // one-row decode step as one launch (engine_slots = its LDS ring depth)
  int b1_engine = 0, engine_slots = 7, engine_depth = 2, engine_loaders = 2, engine_grid = 0;
  int engine_dbg = 0;  // option engine_dbg: timing experiments (outputs invalid when != 0)
  int engine_timeout_ticks = 5000000;  // option engine_timeout: bound of every engine wait in
                                       // 100 MHz ticks (50 ms; a step takes ~1.5 ms)
  uint2 *g_qkv = nullptr, *g_att = nullptr, *g_h1 = nullptr, *g_act = nullptr, *g_h2 = nullptr;
  float* eng_part = nullptr;
  int* eng_tickets = nullptr;
  uint32_t* eng_epoch = nullptr;
  int* eng_status_h = nullptr;  // host-mapped status word of the last engine launches
  int* eng_status_d = nullptr;
  uint64_t* eng_trace = nullptr;  // option engine_trace: per-CU, per-layer phase stamps
  // every layer's matrices / norms / fp8 scales of one kind are contiguous
  void *wqkv_all = nullptr, *wo_all = nullptr, *wgu_all = nullptr, *wd_all = nullptr;
  float *sqkv_all = nullptr, *so_all = nullptr, *sgu_all = nullptr, *sd_all = nullptr;
  float *attn_norm_all = nullptr, *mlp_norm_all = nullptr;

  template <class T>
  hipError_t alloc(T** p, size_t n) {
    void* v = nullptr;
    hipError_t e = hipMalloc(&v, n * sizeof(T) + 256);
    if (e == hipSuccess) {
      allocs.push_back(v);
      *p = reinterpret_cast<T*>(v);
    }
    return e;
  }
};

static void drop_graphs(mx_llm* x);

extern "C" int mx_llm_create(int device, const mx_llm_config* cfg, mx_llm** out) {
  if (!cfg || !out) return MX_ERR_ARG;
  auto* x = new mx_llm();
  x->device = device;
  x->c = *cfg;
  const auto& c = x->c;
  auto bad = [&](const char* m) {
    g_err = m;
    delete x;
    return MX_ERR_ARG;
  };
  if (c.head_dim != 128) return bad("head_dim must be 128");
  if (c.hidden % 256 || c.ffn % 256) return bad("hidden and ffn must be multiples of 256");
  if (c.heads % c.kv_heads || c.heads / c.kv_heads > ATT_MAXG) return bad("bad GQA grouping");
  if (c.heads * 128 % 256) return bad("heads*128 must be a multiple of 256");
  if (c.max_pos % 128) return bad("max_pos must be a multiple of 128");
  if (c.max_batch < 1 || c.max_prefill < 1 || c.max_slots < 1) return bad("bad limits");
  if (c.wdtype != WT_BF16 && c.wdtype != WT_FP8) return bad("bad wdtype");
  if (c.wdtype == WT_FP8 && (c.hidden % 1024 || c.ffn % 1024 || c.heads * 128 % 1024))
    return bad("fp8 needs hidden, ffn and heads*128 multiples of 1024");
  if (hipSetDevice(device) != hipSuccess) return bad("hipSetDevice failed");
  x->L.resize(c.layers);
  x->pos_mirror.assign(c.max_batch, 0);
  x->row_active.assign(c.max_batch, 0);
  x->row_samples.assign(c.max_batch, 0);
  x->row_chain.assign(c.max_batch, 0);
  x->row_origin.assign(c.max_batch, -1);
  x->slot_grammar.assign(c.max_slots, 0);
  x->slot_ids.assign((size_t)c.max_slots * c.max_pos, 0);
  x->slot_len.assign(c.max_slots, 0);
  x->row_slot_h.assign(c.max_batch, -1);
  x->max_rows = c.max_batch > c.max_prefill ? c.max_batch : c.max_prefill;
  x->nsplit_max = c.max_pos / ATT_S_MIN;
  const int qkv_rows = c.heads * 128 + 2 * c.kv_heads * 128;
  const int slots = c.max_slots + 1;  // +1 scratch slot for parked rows
  x->kv_layer_elems = (size_t)slots * c.kv_heads * c.max_pos * 128;
  hipError_t e = hipSuccess;
#define A(p, n) \
  if (e == hipSuccess) e = x->alloc(&(p), (size_t)(n));
  const bool f8 = c.wdtype == WT_FP8;
  x->esz = f8 ? 1 : 2;
  uint8_t* m8 = nullptr;  // byte-typed allocations of matrices
#define AM(p, rows, cols)                                                  \
  if (e == hipSuccess) {                                                   \
    e = x->alloc(&m8, (size_t)(rows) * (cols) * x->esz);                  \
    p = m8;                                                                \
  }
  A(x->embed, (size_t)c.vocab * c.hidden);
  if (!c.tied || f8) AM(x->lm, c.vocab, c.hidden);
  if (f8) A(x->slm, c.vocab);
  A(x->norm, c.hidden);
  const size_t NL = (size_t)c.layers;
  A(x->attn_norm_all, NL * c.hidden);
  A(x->mlp_norm_all, NL * c.hidden);
  AM(x->wqkv_all, NL * qkv_rows, c.hidden);
  AM(x->wo_all, NL * c.hidden, c.heads * 128);
  AM(x->wgu_all, NL * 2 * c.ffn, c.hidden);
  AM(x->wd_all, NL * c.hidden, c.ffn);
  if (f8) {
    A(x->sqkv_all, NL * qkv_rows);
    A(x->so_all, NL * c.hidden);
    A(x->sgu_all, NL * 2 * c.ffn);
    A(x->sd_all, NL * c.hidden);
  }
  if (e == hipSuccess) {
    for (size_t li = 0; li < NL; ++li) {
      LayerW& l = x->L[li];
      l.attn_norm = x->attn_norm_all + li * c.hidden;
      l.mlp_norm = x->mlp_norm_all + li * c.hidden;
      l.wqkv = (uint8_t*)x->wqkv_all + li * qkv_rows * c.hidden * x->esz;
      l.wo = (uint8_t*)x->wo_all + li * c.hidden * c.heads * 128 * x->esz;
      l.wgu = (uint8_t*)x->wgu_all + li * 2 * c.ffn * c.hidden * x->esz;
      l.wd = (uint8_t*)x->wd_all + li * c.hidden * c.ffn * x->esz;
      if (f8) {
        l.sqkv = x->sqkv_all + li * qkv_rows;
        l.so = x->so_all + li * c.hidden;
        l.sgu = x->sgu_all + li * 2 * c.ffn;
        l.sd = x->sd_all + li * c.hidden;
      }
    }
  }
#undef AM
  A(x->kcache, x->kv_layer_elems * c.layers);
  A(x->vcache, x->kv_layer_elems * c.layers);
  A(x->h_dec, (size_t)c.max_batch * c.hidden);
  A(x->h_pre, (size_t)c.max_prefill * c.hidden);
  A(x->q, (size_t)x->max_rows * c.heads * 128);
  A(x->att, (size_t)x->max_rows * c.heads * 128);
  A(x->act, (size_t)x->max_rows * c.ffn);
  // split partials: prefill rows use 128-position splits, decode rows down to 32
  const size_t part_rows = (size_t)x->max_rows * (c.max_pos / ATT_S_MIN);
  A(x->part_ml, part_rows * c.heads * 2);
  A(x->part_acc, part_rows * c.heads * 128);
  A(x->att_cnt, (size_t)x->max_rows * c.kv_heads);
  {  // multi-row GEMM workspace: the largest of the step's projections and the lm_head
    // the tile geometry changes with the row count (16 / 32 / 64-row batch tiles), so take
    // the largest need over every row-count class up to the maximum
    const int Rm = x->max_rows;
    const int shapes[5][4] = {{qkv_rows, c.hidden, Rm, EPI_QKV},
                              {c.hidden, c.heads * 128, Rm, EPI_RESID},
                              {2 * c.ffn, c.hidden, Rm, EPI_SILU},
                              {c.hidden, c.ffn, Rm, EPI_RESID},
                              {c.vocab, c.hidden, c.max_batch, EPI_ARGMAX}};
    for (auto& sh : shapes)
      for (int r : {16, 32, 64, sh[2]}) {
        size_t wf = 0, tk = 0;
        v4::gemm_rows_workspace_v4(sh[0], sh[1], std::min(r, sh[2]), sh[3], &wf, &tk);
        x->rows_ws_floats = std::max(x->rows_ws_floats, wf);
        x->rows_tickets_n = std::max(x->rows_tickets_n, tk);
      }
  }
  A(x->rows_ws, std::max<size_t>(x->rows_ws_floats, 1));
  A(x->qkv_parts, (size_t)mx_llm::qkv_nkc_cap * c.max_batch * qkv_rows);
  A(x->qkv_ss, (size_t)mx_llm::qkv_nkc_cap * c.max_batch);
  A(x->rows_tickets, x->rows_tickets_n);
  A(x->row_slot, c.max_batch);
  A(x->row_pos, c.max_batch);
  A(x->row_token, c.max_batch);
  A(x->pre_slot, c.max_prefill);
  A(x->pre_pos, c.max_prefill);
  A(x->pre_ids, c.max_prefill);
  A(x->best, c.max_batch);
  A(x->seen, (size_t)slots * c.vocab);
  A(x->penalty, slots);
  A(x->samp_temp, slots);
  A(x->samp_top_p, slots);
  A(x->samp_seed, 2 * slots);
  A(x->logits, (size_t)c.max_batch * c.vocab);
  {  // engine hand-off granules and attention partials (small: ~1 MB)
    const size_t QD = (size_t)c.heads * 128, KVD = (size_t)c.kv_heads * 128;
    A(x->g_qkv, QD + 2 * KVD);
    A(x->g_att, QD);
    A(x->g_h1, c.hidden);
    A(x->g_act, c.ffn);
    A(x->g_h2, c.hidden);
    A(x->eng_part, (size_t)c.kv_heads * ((c.max_pos + 127) / 128) * (c.heads / c.kv_heads) * 130);
    A(x->eng_tickets, (size_t)c.layers * c.kv_heads);
    A(x->eng_epoch, 2);
  }
#undef A
  if (c.tied && !f8) x->lm = x->embed;
  if (e != hipSuccess) {
    g_err = std::string("allocation failed: ") + hipGetErrorString(e);
    for (void* p : x->allocs) (void)hipFree(p);
    delete x;
    return MX_ERR_OOM;
  }
  void* hh = nullptr;
  void* hd = nullptr;
  if (mx_host_alloc((size_t)slots * c.max_pos * sizeof(int32_t), &hh, &hd) != MX_OK) {
    g_err = "host history alloc failed";
    for (void* p : x->allocs) (void)hipFree(p);
    delete x;
    return MX_ERR_OOM;
  }
  x->hist_host = (int32_t*)hh;
  x->hist_dev = (int32_t*)hd;
  if (mx_host_alloc(64, &hh, &hd) != MX_OK) {
    g_err = "host status alloc failed";
    (void)hipHostFree(x->hist_host);
    for (void* p : x->allocs) (void)hipFree(p);
    delete x;
    return MX_ERR_OOM;
  }
  x->eng_status_h = (int*)hh;
  x->eng_status_d = (int*)hd;
  e = hipMemset(x->kcache, 0, x->kv_layer_elems * c.layers * 2);
  if (e == hipSuccess) e = hipMemset(x->vcache, 0, x->kv_layer_elems * c.layers * 2);
  if (e == hipSuccess) e = hipMemset(x->best, 0, c.max_batch * 8);
  if (e == hipSuccess) e = hipMemset(x->att_cnt, 0, (size_t)x->max_rows * c.kv_heads * 4);
  if (e == hipSuccess) e = hipMemset(x->rows_tickets, 0, x->rows_tickets_n * 4);
  if (e == hipSuccess) e = hipMemset(x->seen, 0, (size_t)slots * c.vocab);
  if (e == hipSuccess) e = hipMemset(x->h_dec, 0, (size_t)c.max_batch * c.hidden * 4);
  if (e == hipSuccess) e = hipMemset(x->samp_temp, 0, slots * 4);  // greedy everywhere
  if (e == hipSuccess) e = hipMemset(x->samp_seed, 0, slots * 8);
  if (e == hipSuccess) {
    const size_t QD = (size_t)c.heads * 128, KVD = (size_t)c.kv_heads * 128;
    const uint32_t ep[2] = {1u, 0u};  // granule tags of epoch 0 would match zeroed buffers
    e = hipMemset(x->g_qkv, 0, (QD + 2 * KVD) * 8);
    if (e == hipSuccess) e = hipMemset(x->g_att, 0, QD * 8);
    if (e == hipSuccess) e = hipMemset(x->g_h1, 0, (size_t)c.hidden * 8);
    if (e == hipSuccess) e = hipMemset(x->g_act, 0, (size_t)c.ffn * 8);
    if (e == hipSuccess) e = hipMemset(x->g_h2, 0, (size_t)c.hidden * 8);
    if (e == hipSuccess) e = hipMemset(x->eng_tickets, 0, (size_t)c.layers * c.kv_heads * 4);
    if (e == hipSuccess) e = hipMemcpy(x->eng_epoch, ep, 8, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) {
    std::vector<float> ones(slots, 1.0f);
    e = hipMemcpy(x->penalty, ones.data(), slots * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(x->samp_top_p, ones.data(), slots * 4, hipMemcpyHostToDevice);
  }
  // every decode row starts parked on the scratch slot at position 0
  std::vector<int32_t> park(c.max_batch, c.max_slots), zero(c.max_batch, 0);
  if (e == hipSuccess)
    e = hipMemcpy(x->row_slot, park.data(), c.max_batch * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(x->row_pos, zero.data(), c.max_batch * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&x->cap, hipStreamNonBlocking);
  if (e == hipSuccess) e = gemv_prepare(std::max(std::max(c.hidden, c.ffn), c.heads * 128));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    g_err = std::string("init failed: ") + hipGetErrorString(e);
    mx_llm_destroy(x);
    return MX_ERR_HIP;
  }
  *out = x;
  return MX_OK;
}

// Packing: source row i of a named matrix lands on packed row dmap[i] of its target:
// q/k rows of each head go to (2i, 2i+1) <- (i, i+64) so the RoPE epilogue sees both
// partners in one wave; gate/up rows are interleaved (g_i -> 2i, u_i -> 2i+1) so SiLU*up
// is a per-wave epilogue; v/o/down/embed/lm_head keep their order.  fp8 row scales
// ("<name>.scale") follow the same map.
struct PackTarget {
  void* base = nullptr;   // matrix storage
  float* scale = nullptr; // fp8 scales of the same packed rows
  std::vector<int32_t> dmap;
  int cols = 0;
  unsigned bit = 0;       // LayerW::loaded / scaled bit
};

static bool pack_target(mx_llm* x, const std::string& nm, PackTarget& t, LayerW** lw) {
  const auto& c = x->c;
  const int H = c.hidden, F = c.ffn, QD = c.heads * 128, KD = c.kv_heads * 128;
  auto seq = [](int rows, int row0, int step) {
    std::vector<int32_t> p(rows);
    for (int i = 0; i < rows; ++i) p[i] = row0 + step * i;
    return p;
  };
  auto qk = [](int heads, int row0) {
    std::vector<int32_t> p(heads * 128);
    for (int h = 0; h < heads; ++h)
      for (int i = 0; i < 64; ++i) {
        p[h * 128 + i] = row0 + h * 128 + 2 * i;
        p[h * 128 + i + 64] = row0 + h * 128 + 2 * i + 1;
      }
    return p;
  };
  *lw = nullptr;
  if (nm == "embed") { t.base = x->embed; t.dmap = seq(c.vocab, 0, 1); t.cols = H; return true; }
  if (nm == "lm_head") {
    t.base = x->lm; t.scale = x->slm; t.dmap = seq(c.vocab, 0, 1); t.cols = H; return true;
  }
  int li = -1;
  char field[32] = {0};
  if (std::sscanf(nm.c_str(), "l%d.%31s", &li, field) != 2 || li < 0 || li >= c.layers) return false;
  LayerW& l = x->L[li];
  *lw = &l;
  const std::string f(field);
  if (f == "wq") { t.base = l.wqkv; t.scale = l.sqkv; t.dmap = qk(c.heads, 0); t.cols = H; t.bit = 4; }
  else if (f == "wk") { t.base = l.wqkv; t.scale = l.sqkv; t.dmap = qk(c.kv_heads, QD); t.cols = H; t.bit = 8; }
  else if (f == "wv") { t.base = l.wqkv; t.scale = l.sqkv; t.dmap = seq(KD, QD + KD, 1); t.cols = H; t.bit = 16; }
  else if (f == "wo") { t.base = l.wo; t.scale = l.so; t.dmap = seq(H, 0, 1); t.cols = QD; t.bit = 32; }
  else if (f == "wg") { t.base = l.wgu; t.scale = l.sgu; t.dmap = seq(F, 0, 2); t.cols = H; t.bit = 64; }
  else if (f == "wu") { t.base = l.wgu; t.scale = l.sgu; t.dmap = seq(F, 1, 2); t.cols = H; t.bit = 128; }
  else if (f == "wd") { t.base = l.wd; t.scale = l.sd; t.dmap = seq(H, 0, 1); t.cols = F; t.bit = 256; }
  else return false;
  return true;
}

extern "C" int mx_llm_set_weight(mx_llm* x, const char* name, const void* data, int64_t numel,
                                 int dtype) {
  if (!x || !name || !data) return MX_ERR_ARG;
  if (dtype != MX_DTYPE_F32 && dtype != MX_DTYPE_BF16 && dtype != MX_DTYPE_FP8)
    MX_FAIL(x, MX_ERR_ARG, "bad dtype");
  // finalize derived the fragment-major copies and captured graphs from these weights
  if (x->final) MX_FAIL(x, MX_ERR_STATE, "weights are frozen after mx_llm_finalize");
  MX_TRY(x, hipSetDevice(x->device));
  const auto& c = x->c;
  const int H = c.hidden;
  const bool f8 = c.wdtype == WT_FP8;
  std::string n(name);
  if (n == "norm") {
    if (numel != H) MX_FAIL(x, MX_ERR_ARG, "norm: bad numel");
    MX_TRY(x, launch_to_f32(x->norm, data, H, dtype == MX_DTYPE_BF16 ? 1 : 0, nullptr));
    MX_TRY(x, hipDeviceSynchronize());
    return MX_OK;
  }
  int li = -1;
  char field[32] = {0};
  if (std::sscanf(name, "l%d.%31s", &li, field) == 2 && li >= 0 && li < c.layers &&
      (std::string(field) == "attn_norm" || std::string(field) == "mlp_norm")) {
    if (numel != H) MX_FAIL(x, MX_ERR_ARG, n + ": bad numel");
    LayerW& l = x->L[li];
    const bool an = std::string(field) == "attn_norm";
    MX_TRY(x, launch_to_f32(an ? l.attn_norm : l.mlp_norm, data, H, dtype == MX_DTYPE_BF16 ? 1 : 0,
                            nullptr));
    MX_TRY(x, hipDeviceSynchronize());
    l.loaded |= an ? 1u : 2u;
    return MX_OK;
  }
  const bool is_scale = n.size() > 6 && n.compare(n.size() - 6, 6, ".scale") == 0;
  if (is_scale) n = n.substr(0, n.size() - 6);
  PackTarget t;
  LayerW* lw = nullptr;
  if (!pack_target(x, n, t, &lw)) MX_FAIL(x, MX_ERR_ARG, "unknown weight " + std::string(name));
  const int rows = (int)t.dmap.size();
  if (n == "lm_head" && c.tied && !f8) MX_FAIL(x, MX_ERR_ARG, "lm_head given but config is tied");
  if (is_scale) {  // fp8 dequant scales [rows] fp32, host-permuted into packed order
    if (!f8 || n == "embed") MX_FAIL(x, MX_ERR_ARG, n + ".scale only exists for fp8 matrices");
    if (numel != rows || dtype != MX_DTYPE_F32) MX_FAIL(x, MX_ERR_ARG, n + ".scale: bad shape/dtype");
    std::vector<float> src(rows), dst;
    MX_TRY(x, hipMemcpy(src.data(), data, rows * 4, hipMemcpyDeviceToHost));
    // rows of one target may be spread (interleaved): write through the map
    std::vector<float> cur;
    int lo = *std::min_element(t.dmap.begin(), t.dmap.end());
    int hi = *std::max_element(t.dmap.begin(), t.dmap.end());
    cur.resize(hi - lo + 1);
    MX_TRY(x, hipMemcpy(cur.data(), t.scale + lo, cur.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < rows; ++i) cur[t.dmap[i] - lo] = src[i];
    MX_TRY(x, hipMemcpy(t.scale + lo, cur.data(), cur.size() * 4, hipMemcpyHostToDevice));
    if (lw) lw->scaled |= t.bit;
    else x->lm_scaled = true;
    return MX_OK;
  }
  if ((int64_t)rows * t.cols != numel) MX_FAIL(x, MX_ERR_ARG, n + ": bad numel");
  const bool want_f8 = f8 && n != "embed";
  if (want_f8 != (dtype == MX_DTYPE_FP8))
    MX_FAIL(x, MX_ERR_ARG, n + (want_f8 ? ": fp8 engine expects e4m3 bytes (+ .scale)"
                                        : ": bf16/f32 expected"));
  int32_t* dmap = nullptr;
  MX_TRY(x, hipMalloc(&dmap, rows * 4));
  hipError_t e = hipMemcpy(dmap, t.dmap.data(), rows * 4, hipMemcpyHostToDevice);
  const int mode = dtype == MX_DTYPE_FP8 ? 2 : dtype == MX_DTYPE_F32 ? 1 : 0;
  if (e == hipSuccess) e = launch_scatter_rows(t.base, data, dmap, rows, t.cols, mode, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  (void)hipFree(dmap);
  MX_TRY(x, e);
  if (lw) lw->loaded |= t.bit;
  else if (n == "lm_head") x->lm_loaded = true;
  return MX_OK;
}

extern "C" int mx_llm_set_rope(mx_llm* x, const float* cos_h, const float* sin_h, int n_pos) {
  if (!x || !cos_h || !sin_h || n_pos < x->c.max_pos) {
    if (x) x->err = "rope table must cover max_pos positions";
    return MX_ERR_ARG;
  }
  MX_TRY(x, hipSetDevice(x->device));
  const size_t n = (size_t)x->c.max_pos * 64;
  if (!x->rope_cos) {
    MX_TRY(x, x->alloc(&x->rope_cos, n));
    MX_TRY(x, x->alloc(&x->rope_sin, n));
  }
  MX_TRY(x, hipMemcpy(x->rope_cos, cos_h, n * 4, hipMemcpyHostToDevice));
  MX_TRY(x, hipMemcpy(x->rope_sin, sin_h, n * 4, hipMemcpyHostToDevice));
  x->rope_rows = x->c.max_pos;
  return MX_OK;
}

extern "C" int mx_llm_finalize(mx_llm* x) {
  if (!x) return MX_ERR_ARG;
  const bool f8 = x->c.wdtype == WT_FP8;
  for (int i = 0; i < x->c.layers; ++i) {
    if (x->L[i].loaded != 511u)
      MX_FAIL(x, MX_ERR_STATE, "layer " + std::to_string(i) + " weights incomplete");
    if (f8 && x->L[i].scaled != 508u)
      MX_FAIL(x, MX_ERR_STATE, "layer " + std::to_string(i) + " fp8 scales incomplete");
  }
  if ((!x->c.tied || f8) && !x->lm_loaded) MX_FAIL(x, MX_ERR_STATE, "lm_head not loaded");
  if (f8 && !x->lm_scaled) MX_FAIL(x, MX_ERR_STATE, "lm_head fp8 scales not loaded");
  if (!x->rope_cos) MX_FAIL(x, MX_ERR_STATE, "rope table not set");
  MX_TRY(x, hipSetDevice(x->device));
  MX_TRY(x, hipDeviceGetAttribute(&x->cus, hipDeviceAttributeMultiprocessorCount, x->device));
  // fragment-major copies of every matrix the multi-row GEMM streams (2x the weight bytes
  // in HBM, 13.2 GB for Orpheus-3B bf16; the one-row GEMVs keep reading the row-major ones)
  if (!x->lm_f) {
    MX_TRY(x, hipSetDevice(x->device));
    const auto& c = x->c;
    const int H = c.hidden, QD = c.heads * 128, qkv_rows = QD + 2 * c.kv_heads * 128;
    auto make = [&](const void* src, int N, int K, void** dst) -> hipError_t {
      void* p = nullptr;
      hipError_t e = hipMalloc(&p, frag_major_bytes(N, K, x->esz) + 256);
      if (e != hipSuccess) return e;
      x->allocs.push_back(p);
      *dst = p;
      return launch_frag_major(src, p, N, K, x->esz, nullptr);
    };
    for (auto& l : x->L) {
      MX_TRY(x, make(l.wqkv, qkv_rows, H, &l.wqkv_f));
      MX_TRY(x, make(l.wo, H, QD, &l.wo_f));
      MX_TRY(x, make(l.wgu, 2 * c.ffn, H, &l.wgu_f));
      MX_TRY(x, make(l.wd, H, c.ffn, &l.wd_f));
    }
    MX_TRY(x, make(x->lm, c.vocab, H, &x->lm_f));
    MX_TRY(x, hipDeviceSynchronize());
  }
  // sampler-chain state, one block allocated last: every other buffer keeps the address it
  // has without it (the multi-row GEMM's atomic arrival order is sensitive to placement).
  // All zero = neutral: no top-k, no min-p, whole-sequence penalty.
  if (!x->last_n) {
    const size_t slots = (size_t)x->c.max_slots + 1;
    const size_t words = (3 + PEN_RING) * slots + 2 + 2;  // ... + dbg_pos[2] + dbg_best (u64)
    int32_t* blk = nullptr;
    MX_TRY(x, x->alloc(&blk, words + 1));
    MX_TRY(x, hipMemset(blk, 0, (words + 1) * 4));
    x->dbg_best = reinterpret_cast<unsigned long long*>(blk);  // 8-byte aligned: block start
    x->dbg_pos = blk + 2;
    x->samp_top_k = blk + 4;
    x->samp_min_p = reinterpret_cast<float*>(blk + 4 + slots);
    x->last_n = blk + 4 + 2 * slots;
    x->recent = blk + 4 + 3 * slots;
  }
  x->final = true;
  return MX_OK;
}

// ---- one forward over `R` rows (decode rows or prefill rows) -------------------------
// Multi-row attention: 32-position chunks per wave.  An 8-wave attention block needs ~250
// VGPRs per wave, so it fills a CU: the grid should be ONE round of <= 256 blocks.  Give each
// (row, kv head) pair 256 / pairs splits (at least 1) and every wave ceil(chunks / (splits *
// waves)) chunks, rounded up to an instantiated count.  Measured (scripts/gpu_attn*.sh, 32 rows):
// at L = 1200 the old "largest of {4, 2} with >= 256 blocks" rule made 512 blocks in two uneven
// rounds (42.5 us); one split of <= 5 chunks per wave (the CPW 6 kernel) is one round
// (27.2 us, 5.8 TB/s).  CPW 6 / 8 run a runtime chunk loop (a full unroll spills); at L = 2048
// CPW 8 is 49.5 us against 53.0 us for two rounds of CPW 4.
static int att_cpw_pick(int want, int nw) {
  if (nw != 8) return want <= 1 ? 1 : want <= 2 ? 2 : 4;
  if (want <= 4) return want < 1 ? 1 : want;
  return want <= 6 ? 6 : 8;
}
// One-row steps: the o-proj prologue merges at most 8 split partials (gemv1 NSM), so the
// split is the shortest of 128 / 256 / 512 (4 waves x 1 / 2 / 4 chunks) or 1024 / 2048
// positions (8 waves x 4 / 8 chunks) that covers the context in <= 8 splits.
static void att_b1_shape(const mx_llm* x, int max_len, int* nw, int* cpw) {
  if (x->att_cpw_b1 > 0) {  // option override (4-wave blocks)
    *nw = x->att_nw_b1;
    *cpw = x->att_cpw_b1;
    return;
  }
  // option att_b1_short: splits of 64 / 96 positions (2- / 3-wave blocks) first, i.e. more
  // blocks with fewer KV bytes each, for contexts they cover in <= 8 splits
  // option att_b1_nw6: 192-position splits (6-wave blocks) between 128 and 256, i.e. 6..8
  // splits at L 1,025..1,536 instead of 5..6 of 256 (profiles/r06_att_b1_nw6.log)
  static const int shapes[8][2] = {{2, 1}, {3, 1}, {4, 1}, {6, 1}, {4, 2}, {4, 4}, {8, 4}, {8, 8}};
  const bool fits = x->c.max_pos % 64 == 0 && x->max_rows >= 2;  // (the 64-position stride)
  const int first = !fits ? 2 : x->att_b1_short == 2 ? 0 : x->att_b1_short == 1 ? 1 : 2;
  for (int i = first; i < 8; ++i) {
    if (i == 3 && !x->att_b1_nw6) continue;
    *nw = shapes[i][0];
    *cpw = shapes[i][1];
    if ((max_len + 32 * *nw * *cpw - 1) / (32 * *nw * *cpw) <= 8) return;
  }
}

// Multi-row steps: (waves per block, chunks per wave) of the attention launch.
static void att_batch_shape(const mx_llm* x, int R, int max_len, int* nw, int* cpw) {
  *nw = x->att_nw_batch;
  if (x->att_cpw_batch > 0) {
    *cpw = x->att_cpw_batch;
    return;
  }
  const int pairs = R * x->c.kv_heads;
  // one split above 64 (row, kv-head) pairs: at 16 rows x 8 kv heads two splits + the ticket
  // merge took 1.966 ms per fp8 step against 1.846 for one split; at 8 rows the 3-split
  // choice and one split are equal (1.752 / 1.763 ms; profiles/r03_attn_rows_split_ab.log)
  const int splits = pairs > 64 ? 1 : std::max(1, 256 / pairs);
  const int chunks = (max_len + 31) / 32;
  if (x->att_nw6 && splits > 1) {
    // option att_nw6: the shortest split (6- or 8-wave blocks) that covers the context in
    // <= `splits` splits: more blocks, fewer KV bytes per block (at 8 rows, L 600: 4 splits of
    // 192 positions instead of 3 of 256)
    static const int shapes[][2] = {{6, 1}, {8, 1}, {6, 2}, {8, 2}, {6, 3}, {8, 3}, {8, 4}, {8, 6}, {8, 8}};
    for (const auto& sh : shapes) {
      *nw = sh[0];
      *cpw = sh[1];
      if ((chunks + sh[0] * sh[1] - 1) / (sh[0] * sh[1]) <= splits) return;
    }
    return;
  }
  *cpw = att_cpw_pick((chunks + splits * *nw - 1) / (splits * *nw), *nw);
}

// The attention launch of R rows over contexts up to max_len: waves per block, chunks per
// wave and the split count (grid x) that follows from them.
// A captured decode step serves every length of its split count, so its grid is sized for
// nsplit * S positions (S = 32 * nw * cpw) while the shape is chosen from the true length.  The
// two agree because the shape lists of att_b1_shape and of att_batch_shape's att_nw6 branch are in
// increasing split size: a length rounded up to nsplit * S still fails every earlier entry and
// still fits the chosen one.  New entries must keep that order.
struct AttShape {
  int nw, cpw, nsplit;
  int S() const { return 32 * nw * cpw; }  // positions per split
};

static AttShape att_shape(const mx_llm* x, int R, int max_len) {
  AttShape s{4, 1, 0};
  if (R == 1)
    att_b1_shape(x, max_len, &s.nw, &s.cpw);
  else
    att_batch_shape(x, R, max_len, &s.nw, &s.cpw);
  s.nsplit = (max_len + s.S() - 1) / s.S();
  return s;
}

struct RowSet {
  float* h;
  const int32_t* slot;
  const int32_t* pos;
  int R;
  int max_len;  // upper bound of any row's position + 1 (sizes the attention grid)
  int cpw;      // attention chunks per wave (att_shape)
  int nw;       // attention waves per block
  int nsplit;   // attention splits of the launch (grid x)
  bool decode;  // decode rows (one position each, own KV slots), not a prefill's prompt rows
};

static RowSet row_set(const mx_llm* x, float* h, const int32_t* slot, const int32_t* pos, int R,
                      int max_len, bool decode) {
  const AttShape s = att_shape(x, R, max_len);
  return RowSet{h, slot, pos, R, max_len, s.cpw, s.nw, s.nsplit, decode};
}

static void attach_ws(mx_llm* x, GemvArgs& g) {
  g.rows_lds_pad = x->rows_lds_pad;
  g.rows_pw = x->rows_pw;
  g.rows_pw_f8 = x->rows_pw_f8;
  g.rows_target = x->rows_target;
  g.rows_nt_max = x->rows_nt_max;
  g.rows_head_target = x->rows_head_target;
  g.rows_head_mt = x->rows_head_mt;
  g.rows_atomic = x->rows_atomic;
  g.gemv_cus = x->gemv_balance ? x->cus : 0;
  g.head_b1 = x->head_b1;
  g.ws = x->rows_ws;
  g.ws_floats = x->rows_ws_floats;
  g.tickets = x->rows_tickets;
  g.tickets_n = x->rows_tickets_n;
}

// option rows_nt1: this kind's 17-32-row launch in two 16-row batch tiles instead of one
// 32-row tile: twice the blocks (every CU streams; two 8-wave blocks fit a CU at 128 VGPRs),
// each batch tile reading the weights once more (the two tiles' blocks run together, so the
// second read is served on-die in part).  Measured at 20-32 rows, L 300 / 900: qkv + o-proj +
// down (mask 11, the default) 4-5 % per step; gate/up and the lm_head lose
// (profiles/r05_rows_nt1.log)
// Above 32 rows (prefill, 64-row decode) the layer launches take 32-row batch tiles when
// rows_nt_max is 0 (auto) and the weights are e4m3 or the rows at most 128: measured per
// prefill, bf16 48 / 64 ids 3.19 / 3.34 -> 2.75 / 2.77 ms, 128 equal, 256 / 512 slower
// (8.03 -> 8.52 ms); e4m3 faster at every length (48 ids -20 %, 512 ids -5 %)
// (profiles/r06_prefill_batch_tiles.log)
static void nt_cap(const mx_llm* x, GemvArgs& g, int kind_bit, int R) {
  if ((x->rows_nt1 >> kind_bit) & 1 && R <= 32) g.rows_nt_max = 1;
  else if (x->rows_nt_max == 0 && kind_bit < 4 && R > 32 && (x->c.wdtype == WT_FP8 || R <= 128))
    g.rows_nt_max = 2;
  if (kind_bit < 4 && x->rows_target_k[kind_bit] > 0) g.rows_target = x->rows_target_k[kind_bit];
}

// ---- GEMV launch arguments: one builder per projection kind ---------------------------
// Each returns what the kind's launch over R rows carries wherever it is enqueued (the step,
// the prefills, the probes): weights, fragment-major copy and scales, N / K, strides, norm
// weight, workspace, tile options.  The callers add X / Y, the row tables and what is theirs
// alone.  A field no builder or caller sets stays zero: the kernels branch on null pointers.
static GemvArgs gemv_base(mx_llm* x, int kind_bit, int R, const void* W, const void* Wf,
                          const float* wscale, int N, int K) {
  GemvArgs g{};
  attach_ws(x, g);
  nt_cap(x, g, kind_bit, R);
  g.R = R; g.W = W; g.wscale = wscale; g.wdtype = x->c.wdtype; g.N = N; g.K = K; g.xstride = K;
  if (x->rows_frag) g.Wf = Wf;
  if (kind_bit < 4) {  // (the lm_head launch carries neither)
    g.force_legacy = x->legacy_gemv;
    g.wpb = x->gemv_wpb;
  }
  return g;
}

// QKV + RoPE + KV append of layer li (the caller: X, row_slot, row_pos, attach_qkv_parts)
static GemvArgs qkv_args(mx_llm* x, int li, int R) {
  const auto& c = x->c;
  const LayerW& l = x->L[li];
  GemvArgs g = gemv_base(x, 0, R, l.wqkv, l.wqkv_f, l.sqkv, (c.heads + 2 * c.kv_heads) * 128, c.hidden);
  g.eps = c.eps; g.norm_w = l.attn_norm;
  g.rope_cos = x->rope_cos; g.rope_sin = x->rope_sin;
  g.kcache = x->kcache + x->kv_layer_elems * li; g.vcache = x->vcache + x->kv_layer_elems * li;
  g.heads = c.heads; g.kv_heads = c.kv_heads; g.max_pos = c.max_pos; g.Q = x->q;
  return g;
}

// Decode rows at >= 2 rows: the qkv GEMM's K ranges store raw partials for the attention
// launch to sum (no split-K seam), when the option is on and the ranges fit the buffers.
static bool attach_qkv_parts(const mx_llm* x, GemvArgs& g) {
  if (g.R < 2 || !x->rows_qkv_parts || x->legacy_gemv || v4::rows_qkv_nkc_v4(g) > mx_llm::qkv_nkc_cap)
    return false;
  g.qkv_parts = x->qkv_parts;
  g.qkv_ss = x->qkv_ss;
  return true;
}

// O projection + residual (the caller: X, Y and the attention-merge fields)
static GemvArgs o_args(mx_llm* x, int li, int R) {
  const LayerW& l = x->L[li];
  GemvArgs g = gemv_base(x, 1, R, l.wo, l.wo_f, l.so, x->c.hidden, x->c.heads * 128);
  g.ystride = x->c.hidden; g.rpw = x->rpw_o;
  return g;
}

// gate/up + SiLU*up (the caller: X, Y)
static GemvArgs gu_args(mx_llm* x, int li, int R) {
  const LayerW& l = x->L[li];
  GemvArgs g = gemv_base(x, 2, R, l.wgu, l.wgu_f, l.sgu, 2 * x->c.ffn, x->c.hidden);
  g.eps = x->c.eps; g.norm_w = l.mlp_norm; g.rpw = x->rpw_gu;
  return g;
}

// down + residual (the caller: X, Y)
static GemvArgs down_args(mx_llm* x, int li, int R) {
  const LayerW& l = x->L[li];
  GemvArgs g = gemv_base(x, 3, R, l.wd, l.wd_f, l.sd, x->c.hidden, x->c.ffn);
  g.ystride = x->c.hidden; g.rpw = x->rpw_down;
  return g;
}

// lm_head + penalty + argmax (the caller: X, row_slot, best, logits; the step also row_pos, V,
// the grammar and the row window)
static GemvArgs head_args(mx_llm* x, int R) {
  const auto& c = x->c;
  GemvArgs g = gemv_base(x, 4, R, x->lm, x->lm_f, x->slm, c.vocab, c.hidden);
  g.eps = c.eps; g.norm_w = x->norm; g.seen = x->seen; g.penalty = x->penalty;
  g.samp_temp = x->samp_temp; g.logits_all = x->logits_all;
  return g;
}

// Optional per-launch timing (eager runs only): prof->ev[k] brackets launch class k.
enum { PK_QKV = 0, PK_ATTN, PK_O, PK_GU, PK_DOWN, PK_HEAD, PK_COMMIT, PK_ENGINE, PK_N };
struct Prof {
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> ev;
  void begin(int k, hipStream_t st) {
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    (void)hipEventRecord(a, st);
    ev.push_back({k, {a, b}});
  }
  void end(hipStream_t st) { (void)hipEventRecord(ev.back().second.second, st); }
};
#define PROF_BEGIN(k) if (prof) prof->begin(k, st)
#define PROF_END() if (prof) prof->end(st)

static hipError_t enqueue_layers(mx_llm* x, const RowSet& rs, hipStream_t st, Prof* prof) {
  const auto& c = x->c;
  const int H = c.hidden, QD = c.heads * 128;
  const int qkv_rows = QD + 2 * c.kv_heads * 128;
  hipError_t e = hipSuccess;
  for (int li = 0; li < c.layers && e == hipSuccess; ++li) {
    // QKV + RoPE + KV append
    GemvArgs g = qkv_args(x, li, rs.R);
    g.X = rs.h; g.row_slot = rs.slot; g.row_pos = rs.pos;
    // decode at >= 2 rows: the K ranges' raw partials go to the attention launch (no seam)
    const bool parts = rs.decode && attach_qkv_parts(x, g);
    PROF_BEGIN(PK_QKV);
    e = launch_gemv(g, EPI_QKV, true, st);
    PROF_END();
    if (e != hipSuccess) break;
    AttnArgs at{};
    if (parts) {
      at.qkv_parts = x->qkv_parts; at.qkv_ss = x->qkv_ss; at.qkv_nkc = v4::rows_qkv_nkc_v4(g);
      at.qkv_n = qkv_rows; at.hidden = H; at.eps = c.eps;
      at.rope_cos = x->rope_cos; at.rope_sin = x->rope_sin;
    }
    at.Q = x->q; at.kcache = g.kcache; at.vcache = g.vcache; at.row_slot = rs.slot; at.row_pos = rs.pos;
    at.heads = c.heads; at.kv_heads = c.kv_heads; at.max_pos = c.max_pos;
    at.scale = 1.0f / sqrtf(128.0f);
    at.cpw = rs.cpw;
    at.nw = rs.nw;
    // (splits shorter than ATT_S_MIN, one-row steps only: the row's partial slots then use the
    // stride of 64-position splits, which one row fits in the buffers sized for max_rows >= 2)
    at.split_stride = 32 * rs.nw * rs.cpw < ATT_S_MIN ? c.max_pos / 64 : c.max_pos / ATT_S_MIN;
    // O projection + residual; it merges the attention splits itself (no ticket round trip)
    // at one row, and at 2-16 rows when its tiling allows (option rows_merge)
    GemvArgs o = o_args(x, li, rs.R);
    o.X = x->att; o.Y = rs.h;
    o.att_S = 32 * rs.nw * rs.cpw; o.att_stride = at.split_stride; o.att_nsm = rs.nsplit;
    o.heads = c.heads; o.kv_heads = c.kv_heads; o.row_pos = rs.pos;
    const bool b1_merge = rs.R == 1 && !x->legacy_gemv && x->o_merge && rs.nsplit <= 8;
    const bool rows_merge = rs.R >= 2 && rs.nsplit > 1 && !x->legacy_gemv && x->rows_merge &&
                            v4::rows_merge_ok_v4(o);
    at.no_merge = (b1_merge || rows_merge) ? 1 : 0;
    at.part_ml = x->part_ml; at.part_acc = x->part_acc; at.counter = x->att_cnt;
    at.out = x->att;
    PROF_BEGIN(PK_ATTN);
    e = launch_attention(at, rs.R, rs.max_len, st);
    PROF_END();
    if (e != hipSuccess) break;
    if (b1_merge || rows_merge) {
      if (b1_merge && o.rpw == 0) o.rpw = 2;  // 192 blocks of 8 waves: measured 20-37 us/step
                                              // faster than 1 row per wave (fewer re-reads)
      o.att_ml = x->part_ml; o.att_acc = x->part_acc;
    }
    PROF_BEGIN(PK_O);
    e = launch_gemv(o, EPI_RESID, false, st);
    PROF_END();
    if (e != hipSuccess) break;
    // gate/up + SiLU*up
    GemvArgs gu = gu_args(x, li, rs.R);
    gu.X = rs.h; gu.Y = x->act;
    PROF_BEGIN(PK_GU);
    e = launch_gemv(gu, EPI_SILU, true, st);
    PROF_END();
    if (e != hipSuccess) break;
    // down + residual
    GemvArgs d = down_args(x, li, rs.R);
    d.X = x->act; d.Y = rs.h;
    PROF_BEGIN(PK_DOWN);
    e = launch_gemv(d, EPI_RESID, false, st);
    PROF_END();
  }
  return e;
}

static GrammarArgs grammar_args(const mx_llm* x) {
  GrammarArgs g{};
  if (x->gram_on) {
    g.origin = x->gram_origin; g.base = x->gram.code_base; g.codes = x->gram.codes;
    g.phases = x->gram.phases; g.cmin = x->gram.code_min; g.stop = x->gram.stop_id;
  }
  return g;
}

// The sampler node of a step (part of the graph key): none when every row is greedy,
// sample_kernel, or sample_chain_kernel when a sampling row has a non-neutral top-k / min-p.
enum { SMP_NONE = 0, SMP_PLAIN = 1, SMP_CHAIN = 2 };

static hipError_t enqueue_sampler(mx_llm* x, const float* lg, const int32_t* slot,
                                  const int32_t* pos, int R, unsigned long long* best,
                                  int sampler, hipStream_t st) {
  SampleChainArgs ca{};
  SampleArgs& sa = ca.s;
  sa.logits = lg; sa.row_slot = slot; sa.row_pos = pos; sa.temp = x->samp_temp;
  sa.top_p = x->samp_top_p; sa.seed = x->samp_seed; sa.best = best; sa.V = x->c.vocab;
  sa.gram = grammar_args(x);
  if (sampler != SMP_CHAIN) return launch_sample(sa, R, st);
  ca.top_k = x->samp_top_k; ca.min_p = x->samp_min_p;
  return launch_sample_chain(ca, R, st);
}

// lm_head + penalty + argmax for R rows, then -- only when one of them samples -- the
// sampler (greedy rows return at once).  `best` points into x->best; its offset selects the
// rows of x->logits used.
// `window`: every row of the launch that commits is constrained, so only the ids a grammar can
// allow are computed (x->win_lo, x->win_n); otherwise the whole vocabulary, constrained rows masked.
// (`lg`: where the launch keeps its rows' penalised logits, [R][vocab])
static hipError_t enqueue_head_at(mx_llm* x, const float* h, const int32_t* slot,
                                  const int32_t* pos, int R, unsigned long long* best, float* lg,
                                  int sampler, bool window, hipStream_t st) {
  const auto& c = x->c;
  GemvArgs g = head_args(x, R);
  g.X = h; g.row_slot = slot; g.best = best; g.logits = lg;
  g.V = c.vocab; g.row_pos = pos; g.gram = grammar_args(x);
  if (window) {
    // row-major weights and scales by pointer; the fragment-major copy by tile offset
    g.id0 = x->win_lo; g.N = x->win_n;
    g.W = (const uint8_t*)x->lm + (size_t)x->win_lo * c.hidden * x->esz;
    if (g.wscale) g.wscale += x->win_lo;
    g.wf_t0 = x->win_lo / 16; g.wf_T = (c.vocab + 15) / 16;
    ++x->win_heads;
  }
  hipError_t e = launch_gemv(g, EPI_ARGMAX, true, st);
  if (e != hipSuccess || sampler == SMP_NONE) return e;  // all-greedy steps carry no sampler node
  return enqueue_sampler(x, lg, slot, pos, R, best, sampler, st);
}

static hipError_t enqueue_head(mx_llm* x, const float* h, const int32_t* slot,
                               const int32_t* pos, int R, unsigned long long* best,
                               int sampler, bool window, hipStream_t st) {
  float* lg = x->logits + (size_t)(best - x->best) * x->c.vocab;
  return enqueue_head_at(x, h, slot, pos, R, best, lg, sampler, window, st);
}

// Longest attention span of the next step over rows [0, n_rows) (host mirror of row_pos).
static int decode_max_len(const mx_llm* x, int n_rows) {
  int m = 1;
  for (int r = 0; r < n_rows; ++r)
    if (x->row_active[r]) m = std::max(m, x->pos_mirror[r] + 1);
  return m;
}

// A step runs the lm_head over the grammar's row window when every active row is constrained
// (parked rows commit nothing and do not count).
static bool window_of(const mx_llm* x, int n_rows) {
  if (!x->gram_on || !x->grammar_head || x->win_n <= 0) return false;
  bool any = false;
  for (int r = 0; r < n_rows; ++r)
    if (x->row_active[r]) {
      if (x->row_origin[r] < 0) return false;
      any = true;
    }
  return any;
}

static int sampler_of(const mx_llm* x, int n_rows) {
  int s = SMP_NONE;
  for (int r = 0; r < n_rows; ++r)
    if (x->row_samples[r]) s = std::max(s, x->row_chain[r] ? (int)SMP_CHAIN : (int)SMP_PLAIN);
  return s;
}

static EngineArgs engine_args(const mx_llm* x) {
  const auto& c = x->c;
  EngineArgs a{};
  a.wqkv = x->wqkv_all; a.wo = x->wo_all; a.wgu = x->wgu_all; a.wd = x->wd_all;
  a.sqkv = x->sqkv_all; a.so = x->so_all; a.sgu = x->sgu_all; a.sd = x->sd_all;
  a.attn_norm = x->attn_norm_all; a.mlp_norm = x->mlp_norm_all;
  a.rope_cos = x->rope_cos; a.rope_sin = x->rope_sin;
  a.kcache = x->kcache; a.vcache = x->vcache; a.kv_layer_elems = x->kv_layer_elems;
  a.row_slot = x->row_slot; a.row_pos = x->row_pos; a.h = x->h_dec;
  a.g_qkv = x->g_qkv; a.g_att = x->g_att; a.g_h1 = x->g_h1; a.g_act = x->g_act; a.g_h2 = x->g_h2;
  a.part = x->eng_part; a.tickets = x->eng_tickets; a.epoch = x->eng_epoch; a.status = x->eng_status_d;
  a.layers = c.layers; a.H = c.hidden; a.heads = c.heads; a.kv_heads = c.kv_heads; a.F = c.ffn;
  a.max_pos = c.max_pos; a.smax = (c.max_pos + 127) / 128; a.ring_slots = x->engine_slots;
  a.f8 = c.wdtype == WT_FP8 ? 1 : 0; a.eps = c.eps; a.depth = x->engine_depth; a.loaders = x->engine_loaders;
  a.xb = engine_xb_floats(c.heads, c.kv_heads, c.ffn);
  a.timeout_ticks = x->engine_timeout_ticks;
  a.trace = x->eng_trace;
  a.dbg = x->engine_dbg;
  return a;
}

// The fields every commit launch shares; the callers set best, the row pointers, h, dst_row
// and abort_word.
static CommitArgs commit_args(const mx_llm* x) {
  const auto& c = x->c;
  CommitArgs cm{};
  cm.seen = x->seen; cm.hist = x->hist_dev; cm.embed = x->embed; cm.hidden = c.hidden;
  cm.vocab = c.vocab; cm.max_pos = c.max_pos; cm.pos_advance = 1; cm.scratch_slot = c.max_slots;
  cm.last_n = x->last_n; cm.recent = x->recent;
  return cm;
}

// One decode step over rs's rows (the attention shape is the caller's: mx_llm_decode).
static hipError_t enqueue_decode(mx_llm* x, const RowSet& rs, int sampler, bool window,
                                 hipStream_t st, Prof* prof) {
  const int n_rows = rs.R;
  hipError_t e = hipSuccess;
  if (n_rows == 1 && x->b1_engine) {  // every layer in one persistent launch
    PROF_BEGIN(PK_ENGINE);
    e = launch_engine_b1(engine_args(x), x->engine_grid, st);
    PROF_END();
  } else {
    e = enqueue_layers(x, rs, st, prof);
  }
  PROF_BEGIN(PK_HEAD);
  if (e == hipSuccess)
    e = enqueue_head(x, x->h_dec, x->row_slot, x->row_pos, n_rows, x->best, sampler, window, st);
  PROF_END();
  PROF_BEGIN(PK_COMMIT);
  if (e == hipSuccess) {
    CommitArgs cm = commit_args(x);
    cm.best = x->best; cm.row_slot = x->row_slot; cm.row_pos = x->row_pos;
    cm.row_token = x->row_token; cm.h = x->h_dec;
    // an engine launch that gave up commits nothing (its history entry reads -1)
    cm.abort_word = (n_rows == 1 && x->b1_engine) ? x->eng_status_d : nullptr;
    e = launch_commit(cm, n_rows, st);
  }
  PROF_END();
  return e;
}

// Host mirror of a slot's prompt: ids [pos0, pos0 + n) recorded, the slot then holds pos0 + n.
static void record_prompt(mx_llm* x, int slot, int pos0, const int32_t* ids, int n) {
  std::memcpy(x->slot_ids.data() + (size_t)slot * x->c.max_pos + pos0, ids, (size_t)n * 4);
  x->slot_len[slot] = pos0 + n;
}

// The active decode row bound to `slot`, or -1.
static int row_of_slot(const mx_llm* x, int slot) {
  for (int r = 0; r < x->c.max_batch; ++r)
    if (x->row_active[r] && x->row_slot_h[r] == slot) return r;
  return -1;
}

// ---- what the prefill entry points share -----------------------------------------------
// The refusal of a request's sampling parameters, or null.
static const char* check_sampling(const mx_sampling& sp, const mx_sampling_ext& xe) {
  if (!(sp.repetition_penalty > 0.f) || !(sp.top_p > 0.f) || sp.temperature < 0.f)
    return "sampling: need repetition_penalty > 0, top_p > 0, temperature >= 0";
  if (xe.top_k < 0 || !(xe.min_p >= 0.f && xe.min_p <= 1.f) || xe.penalty_last_n < 0 ||
      xe.penalty_last_n >= PEN_RING)
    return "sampling: need top_k >= 0, 0 <= min_p <= 1, 0 <= penalty_last_n <= 255";
  return nullptr;
}

static bool ids_in_vocab(const mx_llm* x, const int32_t* ids, int n) {
  for (int i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= x->c.vocab) return false;
  return true;
}

// The sampler node a stream with these parameters needs.
static int sampler_kind(const mx_sampling& sp, const mx_sampling_ext& xe) {
  if (!(sp.temperature > 0.f)) return SMP_NONE;
  return xe.top_k > 0 || xe.min_p > 0.f ? SMP_CHAIN : SMP_PLAIN;
}

// Host mirror of a decode row bound to `slot`, its next token at position `pos`.
static void bind_row(mx_llm* x, int row, int slot, int pos, int sampler, int origin) {
  x->pos_mirror[row] = pos;
  x->row_active[row] = 1;
  x->row_samples[row] = sampler != SMP_NONE ? 1 : 0;
  x->row_chain[row] = sampler == SMP_CHAIN ? 1 : 0;
  x->row_origin[row] = origin;
  x->row_slot_h[row] = slot;
}

// One prompt span: n ids onto `slot` behind the pos0 positions it holds.  The rows carry
// pos = pos0 + i; the attention grid is sized by max_len = pos0 + n (behind a history: prompt
// rows attending over more positions than there are rows, i.e. the multi-row kernel with the
// split counts decode rows reach, the one-row kernels for a one-id span).  A span that is not
// the prompt's last runs the layers and appends K / V, nothing else.  The last one builds the
// slot's penalty state over the whole prompt [0, pos0 + n), sets the grammar origin to
// pos0 + n, runs head, sampler and commit on its last row and binds `row`.  A whole prompt
// (pos0 = 0, last) has its ids in pre_ids, and embed_rows marks them seen on the way; behind a
// history the id history (the host mirror) is uploaded once to cont_ids and marked behind the
// layers.  The callers have made every refusal: from here on only the runtime can fail.
static int prefill_span(mx_llm* x, int slot, int row, const int32_t* ids, int n, int pos0,
                        bool last, const mx_sampling& sp, const mx_sampling_ext& xe,
                        hipStream_t st) {
  const auto& c = x->c;
  const int max_len = pos0 + n, win = xe.penalty_last_n;
  const bool hist = last && pos0 != 0;  // the prompt's earlier ids are needed again
  MX_TRY(x, hipSetDevice(x->device));
  if (hist && !x->cont_ids) MX_TRY(x, x->alloc(&x->cont_ids, (size_t)c.max_pos));
  if (last) {
    MX_TRY(x, launch_set_slot_params(x->penalty, x->samp_temp, x->samp_top_p, x->samp_seed, slot,
                                     sp.repetition_penalty, sp.temperature,
                                     sp.top_p < 1.f ? sp.top_p : 1.f, sp.seed, st));
    // every prefill starts the slot clean: seen flags / window counts here, the ring below
    MX_TRY(x, hipMemsetAsync(x->seen + (size_t)slot * c.vocab, 0, c.vocab, st));
  }
  int32_t* dev_ids = x->pre_ids;  // the span's ids on the device
  if (hist) {  // the slot's history [0, pos0) and the span's ids behind it, one contiguous copy
    MX_TRY(x, hipMemcpyAsync(x->cont_ids, x->slot_ids.data() + (size_t)slot * c.max_pos,
                             (size_t)pos0 * 4, hipMemcpyHostToDevice, st));
    dev_ids = x->cont_ids + pos0;
  }
  MX_TRY(x, hipMemcpyAsync(dev_ids, ids, (size_t)n * 4, hipMemcpyHostToDevice, st));
  MX_TRY(x, launch_set_rows(x->pre_slot, x->pre_pos, n, slot, pos0, st));
  // (seen marks here only for a whole prompt without a window; otherwise behind the layers)
  MX_TRY(x, launch_embed_rows(dev_ids, n, slot, x->embed, c.hidden, c.vocab,
                              last && pos0 == 0 && win == 0 ? x->seen : nullptr, x->h_pre, st));
  MX_TRY(x, enqueue_layers(x, row_set(x, x->h_pre, x->pre_slot, x->pre_pos, n, max_len, false),
                           st, nullptr));
  if (!last) {
    record_prompt(x, slot, pos0, ids, n);
    return MX_OK;
  }
  // the extras, the ring and (window mode: the bytes are counts, filled serially, since
  // embed_rows marks from many blocks) the window are first read by the head and the commit:
  // set behind the layers, the launches in front of them are the same with and without extras
  MX_TRY(x, launch_set_slot_ext(x->samp_top_k, x->samp_min_p, x->last_n, slot, xe.top_k,
                                xe.min_p, win, st));
  MX_TRY(x, hipMemsetAsync(x->recent + (size_t)slot * PEN_RING, 0, PEN_RING * 4, st));
  const int32_t* all_ids = dev_ids - pos0;  // the whole prompt [0, max_len)
  if (win > 0)  // its last N positions: they may straddle a seam
    MX_TRY(x, launch_window_prefill(all_ids, max_len, win, slot, c.vocab, x->seen, x->recent, st));
  else if (pos0 != 0)
    MX_TRY(x, launch_mark_seen(all_ids, max_len, slot, c.vocab, x->seen, st));
  // a constrained slot counts its phases from the prompt's end (-1: unconstrained)
  const int origin = x->gram_on && x->slot_grammar[slot] ? max_len : -1;
  if (x->gram_on) MX_TRY(x, launch_set_slot_origin(x->gram_origin, slot, origin, st));
  MX_TRY(x, hipMemsetAsync(x->best + row, 0, 8, st));
  const int sampler = sampler_kind(sp, xe);
  MX_TRY(x, enqueue_head(x, x->h_pre + (size_t)(n - 1) * c.hidden, x->pre_slot + (n - 1),
                         x->pre_pos + (n - 1), 1, x->best + row, sampler,
                         origin >= 0 && x->grammar_head && x->win_n > 0, st));
  // bind decode row -> slot at the prompt's last position, then commit (advances to pos0 + n)
  MX_TRY(x, launch_set_rows(x->row_slot + row, x->row_pos + row, 1, slot, max_len - 1, st));
  CommitArgs cm = commit_args(x);
  cm.best = x->best + row; cm.row_slot = x->row_slot + row; cm.row_pos = x->row_pos + row;
  cm.row_token = x->row_token + row; cm.h = x->h_dec + (size_t)row * c.hidden;
  MX_TRY(x, launch_commit(cm, 1, st));
  bind_row(x, row, slot, max_len, sampler, origin);
  record_prompt(x, slot, pos0, ids, n);
  return MX_OK;
}

extern "C" int mx_llm_prefill(mx_llm* x, int slot, int row, const int32_t* ids, int n,
                              const mx_sampling* sp, void* stream) {
  return mx_llm_prefill_ex(x, slot, row, ids, n, sp, nullptr, stream);
}

extern "C" int mx_llm_prefill_ex(mx_llm* x, int slot, int row, const int32_t* ids, int n,
                                 const mx_sampling* sp, const mx_sampling_ext* ext,
                                 void* stream) {
  if (!x || !ids || !sp) return MX_ERR_ARG;
  const mx_sampling_ext neutral{0, 0.f, 0};
  const mx_sampling_ext& xe = ext ? *ext : neutral;
  if (const char* m = check_sampling(*sp, xe)) MX_FAIL(x, MX_ERR_ARG, m);
  if (!x->final) MX_FAIL(x, MX_ERR_STATE, "not finalized");
  const auto& c = x->c;
  if (slot < 0 || slot >= c.max_slots || row < 0 || row >= c.max_batch)
    MX_FAIL(x, MX_ERR_ARG, "slot/row out of range");
  if (n < 1 || n > c.max_prefill || n >= c.max_pos) MX_FAIL(x, MX_ERR_ARG, "bad prompt length");
  if (!ids_in_vocab(x, ids, n)) MX_FAIL(x, MX_ERR_ARG, "prompt id out of vocab");
  return prefill_span(x, slot, row, ids, n, 0, true, *sp, xe, (hipStream_t)stream);
}

// Packed prefill: the segments' prompt rows as ONE row set through the layers (each row
// carries its own slot and position: the qkv epilogue appends K / V there, the attention reads
// the row's slot up to its position), then one lm_head launch over the segments' last rows, one
// sampler node, one commit through the rows' remap.  Around them, one launch each: the slots'
// clear, the per-row / per-segment setup, the window fill (only with a windowed segment), the
// tail gather + bind, and (kept logits only) their copy to the decode rows' lines.
// Both entry points run this body.  An entry is a final chunk: n ids behind the pos0 positions
// its slot holds (mx_llm_prefill_batch: every pos0 is 0, and the launches are the ones it has
// always enqueued).  Behind a history the rows carry pos0 + i, the tail, head and commit sit at
// pos0 + n, and the penalty state covers [0, pos0 + n): the ids [0, pos0) come from the host id
// history, staged back to back in pk_hist by one upload (never the host-mapped hist: DESIGN.md
// §3 "Where the id history lives"), marked by one more launch (whole-sequence segments) or walked
// by the window fill.
struct PackEntry {
  int slot, row, n, pos0;
  const int32_t* ids;
  const mx_sampling* sp;
  const mx_sampling_ext* xe;
};

static int prefill_pack(mx_llm* x, const std::vector<PackEntry>& es, bool continuation,
                        void* stream) {
  const auto& c = x->c;
  const int n_segs = (int)es.size();
  // every refusal first: a refused call enqueues nothing and changes no host state
  std::vector<char> slot_used(c.max_slots, 0), row_used(c.max_batch, 0);
  long long R64 = 0;
  int max_len = 0, max_pos0 = 0, sampler = SMP_NONE;
  size_t hist_ids = 0;
  bool any_window = false, any_marks = false, all_constrained = x->gram_on;
  for (const PackEntry& g : es) {
    if (!g.ids) MX_FAIL(x, MX_ERR_ARG, "segment without ids");
    if (const char* m = check_sampling(*g.sp, *g.xe)) MX_FAIL(x, MX_ERR_ARG, m);
    if (g.slot < 0 || g.slot >= c.max_slots || g.row < 0 || g.row >= c.max_batch)
      MX_FAIL(x, MX_ERR_ARG, "slot/row out of range");
    if (slot_used[g.slot] || row_used[g.row])
      MX_FAIL(x, MX_ERR_ARG, "slot/row named twice in one call");
    slot_used[g.slot] = row_used[g.row] = 1;
    if (g.n < 1 || g.n >= c.max_pos) MX_FAIL(x, MX_ERR_ARG, "bad prompt length");
    R64 += g.n;
    if (R64 > c.max_prefill) MX_FAIL(x, MX_ERR_ARG, "prompts exceed max_prefill rows");
    if (g.pos0 < 0 || (long long)g.pos0 + g.n >= c.max_pos)
      MX_FAIL(x, MX_ERR_ARG, "chunk does not fit max_pos");
    if (!ids_in_vocab(x, g.ids, g.n)) MX_FAIL(x, MX_ERR_ARG, "prompt id out of vocab");
    max_len = std::max(max_len, g.pos0 + g.n);
    max_pos0 = std::max(max_pos0, g.pos0);
    hist_ids += (size_t)g.pos0;
    sampler = std::max(sampler, sampler_kind(*g.sp, *g.xe));
    any_window = any_window || g.xe->penalty_last_n > 0;
    any_marks = any_marks || (g.pos0 > 0 && g.xe->penalty_last_n == 0);
    all_constrained = all_constrained && x->slot_grammar[g.slot];
  }
  const int R = (int)R64;
  if (continuation) {
    // (pos0 = 0 starts the slot over, as every prefill does)
    for (const PackEntry& g : es) {
      if (g.pos0 == 0) continue;
      if (g.pos0 != x->slot_len[g.slot])
        MX_FAIL(x, MX_ERR_STATE, "chunk at position " + std::to_string(g.pos0) +
                                     ": the slot holds " + std::to_string(x->slot_len[g.slot]));
      if (row_of_slot(x, g.slot) >= 0)
        MX_FAIL(x, MX_ERR_STATE, "chunk onto a slot bound to an active row");
    }
    // the launch's own argument checks, as mx_llm_prefill_chunk makes them
    const AttShape sh = att_shape(x, R, max_len);
    const int stride = sh.S() < ATT_S_MIN ? c.max_pos / 64 : c.max_pos / ATT_S_MIN;
    if (sh.nsplit > ATT_MAX_SPLITS || (c.max_pos + sh.S() - 1) / sh.S() > stride)
      MX_FAIL(x, MX_ERR_ARG, "pack: the context needs more attention splits than one launch merges");
  }
  hipStream_t st = (hipStream_t)stream;
  MX_TRY(x, hipSetDevice(x->device));
  const size_t seg_words = (size_t)c.max_batch * (sizeof(PackSeg) / 4);
  if (!x->pk_tab) {
    MX_TRY(x, x->alloc(&x->pk_tab, seg_words + (size_t)c.max_prefill * (sizeof(PackRow) / 4)));
    MX_TRY(x, x->alloc(&x->pk_idx, (size_t)3 * c.max_batch));
    MX_TRY(x, x->alloc(&x->pk_best, (size_t)c.max_batch));
    MX_TRY(x, x->alloc(&x->pk_h, (size_t)c.max_batch * c.hidden));
    MX_TRY(x, x->alloc(&x->pk_logits, (size_t)c.max_batch * c.vocab));
  }
  if (hist_ids && !x->pk_hist) MX_TRY(x, x->alloc(&x->pk_hist, (size_t)c.max_batch * c.max_pos));
  // the table: the segments, then their rows; the histories back to back
  x->pk_host.assign(seg_words + (size_t)R * (sizeof(PackRow) / 4), 0);
  x->pk_hist_host.resize(hist_ids);
  PackSeg* hs = reinterpret_cast<PackSeg*>(x->pk_host.data());
  PackRow* hr = reinterpret_cast<PackRow*>(x->pk_host.data() + seg_words);
  size_t hoff = 0;
  for (int s = 0, r = 0; s < n_segs; ++s) {
    const PackEntry& g = es[s];
    PackSeg& t = hs[s];
    t.slot = g.slot; t.row = g.row; t.first = r; t.n = g.n;
    // a constrained slot counts its phases from the prompt's end (-1: unconstrained)
    t.origin = x->gram_on && x->slot_grammar[g.slot] ? g.pos0 + g.n : -1;
    t.top_k = g.xe->top_k; t.last_n = g.xe->penalty_last_n;
    t.pen = g.sp->repetition_penalty; t.temp = g.sp->temperature;
    t.top_p = g.sp->top_p < 1.f ? g.sp->top_p : 1.f; t.min_p = g.xe->min_p;
    t.seed_lo = (uint32_t)g.sp->seed; t.seed_hi = (uint32_t)(g.sp->seed >> 32);
    t.pos0 = g.pos0; t.hist = (int32_t)hoff;
    if (g.pos0 > 0)
      std::memcpy(x->pk_hist_host.data() + hoff, x->slot_ids.data() + (size_t)g.slot * c.max_pos,
                  (size_t)g.pos0 * 4);
    hoff += (size_t)g.pos0;
    for (int i = 0; i < g.n; ++i, ++r)
      hr[r] = PackRow{g.ids[i], g.slot, g.pos0 + i, g.xe->penalty_last_n > 0 ? 0 : 1};
  }
  const PackSeg* dsegs = reinterpret_cast<const PackSeg*>(x->pk_tab);
  const PackRow* drows = reinterpret_cast<const PackRow*>(x->pk_tab + seg_words);
  // (pageable source, as prefill_span's copy of the caller's ids: the runtime has read it
  // when the call returns, so the next call may rebuild the table)
  MX_TRY(x, hipMemcpyAsync(x->pk_tab, x->pk_host.data(), x->pk_host.size() * 4,
                           hipMemcpyHostToDevice, st));
  if (hist_ids)
    MX_TRY(x, hipMemcpyAsync(x->pk_hist, x->pk_hist_host.data(), hist_ids * 4,
                             hipMemcpyHostToDevice, st));
  MX_TRY(x, launch_pack_clear(dsegs, n_segs, c.vocab, x->seen, x->recent, st));
  PackSetupArgs ps{};
  ps.rows = drows; ps.segs = dsegs; ps.R = R; ps.n_segs = n_segs; ps.embed = x->embed;
  ps.hidden = c.hidden; ps.vocab = c.vocab; ps.seen = x->seen; ps.h = x->h_pre;
  ps.pre_slot = x->pre_slot; ps.pre_pos = x->pre_pos; ps.penalty = x->penalty;
  ps.temp = x->samp_temp; ps.top_p = x->samp_top_p; ps.seed = x->samp_seed;
  ps.top_k = x->samp_top_k; ps.min_p = x->samp_min_p; ps.last_n = x->last_n;
  ps.origin = x->gram_on ? x->gram_origin : nullptr;
  MX_TRY(x, launch_pack_setup(ps, st));
  // the attention grid is sized by the longest context; shorter rows leave its later splits
  MX_TRY(x, enqueue_layers(x, row_set(x, x->h_pre, x->pre_slot, x->pre_pos, R, max_len, false),
                           st, nullptr));
  if (any_marks)
    MX_TRY(x, launch_pack_hist_marks(dsegs, x->pk_hist, n_segs, max_pos0, c.vocab, x->seen, st));
  if (any_window)
    MX_TRY(x, launch_pack_window(drows, dsegs, x->pk_hist, n_segs, c.vocab, x->seen, x->recent, st));
  int32_t *hslot = x->pk_idx, *hpos = x->pk_idx + c.max_batch, *hrow = x->pk_idx + 2 * c.max_batch;
  PackTailArgs pt{};
  pt.segs = dsegs; pt.h = x->h_pre; pt.hidden = c.hidden; pt.head_h = x->pk_h;
  pt.head_slot = hslot; pt.head_pos = hpos; pt.head_row = hrow; pt.head_best = x->pk_best;
  pt.row_slot = x->row_slot; pt.row_pos = x->row_pos;
  MX_TRY(x, launch_pack_tail(pt, n_segs, st));
  // the window rule of a step (window_of): only when every segment is constrained
  const bool window = all_constrained && x->grammar_head && x->win_n > 0;
  MX_TRY(x, enqueue_head_at(x, x->pk_h, hslot, hpos, n_segs, x->pk_best, x->pk_logits, sampler,
                            window, st));
  if (x->logits_all || sampler != SMP_NONE)
    MX_TRY(x, launch_pack_logits(x->logits, x->pk_logits, hrow, n_segs, c.vocab, st));
  CommitArgs cm = commit_args(x);
  cm.best = x->pk_best; cm.dst_row = hrow; cm.row_slot = x->row_slot; cm.row_pos = x->row_pos;
  cm.row_token = x->row_token; cm.h = x->h_dec;
  MX_TRY(x, launch_commit(cm, n_segs, st));
  for (int s = 0; s < n_segs; ++s) {
    const PackEntry& g = es[s];
    bind_row(x, g.row, g.slot, g.pos0 + g.n, sampler_kind(*g.sp, *g.xe), hs[s].origin);
    record_prompt(x, g.slot, g.pos0, g.ids, g.n);
  }
  return MX_OK;
}

extern "C" int mx_llm_prefill_batch(mx_llm* x, const mx_prefill_seg* segs, int n_segs,
                                    void* stream) {
  if (!x || !segs) return MX_ERR_ARG;
  if (!x->final) MX_FAIL(x, MX_ERR_STATE, "not finalized");
  if (n_segs < 1 || n_segs > x->c.max_batch) MX_FAIL(x, MX_ERR_ARG, "bad n_segs");
  std::vector<PackEntry> es(n_segs);
  for (int s = 0; s < n_segs; ++s) {
    const mx_prefill_seg& g = segs[s];
    es[s] = PackEntry{g.slot, g.row, g.n_ids, 0, g.ids_host, &g.params, &g.ext};
  }
  return prefill_pack(x, es, false, stream);
}

// A pack of final chunks (DESIGN.md §3 "Packed continuation").
extern "C" int mx_llm_prefill_pack(mx_llm* x, const mx_prefill_chunk* chunks, int n_chunks,
                                   void* stream) {
  if (!x || !chunks) return MX_ERR_ARG;
  if (!x->final) MX_FAIL(x, MX_ERR_STATE, "not finalized");
  if (n_chunks < 1 || n_chunks > x->c.max_batch) MX_FAIL(x, MX_ERR_ARG, "bad n_segs");
  std::vector<PackEntry> es(n_chunks);
  for (int s = 0; s < n_chunks; ++s) {
    const mx_prefill_chunk& g = chunks[s];
    if (!g.last) MX_FAIL(x, MX_ERR_ARG, "pack: every chunk must be its prompt's last");
    es[s] = PackEntry{g.slot, g.row, g.n_ids, g.pos0, g.ids_host, &g.params, &g.ext};
  }
  return prefill_pack(x, es, true, stream);
}

// Prompt continuation: a chunk of a prompt behind the pos0 positions its slot already holds
// (prefill_span).  pos0 = 0 with last = 1 IS mx_llm_prefill_ex: the same launches, and the same
// refusals, so the state checks below (which mx_llm_prefill_ex does not make) leave it out.
extern "C" int mx_llm_prefill_chunk(mx_llm* x, const mx_prefill_chunk* ck, void* stream) {
  if (!x || !ck) return MX_ERR_ARG;
  if (!ck->ids_host) MX_FAIL(x, MX_ERR_ARG, "chunk without ids");
  if (!x->final) MX_FAIL(x, MX_ERR_STATE, "not finalized");
  const auto& c = x->c;
  const int slot = ck->slot, row = ck->row, n = ck->n_ids, pos0 = ck->pos0;
  const bool last = ck->last != 0;
  const int32_t* ids = ck->ids_host;
  // every refusal first: a refused call enqueues nothing and changes no host state
  if (slot < 0 || slot >= c.max_slots || (last && (row < 0 || row >= c.max_batch)))
    MX_FAIL(x, MX_ERR_ARG, "slot/row out of range");
  if (n < 1 || n > c.max_prefill) MX_FAIL(x, MX_ERR_ARG, "bad chunk length");
  if (pos0 < 0 || (long long)pos0 + n >= c.max_pos)
    MX_FAIL(x, MX_ERR_ARG, "chunk does not fit max_pos");
  if (!ids_in_vocab(x, ids, n)) MX_FAIL(x, MX_ERR_ARG, "prompt id out of vocab");
  if (last)
    if (const char* m = check_sampling(ck->params, ck->ext)) MX_FAIL(x, MX_ERR_ARG, m);
  if (!(pos0 == 0 && last)) {
    // (pos0 = 0 starts the slot over, as every prefill does)
    if (pos0 != 0 && pos0 != x->slot_len[slot])
      MX_FAIL(x, MX_ERR_STATE, "chunk at position " + std::to_string(pos0) + ": the slot holds " +
                                   std::to_string(x->slot_len[slot]));
    if (row_of_slot(x, slot) >= 0)
      MX_FAIL(x, MX_ERR_STATE, "chunk onto a slot bound to an active row");
    // the launch's own argument checks (launch_attention), made before anything is enqueued: the
    // split count one launch may merge, and the partial slots a (row, kv head) has
    const AttShape sh = att_shape(x, n, pos0 + n);
    const int stride = sh.S() < ATT_S_MIN ? c.max_pos / 64 : c.max_pos / ATT_S_MIN;
    if (sh.nsplit > ATT_MAX_SPLITS || (c.max_pos + sh.S() - 1) / sh.S() > stride)
      MX_FAIL(x, MX_ERR_ARG, "chunk: the context needs more attention splits than one launch merges");
  }
  return prefill_span(x, slot, row, ids, n, pos0, last, ck->params, ck->ext, (hipStream_t)stream);
}

// dst holds src's first n_pos positions afterwards: K / V of every layer (one kv_fork_kernel
// launch, ordered on the stream) and the id history (host mirror).  No penalty state: the
// request's final chunk builds that for its own parameters.
extern "C" int mx_llm_fork_slot(mx_llm* x, int dst, int src, int n_pos, void* stream) {
  if (!x) return MX_ERR_ARG;
  if (!x->final) MX_FAIL(x, MX_ERR_STATE, "not finalized");
  const auto& c = x->c;
  if (dst < 0 || dst >= c.max_slots || src < 0 || src >= c.max_slots)
    MX_FAIL(x, MX_ERR_STATE, "fork: slot out of range");
  if (dst == src) MX_FAIL(x, MX_ERR_STATE, "fork: dst is src");
  if (n_pos < 1 || n_pos > x->slot_len[src])
    MX_FAIL(x, MX_ERR_STATE, "fork of " + std::to_string(n_pos) + " positions: the source holds " +
                                 std::to_string(x->slot_len[src]));
  if (row_of_slot(x, dst) >= 0) MX_FAIL(x, MX_ERR_STATE, "fork: dst is bound to an active row");
  MX_TRY(x, hipSetDevice(x->device));
  KvForkArgs a{};
  a.kcache = x->kcache; a.vcache = x->vcache; a.kv_layer_elems = x->kv_layer_elems;
  a.layers = c.layers; a.kv_heads = c.kv_heads; a.max_pos = c.max_pos;
  a.src = src; a.dst = dst; a.chunks = (n_pos + 31) / 32; a.runs = 2 * c.layers * c.kv_heads;
  MX_TRY(x, launch_kv_fork(a, x->cus, (hipStream_t)stream));
  std::memcpy(x->slot_ids.data() + (size_t)dst * c.max_pos,
              x->slot_ids.data() + (size_t)src * c.max_pos, (size_t)n_pos * 4);
  x->slot_len[dst] = n_pos;
  return MX_OK;
}

// n forks as one kv_fork_many_kernel launch: the table goes up once, the id histories are
// copied on the host.  The refusals are mx_llm_fork_slot's per triple, plus the two that keep
// the launch's units independent: no dst twice, no dst that the call also reads.
extern "C" int mx_llm_fork_slots(mx_llm* x, const int32_t* dst, const int32_t* src,
                                 const int32_t* n_pos, int n, void* stream) {
  if (!x) return MX_ERR_ARG;
  const auto& c = x->c;
  if (!dst || !src || !n_pos || n < 1 || n > c.max_slots)
    MX_FAIL(x, MX_ERR_ARG, "fork_slots: need 1 <= n <= max_slots and three arrays");
  if (!x->final) MX_FAIL(x, MX_ERR_STATE, "not finalized");
  std::vector<char> is_dst(c.max_slots, 0), is_src(c.max_slots, 0);
  for (int i = 0; i < n; ++i) {
    if (dst[i] < 0 || dst[i] >= c.max_slots || src[i] < 0 || src[i] >= c.max_slots)
      MX_FAIL(x, MX_ERR_STATE, "fork: slot out of range");
    if (dst[i] == src[i]) MX_FAIL(x, MX_ERR_STATE, "fork: dst is src");
    if (n_pos[i] < 1 || n_pos[i] > x->slot_len[src[i]])
      MX_FAIL(x, MX_ERR_STATE, "fork of " + std::to_string(n_pos[i]) +
                                   " positions: the source holds " +
                                   std::to_string(x->slot_len[src[i]]));
    if (row_of_slot(x, dst[i]) >= 0) MX_FAIL(x, MX_ERR_STATE, "fork: dst is bound to an active row");
    if (is_dst[dst[i]]) MX_FAIL(x, MX_ERR_STATE, "fork: dst named twice in one call");
    is_dst[dst[i]] = 1;
    is_src[src[i]] = 1;
  }
  for (int i = 0; i < n; ++i)
    if (is_src[dst[i]]) MX_FAIL(x, MX_ERR_STATE, "fork: dst is a src of the same call");
  MX_TRY(x, hipSetDevice(x->device));
  if (!x->fork_tab) MX_TRY(x, x->alloc(&x->fork_tab, (size_t)c.max_slots * (sizeof(KvFork) / 4)));
  std::vector<KvFork> tab(n);
  int max_chunks = 0;
  for (int i = 0; i < n; ++i) {
    tab[i] = KvFork{dst[i], src[i], (n_pos[i] + 31) / 32, 0};
    max_chunks = std::max(max_chunks, tab[i].chunks);
  }
  hipStream_t st = (hipStream_t)stream;
  // (pageable source: the runtime has read it when the call returns)
  MX_TRY(x, hipMemcpyAsync(x->fork_tab, tab.data(), (size_t)n * sizeof(KvFork),
                           hipMemcpyHostToDevice, st));
  KvForkManyArgs a{};
  a.kcache = x->kcache; a.vcache = x->vcache; a.kv_layer_elems = x->kv_layer_elems;
  a.layers = c.layers; a.kv_heads = c.kv_heads; a.max_pos = c.max_pos;
  a.runs = 2 * c.layers * c.kv_heads;
  a.forks = reinterpret_cast<const KvFork*>(x->fork_tab); a.n = n; a.max_chunks = max_chunks;
  MX_TRY(x, launch_kv_fork_many(a, x->cus, st));
  for (int i = 0; i < n; ++i) {
    std::memcpy(x->slot_ids.data() + (size_t)dst[i] * c.max_pos,
                x->slot_ids.data() + (size_t)src[i] * c.max_pos, (size_t)n_pos[i] * 4);
    x->slot_len[dst[i]] = n_pos[i];
  }
  return MX_OK;
}

extern "C" int mx_llm_slot_len(const mx_llm* x, int slot, int* n_pos) {
  if (!x || !n_pos || slot < 0 || slot >= x->c.max_slots) return MX_ERR_ARG;
  *n_pos = x->slot_len[slot];
  return MX_OK;
}

// Advance the host mirror after a step over rows [0, n_rows) was enqueued.
static void mirror_step(mx_llm* x, int n_rows) {
  for (int r = 0; r < n_rows; ++r)
    if (x->row_active[r]) x->pos_mirror[r] = std::min(x->pos_mirror[r] + 1, x->c.max_pos - 1);
}

// A persistent-engine launch that gave up (a bounded wait expired) leaves its status word set.
// Its attention tickets may be non-zero (a split that arrived before the abort), and the next
// launch would then take `t == S - 1` early and merge stale partials: wait for the stream, clear
// the tickets (the epoch finish counter is consistent -- every workgroup counts itself out, abort
// or not), clear the word, report.  Returns 1 (x->err set) when it gave up.
static int engine_gave_up(mx_llm* x, hipStream_t st) {
  if (!x->eng_status_h || !__atomic_load_n(x->eng_status_h, __ATOMIC_ACQUIRE)) return 0;
  (void)hipStreamSynchronize(st);
  (void)hipDeviceSynchronize();
  (void)hipMemset(x->eng_tickets, 0, (size_t)x->c.layers * x->c.kv_heads * 4);
  // the steps that did not commit did not advance their rows: re-read the positions
  std::vector<int32_t> pos(x->c.max_batch, 0);
  if (hipMemcpy(pos.data(), x->row_pos, pos.size() * 4, hipMemcpyDeviceToHost) == hipSuccess)
    for (int r = 0; r < x->c.max_batch; ++r)
      if (x->row_active[r]) x->pos_mirror[r] = pos[r];
  const int s = __atomic_exchange_n(x->eng_status_h, 0, __ATOMIC_ACQ_REL);
  x->err = "persistent engine launch gave up (status " + std::to_string(s) +
           "): a hand-off timed out; that step's token was not committed";
  return 1;
}

extern "C" int mx_llm_check(mx_llm* x, void* stream) {
  if (!x) return MX_ERR_ARG;
  return engine_gave_up(x, (hipStream_t)stream) ? MX_ERR_HIP : MX_OK;
}

static int check_room(mx_llm* x, int n_rows) {
  for (int r = 0; r < n_rows; ++r)
    if (x->row_active[r] && x->pos_mirror[r] >= x->c.max_pos - 1)
      MX_FAIL(x, MX_ERR_STATE, "row " + std::to_string(r) + " reached max_pos");
  return MX_OK;
}

extern "C" int mx_llm_decode(mx_llm* x, int n_rows, void* stream) {
  if (!x) return MX_ERR_ARG;
  if (!x->final) MX_FAIL(x, MX_ERR_STATE, "not finalized");
  if (n_rows < 1 || n_rows > x->c.max_batch) MX_FAIL(x, MX_ERR_ARG, "bad n_rows");
  if (check_room(x, n_rows)) return MX_ERR_STATE;
  hipStream_t st = (hipStream_t)stream;
  MX_TRY(x, hipSetDevice(x->device));
  if (engine_gave_up(x, st)) return MX_ERR_HIP;
  // one graph per (row count, attention split count): kernels read positions from device
  // memory; the split count only sizes the attention grid (the engine sizes its own)
  // the shape comes from the true length, once; the captured launch is sized for every length
  // of its split count (att_shape)
  RowSet rs = row_set(x, x->h_dec, x->row_slot, x->row_pos, n_rows, decode_max_len(x, n_rows), true);
  if (n_rows == 1 && x->b1_engine) {
    rs.cpw = rs.nw = 1;
    rs.nsplit = 0;
  }
  rs.max_len = rs.nsplit * 32 * rs.nw * rs.cpw;
  // (chunks and waves are part of the key: one nsplit can come from several shapes; so is
  // the sampler node: all-greedy graphs have none, the others sample_kernel or the chain)
  // ... and whether the lm_head runs over the grammar's row window
  const int sampler = sampler_of(x, n_rows);
  const bool window = window_of(x, n_rows);
  const int key = ((((n_rows * 16 + rs.cpw) * 16 + rs.nw) * 4096 + rs.nsplit) * 4 + sampler) * 2 + (window ? 1 : 0);
  auto it = x->graphs.find(key);
  if (it == x->graphs.end()) {
    MX_TRY(x, hipStreamSynchronize(st));
    MX_TRY(x, hipStreamBeginCapture(x->cap, hipStreamCaptureModeRelaxed));
    hipError_t e = enqueue_decode(x, rs, sampler, window, x->cap, nullptr);
    hipGraph_t g = nullptr;
    hipError_t e2 = hipStreamEndCapture(x->cap, &g);
    MX_TRY(x, e);
    MX_TRY(x, e2);
    hipGraphExec_t ex = nullptr;
    MX_TRY(x, hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
    x->graph_defs[key] = g;
    it = x->graphs.emplace(key, ex).first;
  }
  MX_TRY(x, hipGraphLaunch(it->second, st));
  mirror_step(x, n_rows);
  return MX_OK;
}

extern "C" int mx_llm_decode_profiled(mx_llm* x, int n_rows, void* stream,
                                      double* ms_by_class, int n_classes) {
  if (!x || !ms_by_class) return MX_ERR_ARG;
  if (!x->final) MX_FAIL(x, MX_ERR_STATE, "not finalized");
  if (n_rows < 1 || n_rows > x->c.max_batch) MX_FAIL(x, MX_ERR_ARG, "bad n_rows");
  hipStream_t st = (hipStream_t)stream;
  MX_TRY(x, hipSetDevice(x->device));
  if (check_room(x, n_rows)) return MX_ERR_STATE;
  Prof prof;
  hipError_t e = enqueue_decode(x, row_set(x, x->h_dec, x->row_slot, x->row_pos, n_rows,
                                          decode_max_len(x, n_rows), true),
                                sampler_of(x, n_rows), window_of(x, n_rows), st, &prof);
  mirror_step(x, n_rows);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  for (auto& p : prof.ev) {
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, p.second.first, p.second.second);
    if (p.first < n_classes) ms_by_class[p.first] += ms;
    (void)hipEventDestroy(p.second.first);
    (void)hipEventDestroy(p.second.second);
  }
  MX_TRY(x, e);
  return MX_OK;
}

// Diagnostic: time `reps` launches of layer 0's attention, captured in one hipGraph (so
// host launch rate does not floor the measurement), for n_rows rows of length L; row i
// uses KV slot i % max_slots (KV contents are irrelevant to the timing).  Writes the mean
// microseconds per launch, inter-kernel gap included.  Clobbers decode-row state: call on
// an idle context only.
extern "C" int mx_llm_bench_attention(mx_llm* x, int L, int n_rows, int cpw, int debug,
                                      int reps, float* us_out) {
  if (!x || !us_out || L < 1 || L > x->c.max_pos || n_rows < 1 || n_rows > x->c.max_batch ||
      reps < 1)
    return MX_ERR_ARG;
  const auto& c = x->c;
  MX_TRY(x, hipSetDevice(x->device));
  hipStream_t st = x->cap;
  std::vector<int32_t> slots(n_rows), pos(n_rows, L - 1);
  for (int i = 0; i < n_rows; ++i) slots[i] = i % c.max_slots;
  MX_TRY(x, hipMemcpy(x->row_slot, slots.data(), n_rows * 4, hipMemcpyHostToDevice));
  MX_TRY(x, hipMemcpy(x->row_pos, pos.data(), n_rows * 4, hipMemcpyHostToDevice));
  AttnArgs at{};
  at.Q = x->q; at.kcache = x->kcache; at.vcache = x->vcache; at.row_slot = x->row_slot;
  at.row_pos = x->row_pos; at.heads = c.heads; at.kv_heads = c.kv_heads; at.max_pos = c.max_pos;
  at.scale = 1.0f / sqrtf(128.0f); at.cpw = cpw; at.split_stride = c.max_pos / ATT_S_MIN;
  at.nw = n_rows == 1 ? x->att_nw_b1 : x->att_nw_batch;
  at.part_ml = x->part_ml; at.part_acc = x->part_acc; at.counter = x->att_cnt; at.out = x->att;
  at.debug = debug;
  MX_TRY(x, launch_attention(at, n_rows, L, st));  // warm + argument check
  MX_TRY(x, hipStreamSynchronize(st));
  hipGraph_t g = nullptr;
  hipGraphExec_t ge = nullptr;
  MX_TRY(x, hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
  hipError_t e = hipSuccess;
  for (int i = 0; i < reps && e == hipSuccess; ++i) e = launch_attention(at, n_rows, L, st);
  hipError_t e2 = hipStreamEndCapture(st, &g);
  MX_TRY(x, e);
  MX_TRY(x, e2);
  MX_TRY(x, hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
  hipEvent_t e0, e1;
  MX_TRY(x, hipEventCreate(&e0));
  MX_TRY(x, hipEventCreate(&e1));
  MX_TRY(x, hipGraphLaunch(ge, st));  // warm replay
  MX_TRY(x, hipEventRecord(e0, st));
  MX_TRY(x, hipGraphLaunch(ge, st));
  MX_TRY(x, hipEventRecord(e1, st));
  MX_TRY(x, hipEventSynchronize(e1));
  float ms = 0.f;
  MX_TRY(x, hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipGraphExecDestroy(ge);
  (void)hipGraphDestroy(g);
  // park the rows again
  MX_TRY(x, launch_set_rows(x->row_slot, x->row_pos, n_rows, c.max_slots, 0, st));
  MX_TRY(x, hipStreamSynchronize(st));
  *us_out = 1e3f * ms / reps;
  return MX_OK;
}

// The GEMV probes' launch arguments: layer li's projection `which` exactly as the decode step
// sets it up (weights, fragment-major copies for the multi-row kernel, epilogue operands);
// 0 qkv, 1 o-proj, 2 gate/up, 3 down, 4 the one-row merging o-proj, 5 lm_head.
static GemvArgs bench_args(mx_llm* x, int which, int li, int n_rows, int merge_pos) {
  const auto& c = x->c;
  GemvArgs g;
  if (which == 0) {
    g = qkv_args(x, li, n_rows);
    g.X = x->h_dec; g.row_slot = x->row_slot; g.row_pos = x->row_pos;
  } else if (which == 1) {
    g = o_args(x, li, n_rows);
    g.X = x->att; g.Y = x->act;
  } else if (which == 2) {
    g = gu_args(x, li, n_rows);
    g.X = x->h_dec; g.Y = x->act;
  } else if (which == 3) {
    g = down_args(x, li, n_rows);
    g.X = x->act; g.Y = x->q;
  } else if (which == 4) {  // (row-major weights only, as the one-row kernel reads them)
    g = o_args(x, li, n_rows);
    g.Wf = nullptr; g.X = x->att; g.Y = x->act;
    if (g.rpw == 0) g.rpw = 2;
    g.att_ml = x->part_ml; g.att_acc = x->part_acc; g.att_S = 128;
    g.att_stride = c.max_pos / ATT_S_MIN; g.att_nsm = (merge_pos + 128) / 128;
    g.heads = c.heads; g.kv_heads = c.kv_heads; g.row_pos = x->row_pos;
  } else {  // 5: lm_head + penalty + argmax (the same matrix every launch: 964 MB > MALL)
    g = head_args(x, n_rows);
    g.X = x->h_dec; g.row_slot = x->row_slot; g.best = x->best; g.logits = x->logits;
  }
  // the probes' own: on every kind, also where the step leaves them zero (eps of the residual
  // projections, ystride of qkv / gate/up / lm_head, wpb and force_legacy of the lm_head)
  g.eps = c.eps; g.wpb = x->gemv_wpb; g.force_legacy = x->legacy_gemv; g.ystride = g.N;
  // the multi-row qkv as the decode step launches it: raw K-range partials, no seam
  if (which == 0) attach_qkv_parts(x, g);
  return g;
}

// Roofline probe: one hipGraph of `reps` sweeps over all layers' GEMV `which` (0 qkv,
// 1 o-proj, 2 gate/up, 3 down) for a single row, exactly as the decode step launches them
// (same kernels, grids and epilogues; decode row 0's state is used and clobbered: the
// residual / KV scratch written are meaningless).  Sweeping every layer keeps the stream
// out of the 256 MB Infinity Cache, as in a real step.  Writes mean microseconds per
// launch (inter-kernel gap in the graph included) and the weight bytes of one launch.
static int bench_gemv_impl(mx_llm* x, int which, int n_rows, int reps, float* us_out,
                           double* bytes_out, unsigned long long* trace, int trace_cap = 0) {
  if (!x || !us_out || which < 0 || which > 5 || reps < 1) return MX_ERR_ARG;
  if (!x->final) MX_FAIL(x, MX_ERR_STATE, "not finalized");
  const auto& c = x->c;
  if (n_rows < 1 || n_rows > c.max_batch) MX_FAIL(x, MX_ERR_ARG, "bad n_rows");
  MX_TRY(x, hipSetDevice(x->device));
  hipStream_t st = x->cap;
  if (which == 4 && n_rows != 1) MX_FAIL(x, MX_ERR_ARG, "the merging o-proj is one-row");
  // 4: the one-row o-proj merging 8 attention splits of 128 positions (row at L = 1,001; the
  // partial buffers' contents are whatever the last step left: traffic, not values)
  const int merge_pos = std::min(1000, c.max_pos - 1);
  if (which == 4 && (merge_pos + 1 + 127) / 128 > 8) MX_FAIL(x, MX_ERR_ARG, "max_pos too small");
  if (which == 0 || which == 4 || which == 5) {  // keep (row_slot, row_pos) in range
    std::vector<int32_t> slots(n_rows), pos(n_rows, which == 4 ? merge_pos : 0);
    for (int i = 0; i < n_rows; ++i) slots[i] = i % c.max_slots;
    MX_TRY(x, hipMemcpy(x->row_slot, slots.data(), n_rows * 4, hipMemcpyHostToDevice));
    MX_TRY(x, hipMemcpy(x->row_pos, pos.data(), n_rows * 4, hipMemcpyHostToDevice));
  }
  auto args = [&](int li) { return bench_args(x, which, x->bench_one_layer ? 0 : li, n_rows, merge_pos); };
  const int epi = which == 0 ? EPI_QKV : which == 2 ? EPI_SILU : which == 5 ? EPI_ARGMAX : EPI_RESID;
  const bool norm = which == 0 || which == 2 || which == 5;
  MX_TRY(x, launch_gemv(args(0), epi, norm, st));
  MX_TRY(x, hipStreamSynchronize(st));
  hipGraph_t g = nullptr;
  hipGraphExec_t ge = nullptr;
  MX_TRY(x, hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
  hipError_t e = hipSuccess;
  for (int i = 0; i < reps && e == hipSuccess; ++i)
    for (int li = 0; li < c.layers && e == hipSuccess; ++li) {
      GemvArgs g = args(li);
      if (i == reps - 1 && li == c.layers - 1) {  // the sweep's last launch
        g.trace = trace;
        g.trace_cap = trace_cap;  // stamps of blocks past the buffer are dropped
      }
      e = launch_gemv(g, epi, norm, st);
    }
  hipError_t e2 = hipStreamEndCapture(st, &g);
  MX_TRY(x, e);
  MX_TRY(x, e2);
  MX_TRY(x, hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
  hipEvent_t e0, e1;
  MX_TRY(x, hipEventCreate(&e0));
  MX_TRY(x, hipEventCreate(&e1));
  MX_TRY(x, hipGraphLaunch(ge, st));
  MX_TRY(x, hipEventRecord(e0, st));
  MX_TRY(x, hipGraphLaunch(ge, st));
  MX_TRY(x, hipEventRecord(e1, st));
  MX_TRY(x, hipEventSynchronize(e1));
  float ms = 0.f;
  MX_TRY(x, hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipGraphExecDestroy(ge);
  (void)hipGraphDestroy(g);
  *us_out = 1e3f * ms / (reps * c.layers);
  const GemvArgs a0 = args(0);
  if (bytes_out) *bytes_out = (double)x->esz * a0.N * a0.K + (x->esz == 1 ? 4.0 * a0.N : 0.0);
  return MX_OK;
}

extern "C" int mx_llm_bench_gemv(mx_llm* x, int which, int n_rows, int reps, float* us_out,
                                 double* bytes_out) {
  return bench_gemv_impl(x, which, n_rows, reps, us_out, bytes_out, nullptr);
}

// Diagnostic: the same all-layer sweep of GEMV `which` replayed on `nstreams` streams at once
// (each with its own split-K workspace and tickets; the activations and outputs are shared
// scratch, so the values are meaningless): do concurrent row groups overlap each other's ramps
// and seams, and do they share the weight stream through the Infinity Cache?  Writes the wall
// time per launch of one stream's sweep.
extern "C" int mx_llm_bench_gemv_streams(mx_llm* x, int which, int n_rows, int reps,
                                         int nstreams, float* us_out) {
  if (!x || !us_out || which < 0 || which > 5 || which == 4 || reps < 1 || nstreams < 1 ||
      nstreams > 4)
    return MX_ERR_ARG;
  if (!x->final) MX_FAIL(x, MX_ERR_STATE, "not finalized");
  const auto& c = x->c;
  if (n_rows < 2 || n_rows > c.max_batch) MX_FAIL(x, MX_ERR_ARG, "bad n_rows (multi-row only)");
  MX_TRY(x, hipSetDevice(x->device));
  {
    std::vector<int32_t> slots(n_rows), pos(n_rows, 0);
    for (int i = 0; i < n_rows; ++i) slots[i] = i % c.max_slots;
    MX_TRY(x, hipMemcpy(x->row_slot, slots.data(), n_rows * 4, hipMemcpyHostToDevice));
    MX_TRY(x, hipMemcpy(x->row_pos, pos.data(), n_rows * 4, hipMemcpyHostToDevice));
  }
  std::vector<float*> ws(nstreams, nullptr);
  std::vector<int*> tk(nstreams, nullptr);
  std::vector<hipStream_t> sts(nstreams, nullptr);
  std::vector<hipGraphExec_t> ex(nstreams, nullptr);
  hipGraph_t gr = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  std::vector<hipEvent_t> done(nstreams, nullptr);
  hipError_t e = hipSuccess;
  for (int s = 0; s < nstreams && e == hipSuccess; ++s) {
    e = hipMalloc(&ws[s], std::max<size_t>(x->rows_ws_floats, 1) * 4);
    if (e == hipSuccess) e = hipMalloc(&tk[s], x->rows_tickets_n * 4);
    if (e == hipSuccess) e = hipMemset(tk[s], 0, x->rows_tickets_n * 4);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&sts[s], hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&done[s]);
  }
  auto args = [&](int li, int s) {
    GemvArgs g = bench_args(x, which, li, n_rows, 0);
    g.ws = ws[s];
    g.tickets = tk[s];
    return g;
  };
  const int epi = which == 0 ? EPI_QKV : which == 2 ? EPI_SILU : which == 5 ? EPI_ARGMAX : EPI_RESID;
  const bool norm = which == 0 || which == 2 || which == 5;
  for (int s = 0; s < nstreams && e == hipSuccess; ++s) {
    hipGraph_t g = nullptr;
    e = hipStreamBeginCapture(sts[s], hipStreamCaptureModeRelaxed);
    for (int i = 0; i < reps && e == hipSuccess; ++i)
      for (int li = 0; li < c.layers && e == hipSuccess; ++li) e = launch_gemv(args(li, s), epi, norm, sts[s]);
    const hipError_t e2 = hipStreamEndCapture(sts[s], &g);
    if (e == hipSuccess) e = e2;
    if (e == hipSuccess) e = hipGraphInstantiate(&ex[s], g, nullptr, nullptr, 0);
    if (g) (void)hipGraphDestroy(g);
  }
  (void)gr;
  if (e == hipSuccess) e = hipEventCreate(&e0);
  if (e == hipSuccess) e = hipEventCreate(&e1);
  for (int s = 0; s < nstreams && e == hipSuccess; ++s) e = hipGraphLaunch(ex[s], sts[s]);  // warm
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipEventRecord(e0, sts[0]);
  for (int s = 1; s < nstreams && e == hipSuccess; ++s) e = hipStreamWaitEvent(sts[s], e0, 0);
  for (int s = 0; s < nstreams && e == hipSuccess; ++s) e = hipGraphLaunch(ex[s], sts[s]);
  for (int s = 1; s < nstreams && e == hipSuccess; ++s) {
    e = hipEventRecord(done[s], sts[s]);
    if (e == hipSuccess) e = hipStreamWaitEvent(sts[0], done[s], 0);
  }
  if (e == hipSuccess) e = hipEventRecord(e1, sts[0]);
  if (e == hipSuccess) e = hipEventSynchronize(e1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  (void)hipDeviceSynchronize();
  for (int s = 0; s < nstreams; ++s) {
    if (ex[s]) (void)hipGraphExecDestroy(ex[s]);
    if (sts[s]) (void)hipStreamDestroy(sts[s]);
    if (done[s]) (void)hipEventDestroy(done[s]);
    if (ws[s]) (void)hipFree(ws[s]);
    if (tk[s]) (void)hipFree(tk[s]);
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  MX_TRY(x, e);
  *us_out = 1e3f * ms / (reps * c.layers);
  return MX_OK;
}

// Diagnostic: the multi-row (generation 4) launch of mx_llm_bench_gemv's last layer, replayed
// in its sweep, with per-block s_memrealtime stamps (100 MHz): host_out[block * 8 + k], k =
// 0 entry, 1 first activation sub-chunk staged, 2 first weight sub-chunk consumed, 3 main loop
// done, 4 partial published + ticket taken (split-K only), 5 K ranges merged (last arriver),
// 6 epilogue done; 0 = not reached.  *blocks_out = the launch's grid size.
extern "C" int mx_llm_bench_gemv_trace(mx_llm* x, int which, int n_rows, uint64_t* host_out,
                                       int cap_blocks, int* blocks_out) {
  if (!x || !host_out || !blocks_out || cap_blocks < 1 || n_rows < 2) return MX_ERR_ARG;
  MX_TRY(x, hipSetDevice(x->device));
  unsigned long long* d = nullptr;
  const size_t n = (size_t)cap_blocks * 8;
  MX_TRY(x, hipMalloc(&d, n * 8));
  hipError_t e = hipMemset(d, 0, n * 8);
  float us = 0.f;
  int rc = e == hipSuccess ? bench_gemv_impl(x, which, n_rows, 1, &us, nullptr, d, cap_blocks) : MX_ERR_HIP;
  if (rc == MX_OK) e = hipMemcpy(host_out, d, n * 8, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (rc != MX_OK) return rc;
  MX_TRY(x, e);
  int blocks = 0;
  for (int b = 0; b < cap_blocks; ++b)
    if (host_out[(size_t)b * 8]) blocks = b + 1;
  *blocks_out = blocks;
  if (!blocks)
    MX_FAIL(x, MX_ERR_STATE, "no stamps: the library was built without MX_ROWS_TRACE "
                             "(MORPHEUS_MX_ROWS_TRACE=1 python -m project_morpheus_amd.build)");
  return MX_OK;
}

// The options that are one int member with a small set or a range of values (the others, with
// side effects or cross-checks, are explicit code in mx_llm_set_option).
struct IntOption {
  const char* key;
  int& (*ref)(mx_llm&);
  int lo, hi;     // allowed: lo..hi ...
  unsigned only;  // ... and, when non-zero, only the values whose bit is set

  bool allows(int v) const { return v >= lo && v <= hi && (!only || (only >> v) & 1u); }
  std::string allowed() const {  // "0 or 1", "0, 2 or 4", "0..4096"
    if (!only && hi - lo > 2) return std::to_string(lo) + ".." + std::to_string(hi);
    std::string t;
    for (int v = lo, left = 0; v <= hi; ++v)
      if (allows(v)) t += (left++ ? ", " : "") + std::to_string(v);
    const size_t last = t.rfind(", ");
    return last == std::string::npos ? t : t.replace(last, 2, " or ");
  }
};
#define OPT(m) [](mx_llm& x) -> int& { return x.m; }
#define BITS2(a, b) (1u << (a) | 1u << (b))
static const IntOption kIntOptions[] = {
    {"legacy_gemv", OPT(legacy_gemv), INT_MIN, INT_MAX, 0},  // (any value: zero or not)
    {"rows_head_mt", OPT(rows_head_mt), 1, 2, 0},
    {"bench_one_layer", OPT(bench_one_layer), 0, 1, 0},
    {"engine_dbg", OPT(engine_dbg), 0, 3, 0},
    {"rows_qkv_parts", OPT(rows_qkv_parts), 0, 1, 0},
    {"rows_atomic", OPT(rows_atomic), 0, 1, 0},
    {"grammar_head", OPT(grammar_head), 0, 1, 0},
    {"head_b1", OPT(head_b1), 0, 1, 0},
    {"rows_frag", OPT(rows_frag), 0, 1, 0},
    {"rows_lds_pad", OPT(rows_lds_pad), 0, 128, 0},  // KB
    {"gemv_wpb", OPT(gemv_wpb), 4, 8, BITS2(4, 8)},
    {"rpw_o", OPT(rpw_o), 0, 2, 0},
    {"rpw_down", OPT(rpw_down), 0, 2, 0},
    {"rpw_gu", OPT(rpw_gu), 0, 4, BITS2(0, 2) | 1u << 4},
    {"o_merge", OPT(o_merge), 0, 1, 0},
    {"rows_merge", OPT(rows_merge), 0, 1, 0},
    {"gemv_balance", OPT(gemv_balance), 0, 1, 0},
    {"att_b1_nw6", OPT(att_b1_nw6), 0, 1, 0},
    {"att_nw6", OPT(att_nw6), 0, 1, 0},
    {"rows_pw", OPT(rows_pw), 1, 2, 0},
    {"rows_pw_f8", OPT(rows_pw_f8), 1, 2, 0},
    {"rows_nt1", OPT(rows_nt1), 0, 31, 0},  // a 5-bit kind mask
    {"rows_nt_max", OPT(rows_nt_max), 0, 4, BITS2(0, 1) | BITS2(2, 4)},
    {"rows_head_target", OPT(rows_head_target), 0, 4096, 0},
    {"rows_target", OPT(rows_target), 0, 4096, 0},
    {"rows_target_qkv", OPT(rows_target_k[0]), 0, 4096, 0},
    {"rows_target_o", OPT(rows_target_k[1]), 0, 4096, 0},
    {"rows_target_gu", OPT(rows_target_k[2]), 0, 4096, 0},
    {"rows_target_down", OPT(rows_target_k[3]), 0, 4096, 0},
};
#undef BITS2
#undef OPT

static const IntOption* int_option(const std::string& key) {
  for (const IntOption& o : kIntOptions)
    if (key == o.key) return &o;
  return nullptr;
}

extern "C" int mx_llm_set_option(mx_llm* x, const char* key, int value) {
  if (!x || !key) return MX_ERR_ARG;
  const std::string k(key);
  if (k == "debug_poison_att_partials") {
    // test hook, not a knob and not part of any step: on the call, every attention split
    // partial becomes 0xFF bytes (quiet NaNs), so a consumer that lets a dead split slot into
    // its result shows.  Waits for the device on both sides; the captured graphs stay.
    if (value != 0 && value != 1) MX_FAIL(x, MX_ERR_ARG, "debug_poison_att_partials must be 0 or 1");
    if (value) {
      const size_t part_rows = (size_t)x->max_rows * (x->c.max_pos / ATT_S_MIN);
      MX_TRY(x, hipSetDevice(x->device));
      MX_TRY(x, hipDeviceSynchronize());
      MX_TRY(x, hipMemset(x->part_ml, 0xFF, part_rows * x->c.heads * 2 * sizeof(float)));
      MX_TRY(x, hipMemset(x->part_acc, 0xFF, part_rows * x->c.heads * 128 * sizeof(float)));
      MX_TRY(x, hipDeviceSynchronize());
    }
    return MX_OK;
  } else if (k == "engine_loaders") {
    if (value != 1 && value != 2) MX_FAIL(x, MX_ERR_ARG, "engine_loaders must be 1 or 2");
    x->engine_loaders = value;
    if (x->b1_engine) {
      int per_cu = 0;
      MX_TRY(x, engine_per_cu(engine_args(x), &per_cu));
      if (per_cu < 1) MX_FAIL(x, MX_ERR_ARG, "engine_loaders: a workgroup does not fit one CU");
    }
  } else if (k == "b1_engine" || k == "engine_slots" || k == "engine_depth") {
    const bool en = k == "b1_engine" ? value != 0 : x->b1_engine != 0;
    const int slots = k == "engine_slots" ? value : x->engine_slots;
    const int depth = k == "engine_depth" ? value : x->engine_depth;
    if (k == "b1_engine" && value != 0 && value != 1) MX_FAIL(x, MX_ERR_ARG, "b1_engine must be 0 or 1");
    if (depth != 2 && depth != 3) MX_FAIL(x, MX_ERR_ARG, "engine_depth must be 2 or 3");
    if (slots < 3 || slots > engine_ring_max() || slots <= depth ||
        engine_lds_bytes(slots, x->c.hidden, engine_xb_floats(x->c.heads, x->c.kv_heads, x->c.ffn)) > 160 * 1024)
      MX_FAIL(x, MX_ERR_ARG, "engine_slots must be 3.." + std::to_string(engine_ring_max()) +
                                 ", above engine_depth, and fit the CU's 160 KB of LDS");
    if (en) {
      const auto& c = x->c;
      MX_TRY(x, hipSetDevice(x->device));
      int cus = 0, per_cu = 0;
      MX_TRY(x, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, x->device));
      // per-CU row counts must fit the engine's LDS tables (engine_b1.hip Ctl: 32 qkv / o /
      // down rows, 64 gate/up rows)
      auto per = [&](int n) { return (((n + cus - 1) / cus) + 1) & ~1; };
      const int qkv_rows = (c.heads + 2 * c.kv_heads) * 128;
      if (c.hidden % 1024 || c.ffn % 1024 || c.heads * 128 != c.hidden || c.layers > 31 ||
          c.heads / c.kv_heads > 4 || per(c.hidden) > 32 || per(qkv_rows) > 32 || per(2 * c.ffn) > 64)
        MX_FAIL(x, MX_ERR_ARG, "b1_engine: model shape outside the engine's (hidden = heads x 128, "
                               "multiples of 1024, <= 31 layers, GQA <= 4)");
      EngineArgs ea = engine_args(x);
      ea.ring_slots = slots;
      ea.depth = depth;
      if (c.heads / c.kv_heads < 3)
        MX_FAIL(x, MX_ERR_ARG, "b1_engine: instantiated for GQA 3 (Orpheus) and 4 only");
      MX_TRY(x, engine_per_cu(ea, &per_cu));
      if (per_cu < 1) MX_FAIL(x, MX_ERR_ARG, "b1_engine: a workgroup does not fit one CU");
      x->engine_grid = cus;  // one per CU, all co-resident (every wait is also time-bounded)
    }
    x->engine_slots = slots;
    x->engine_depth = depth;
    x->b1_engine = en ? 1 : 0;
  } else if (k == "engine_timeout") {
    // (tests force a give-up with a tiny bound; 0 restores the default)
    if (value < 0) MX_FAIL(x, MX_ERR_ARG, "engine_timeout must be >= 0 (ticks of 100 MHz; 0 = 50 ms)");
    x->engine_timeout_ticks = value ? value : 5000000;
  } else if (k == "engine_trace") {
    if (value != 0 && value != 1) MX_FAIL(x, MX_ERR_ARG, "engine_trace must be 0 or 1");
    if (value && !x->eng_trace) {
      MX_TRY(x, hipSetDevice(x->device));
      MX_TRY(x, x->alloc(&x->eng_trace, (size_t)1024 * x->c.layers * 12));
      MX_TRY(x, hipMemset(x->eng_trace, 0, (size_t)1024 * x->c.layers * 12 * 8));
    }
    if (!value) x->eng_trace = nullptr;  // (the buffer stays allocated until destroy)
  } else if (k == "att_b1_short") {
    if (value < 0 || value > 2) MX_FAIL(x, MX_ERR_ARG, "att_b1_short must be 0, 1 or 2");
    if (value && (x->c.max_pos % 64 || x->max_rows < 2))
      MX_FAIL(x, MX_ERR_ARG, "att_b1_short needs max_pos % 64 == 0 and max(max_batch, max_prefill) >= 2");
    x->att_b1_short = value;
  } else if (k == "att_nw" || k == "att_nw_batch") {
    // (one-row overrides with att_cpw > 0 may also take 3- / 6-wave blocks)
    const bool b1_only = (value == 3 || value == 6) && k == "att_nw";
    if (value != 4 && value != 8 && !b1_only) MX_FAIL(x, MX_ERR_ARG, "att_nw must be 4 or 8 (att_nw also 3 / 6)");
    (k == "att_nw" ? x->att_nw_b1 : x->att_nw_batch) = value;
  } else if (k == "att_cpw" || k == "att_cpw_batch") {
    const bool any = value == 1 || value == 2 || value == 4 || (value == 0 && k == "att_cpw");
    const bool wide = value == 3 || value == 6 || value == 8;  // 8-wave blocks only
    if (!(any || (wide && k == "att_cpw_batch") || (value == 0 && k == "att_cpw_batch")))
      MX_FAIL(x, MX_ERR_ARG, "att_cpw must be 0 (auto), 1, 2 or 4 (att_cpw_batch also 3/6/8, 0 = auto)");
    (k == "att_cpw" ? x->att_cpw_b1 : x->att_cpw_batch) = value;
  } else if (const IntOption* o = int_option(k)) {
    if (!o->allows(value)) MX_FAIL(x, MX_ERR_ARG, k + " must be " + o->allowed());
    o->ref(*x) = value;
  } else {
    MX_FAIL(x, MX_ERR_ARG, "unknown option " + k);
  }
  // captured graphs baked the old choice in: drop them
  drop_graphs(x);
  return MX_OK;
}

static void drop_graphs(mx_llm* x) {
  for (auto& kv : x->graphs) (void)hipGraphExecDestroy(kv.second);
  for (auto& kv : x->graph_defs) (void)hipGraphDestroy(kv.second);
  x->graphs.clear();
  x->graph_defs.clear();
}

extern "C" int mx_llm_set_grammar(mx_llm* x, const mx_code_grammar* g) {
  if (!x) return MX_ERR_ARG;
  if (!x->final) MX_FAIL(x, MX_ERR_STATE, "not finalized");
  for (char act : x->row_active)
    if (act) MX_FAIL(x, MX_ERR_STATE, "set_grammar: a row is active");
  const auto& c = x->c;
  if (g) {
    if (g->phases < 1 || g->codes < 1 || g->code_min < 0 || g->code_min >= g->codes || g->code_base < 0 ||
        (long long)g->code_base + (long long)g->phases * g->codes > c.vocab)
      MX_FAIL(x, MX_ERR_ARG, "grammar: need phases >= 1, codes >= 1, 0 <= code_min < codes, code_base >= 0, "
                             "code_base + phases * codes <= vocab");
    if (g->stop_id >= c.vocab ||
        (g->stop_id >= g->code_base && g->stop_id < g->code_base + g->phases * g->codes))
      MX_FAIL(x, MX_ERR_ARG, "grammar: stop_id inside a code range or past the vocabulary");
  }
  MX_TRY(x, hipSetDevice(x->device));
  MX_TRY(x, hipDeviceSynchronize());
  const size_t slots = (size_t)c.max_slots + 1;
  // (allocated on the first call, behind every other buffer: a context that never sets a
  // grammar keeps its allocations)
  if (g && !x->gram_origin) MX_TRY(x, x->alloc(&x->gram_origin, slots));
  if (x->gram_origin) MX_TRY(x, hipMemset(x->gram_origin, 0xFF, slots * 4));  // -1: unconstrained
  std::fill(x->slot_grammar.begin(), x->slot_grammar.end(), 0);
  std::fill(x->row_origin.begin(), x->row_origin.end(), -1);
  x->gram_on = g != nullptr;
  x->win_lo = x->win_n = 0;
  x->win_heads = 0;
  if (g) {
    x->gram = *g;
    // the row window: from the largest multiple of 256 not above the smallest allowed id to
    // the end of the code ranges rounded up to 256 (capped by the vocabulary).  The kernels
    // need a multiple of 4 rows (head_b1's row groups, the multi-row epilogue's 4-byte `seen`
    // loads) and the multi-row workspace sized at create; a window that does not fit leaves
    // every step on the whole vocabulary with the mask.
    int first = g->code_base + g->code_min;
    if (g->stop_id >= 0 && g->stop_id < first) first = g->stop_id;
    int last = g->code_base + g->phases * g->codes;  // one past the last code
    if (g->stop_id >= last) last = g->stop_id + 1;
    const int lo = first / 256 * 256;
    const int hi = (int)std::min<long long>(c.vocab, ((long long)last + 255) / 256 * 256);
    bool fits = (hi - lo) % 4 == 0 && c.vocab % 4 == 0 && hi - lo < c.vocab;
    for (int r : {16, 32, 64, c.max_batch}) {
      size_t wf = 0, tk = 0;
      v4::gemm_rows_workspace_v4(hi - lo, c.hidden, std::min(r, c.max_batch), EPI_ARGMAX, &wf, &tk);
      if (wf > x->rows_ws_floats || tk > x->rows_tickets_n) fits = false;
    }
    if (fits) {
      x->win_lo = lo;
      x->win_n = hi - lo;
    }
  }
  drop_graphs(x);
  return MX_OK;
}

extern "C" int mx_llm_grammar_window(const mx_llm* x, int* lo, int* n, long long* heads) {
  if (!x || !lo || !n || !heads) return MX_ERR_ARG;
  *lo = x->win_lo;
  *n = x->win_n;
  *heads = x->win_heads;
  return MX_OK;
}

extern "C" int mx_llm_set_slot_grammar(mx_llm* x, int slot, int on) {
  if (!x || slot < 0 || slot >= x->c.max_slots) return MX_ERR_ARG;
  if (on && !x->gram_on) MX_FAIL(x, MX_ERR_STATE, "set_slot_grammar: the context has no grammar");
  x->slot_grammar[slot] = on ? 1 : 0;
  return MX_OK;
}

extern "C" int mx_llm_release_row(mx_llm* x, int row, void* stream) {
  if (!x || row < 0 || row >= x->c.max_batch) return MX_ERR_ARG;
  MX_TRY(x, hipSetDevice(x->device));
  MX_TRY(x, launch_set_rows(x->row_slot + row, x->row_pos + row, 1, x->c.max_slots, 0,
                            (hipStream_t)stream));
  x->pos_mirror[row] = 0;
  x->row_active[row] = 0;
  x->row_samples[row] = 0;
  x->row_chain[row] = 0;
  x->row_origin[row] = -1;
  x->row_slot_h[row] = -1;
  return MX_OK;
}

extern "C" int mx_llm_move_row(mx_llm* x, int dst, int src, void* stream) {
  if (!x || dst < 0 || src < 0 || dst >= x->c.max_batch || src >= x->c.max_batch || dst == src)
    return MX_ERR_ARG;
  if (x->row_active[dst]) MX_FAIL(x, MX_ERR_STATE, "move_row: destination row is live");
  MX_TRY(x, hipSetDevice(x->device));
  MX_TRY(x, launch_move_row(x->row_slot, x->row_pos, x->row_token, x->h_dec, x->c.hidden, dst,
                            src, x->c.max_slots, (hipStream_t)stream));
  x->pos_mirror[dst] = x->pos_mirror[src];
  x->row_active[dst] = x->row_active[src];
  x->row_samples[dst] = x->row_samples[src];
  x->row_chain[dst] = x->row_chain[src];
  x->row_origin[dst] = x->row_origin[src];
  x->row_origin[src] = -1;
  x->row_slot_h[dst] = x->row_slot_h[src];
  x->row_slot_h[src] = -1;
  x->pos_mirror[src] = 0;
  x->row_active[src] = 0;
  x->row_samples[src] = 0;
  x->row_chain[src] = 0;
  return MX_OK;
}

extern "C" int mx_llm_row_state(const mx_llm* x, int row, int* active, int* next_pos) {
  if (!x || !active || !next_pos || row < 0 || row >= x->c.max_batch) return MX_ERR_ARG;
  *active = x->row_active[row];
  *next_pos = x->pos_mirror[row];
  return MX_OK;
}

extern "C" int32_t* mx_llm_history(mx_llm* x) { return x ? x->hist_host : nullptr; }

extern "C" int mx_llm_engine_trace(mx_llm* x, uint64_t* host_out, int n, int* grid_out) {
  if (!x || !host_out || !grid_out) return MX_ERR_ARG;
  if (!x->eng_trace) MX_FAIL(x, MX_ERR_STATE, "engine_trace is off");
  const size_t need = (size_t)x->engine_grid * x->c.layers * 12;
  if ((size_t)n < need) MX_FAIL(x, MX_ERR_ARG, "trace buffer too small");
  MX_TRY(x, hipSetDevice(x->device));
  MX_TRY(x, hipDeviceSynchronize());
  MX_TRY(x, hipMemcpy(host_out, x->eng_trace, need * 8, hipMemcpyDeviceToHost));
  *grid_out = x->engine_grid;
  return MX_OK;
}

// Allowed set of the token a stream of origin `origin` puts at position p: ids [lo, lo + n)
// and `stop` (-1: none).
static void allowed_span(const mx_llm* x, int origin, int p, int* lo, int* n, int* stop) {
  const mx_code_grammar& g = x->gram;
  int k = (p - origin) % g.phases;
  if (k < 0) k += g.phases;
  *lo = g.code_base + k * g.codes + g.code_min;
  *n = g.codes - g.code_min;
  *stop = k == 0 ? g.stop_id : -1;
}

extern "C" int mx_llm_debug_logits(mx_llm* x, int enable) {
  if (!x) return MX_ERR_ARG;
  if (!x->graphs.empty()) MX_FAIL(x, MX_ERR_STATE, "enable logits before the first decode");
  x->logits_all = enable ? 1 : 0;
  return MX_OK;
}

extern "C" int mx_llm_read_logits(mx_llm* x, int row, float* host_out, void* stream) {
  if (!x || !host_out || row < 0 || row >= x->c.max_batch) return MX_ERR_ARG;
  if (!x->logits_all) MX_FAIL(x, MX_ERR_STATE, "logits not enabled");
  MX_TRY(x, hipMemcpyAsync(host_out, x->logits + (size_t)row * x->c.vocab,
                           (size_t)x->c.vocab * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
  MX_TRY(x, hipStreamSynchronize((hipStream_t)stream));
  // a constrained row: -inf outside the allowed set of the token the logits picked (the kernels
  // skip those ids, and a windowed head does not compute most of them)
  if (x->gram_on && x->row_origin[row] >= 0) {
    int lo = 0, n = 0, stop = -1;
    allowed_span(x, x->row_origin[row], x->pos_mirror[row], &lo, &n, &stop);
    for (int i = 0; i < x->c.vocab; ++i)
      if (!(i >= lo && i < lo + n) && i != stop) host_out[i] = -INFINITY;
  }
  return MX_OK;
}

extern "C" int mx_llm_debug_sample(mx_llm* x, int row, const float* logits_host, int pos,
                                   int32_t* token_out, void* stream) {
  if (!x || !logits_host || !token_out || row < 0 || row >= x->c.max_batch || pos < 0)
    return MX_ERR_ARG;
  if (!x->final) MX_FAIL(x, MX_ERR_STATE, "not finalized");
  if (!x->row_active[row]) MX_FAIL(x, MX_ERR_STATE, "debug_sample: row has no stream");
  const auto& c = x->c;
  hipStream_t st = (hipStream_t)stream;
  MX_TRY(x, hipSetDevice(x->device));
  // the row's logits buffer is free between steps; the key and the counter are the call's own
  float* lg = x->logits + (size_t)row * c.vocab;
  MX_TRY(x, hipMemcpyAsync(lg, logits_host, (size_t)c.vocab * 4, hipMemcpyHostToDevice, st));
  MX_TRY(x, launch_set_rows(x->dbg_pos, x->dbg_pos + 1, 1, 0, pos, st));
  if (x->row_samples[row])
    MX_TRY(x, enqueue_sampler(x, lg, x->row_slot + row, x->dbg_pos + 1, 1, x->dbg_best,
                              x->row_chain[row] ? SMP_CHAIN : SMP_PLAIN, st));
  else {
    int lo = 0, n = c.vocab, stop = -1;
    if (x->gram_on && x->row_origin[row] >= 0) allowed_span(x, x->row_origin[row], pos + 1, &lo, &n, &stop);
    MX_TRY(x, launch_argmax_row(lg, lo, n, stop < 0 ? -1 : stop, x->dbg_best, st));
  }
  unsigned long long key = 0ull;
  MX_TRY(x, hipMemcpyAsync(&key, x->dbg_best, 8, hipMemcpyDeviceToHost, st));
  MX_TRY(x, hipStreamSynchronize(st));
  *token_out = (int32_t)~(uint32_t)(key & 0xffffffffull);  // argmax_index (mx_common.h)
  return MX_OK;
}

extern "C" const char* mx_llm_last_error(const mx_llm* x) {
  return x ? x->err.c_str() : g_err.c_str();
}

extern "C" void mx_llm_destroy(mx_llm* x) {
  if (!x) return;
  (void)hipSetDevice(x->device);
  for (auto& kv : x->graphs) (void)hipGraphExecDestroy(kv.second);
  for (auto& kv : x->graph_defs) (void)hipGraphDestroy(kv.second);
  if (x->cap) (void)hipStreamDestroy(x->cap);
  for (void* p : x->allocs) (void)hipFree(p);
  if (x->hist_host) (void)hipHostFree(x->hist_host);
  if (x->eng_status_h) (void)hipHostFree(x->eng_status_h);
  delete x;
}

// =====================================================================================
// SNAC context
// =====================================================================================
static const int kRates[4] = {8, 8, 4, 2};
static const int kDil[3] = {1, 3, 9};

// What both SNAC contexts hold: the named weights as fp32 on the device, each allocated by its
// first set, and the bf16 planes finalize derives from the dense ones.
struct SnacStore {
  int device = 0;
  std::string err;
  std::map<std::string, float*> w;
  std::map<std::string, int64_t> expect;
  std::vector<void*> allocs;
  std::map<std::string, uint16_t*> wbf;  // conv-GEMM weights as bf16 planes [3][M][K]
};

// (`what`: how the context names its weights in a refusal)
static int snac_store_set(SnacStore* s, const char* what, const char* name, const void* data,
                          int64_t numel, int dtype) {
  const std::string n(name);
  auto it = s->expect.find(n);
  if (it == s->expect.end()) MX_FAIL(s, MX_ERR_ARG, std::string("unknown ") + what + " " + n);
  if (it->second != numel) MX_FAIL(s, MX_ERR_ARG, n + ": bad numel");
  MX_TRY(s, hipSetDevice(s->device));
  auto f = s->w.find(n);
  if (f == s->w.end()) {
    void* p = nullptr;
    MX_TRY(s, hipMalloc(&p, numel * 4 + 256));
    s->allocs.push_back(p);
    f = s->w.emplace(n, (float*)p).first;
  }
  MX_TRY(s, launch_to_f32(f->second, data, numel, dtype == MX_DTYPE_BF16 ? 1 : 0, nullptr));
  MX_TRY(s, hipDeviceSynchronize());
  return MX_OK;
}

struct mx_snac : SnacStore {
  int max_frames = 0, max_batch = 0;
  float* up_packed[4][8] = {};  // per block, per phase: [Cout][2*Cin]
  uint16_t* up_bf[4][8] = {};
  int up_delta[4][8][2] = {};
  float *bufA = nullptr, *bufB = nullptr, *bufC = nullptr, *noise = nullptr;
  float* bufD = nullptr;  // block 0's Snake output cut to the kept slice's receptive field
  size_t buf_elems = 0;
  bool final = false;
  SnacIO* io = nullptr;  // device copy of the per-call pointers read by captured windows
  hipStream_t cap = nullptr;  // capture stream (the caller's may be the null stream)
  std::map<std::array<int, 5>, hipGraphExec_t> graphs;  // (n_frames, batch, lo, hi, pcm only)
  std::vector<hipGraph_t> graph_defs;
};

static void snac_expect(mx_snac* s) {
  auto& e = s->expect;
  for (int i = 0; i < 3; ++i) {
    const std::string p = "q" + std::to_string(i) + ".";
    e[p + "codebook"] = 4096 * 8;
    e[p + "out_proj.w"] = 768 * 8;
    e[p + "out_proj.b"] = 768;
  }
  e["in.dw.w"] = 768 * 7;
  e["in.dw.b"] = 768;
  e["in.pw.w"] = 1024 * 768;
  e["in.pw.b"] = 1024;
  for (int b = 0; b < 4; ++b) {
    const int cin = 1024 >> b, cout = cin / 2, s = kRates[b];
    const std::string p = "b" + std::to_string(b) + ".";
    e[p + "alpha"] = cin;
    e[p + "up.w"] = (int64_t)cin * cout * 2 * s;
    e[p + "up.b"] = cout;
    e[p + "noise.w"] = (int64_t)cout * cout;
    for (int r = 0; r < 3; ++r) {
      const std::string q = p + "r" + std::to_string(r) + ".";
      e[q + "alpha1"] = cout;
      e[q + "dw.w"] = cout * 7;
      e[q + "dw.b"] = cout;
      e[q + "alpha2"] = cout;
      e[q + "pw.w"] = (int64_t)cout * cout;
      e[q + "pw.b"] = cout;
    }
  }
  e["out.alpha"] = 64;
  e["out.conv.w"] = 64 * 7;
  e["out.conv.b"] = 1;
}

extern "C" int mx_snac_create(int device, int max_frames, int max_batch, mx_snac** out) {
  if (!out || max_frames < 1 || max_batch < 1) return MX_ERR_ARG;
  if (hipSetDevice(device) != hipSuccess) {
    g_err = "hipSetDevice failed";
    return MX_ERR_HIP;
  }
  auto* s = new mx_snac();
  s->device = device;
  s->max_frames = max_frames;
  s->max_batch = max_batch;
  snac_expect(s);
  s->buf_elems = (size_t)131072 * max_frames * max_batch;
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, s->buf_elems * 4);
  if (e == hipSuccess) { s->allocs.push_back(p); s->bufA = (float*)p; e = hipMalloc(&p, s->buf_elems * 4); }
  if (e == hipSuccess) { s->allocs.push_back(p); s->bufB = (float*)p; e = hipMalloc(&p, s->buf_elems * 4); }
  if (e == hipSuccess) { s->allocs.push_back(p); s->bufC = (float*)p; e = hipMalloc(&p, (size_t)3360 * max_frames * max_batch * 4); }
  if (e == hipSuccess) { s->allocs.push_back(p); s->noise = (float*)p; e = hipMalloc(&p, (size_t)16384 * max_frames * max_batch * 4); }
  if (e == hipSuccess) { s->allocs.push_back(p); s->bufD = (float*)p; e = hipMalloc(&p, sizeof(SnacIO)); }
  if (e == hipSuccess) { s->allocs.push_back(p); s->io = (SnacIO*)p; }
  if (e != hipSuccess) {
    g_err = std::string("snac alloc failed: ") + hipGetErrorString(e);
    for (void* q : s->allocs) (void)hipFree(q);
    delete s;
    return MX_ERR_OOM;
  }
  *out = s;
  return MX_OK;
}

extern "C" int mx_snac_set_weight(mx_snac* s, const char* name, const void* data, int64_t numel,
                                  int dtype) {
  if (!s || !name || !data) return MX_ERR_ARG;
  return snac_store_set(s, "snac weight", name, data, numel, dtype);
}

extern "C" int mx_snac_finalize(mx_snac* s) {
  if (!s) return MX_ERR_ARG;
  for (auto& kv : s->expect)
    if (!s->w.count(kv.first)) MX_FAIL(s, MX_ERR_STATE, "missing snac weight " + kv.first);
  MX_TRY(s, hipSetDevice(s->device));
  // ConvTranspose1d(k=2s, stride s, pad ceil(s/2)) as s phase GEMMs with 2 taps each:
  // out[co][s*t+ph] = sum_ci W[ci][co][rm] x[ci][t+q] + W[ci][co][rm+s] x[ci][t+q-1],
  // q = (ph+p) / s, rm = (ph+p) % s.
  for (int b = 0; b < 4; ++b) {
    const int cin = 1024 >> b, cout = cin / 2, st = kRates[b], k = 2 * st, pad = (st + 1) / 2;
    const std::string name = "b" + std::to_string(b) + ".up.w";
    std::vector<float> W((size_t)cin * cout * k);
    MX_TRY(s, hipMemcpy(W.data(), s->w[name], W.size() * 4, hipMemcpyDeviceToHost));
    for (int ph = 0; ph < st; ++ph) {
      const int q = (ph + pad) / st, rm = (ph + pad) % st;
      std::vector<float> A((size_t)cout * 2 * cin);
      for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci) {
          A[(size_t)co * 2 * cin + ci] = W[((size_t)ci * cout + co) * k + rm];
          A[(size_t)co * 2 * cin + cin + ci] = W[((size_t)ci * cout + co) * k + rm + st];
        }
      if (!s->up_packed[b][ph]) {
        void* p = nullptr;
        MX_TRY(s, hipMalloc(&p, A.size() * 4));
        s->allocs.push_back(p);
        s->up_packed[b][ph] = (float*)p;
      }
      MX_TRY(s, hipMemcpy(s->up_packed[b][ph], A.data(), A.size() * 4, hipMemcpyHostToDevice));
      s->up_delta[b][ph][0] = q;
      s->up_delta[b][ph][1] = q - 1;
    }
  }
  // the conv-GEMM operands: every dense weight as three bf16 planes
  auto planes = [&](const float* src, int64_t n, uint16_t** dst) -> int {
    if (!*dst) {
      void* p = nullptr;
      MX_TRY(s, hipMalloc(&p, (size_t)n * 3 * 2));
      s->allocs.push_back(p);
      *dst = (uint16_t*)p;
    }
    MX_TRY(s, launch_split_planes(src, *dst, n, nullptr));
    return MX_OK;
  };
  std::vector<std::string> dense{"in.pw.w"};
  for (int b = 0; b < 4; ++b) {
    const std::string p = "b" + std::to_string(b) + ".";
    dense.push_back(p + "noise.w");
    for (int r = 0; r < 3; ++r) dense.push_back(p + "r" + std::to_string(r) + ".pw.w");
    const int cin = 1024 >> b, cout = cin / 2;
    for (int ph = 0; ph < kRates[b]; ++ph) {
      const int rc = planes(s->up_packed[b][ph], (int64_t)cout * 2 * cin, &s->up_bf[b][ph]);
      if (rc != MX_OK) return rc;
    }
  }
  for (const auto& n : dense) {
    uint16_t*& d = s->wbf[n];
    const int rc = planes(s->w[n], s->expect[n], &d);
    if (rc != MX_OK) return rc;
  }
  MX_TRY(s, hipDeviceSynchronize());
  s->final = true;
  return MX_OK;
}

// Tile choice for one conv-GEMM: 64-wide column tiles on long sequences, and as many
// K-splitting waves per tile as keep the launch near 2k waves (early stages have few
// output columns and long K, late stages the opposite).
// Window batch from which the block-tiled conv-GEMM is used.  Its point is sharing each A
// (weight) fragment across the windows' columns; one window gains nothing from it and the
// one-wave kernels give small batches 4-8x the blocks (N7_B1 0.41 vs 0.55 ms, N7_B4 0.18 vs
// 0.23 ms per window; profiles/r02_snac_tiled_timing.log).  On the receptive-field-cut shapes
// a lone call of 8 windows runs 10-14 % faster on the one-wave kernels
// (profiles/r06_snac_tiled_threshold.log), but inside the configs[2] loop, beside the decode
// stream, the tiled kernel from 8 windows gives the shorter wall (3.245 vs 3.275 s;
// profiles/r06_snac_coalescing_sweep.log), so 8 stays.
static int snac_tiled_min_batch() {
  static const int v = [] {
    const char* e = getenv("MORPHEUS_MX_SNAC_TILED_MIN_BATCH");
    return e ? atoi(e) : 8;
  }();
  return v;
}

static void pick_tiles(ConvGemmArgs& g, int nphase) {
  g.tiled = g.M % 64 == 0 && g.B >= snac_tiled_min_batch() ? 1 : 0;
  g.nsub = g.Tin >= 2048 ? 4 : 2;
  const int tiles = (g.M / 32) * ((g.Tin + 16 * g.nsub - 1) / (16 * g.nsub)) * nphase * g.B;
  const int Ktot = g.nseg * g.Cin;
  g.wk = 1;
  while (g.wk < 8 && tiles * g.wk * 2 <= 2048 && Ktot % (128 * g.wk) == 0 && Ktot / (2 * g.wk) >= 64)
    g.wk *= 2;
}

// Receptive-field cut of a PCM-only window decode (round 6): the kept samples [lo, hi) of a
// window depend on block 0's output positions [c0, c1) only (the output conv's 7 taps, each
// block's three residual units -- dilations 1, 3, 9, 7 taps: 39 positions either side -- and its
// ConvTranspose1d(k = 2s, stride s, pad ceil(s / 2)), whose output o reads the inputs i with
// 0 <= o + pad - i s < 2s), plus one position of margin.  Blocks 1-3 then run on that range
// alone (origins 8 c0, 32 c0, 64 c0): a zero at the cut edges stands where the full window has
// values, but no position the kept slice reads depends on one.  [0, 32 n) when nothing is cut.
static void snac_cut(int n_frames, int lo, int hi, int* c0, int* c1) {
  const int T1 = 32 * n_frames;
  *c0 = 0;
  *c1 = T1;
  if (hi <= lo) return;
  auto fdiv = [](int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
  int L = lo - 3, H = hi + 3;  // Snake(block 3 output) positions the output conv reads: [L, H)
  for (int b = 3; b >= 1; --b) {
    L -= 3 * (kDil[0] + kDil[1] + kDil[2]);
    H += 3 * (kDil[0] + kDil[1] + kDil[2]);
    const int st = kRates[b], pad = (st + 1) / 2;
    L = -fdiv(-(L + pad - 2 * st + 1), st);  // ceil
    H = fdiv(H - 1 + pad, st) + 1;
  }
  *c0 = std::max(0, L - 1);
  *c1 = std::min(T1, H + 1);
}

// Every launch of one window decode (io != null: the pointers come from s->io at run time).
static int snac_enqueue(mx_snac* s, const int32_t* frames, int n_frames, int batch,
                        const float* noise, uint64_t seed, const uint64_t* seeds, int16_t* pcm,
                        float* audio, int lo, int hi, hipStream_t st, const SnacIO* io,
                        bool pcm_only) {
  auto W = [&](const std::string& n) { return s->w[n]; };
  auto WB = [&](const std::string& n) -> const uint16_t* { return s->wbf.at(n); };
  const int B = batch;
  int T = 4 * n_frames;
  float* A = s->bufA;  // block activations x
  float* Bf = s->bufB; // scratch (dwconv output, ConvTranspose output)
  float* Cs = s->bufC; // Snake(x) for the next ConvTranspose / output conv
  // noise layout per window: [32N | 256N | 1024N | 2048N]
  const int nlen = 3360 * n_frames;
  // device-drawn noise (noise == null) is generated by the embed launch below
  const float* nz = noise ? noise : s->noise;
  const float* cb[3] = {W("q0.codebook"), W("q1.codebook"), W("q2.codebook")};
  const float* pw[3] = {W("q0.out_proj.w"), W("q1.out_proj.w"), W("q2.out_proj.w")};
  const float* pb[3] = {W("q0.out_proj.b"), W("q1.out_proj.b"), W("q2.out_proj.b")};
  MX_TRY(s, launch_snac_embed(frames, n_frames, B, cb, pw, pb, A, st, io,      // A: [T][768]
                              noise ? nullptr : s->noise, (int64_t)nlen * B, nlen, seed, seeds));
  MX_TRY(s, launch_dwconv(A, Bf, W("in.dw.w"), W("in.dw.b"), nullptr, nullptr, B, 768, T, 1, st));
  {
    ConvGemmArgs g{};
    g.Abf[0] = WB("in.pw.w"); g.X = Bf; g.bias = W("in.pw.b"); g.out = A; g.M = 1024; g.Cin = 768;
    g.Tin = T; g.Tout = T; g.B = B; g.nseg = 1; g.col_stride = 1; g.epi = CG_STORE;
    g.out2 = Cs; g.alpha2 = W("b0.alpha");
    pick_tiles(g, 1);
    MX_TRY(s, launch_conv_gemm(g, 1, st));                                      // A: [T][1024]
  }
  // PCM-only calls run blocks 1-3 on the kept slice's receptive field (snac_cut); a call that
  // also wants the whole window's audio runs them whole
  int c0 = 0, c1 = 32 * n_frames;
  if (pcm_only) snac_cut(n_frames, lo, hi, &c0, &c1);
  const bool cut = c1 - c0 < 32 * n_frames;
  int noff = 0, org = 0;  // noise offset of the block (full-window layout), cut origin
  for (int b = 0; b < 4; ++b) {
    const int cin = 1024 >> b, cout = cin / 2, sr = kRates[b];
    const std::string p = "b" + std::to_string(b) + ".";
    const float* Xin = Cs;
    if (b == 1 && cut) {  // block 0's Snake output, positions [c0, c1) of each window
      MX_TRY(s, launch_snac_cut(Cs, s->bufD, B, T, cin, c0, c1 - c0, st));
      Xin = s->bufD;
      T = c1 - c0;
      org = c0;
    }
    const int To = T * sr;
    org *= sr;
    {  // ConvTranspose1d on Snake(x): all sr phases in one launch, Cs [T][cin] -> Bf [To][cout]
      ConvGemmArgs g{};
      for (int ph = 0; ph < sr; ++ph) {
        g.Abf[ph] = s->up_bf[b][ph];
        g.dph[ph][0] = s->up_delta[b][ph][0];
        g.dph[ph][1] = s->up_delta[b][ph][1];
      }
      g.X = Xin; g.bias = W(p + "up.b"); g.out = Bf; g.M = cout; g.Cin = cin; g.Tin = T;
      g.Tout = To; g.B = B; g.nseg = 2; g.col_stride = sr; g.epi = CG_STORE;
      pick_tiles(g, sr);
      MX_TRY(s, launch_conv_gemm(g, sr, st));
    }
    T = To;
    {  // NoiseBlock: A = Bf + noise * (Wn Bf)
      ConvGemmArgs g{};
      g.Abf[0] = WB(p + "noise.w"); g.X = Bf; g.R = Bf; g.noise = nz + noff + org;
      g.noise_stride = nlen;
      g.out = A; g.M = cout; g.Cin = cout; g.Tin = T; g.Tout = T; g.B = B; g.nseg = 1;
      g.col_stride = 1; g.epi = CG_NOISE;
      pick_tiles(g, 1);
      MX_TRY(s, launch_conv_gemm(g, 1, st));
    }
    noff += 4 * n_frames * (b == 0 ? 8 : b == 1 ? 64 : b == 2 ? 256 : 512);  // full block output
    for (int r = 0; r < 3; ++r) {  // ResidualUnit(d): A += pw(Snake(dw_d(Snake(A))))
      const std::string q = p + "r" + std::to_string(r) + ".";
      MX_TRY(s, launch_dwconv(A, Bf, W(q + "dw.w"), W(q + "dw.b"), W(q + "alpha1"),
                              W(q + "alpha2"), B, cout, T, kDil[r], st));
      ConvGemmArgs g{};
      g.Abf[0] = WB(q + "pw.w"); g.X = Bf; g.bias = W(q + "pw.b"); g.R = A; g.out = A;
      g.M = cout; g.Cin = cout; g.Tin = T; g.Tout = T; g.B = B; g.nseg = 1; g.col_stride = 1;
      g.epi = CG_RESID;
      if (r == 2) {  // the block's output feeds Snake -> next ConvTranspose / output conv
        g.out2 = Cs;
        g.alpha2 = b < 3 ? W("b" + std::to_string(b + 1) + ".alpha") : W("out.alpha");
      }
      pick_tiles(g, 1);
      MX_TRY(s, launch_conv_gemm(g, 1, st));
    }
  }
  MX_TRY(s, launch_snac_out(Cs, W("out.conv.w"), W("out.conv.b"), B, T, lo - org, hi - org,
                            audio, pcm, st, io));
  return MX_OK;
}

// One window batch.  Device-drawn noise (noise == NULL, the serving path): the 36 launches (37
// with the receptive-field cut) are captured once per (n_frames, batch, slice, PCM only) into a
// hipGraph and replayed after a 1-thread
// kernel stores this call's pointers for the captured kernels to read.  Explicit noise (the
// parity tests) runs eagerly.
extern "C" int mx_snac_decode(mx_snac* s, const int32_t* frames, int n_frames, int batch,
                              const float* noise, uint64_t seed, const uint64_t* seeds,
                              int16_t* pcm, float* audio, int lo, int hi, void* stream) {
  if (!s || !frames) return MX_ERR_ARG;
  if (!s->final) MX_FAIL(s, MX_ERR_STATE, "not finalized");
  if (n_frames < 1 || n_frames > s->max_frames || batch < 1 || batch > s->max_batch)
    MX_FAIL(s, MX_ERR_ARG, "n_frames/batch out of range");
  const int Tout = 2048 * n_frames;
  if (pcm && (lo < 0 || hi < lo)) MX_FAIL(s, MX_ERR_ARG, "bad slice");
  if (hi > Tout) hi = Tout;  // torch slicing clamps: [2048:4096] of a 2048-sample window is empty
  if (lo > hi) lo = hi;
  hipStream_t st = (hipStream_t)stream;
  MX_TRY(s, hipSetDevice(s->device));
  // (a call that wants the whole window's audio runs every position: snac_cut)
  const bool pcm_only = pcm && !audio;
  if (noise) return snac_enqueue(s, frames, n_frames, batch, noise, seed, seeds, pcm, audio, lo,
                                 hi, st, nullptr, pcm_only);
  const std::array<int, 5> key{n_frames, batch, lo, hi, pcm_only ? 1 : 0};
  auto it = s->graphs.find(key);
  if (it == s->graphs.end()) {
    hipGraph_t g = nullptr;
    if (!s->cap) MX_TRY(s, hipStreamCreateWithFlags(&s->cap, hipStreamNonBlocking));
    MX_TRY(s, hipStreamBeginCapture(s->cap, hipStreamCaptureModeRelaxed));
    const int rc = snac_enqueue(s, nullptr, n_frames, batch, nullptr, 0, nullptr, nullptr,
                                nullptr, lo, hi, s->cap, s->io, pcm_only);
    hipError_t e2 = hipStreamEndCapture(s->cap, &g);
    if (rc != MX_OK) {
      if (g) (void)hipGraphDestroy(g);
      return rc;
    }
    MX_TRY(s, e2);
    hipGraphExec_t ex = nullptr;
    MX_TRY(s, hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
    s->graph_defs.push_back(g);
    it = s->graphs.emplace(key, ex).first;
  }
  SnacIO v{frames, seeds, seed, pcm, audio};
  MX_TRY(s, launch_set_io(s->io, v, st));
  MX_TRY(s, hipGraphLaunch(it->second, st));
  return MX_OK;
}


extern "C" const char* mx_snac_last_error(const mx_snac* s) {
  return s ? s->err.c_str() : g_err.c_str();
}

extern "C" void mx_snac_destroy(mx_snac* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  for (auto& kv : s->graphs) (void)hipGraphExecDestroy(kv.second);
  for (auto g : s->graph_defs) (void)hipGraphDestroy(g);
  if (s->cap) (void)hipStreamDestroy(s->cap);
  for (void* p : s->allocs) (void)hipFree(p);
  delete s;
}

// =====================================================================================
// SNAC encoder context (mx_snac_enc_*): audio -> speechpipe frames.  A context of its own: the
// decoder's buffers, graphs and addresses are untouched, and the codebooks (393 KB) are simply
// held twice.  Launches per encode: 1 stem + 4 x (3 x (depthwise + 1x1) + down-conv) + output
// depthwise + 3 quantiser levels = 33, enqueued eagerly on the caller's stream.
// =====================================================================================
static const int kEncRates[4] = {2, 4, 8, 8};
static const int kEncMaxFrames = 4096;  // 2048 * 48 floats per frame: offsets stay below 2^31

struct mx_snac_enc : SnacStore {  // (the planes here: [3][M][Kp])
  int max_frames = 0;
  float *cn[3] = {}, *cn2[3] = {};       // normalised codebooks and their squared lengths
  float *bufA = nullptr, *bufB = nullptr, *bufS = nullptr;
  bool final = false;
};

static void snac_enc_expect(mx_snac_enc* s) {
  auto& e = s->expect;
  e["enc.in.w"] = 48 * 7;
  e["enc.in.b"] = 48;
  for (int k = 0; k < 4; ++k) {
    const int c = 48 << k;
    const std::string p = "enc.b" + std::to_string(k) + ".";
    for (int r = 0; r < 3; ++r) {
      const std::string q = p + "r" + std::to_string(r) + ".";
      e[q + "alpha1"] = c;
      e[q + "dw.w"] = c * 7;
      e[q + "dw.b"] = c;
      e[q + "alpha2"] = c;
      e[q + "pw.w"] = (int64_t)c * c;
      e[q + "pw.b"] = c;
    }
    e[p + "alpha"] = c;
    e[p + "down.w"] = (int64_t)2 * c * c * 2 * kEncRates[k];
    e[p + "down.b"] = 2 * c;
  }
  e["enc.out.dw.w"] = 768 * 7;
  e["enc.out.dw.b"] = 768;
  for (int i = 0; i < 3; ++i) {
    const std::string p = "q" + std::to_string(i) + ".";
    e[p + "in_proj.w"] = 8 * 768;
    e[p + "in_proj.b"] = 8;
    e[p + "codebook"] = 4096 * 8;
    e[p + "out_proj.w"] = 768 * 8;
    e[p + "out_proj.b"] = 768;
  }
}

extern "C" int mx_snac_enc_create(int device, int max_frames, mx_snac_enc** out) {
  if (!out || max_frames < 1 || max_frames > kEncMaxFrames) {
    g_err = "max_frames out of range";
    return MX_ERR_ARG;
  }
  if (hipSetDevice(device) != hipSuccess) {
    g_err = "hipSetDevice failed";
    return MX_ERR_HIP;
  }
  auto* s = new mx_snac_enc();
  s->device = device;
  s->max_frames = max_frames;
  snac_enc_expect(s);
  *out = s;
  return MX_OK;
}

extern "C" int mx_snac_enc_set_weight(mx_snac_enc* s, const char* name, const void* data,
                                      int64_t numel, int dtype) {
  if (!s || !name || !data) return MX_ERR_ARG;
  if (dtype != MX_DTYPE_F32 && dtype != MX_DTYPE_BF16) MX_FAIL(s, MX_ERR_ARG, "bad dtype");
  if (s->final) MX_FAIL(s, MX_ERR_STATE, "weights are frozen after mx_snac_enc_finalize");
  return snac_store_set(s, "snac encoder weight", name, data, numel, dtype);
}

// fp32 [M][K] on the host -> three bf16 planes [3][M][Kp] on the device (zero columns past K)
static int snac_enc_planes(mx_snac_enc* s, const std::string& name, const std::vector<float>& A,
                           int M, int Kp) {
  void *tmp = nullptr, *p = nullptr;
  const size_t n = (size_t)M * Kp;
  MX_TRY(s, hipMalloc(&tmp, n * 4));
  hipError_t e = hipMemcpy(tmp, A.data(), n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&p, n * 3 * 2);
  if (e == hipSuccess) {
    s->allocs.push_back(p);
    s->wbf[name] = (uint16_t*)p;
    e = launch_split_planes((const float*)tmp, (uint16_t*)p, (int64_t)n, nullptr);
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  (void)hipFree(tmp);
  MX_TRY(s, e);
  return MX_OK;
}

extern "C" int mx_snac_enc_finalize(mx_snac_enc* s) {
  if (!s) return MX_ERR_ARG;
  if (s->final) MX_FAIL(s, MX_ERR_STATE, "already finalized");
  for (auto& kv : s->expect)
    if (!s->w.count(kv.first)) MX_FAIL(s, MX_ERR_STATE, "missing snac encoder weight " + kv.first);
  MX_TRY(s, hipSetDevice(s->device));
  for (int k = 0; k < 4; ++k) {
    const int c = 48 << k, taps = 2 * kEncRates[k];
    const std::string p = "enc.b" + std::to_string(k) + ".";
    const int Kp = (c + 31) / 32 * 32;  // C = 48: two 32-deep MFMA steps, the last 16 columns zero
    std::vector<float> W, A;
    for (int r = 0; r < 3; ++r) {
      const std::string name = p + "r" + std::to_string(r) + ".pw.w";
      W.resize((size_t)c * c);
      MX_TRY(s, hipMemcpy(W.data(), s->w[name], W.size() * 4, hipMemcpyDeviceToHost));
      A.assign((size_t)c * Kp, 0.f);
      for (int m = 0; m < c; ++m)
        for (int ci = 0; ci < c; ++ci) A[(size_t)m * Kp + ci] = W[(size_t)m * c + ci];
      const int rc = snac_enc_planes(s, name, A, c, Kp);
      if (rc != MX_OK) return rc;
    }
    // Conv1d weight [2C][C][taps] -> [2C][tap][C]: the K order of a channels-last input run
    const std::string name = p + "down.w";
    const int K = taps * c;
    W.resize((size_t)2 * c * K);
    MX_TRY(s, hipMemcpy(W.data(), s->w[name], W.size() * 4, hipMemcpyDeviceToHost));
    A.assign(W.size(), 0.f);
    for (int m = 0; m < 2 * c; ++m)
      for (int ci = 0; ci < c; ++ci)
        for (int j = 0; j < taps; ++j)
          A[(size_t)m * K + (size_t)j * c + ci] = W[((size_t)m * c + ci) * taps + j];
    const int rc = snac_enc_planes(s, name, A, 2 * c, K);
    if (rc != MX_OK) return rc;
  }
  for (int i = 0; i < 3; ++i) {
    void* p = nullptr;
    MX_TRY(s, hipMalloc(&p, (size_t)4096 * 9 * 4));
    s->allocs.push_back(p);
    s->cn[i] = (float*)p;
    s->cn2[i] = s->cn[i] + 4096 * 8;
    MX_TRY(s, launch_enc_codebook_norm(s->w["q" + std::to_string(i) + ".codebook"], s->cn[i],
                                       s->cn2[i], nullptr));
  }
  // activations: x, scratch and Snake(x), each sized by the full-rate 48-channel stage
  const size_t elems = (size_t)2048 * 48 * s->max_frames;
  for (float** b : {&s->bufA, &s->bufB, &s->bufS}) {
    void* p = nullptr;
    if (hipMalloc(&p, elems * 4) != hipSuccess) {
      (void)hipGetLastError();
      MX_FAIL(s, MX_ERR_OOM, "snac encoder buffers: allocation failed");
    }
    s->allocs.push_back(p);
    *b = (float*)p;
  }
  MX_TRY(s, hipDeviceSynchronize());
  s->final = true;
  return MX_OK;
}

// Waves splitting K in one run conv-GEMM tile: the deep down-convs (K = 3,072 and 6,144) have few
// output columns and a long serial K loop per wave, so their K is split while a wave keeps at
// least six 32-deep steps and the launch stays within ~8k waves.
static int snac_enc_pick_wk(int M, int Kp, int Tout) {
  const int tiles = (M / 48) * ((Tout + 31) / 32), steps = Kp / 32;
  int wk = 1;
  while (wk < 8 && steps % (2 * wk) == 0 && steps / (2 * wk) >= 6 && tiles * wk * 2 <= 16384) wk *= 2;
  return wk;
}

// audio -> z [4 n_frames][768] in bufB
static int snac_enc_latent_enqueue(mx_snac_enc* s, const float* audio, int64_t n_samples,
                                   int n_frames, hipStream_t st) {
  auto W = [&](const std::string& n) { return s->w.at(n); };
  float *A = s->bufA, *Bf = s->bufB, *S = s->bufS;
  int T = 2048 * n_frames;
  MX_TRY(s, launch_enc_stem(audio, n_samples, W("enc.in.w"), W("enc.in.b"), A, T, st));
  for (int k = 0; k < 4; ++k) {
    const int c = 48 << k, sr = kEncRates[k];
    const std::string p = "enc.b" + std::to_string(k) + ".";
    for (int r = 0; r < 3; ++r) {  // ResidualUnit(d): A += pw(Snake(dw_d(Snake(A))))
      const std::string q = p + "r" + std::to_string(r) + ".";
      if (c % 64)
        MX_TRY(s, launch_enc_dwconv(A, Bf, W(q + "dw.w"), W(q + "dw.b"), W(q + "alpha1"),
                                    W(q + "alpha2"), c, T, kDil[r], st));
      else
        MX_TRY(s, launch_dwconv(A, Bf, W(q + "dw.w"), W(q + "dw.b"), W(q + "alpha1"),
                                W(q + "alpha2"), 1, c, T, kDil[r], st));
      EncGemmArgs g{};
      g.A = s->wbf.at(q + "pw.w"); g.X = Bf; g.bias = W(q + "pw.b"); g.R = A; g.out = A;
      g.M = c; g.K = c; g.Kp = (c + 31) / 32 * 32; g.C = c; g.Tin = T; g.Tout = T;
      g.stride = 1; g.pad = 0;
      if (r == 2) {  // the block's closing Snake, for the down-conv
        g.out2 = S;
        g.alpha2 = W(p + "alpha");
      }
      g.wk = snac_enc_pick_wk(g.M, g.Kp, g.Tout);
      MX_TRY(s, launch_enc_gemm(g, st));
    }
    EncGemmArgs g{};  // Conv1d(C -> 2C, k = 2 sr, stride sr, pad ceil(sr / 2)) on Snake(x)
    g.A = s->wbf.at(p + "down.w"); g.X = S; g.bias = W(p + "down.b"); g.out = A;
    g.M = 2 * c; g.K = 2 * sr * c; g.Kp = g.K; g.C = c; g.Tin = T; g.Tout = T / sr;
    g.stride = sr; g.pad = (sr + 1) / 2;
    g.wk = snac_enc_pick_wk(g.M, g.Kp, g.Tout);
    MX_TRY(s, launch_enc_gemm(g, st));
    T /= sr;
  }
  MX_TRY(s, launch_dwconv(A, Bf, W("enc.out.dw.w"), W("enc.out.dw.b"), nullptr, nullptr, 1, 768, T,
                          1, st));
  return MX_OK;
}

// bufB (z, consumed as the residual) -> frames
static int snac_enc_quant_enqueue(mx_snac_enc* s, int n_frames, int32_t* frames, hipStream_t st) {
  for (int i = 0; i < 3; ++i) {
    const std::string p = "q" + std::to_string(i) + ".";
    EncQuantArgs q{};
    q.res = s->bufB; q.in_w = s->w.at(p + "in_proj.w"); q.in_b = s->w.at(p + "in_proj.b");
    q.cn = s->cn[i]; q.cn2 = s->cn2[i]; q.cb = s->w.at(p + "codebook");
    q.out_w = s->w.at(p + "out_proj.w"); q.out_b = s->w.at(p + "out_proj.b");
    q.frames = frames; q.n_frames = n_frames; q.level = i;
    MX_TRY(s, launch_enc_quant(q, st));
  }
  return MX_OK;
}

// every check of an audio call, before anything is enqueued; -> n_frames through *nf
static int snac_enc_check_audio(mx_snac_enc* s, const void* audio, int64_t n_samples,
                                const void* out, int* nf) {
  if (!audio || !out) MX_FAIL(s, MX_ERR_ARG, "null pointer");
  if (!s->final) MX_FAIL(s, MX_ERR_STATE, "not finalized");
  if (n_samples < 1) MX_FAIL(s, MX_ERR_ARG, "n_samples < 1");
  const int64_t n = (n_samples + 2047) / 2048;
  if (n > s->max_frames) MX_FAIL(s, MX_ERR_ARG, "audio longer than max_frames");
  *nf = (int)n;
  return MX_OK;
}

extern "C" int mx_snac_enc_encode(mx_snac_enc* s, const float* audio, int64_t n_samples,
                                  int32_t* frames_out, void* stream) {
  if (!s) return MX_ERR_ARG;
  int nf = 0;
  int rc = snac_enc_check_audio(s, audio, n_samples, frames_out, &nf);
  if (rc != MX_OK) return rc;
  MX_TRY(s, hipSetDevice(s->device));
  rc = snac_enc_latent_enqueue(s, audio, n_samples, nf, (hipStream_t)stream);
  if (rc != MX_OK) return rc;
  return snac_enc_quant_enqueue(s, nf, frames_out, (hipStream_t)stream);
}

extern "C" int mx_snac_enc_latent(mx_snac_enc* s, const float* audio, int64_t n_samples,
                                  float* z_out, void* stream) {
  if (!s) return MX_ERR_ARG;
  int nf = 0;
  int rc = snac_enc_check_audio(s, audio, n_samples, z_out, &nf);
  if (rc != MX_OK) return rc;
  MX_TRY(s, hipSetDevice(s->device));
  rc = snac_enc_latent_enqueue(s, audio, n_samples, nf, (hipStream_t)stream);
  if (rc != MX_OK) return rc;
  MX_TRY(s, hipMemcpyAsync(z_out, s->bufB, (size_t)nf * 4 * 768 * 4, hipMemcpyDefault,
                           (hipStream_t)stream));
  return MX_OK;
}

extern "C" int mx_snac_enc_quantize(mx_snac_enc* s, const float* z, int n_frames,
                                    int32_t* frames_out, void* stream) {
  if (!s) return MX_ERR_ARG;
  if (!z || !frames_out) MX_FAIL(s, MX_ERR_ARG, "null pointer");
  if (!s->final) MX_FAIL(s, MX_ERR_STATE, "not finalized");
  if (n_frames < 1 || n_frames > s->max_frames) MX_FAIL(s, MX_ERR_ARG, "n_frames out of range");
  MX_TRY(s, hipSetDevice(s->device));
  MX_TRY(s, hipMemcpyAsync(s->bufB, z, (size_t)n_frames * 4 * 768 * 4, hipMemcpyDefault,
                           (hipStream_t)stream));
  return snac_enc_quant_enqueue(s, n_frames, frames_out, (hipStream_t)stream);
}

extern "C" const char* mx_snac_enc_last_error(const mx_snac_enc* s) {
  return s ? s->err.c_str() : g_err.c_str();
}

extern "C" void mx_snac_enc_destroy(mx_snac_enc* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  for (void* p : s->allocs) (void)hipFree(p);
  delete s;
}
