"""Code-grammar decoding on the GPU (Code grammar) against the oracles.

mx_llm_set_grammar / mx_llm_set_slot_grammar through LlmEngine and BatchSynthesizer: the
per-row mask in the three lm_head epilogues (head_b1_kernel, gemv_kernel and the multi-row
gemm_rows_gram_kernel), the lm_head over the grammar's row window (option grammar_head 1) and
over the whole vocabulary (0, mixed steps, windows that cannot be aligned), and the samplers'
sweep over the allowed span.  mx_llm_grammar_window tells which of the two heads ran.

Oracle throughout: LlamaRef teacher-forced with the GPU's tokens, `_sampler_chain.penalise`,
then -inf outside A(k).  Logits at allowed ids within the 5e-3 rule (scaled by the logits'
spread as tests/test_gpu_sampler_chain.py does), exactly -inf elsewhere; greedy tokens through
`check_tokens`; sampled tokens against the restatement's draw from the GPU's own masked logits,
a mismatch accepted only with the race or filter margin below 1e-5, at most one per 12
row-steps.  The seeds of every sampled row below were vetted on the CPU: the restatement run
free (not teacher-forced) on the oracle's own masked logits has no step with a race margin,
a filter margin or a min-p distance under 1e-4.

The narrow model at the Orpheus vocabulary takes the project's parity weights (std 0.05, as
smoke() and the fp8 tests): with std 0.5 or 0.2 the oracle itself is ill-conditioned at
isolated steps of these rows -- its own logits move by up to 3.1 / 1.5 (logit spread 11 / 4.6)
when its bf16 KV rounding is switched off, 50 times the 5e-3 rule -- while at 0.05 the largest
such move is 0.03.
"""
import ctypes
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import llama_ref as L
from project_morpheus_amd import _lib
from project_morpheus_amd import config as C
from project_morpheus_amd.schedule import WindowScheduler, code_of_id
from project_morpheus_amd.weights import dequantize_fp8, quantize_fp8, synthetic_llm_weights

import _sampler_chain as SC
from _parity import check_tokens

pytestmark = pytest.mark.gpu

LOGIT_TOL = 5e-3
NEAR_TIE = 1e-5
ORPHEUS = C.ORPHEUS_GRAMMAR
ORPHEUS_WINDOW = (128256, 28684)                  # ids [128256, 156940): ISSUE / DESIGN §3
SMALL = C.CodeGrammar(1024, 256, 7, 1, 1000)      # vocabulary 5,000: window ids [768, 2816)
ODD = C.CodeGrammar(3000, 500, 4, 0, 2999)        # vocabulary 5,003: no window can be aligned
NARROW = (None, 311, 0.05)                        # the narrow model at the Orpheus vocabulary

Row = namedtuple("Row", "prompt penalty temperature top_p seed top_k min_p grammar",
                 defaults=(0.0, 1.0, 0, 0, 0.0, True))


def _cfg(vocab=None):
    kw = {} if vocab is None else {"vocab": vocab}
    return C.OrpheusConfig(hidden=512, layers=2, heads=4, kv_heads=2, ffn=1024, **kw)


def _ref(cfg, w, max_pos=256):
    rc = L.RefConfig(hidden=cfg.hidden, layers=cfg.layers, heads=cfg.heads,
                     kv_heads=cfg.kv_heads, ffn=cfg.ffn, vocab=cfg.vocab)
    return L.LlamaRef(rc, w, max_pos=max_pos)


@functools.lru_cache(maxsize=None)
def _model(vocab, seed, std):
    """(cfg, weights, oracle) of the narrow model, built once per shape for every test."""
    cfg = _cfg(vocab)
    w = synthetic_llm_weights(cfg, seed=seed, std=std, norm_jitter=0.5)
    return cfg, w, _ref(cfg, w)


def _engine(cfg, w, B, grammar, options=None, wdtype="bf16", logits=True):
    from project_morpheus_amd.engine import LlmEngine
    eng = LlmEngine(cfg, w, device=0, max_slots=B, max_pos=256, max_batch=B, max_prefill=64,
                    wdtype=wdtype)
    for k, v in (options or {}).items():
        eng.set_option(k, v)
    if logits:
        eng.enable_logits()
    if grammar is not None:
        eng.set_grammar(grammar)
    return eng


def _prefill(eng, slot, row, r, st):
    eng.prefill(slot, row, r.prompt, r.penalty, st, temperature=r.temperature, top_p=r.top_p,
                seed=r.seed, top_k=r.top_k, min_p=r.min_p, grammar=r.grammar)


def _run(cfg, w, rows, steps, grammar, options=None, wdtype="bf16", window=None):
    """Rows on their own slots, stepped together -> per row (tokens, logits).  `window`, a list,
    receives the engine's (lo, n, heads) of mx_llm_grammar_window at the end of the run."""
    B = len(rows)
    eng = _engine(cfg, w, B, grammar, options, wdtype)
    st = torch.cuda.Stream()
    out = [([], []) for _ in rows]
    for i, r in enumerate(rows):
        _prefill(eng, i, i, r, st)
        st.synchronize()
        out[i][1].append(eng.read_logits(i, st))    # the prefill's own pick
        out[i][0].append(int(eng.hist[i, len(r.prompt)]))
    for k in range(1, steps):
        eng.decode(B, st)
        st.synchronize()
        for i, r in enumerate(rows):
            out[i][1].append(eng.read_logits(i, st))
            out[i][0].append(int(eng.hist[i, len(r.prompt) + k]))
    if window is not None:
        window.extend(eng.grammar_window())
    eng.close()
    return out


def mask(lg, g, phase):
    """-inf outside A(phase)."""
    ids, stop = g.allowed(phase)
    out = np.full_like(np.asarray(lg, dtype=np.float32), -np.inf)
    out[ids.start:ids.stop] = lg[ids.start:ids.stop]
    if stop is not None:
        out[stop] = lg[stop]
    return out


def oracle_logits(ref, r, toks, g):
    """-> (masked, unmasked) penalised oracle logits per step, teacher-forced with `toks`."""
    _, rl = L.greedy_generate(ref, r.prompt, len(toks), 1.0, return_logits=True, forced=toks)
    seq, n0 = list(r.prompt) + list(toks), len(r.prompt)
    pen = [SC.penalise(rl[k].numpy(), seq, n0 + k, r.penalty, 0) for k in range(len(toks))]
    if not r.grammar:
        return pen, pen
    return [mask(p, g, k % g.phases) for k, p in enumerate(pen)], pen


def _check_row(ref, r, toks, logits, g, what):
    """-> (near-ties accepted, steps whose unmasked oracle argmax lies outside A(k))."""
    want, unmasked = oracle_logits(ref, r, toks, g)
    n0, ties, outside = len(r.prompt), 0, 0
    for k in range(len(toks)):
        ok = np.isfinite(want[k])
        assert np.all(np.isneginf(logits[k][~ok])), f"{what} step {k}: not -inf outside A(k)"
        tol = LOGIT_TOL * max(1.0, float(np.std(unmasked[k])))
        np.testing.assert_allclose(logits[k][ok], want[k][ok], atol=tol, rtol=LOGIT_TOL,
                                   err_msg=f"{what} step {k}")
        if r.grammar:
            assert g.allows(k % g.phases, toks[k]), f"{what} step {k}: {toks[k]} not allowed"
            outside += not g.allows(k % g.phases, int(np.argmax(unmasked[k])))
        if r.temperature > 0:
            tok, (race, fm) = SC.sample(logits[k], r.temperature, r.top_p, r.seed, n0 - 1 + k,
                                        r.top_k, r.min_p, return_margin=True)
            if toks[k] != tok:
                assert min(race, fm) < NEAR_TIE, \
                    f"{what} step {k}: {toks[k]} vs {tok} (race {race:.2e}, filter {fm:.2e})"
                ties += 1
        else:
            assert toks[k] == int(np.argmax(logits[k])), f"{what} step {k}"
    if r.temperature <= 0:
        check_tokens(toks, want, what=what)
    return ties, outside


# ---- 1. narrow model, one row ------------------------------------------------------------
def one_row():
    rng = np.random.default_rng(301)
    text = [int(x) for x in rng.integers(0, 128000, 6)]
    # code ids of several phases in the prompt: the penalty acts inside the spans
    codes = [int(ORPHEUS.code_base + 4096 * k + c) for k in (0, 1, 2, 3, 4, 5, 6)
             for c in rng.integers(1, 4096, 3)]
    return Row(text + codes + [C.START_OF_SPEECH], 1.3)


@pytest.mark.parametrize("grammar_head", [1, 0])
def test_narrow_one_row(grammar_head):
    """gemv_kernel's argmax epilogue (hidden 512 has no head_b1) over the row window and over
    the whole vocabulary; 15 steps: every phase twice and the wrap."""
    cfg, w, ref = _model(*NARROW)
    r, steps = one_row(), 15
    win = []
    toks, logits = _run(cfg, w, [r], steps, ORPHEUS, {"grammar_head": grammar_head}, window=win)[0]
    # the windowed launch really ran (the prefill's head and the decode step's), or never did
    assert tuple(win[:2]) == ORPHEUS_WINDOW
    assert win[2] >= 2 if grammar_head else win[2] == 0
    _, outside = _check_row(ref, r, toks, logits, ORPHEUS, f"grammar_head {grammar_head}")
    # the test cannot pass on code that ignores the mask ...
    assert outside >= 1
    # ... or the penalty inside the span
    want, unmasked = oracle_logits(ref, r, toks, ORPHEUS)
    _, raw = L.greedy_generate(ref, r.prompt, steps, 1.0, return_logits=True, forced=toks)
    assert any(np.any((unmasked[k] != raw[k].numpy())[np.isfinite(want[k])]) for k in range(steps))


# ---- 2. full width, one row: the head_b1 window --------------------------------------------
@pytest.mark.parametrize("wdtype", ["bf16", "fp8"])
def test_full_width_one_row(wdtype):
    """head1::head_b1_kernel (K 3,072) over the 28,684-row window, bf16 and e4m3, from the first
    token the prefill picks."""
    cfg = C.OrpheusConfig(layers=1)
    w = synthetic_llm_weights(cfg, seed=321)
    ref_w = w
    if wdtype == "fp8":
        w = quantize_fp8(w, cfg)
        ref_w = dequantize_fp8(w)
    rc = L.RefConfig(layers=1)
    ref = L.LlamaRef(rc, ref_w, max_pos=256)
    rng = np.random.default_rng(322)
    r = Row([int(x) for x in rng.integers(1000, 128000, 9)] + [C.START_OF_SPEECH], 1.1)
    win = []
    toks, logits = _run(cfg, w, [r], 8, ORPHEUS, wdtype=wdtype, window=win)[0]
    assert tuple(win[:2]) == ORPHEUS_WINDOW and win[2] >= 2
    _, outside = _check_row(ref, r, toks, logits, ORPHEUS, wdtype)
    assert outside >= 1


# ---- 3. narrow model, several rows ---------------------------------------------------------
def four_rows():
    rng = np.random.default_rng(331)
    p = [[int(x) for x in rng.integers(0, 128000, n)] for n in (5, 6, 9, 11)]
    return [Row(p[0], 1.3), Row(p[1], 1.1),
            Row(p[2], 1.1, 0.6, 0.9, 7001),                  # sampled, plain
            # sampled, top-k 40 / min-p 0.05 (temperature 0.1: at 0.6 these weights' 4,095
            # near-equal e leave the 40th and the 41st closer than 1e-4 at some step; the chain
            # at the serving temperature 0.6 is row 16 of seventeen_rows, whose weights spread more)
            Row(p[3], 1.1, 0.1, 0.9, 7002, 40, 0.05)]


def fifth_row():
    rng = np.random.default_rng(332)
    return Row([int(x) for x in rng.integers(0, 128000, 7)], 1.2, grammar=False)


def _check_rows(ref, rows, out, g, steps):
    ties = 0
    for i, r in enumerate(rows):
        t, _ = _check_row(ref, r, out[i][0], out[i][1], g, f"row {i}")
        ties += t
    assert ties <= len(rows) * steps // 12


def test_narrow_four_rows_four_phases():
    """Prompt lengths 5, 6, 9, 11: every step holds four different phases (gemm_rows_gram_kernel's
    argmax epilogue over the row window, sample_kernel / sample_chain_kernel over the spans)."""
    cfg, w, ref = _model(*NARROW)
    rows, steps = four_rows(), 15
    win = []
    _check_rows(ref, rows, _run(cfg, w, rows, steps, ORPHEUS, window=win), ORPHEUS, steps)
    assert tuple(win[:2]) == ORPHEUS_WINDOW and win[2] >= 5     # four prefills, the 4-row step


def test_narrow_mixed_step_runs_the_full_head():
    """A fifth, unconstrained row: the step runs the whole vocabulary (that row's logits match
    the unmasked oracle at every id), and only the constrained rows are masked."""
    cfg, w, ref = _model(*NARROW)
    rows, steps = four_rows() + [fifth_row()], 15
    win = []
    out = _run(cfg, w, rows, steps, ORPHEUS, window=win)
    _check_rows(ref, rows, out, ORPHEUS, steps)
    # only the four constrained prefills ran the window: no step with the fifth row did
    assert tuple(win[:2]) == ORPHEUS_WINDOW and win[2] == 4
    assert all(np.all(np.isfinite(lg)) for lg in out[4][1])
    assert any(not ORPHEUS.allows(k % 7, t) for k, t in enumerate(out[4][0]))


def seventeen_rows():
    rng = np.random.default_rng(341)
    rows = []
    for i in range(17):
        p = [int(x) for x in rng.integers(0, 5000, 4 + i % 7)]
        if i == 3:
            rows.append(Row(p, 1.1, 0.7, 0.9, 7103))
        elif i == 16:
            rows.append(Row(p, 1.1, 0.6, 0.9, 7116, 40, 0.05))
        else:
            rows.append(Row(p, 1.1 + 0.1 * (i % 3)))
    return rows


def test_seventeen_rows_cross_the_batch_tile():
    cfg, w, ref = _model(5000, 312, 0.2)
    rows, steps = seventeen_rows(), 9
    win = []
    _check_rows(ref, rows, _run(cfg, w, rows, steps, SMALL, window=win), SMALL, steps)
    assert tuple(win[:2]) == (768, 2048) and win[2] >= 18       # 17 prefills, the 17-row step


# ---- 4. a window that cannot be aligned ------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 3])
def test_alignment_fallback(n_rows):
    """Vocabulary 5,003 (odd), stop id right below the first range: results as defined,
    whatever head ran."""
    cfg, w, ref = _model(5003, 313, 0.2)
    rng = np.random.default_rng(351)
    rows = [Row([int(x) for x in rng.integers(0, 5003, 5 + 2 * i)] + [3001 + 500 * i], 1.3)
            for i in range(n_rows)]
    win = []
    out = _run(cfg, w, rows, 9, ODD, window=win)
    assert win == [0, 0, 0]                                     # no window: the mask alone
    outside = 0
    for i, r in enumerate(rows):
        outside += _check_row(ref, r, out[i][0], out[i][1], ODD, f"row {i}")[1]
    assert outside >= 1


# ---- 5. crafted logits through mx_llm_debug_sample ----------------------------------------
V5 = 5000
POSITIONS = list(range(0, 40))


def test_crafted_logits_through_debug_sample():
    cfg, w, _ = _model(V5, 312, 0.2)
    eng = _engine(cfg, w, 1, SMALL, logits=False)
    st = torch.cuda.Stream()
    prompt = [3, 1400, 77, 9]
    n0 = len(prompt)

    def phase(p):  # of the token that would take position p + 1
        return (p + 1 - n0) % SMALL.phases

    rng = np.random.default_rng(361)
    base = rng.normal(0, 2.0, V5).astype(np.float32)
    base[4000] = base.max() + 5.0                       # the global maximum: in no A(k)
    stop = base.copy()
    stop[SMALL.stop_id] = base.max() + 5.0              # the stop id above everything
    flat = np.full(V5, 0.25, np.float32)

    eng.prefill(0, 0, prompt, 1.1, st, grammar=True)    # a greedy slot
    st.synchronize()
    for p in POSITIONS:
        k = phase(p)
        got = eng.debug_sample(0, base, p, st)
        assert got == int(np.argmax(mask(base, SMALL, k))) and got != 4000
        got = eng.debug_sample(0, stop, p, st)
        assert (got == SMALL.stop_id) == (k == 0), (p, k, got)
        # the smallest-index maximum inside A(k): the stop id (1000) lies below every range
        ids, s = SMALL.allowed(k)
        assert eng.debug_sample(0, flat, p, st) == (s if s is not None else ids.start)
    for T, top_p, seed, top_k, min_p in ((0.8, 0.9, 41, 0, 0.0), (0.6, 0.9, 42, 40, 0.05),
                                         (1.0, 1.0, 43, 3, 0.0)):
        eng.release_row(0, st)
        eng.prefill(0, 0, prompt, 1.1, st, temperature=T, top_p=top_p, seed=seed, top_k=top_k,
                    min_p=min_p, grammar=True)
        st.synchronize()
        ties = 0
        for lg in (base, stop):
            for p in POSITIONS:
                got = eng.debug_sample(0, lg, p, st)
                assert SMALL.allows(phase(p), got)
                want, (race, fm) = SC.sample(mask(lg, SMALL, phase(p)), T, top_p, seed, p, top_k,
                                             min_p, return_margin=True)
                if got != want:
                    assert min(race, fm) < NEAR_TIE, f"pos {p}: {got} vs {want}"
                    ties += 1
        assert ties <= 2 * len(POSITIONS) // 12
    eng.close()


# ---- 6. lifecycle ---------------------------------------------------------------------------
def test_slot_lifecycle_and_move_row():
    cfg, w, _ = _model(V5, 312, 0.2)
    rng = np.random.default_rng(371)
    r = Row([int(x) for x in rng.integers(0, V5, 7)], 1.2)
    free = r._replace(grammar=False)
    steps = 12

    def stream(eng, st, r, row, move_at=None):
        """`r` on slot 0, decode row `row`, two-row steps throughout."""
        _prefill(eng, 0, row, r, st)
        toks = []
        for k in range(steps):
            if k == move_at:
                eng.move_row(0, row, st)
                row = 0
            if k:
                eng.decode(2, st)
            st.synchronize()
            toks.append(int(eng.hist[0, len(r.prompt) + k]))
        eng.release_row(row, st)
        return toks

    st = torch.cuda.Stream()
    eng = _engine(cfg, w, 2, None, logits=False)
    plain = stream(eng, st, free, 1)                # an engine that never had a grammar
    eng.close()
    eng = _engine(cfg, w, 2, SMALL, logits=False)
    first = stream(eng, st, r, 1)
    assert all(SMALL.allows(k % 7, t) for k, t in enumerate(first)) and first != plain
    assert stream(eng, st, free, 1) == plain
    assert stream(eng, st, r, 1) == first
    assert stream(eng, st, r, 1, move_at=5) == first
    assert stream(eng, st, free, 1, move_at=3) == plain
    eng.close()


# ---- 7. ABI refusals -------------------------------------------------------------------------
def test_abi_refusals():
    cfg, w, _ = _model(V5, 312, 0.2)
    eng = _engine(cfg, w, 1, None, logits=False)
    lib, h, st = eng.lib, eng.h, torch.cuda.Stream()

    def set_grammar(*f):
        g = _lib.CodeGrammar(*f)
        return lib.mx_llm_set_grammar(h, ctypes.byref(g))

    # no context grammar yet
    assert lib.mx_llm_set_slot_grammar(h, 0, 1) == _lib.MX_ERR_STATE
    assert lib.mx_llm_set_slot_grammar(h, 0, 0) == 0
    for bad in ((1024, 256, 0, 1, 1000),     # phases < 1
                (1024, 0, 7, 0, 1000),       # codes < 1
                (1024, 256, 7, -1, 1000),    # code_min outside [0, codes)
                (1024, 256, 7, 256, 1000),
                (-1, 256, 7, 1, 1000),       # code_base < 0
                (1024, 256, 16, 1, 1000),    # code_base + phases * codes > vocab
                (1024, 256, 7, 1, 1024),     # stop id inside a code range
                (1024, 256, 7, 1, 2815),
                (1024, 256, 7, 1, V5)):      # stop id past the vocabulary
        assert set_grammar(*bad) == _lib.MX_ERR_ARG, bad
    assert lib.mx_llm_set_slot_grammar(h, 0, 1) == _lib.MX_ERR_STATE  # (none of them took)
    assert set_grammar(1024, 256, 7, 1, -1) == 0                      # no stop id
    assert set_grammar(1024, 256, 7, 1, 2816) == 0                    # right past the ranges
    assert set_grammar(1024, 256, 7, 1, 1000) == 0
    assert lib.mx_llm_set_slot_grammar(h, 1, 1) == _lib.MX_ERR_ARG    # slot out of range
    assert lib.mx_llm_set_slot_grammar(h, 0, 1) == 0
    eng.prefill(0, 0, [5, 6, 7], 1.1, st)
    st.synchronize()
    assert set_grammar(1024, 256, 7, 1, 1000) == _lib.MX_ERR_STATE    # a row is active
    assert lib.mx_llm_set_grammar(h, None) == _lib.MX_ERR_STATE
    eng.release_row(0, st)
    st.synchronize()
    assert lib.mx_llm_set_grammar(h, None) == 0                       # NULL clears
    assert lib.mx_llm_set_slot_grammar(h, 0, 1) == _lib.MX_ERR_STATE
    with pytest.raises(_lib.MxError) as ei:
        eng.set_option("grammar_head", 2)
    assert ei.value.rc == _lib.MX_ERR_ARG
    eng.close()


# ---- 8. through BatchSynthesizer -----------------------------------------------------------
def test_through_batch_synthesizer():
    from project_morpheus_amd.batching import BatchSynthesizer, StreamRequest
    from project_morpheus_amd.engine import LlmEngine, SnacDecoder
    from project_morpheus_amd.weights import synthetic_snac_weights
    cfg, w, _ = _model(*NARROW)
    llm = LlmEngine(cfg, w, max_slots=2, max_pos=256, max_batch=2, max_prefill=64)
    dec = SnacDecoder(synthetic_snac_weights(seed=5), max_frames=7, max_batch=2)
    rng = np.random.default_rng(381)
    pa = [int(x) for x in rng.integers(0, 128000, 8)] + [C.START_OF_SPEECH]
    pb = [int(x) for x in rng.integers(0, 128000, 6)] + [C.START_OF_SPEECH]
    n = 35

    def reqs(audio):
        return [StreamRequest(prompt_ids=pa, max_tokens=n, stop_ids=(), audio=audio,
                              penalty=1.1, temperature=0.6, top_p=0.9, seed=7201, grammar=True),
                StreamRequest(prompt_ids=pb, max_tokens=n, stop_ids=(), audio=audio,
                              penalty=1.1, temperature=0.6, top_p=0.9, seed=7202)]

    # token-only: together the ids each yields alone
    alone = []
    for i in range(2):
        r = reqs(False)[i]
        BatchSynthesizer(llm, dec, depth=2).run([r])
        assert r.error is None and len(r.tokens) == n
        alone.append(r.tokens)
    both = reqs(False)
    BatchSynthesizer(llm, dec, depth=2).run(both)
    assert [r.tokens for r in both] == alone
    # with the SNAC decoder: the constrained stream's every token carries a code, so it gets
    # exactly the windows the reference schedule gives that many tokens
    sched, want = WindowScheduler(), 0
    for _ in range(n):
        want += len(sched.push(1))
    want += len(sched.flush())
    both = reqs(True)
    BatchSynthesizer(llm, dec, depth=2).run(both)
    con, unc = both
    assert con.error is None and unc.error is None
    assert con.tokens == alone[0] and unc.tokens == alone[1]
    assert all(1 <= code_of_id(t, i) < 4096 for i, t in enumerate(con.tokens))
    assert con.windows == want and want >= 3
    assert unc.windows != want
    assert not all((code_of_id(t, i) or 0) >= 1 for i, t in enumerate(unc.tokens))
    llm.close()
