"""GPU sampler chain (top-k, min-p, the last-n penalty window) vs tests/_sampler_chain.py.

csrc/sample_kernels.hip sample_chain_kernel and the window mode of commit_kernel /
window_prefill_kernel (csrc/llm_kernels.hip), through mx_llm_prefill_ex and
mx_llm_debug_sample.  Logits are checked against the LLM oracle (teacher-forced, raw logits
plus the windowed penalty rule) with the tolerances of tests/test_gpu_sampling.py; every token
against the restatement's draw from the GPU's own logits.  A token mismatch is accepted only
as a near-tie: the race margin or the filter-boundary margin below 1e-5, at most one per 12
row-steps.  The seeds below were vetted on the CPU: the restatement run on the oracle's own
logits has no step with either margin (or the distance of an e to the min-p bound) under 1e-4.
"""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import llama_ref as L
from oracle import sampling_ref as S
from project_morpheus_amd import config as C
from project_morpheus_amd.weights import synthetic_llm_weights

import _sampler_chain as SC
from _parity import check_tokens

pytestmark = pytest.mark.gpu

LOGIT_TOL = 5e-3
NEAR_TIE = 1e-5

Row = namedtuple("Row", "prompt penalty temperature top_p seed top_k min_p last_n",
                 defaults=(0, 0.0, 0))


def _cfg(vocab=None):
    kw = {} if vocab is None else {"vocab": vocab}
    return C.OrpheusConfig(hidden=512, layers=2, heads=4, kv_heads=2, ffn=1024, **kw)


@functools.lru_cache(maxsize=None)
def _model(vocab, seed, std):
    """(cfg, weights, oracle) of the narrow model, built once per shape for every test."""
    cfg = _cfg(vocab)
    w = synthetic_llm_weights(cfg, seed=seed, std=std, norm_jitter=0.5)
    rc = L.RefConfig(hidden=cfg.hidden, layers=cfg.layers, heads=cfg.heads,
                     kv_heads=cfg.kv_heads, ffn=cfg.ffn, vocab=cfg.vocab)
    return cfg, w, L.LlamaRef(rc, w, max_pos=256)


def _engine(cfg, w, B, debug_logits=True):
    from project_morpheus_amd.engine import LlmEngine
    eng = LlmEngine(cfg, w, device=0, max_slots=B, max_pos=256, max_batch=B, max_prefill=64)
    if debug_logits:
        eng.enable_logits()
    return eng


def _prefill(eng, slot, row, r, st):
    eng.prefill(slot, row, r.prompt, r.penalty, st, temperature=r.temperature, top_p=r.top_p,
                seed=r.seed, top_k=r.top_k, min_p=r.min_p, penalty_last_n=r.last_n)


def _run(cfg, w, rows, steps, debug_logits=True):
    """Rows on their own slots, stepped together -> per row (tokens, logits)."""
    from _coverage import check_declared
    B = len(rows)
    check_declared(cfg, [len(r.prompt) for r in rows], steps)
    eng = _engine(cfg, w, B, debug_logits)
    st = torch.cuda.Stream()
    out = [([], []) for _ in rows]
    for i, r in enumerate(rows):
        _prefill(eng, i, i, r, st)
    for k in range(steps):
        if k:
            eng.decode(B, st)
        st.synchronize()
        for i, r in enumerate(rows):
            if debug_logits:
                out[i][1].append(eng.read_logits(i, st))
            out[i][0].append(int(eng.hist[i, len(r.prompt) + k]))
    eng.close()
    return out


def _raw_logits(ref, r, toks):
    """The oracle's unpenalised logits of every step, teacher-forced with the GPU's tokens."""
    _, rl = L.greedy_generate(ref, r.prompt, len(toks), 1.0, return_logits=True, forced=toks)
    return [x.numpy() for x in rl]


def _check_row(ref, r, toks, logits, what):
    """Logits of every step against the oracle under the row's penalty window, tokens against
    the restatement; -> (near-ties accepted, steps where the window changes the logits)."""
    raw = _raw_logits(ref, r, toks)
    seq = list(r.prompt) + list(toks)
    n0, ties, differs = len(r.prompt), 0, 0
    for k in range(len(toks)):
        want_l = SC.penalise(raw[k], seq, n0 + k, r.penalty, r.last_n)
        tol = LOGIT_TOL * max(1.0, float(np.std(want_l)))
        np.testing.assert_allclose(logits[k], want_l, atol=tol, rtol=LOGIT_TOL,
                                   err_msg=f"{what} step {k}")
        whole = SC.penalise(raw[k], seq, n0 + k, r.penalty, 0)
        if np.any(np.abs(whole - want_l) > tol + LOGIT_TOL * np.abs(want_l)):
            differs += 1
        want, (race, fm) = SC.sample(logits[k], r.temperature, r.top_p, r.seed, n0 - 1 + k,
                                     r.top_k, r.min_p, return_margin=True)
        if toks[k] != want:
            assert min(race, fm) < NEAR_TIE, \
                f"{what} step {k}: {toks[k]} vs {want} (race {race:.2e}, filter {fm:.2e})"
            ties += 1
    return ties, differs


def full_vocab_rows():
    rng = np.random.default_rng(72)
    V = _cfg().vocab
    pa = [int(x) for x in rng.integers(0, V, 11)]
    pb = [int(x) for x in rng.integers(0, V, 5)]
    pc = [int(x) for x in rng.integers(0, V, 7)]
    x, a, b = (int(t) for t in rng.integers(0, V, 3))
    return [Row(pa, 1.1, 0.6, 0.9, 1234567, 40, 0.05, 64),    # (a) the llama.cpp preset
            Row(pb, 1.1, 1.0, 1.0, 2**40 + 17),               # (b) neutral extras, chain kernel
            Row(pc, 1.3, 0.0, 1.0, 0, 0, 0.0, 4),             # (c) greedy, evicts from step 0
            Row([x, a, a, b], 1.2, 0.8, 1.0, 99, 5, 0.0, 3)]  # (d) `a` counted twice


FULL_STEPS = 12


def test_full_vocab_four_rows():
    """Orpheus vocabulary (156,940 ids), std-0.5 weights (a penalty factor moves a logit by far
    more than the tolerance), four rows with different chains in one batch."""
    cfg, w, ref = _model(None, 71, 0.5)
    rows = full_vocab_rows()
    out = _run(cfg, w, rows, FULL_STEPS)
    ties = 0
    for i, r in enumerate(rows):
        toks, logits = out[i]
        t, differs = _check_row(ref, r, toks, logits, f"row {'abcd'[i]}")
        ties += t
        if i == 1:  # neutral extras next to a chain row: the oracle's own sampler
            n0 = len(r.prompt)
            for k in range(FULL_STEPS):
                want, margin = S.sample(logits[k], r.temperature, r.top_p, r.seed, n0 - 1 + k,
                                        return_margin=True)
                assert toks[k] == want or margin < NEAR_TIE, f"row b step {k}"
        if i >= 2:  # the test cannot pass on code that ignores the window
            assert differs >= 1, f"row {'abcd'[i]}: the window never changes the logits"
    assert ties <= len(rows) * FULL_STEPS // 12
    # row (d): `a` stays penalised for exactly one more step after the first eviction
    d, a = rows[3], rows[3].prompt[1]
    seq = d.prompt + out[3][0]
    assert a in SC.window_ids(seq, 4, 3) and a in SC.window_ids(seq, 5, 3)
    assert (a in SC.window_ids(seq, 6, 3)) == (a in seq[3:6])


def one_row():
    p = [int(x) for x in np.random.default_rng(74).integers(0, 5000, 9)]
    return Row(p, 1.1, 0.6, 0.9, 4321, 40, 0.05, 64)


def test_single_row_path_and_product_mode():
    """B = 1 (the single-row lm_head keeps the logits for the sampler), the parameters of row
    (a); without the debug switch the tokens are the same (product-mode logits retention)."""
    cfg, w, ref = _model(5000, 73, 0.2)
    r, steps = one_row(), 16
    toks, logits = _run(cfg, w, [r], steps)[0]
    ties, _ = _check_row(ref, r, toks, logits, "one row")
    assert ties <= 1
    product = _run(cfg, w, [r], steps, debug_logits=False)[0][0]
    assert product == toks


# ---- crafted logits through mx_llm_debug_sample ---------------------------------------
V3 = 5000
POSITIONS = list(range(0, 40)) + [77, 255, 4096, 2**31 - 1]


def _crafted():
    """name -> (logits, [(Row parameters, check(tokens, kept ids))])."""
    rng = np.random.default_rng(81)
    base = rng.normal(0, 2.0, V3).astype(np.float32)
    base[1234] = base.max() + 1.0                      # a single maximum
    straddle = np.full(V3, -5.0, np.float32)
    straddle[[5, 900, 901, 2000, 3000, 4000, 4999]] = 2.0
    straddle[5] = 3.0                                  # 1 id, then a group of 6 tied for 2nd
    maxima = np.full(V3, 1.0 - 1e-3, np.float32)
    maxima[[17, 900]] = 1.0                            # two maxima, the rest a hair below
    low = np.full(V3, -200.0, np.float32)              # e = 0
    low[::2] = -30.0                                   # 0 < e < 2^-40: f = 0
    low[[10, 21, 30]] = [0.0, -1.0, -2.0]
    flat = np.full(V3, 0.25, np.float32)
    tail = np.full(V3, -200.0, np.float32)
    tail[100:2100] = np.float32(np.log(1e-3))          # 2,000 ids at e ~ 1e-3: mass 2
    tail[7] = 0.0                                      # one id at e = 1
    return base, straddle, maxima, low, flat, tail


def _draws(eng, st, r, lg):
    eng.release_row(0, st)
    _prefill(eng, 0, 0, r, st)
    st.synchronize()
    got = [eng.debug_sample(0, lg, p, st) for p in POSITIONS]
    ties = 0
    for p, g in zip(POSITIONS, got):
        want, (race, fm) = SC.sample(lg, r.temperature, r.top_p, r.seed, p, r.top_k, r.min_p,
                                     return_margin=True)
        if g != want:
            assert min(race, fm) < NEAR_TIE, f"pos {p}: {g} vs {want}"
            ties += 1
    assert ties <= len(POSITIONS) // 12
    return got


def test_crafted_logits_through_debug_sample():
    cfg, w, _ = _model(V3, 73, 0.2)
    base, straddle, maxima, low, flat, tail = _crafted()
    eng = _engine(cfg, w, 1, debug_logits=False)
    st = torch.cuda.Stream()
    prompt = [3, 1400, 77]

    def row(T, top_p, seed, top_k=0, min_p=0.0):
        return Row(prompt, 1.1, T, top_p, seed, top_k, min_p, 0)

    # top_k = 1: the smallest-index maximum
    assert set(_draws(eng, st, row(1.0, 1.0, 5, top_k=1), base)) == {1234}
    # top_k >= V: the neutral chain
    neutral = _draws(eng, st, row(0.7, 0.9, 6), base)
    assert _draws(eng, st, row(0.7, 0.9, 6, top_k=V3), base) == neutral
    assert _draws(eng, st, row(0.7, 0.9, 6, top_k=V3 + 7), base) == neutral
    # a tie group straddling the k-th place is kept whole
    got = _draws(eng, st, row(1.0, 1.0, 7, top_k=3), straddle)
    group = {5, 900, 901, 2000, 3000, 4000, 4999}
    assert set(got) <= group and len(set(got)) > 3
    # min_p = 1: only the maxima
    got = _draws(eng, st, row(1.0, 1.0, 8, min_p=1.0), maxima)
    assert set(got) == {17, 900}
    # logits so low that f = 0 are never drawn and not counted by top-k (k past the last
    # f > 0 id keeps exactly those)
    got = _draws(eng, st, row(1.0, 1.0, 9, top_k=5), low)
    assert set(got) == {10, 21, 30}
    assert set(_draws(eng, st, row(1.0, 1.0, 9, top_k=2), low)) == {10, 21}
    # all logits equal: one tie group, whatever the filters
    for r in (row(1.0, 0.5, 10, top_k=1, min_p=1.0), row(0.6, 1.0, 10, top_k=40),
              row(1.0, 0.5, 10)):
        got = _draws(eng, st, r, flat)
        assert len(set(got)) > len(POSITIONS) // 2
    # the heavy tail: Z is taken over F.  Unfiltered, top_p 0.5 of Z = 3 keeps the tail's tie
    # group (mass above it 1 < 1.5); with top-k 1 or min-p 0.01 only the top id survives
    got = _draws(eng, st, row(1.0, 0.5, 11), tail)
    assert 7 in got and any(100 <= g < 2100 for g in got)
    assert all(g == 7 or 100 <= g < 2100 for g in got)
    assert set(_draws(eng, st, row(1.0, 0.5, 11, top_k=1), tail)) == {7}
    assert set(_draws(eng, st, row(1.0, 0.5, 11, min_p=0.01), tail)) == {7}
    # a greedy slot returns the smallest-index maximum
    eng.release_row(0, st)
    eng.prefill(0, 0, prompt, 1.1, st)
    st.synchronize()
    assert eng.debug_sample(0, maxima, 3, st) == 17
    assert eng.debug_sample(0, flat, 3, st) == 0
    # the ABI rejects what it cannot run
    from project_morpheus_amd import _lib
    for bad in ({"top_k": -1}, {"min_p": -0.5}, {"min_p": 1.5}, {"min_p": float("nan")},
                {"penalty_last_n": -1}, {"penalty_last_n": 256}):
        with pytest.raises(_lib.MxError) as ei:
            eng.prefill(0, 0, prompt, 1.1, st, **bad)
        assert ei.value.rc == _lib.MX_ERR_ARG
    eng.close()


# ---- slot and row lifecycle -------------------------------------------------------------
def test_window_survives_move_row_and_slots_start_clean():
    """A windowed stream moved mid-utterance continues as if unmoved; a whole-sequence request
    on the released slot, then a windowed one again, each start from clean penalty state."""
    cfg, w, ref = _model(V3, 73, 0.2)
    rng = np.random.default_rng(91)
    win = Row([int(x) for x in rng.integers(0, V3, 7)], 1.3, 0.0, 1.0, 0, 0, 0.0, 4)
    whole = Row([int(x) for x in rng.integers(0, V3, 9)], 1.1, 0.0, 1.0, 0)
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
    eng = _engine(cfg, w, 2, debug_logits=False)
    unmoved = stream(eng, st, win, 1)
    eng.close()
    # the unmoved run follows the oracle under the window (tie-aware, teacher-forced)
    raw = _raw_logits(ref, win, unmoved)
    seq = win.prompt + unmoved
    want = [SC.penalise(raw[k], seq, len(win.prompt) + k, win.penalty, win.last_n)
            for k in range(steps)]
    assert check_tokens(unmoved, want, what="windowed") >= steps - 1
    whole_seq = [SC.penalise(raw[k], seq, len(win.prompt) + k, win.penalty, 0)
                 for k in range(steps)]
    assert any(np.abs(a - b).max() > 0.05 for a, b in zip(want, whole_seq))

    eng = _engine(cfg, w, 2, debug_logits=False)
    assert stream(eng, st, win, 1, move_at=5) == unmoved
    got = stream(eng, st, whole, 0)     # the same slot, whole-sequence penalty
    _, rl = L.greedy_generate(ref, whole.prompt, steps, whole.penalty, return_logits=True,
                              forced=got)
    assert check_tokens(got, rl, what="whole sequence after windowed") >= steps - 1
    assert stream(eng, st, win, 1) == unmoved   # and the reverse order
    eng.close()


# ---- through batching ------------------------------------------------------------------
def test_batching_requests_with_different_extras():
    """Two token-only requests, one windowed and one with top-k, yield together the ids each
    yields alone (fixed seeds): the extras are per-slot state."""
    from project_morpheus_amd.batching import BatchSynthesizer, StreamRequest
    from project_morpheus_amd.engine import LlmEngine, SnacDecoder
    from project_morpheus_amd.weights import synthetic_snac_weights
    cfg, w, _ = _model(1000, 75, 0.5)
    llm = LlmEngine(cfg, w, max_slots=2, max_pos=256, max_batch=2, max_prefill=64)
    dec = SnacDecoder(synthetic_snac_weights(seed=5), max_frames=7, max_batch=1)
    rng = np.random.default_rng(76)
    pa = [int(x) for x in rng.integers(0, cfg.vocab, 8)]
    pb = [int(x) for x in rng.integers(0, cfg.vocab, 6)]

    def reqs():
        return [StreamRequest(prompt_ids=pa, max_tokens=14, stop_ids=(), audio=False,
                              penalty=1.3, temperature=0.7, top_p=0.9, seed=31,
                              penalty_last_n=4),
                StreamRequest(prompt_ids=pb, max_tokens=14, stop_ids=(), audio=False,
                              penalty=1.1, temperature=0.8, top_p=1.0, seed=32, top_k=5)]

    alone = []
    for i in range(2):
        r = reqs()[i]
        BatchSynthesizer(llm, dec, depth=2).run([r])
        assert r.error is None and len(r.tokens) == 14
        alone.append(r.tokens)
    both = reqs()
    BatchSynthesizer(llm, dec, depth=2).run(both)
    assert [r.tokens for r in both] == alone
    llm.close()
