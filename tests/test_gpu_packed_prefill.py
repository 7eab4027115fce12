"""Packed prefill (mx_llm_prefill_batch through LlmEngine.prefill_batch) against the oracles.

Several prompts run the layers as one row set, one lm_head launch covers their last rows, one
sampler node picks the first tokens, one commit binds arbitrary distinct decode rows.  Every
stream of a pack is then stepped with the others and compared, first token included, with
LlamaRef teacher-forced on the GPU's tokens (tests/_packed.py: logits atol = rtol = 5e-3, greedy
tokens tie-aware with margin 1e-2, sampled tokens against the restatement's draw from the GPU's
own logits, race margin 1e-5).

Shapes: the narrow model (hidden 512, 2 layers, 4/2 heads, ffn 1024, vocab 1000) with the
parity weights (std 0.05) unless a test says otherwise; e4m3 weights need widths that are
multiples of 1024, so that test takes the narrow fp8 model of tests/test_gpu_fp8.py.
"""
import ctypes
import functools

import numpy as np
import pytest

from project_morpheus_amd import _lib
from project_morpheus_amd import config as C
from project_morpheus_amd.weights import dequantize_fp8, quantize_fp8, synthetic_llm_weights

import _packed as P
import _sampler_chain as SC
from _packed import Seg

pytestmark = pytest.mark.gpu

GRAMMAR = C.CodeGrammar(256, 64, 7, 1, 200)   # vocabulary 1,000: row window ids [0, 768)


def _cfg(**kw):
    return C.OrpheusConfig(**{**dict(hidden=512, layers=2, heads=4, kv_heads=2, ffn=1024,
                                     vocab=1000), **kw})


@functools.lru_cache(maxsize=None)
def _model(seed=401):
    cfg = _cfg()
    w = synthetic_llm_weights(cfg, seed=seed, std=0.05, norm_jitter=0.5)
    return cfg, w, P.ref_of(cfg, w)


# ---- 1. ragged pack, scrambled placement ---------------------------------------------------
def test_ragged_pack_scrambled_placement():
    """R = 64 rows: the 32-row tile edge falls inside segment 1, segment 2 has a single id.
    Disjoint id sets and different penalties: a seen byte marked on the wrong slot moves a
    logit by 10-30 % of its value."""
    cfg, w, ref = _model()
    prompts = P.disjoint_prompts(cfg.vocab, (5, 37, 1, 21), 402)
    segs = [Seg(p, pen) for p, pen in zip(prompts, (1.3, 1.1, 1.0, 1.2))]
    rows, slots = (2, 0, 3, 1), (3, 1, 0, 2)
    eng, st = P.engine(cfg, w, 4, 64), P.stream()
    out = P.run_pack(eng, st, segs, rows, slots, 12)
    P.check_pack(eng, ref, segs, rows, slots, out, "ragged")
    # the penalty matters at these weights: the check above cannot pass without the seen marks
    raw = P.raw_logits(ref, segs[:1], [out[0][0][:1]])[0][0]
    pen = SC.penalise(raw, segs[0].prompt, len(segs[0].prompt), segs[0].penalty, 0)
    assert np.abs(pen - raw).max() > 10 * P.LOGIT_TOL
    eng.close()


# ---- 2. different split counts in one pack -------------------------------------------------
@pytest.mark.parametrize("options", [None, {"att_nw_batch": 4, "att_cpw_batch": 1}],
                         ids=["default", "splits128"])
def test_different_split_counts(options):
    """Lengths (140, 9, 70).  The default shape of a 219-row launch is one 256-position split;
    with 128-position splits (4 waves x 1 chunk) the 140-id segment takes two splits while the
    others take one, and the grid is sized by the longest."""
    cfg, w, ref = _model()
    rng = np.random.default_rng(403)
    segs = [Seg([int(x) for x in rng.integers(0, cfg.vocab, n)], 1.1) for n in (140, 9, 70)]
    rows, slots = (0, 1, 2), (2, 0, 1)
    eng, st = P.engine(cfg, w, 3, 256, options=options), P.stream()
    out = P.run_pack(eng, st, segs, rows, slots, 6)
    P.check_pack(eng, ref, segs, rows, slots, out, "splits")
    eng.close()


# ---- 3. mixed generation parameters --------------------------------------------------------
def mixed_segments():
    rng = np.random.default_rng(404)
    V = 1000
    p = [[int(x) for x in rng.integers(0, V, n)] for n in (6, 11, 8)]
    a, b = 17, 23
    rest = [int(x) for x in rng.choice([i for i in range(V) if i not in (a, b)], 5, replace=False)]
    return [Seg(p[0], 1.3),                                    # greedy
            Seg(p[1], 1.1, 0.6, 0.9, 1234567),                 # temperature / top-p
            Seg(p[2], 1.1, 0.1, 1.0, 7002, 5, 0.05),           # top-k 5, min-p 0.05
            Seg([a, a, b] + rest, 1.3, 0.0, 1.0, 0, 0, 0.0, 4)]  # window 4; a, b lie outside it


def test_mixed_generation_parameters():
    cfg, w, ref = _model()
    segs = mixed_segments()
    rows, slots = (1, 3, 0, 2), (0, 1, 2, 3)
    eng, st = P.engine(cfg, w, 4, 64), P.stream()
    out = P.run_pack(eng, st, segs, rows, slots, 8)
    ties = P.check_pack(eng, ref, segs, rows, slots, out, "mixed")
    assert ties <= 1            # two sampled rows x 9 tokens: at most one near-tie per 12
    # the window really differs from the whole sequence at the first token: id 17 is in the
    # prompt, outside the last 4 positions
    d = segs[3]
    raw = P.raw_logits(ref, [d], [out[3][0][:1]])[0][0]
    whole = SC.penalise(raw, d.prompt, len(d.prompt), d.penalty, 0)
    assert abs(whole[17] - raw[17]) > 4 * P.LOGIT_TOL
    assert out[3][1][0][17] == pytest.approx(raw[17], abs=P.LOGIT_TOL + P.LOGIT_TOL * abs(raw[17]))
    eng.close()


# ---- 4. grammar ----------------------------------------------------------------------------
def _grammar_segments(free_one):
    rng = np.random.default_rng(405)
    p = [[int(x) for x in rng.integers(0, 1000, n)] for n in (7, 12, 4)]
    return [Seg(p[0], 1.3, grammar=True),
            Seg(p[1], 1.1, 0.6, 0.9, 99, grammar=not free_one),
            Seg(p[2], 1.1, grammar=True)]


@pytest.mark.parametrize("free_one", [False, True], ids=["all_constrained", "one_free"])
def test_grammar(free_one):
    cfg, w, ref = _model()
    segs = _grammar_segments(free_one)
    rows, slots = (2, 0, 1), (0, 1, 2)
    eng, st = P.engine(cfg, w, 3, 64, grammar=GRAMMAR), P.stream()
    lo, n, heads0 = eng.grammar_window()
    assert (lo, n) == (0, 768)
    eng.prefill_batch([P.segment(s, slots[i], rows[i]) for i, s in enumerate(segs)], st)
    st.synchronize()
    heads1 = eng.grammar_window()[2]
    # one lm_head launch over the row window for the whole call, or none when a row is free
    assert heads1 - heads0 == (0 if free_one else 1)
    out = [([], []) for _ in segs]
    P.read_step(eng, st, segs, rows, slots, 0, out)
    for k in range(1, 4):
        eng.decode(3, st)
        st.synchronize()
        P.read_step(eng, st, segs, rows, slots, k, out)
    for i, s in enumerate(segs):
        first, lg = out[i][0][0], out[i][1][0]
        if s.grammar:
            assert GRAMMAR.allows(0, first)
            assert np.isneginf(lg).sum() == cfg.vocab - 64   # 63 codes + the stop id stay
        else:
            assert np.all(np.isfinite(lg))                   # only the constrained rows are masked
    P.check_pack(eng, ref, segs, rows, slots, out, "grammar", GRAMMAR)
    eng.close()


# ---- 5. e4m3 weights -----------------------------------------------------------------------
def test_fp8_pack():
    cfg = C.OrpheusConfig(hidden=1024, layers=2, heads=8, kv_heads=2, ffn=2048, vocab=1000)
    qw = quantize_fp8(synthetic_llm_weights(cfg, seed=406, std=0.05, norm_jitter=0.5), cfg)
    ref = P.ref_of(cfg, dequantize_fp8(qw))
    rng = np.random.default_rng(407)
    segs = [Seg([int(x) for x in rng.integers(0, cfg.vocab, n)], 1.1) for n in (18, 33)]
    rows, slots = (1, 0), (0, 1)
    eng, st = P.engine(cfg, qw, 2, 64, wdtype="fp8"), P.stream()
    out = P.run_pack(eng, st, segs, rows, slots, 6)
    P.check_pack(eng, ref, segs, rows, slots, out, "fp8")
    eng.close()


# ---- 6. Orpheus width ----------------------------------------------------------------------
def test_orpheus_width_pack():
    """The true-width row classes at R = 73 (hidden 3072, 24/8 heads, ffn 8192)."""
    cfg = C.OrpheusConfig(layers=2, vocab=16384)
    w = synthetic_llm_weights(cfg, seed=408)
    ref = P.ref_of(cfg, w)
    rng = np.random.default_rng(409)
    segs = [Seg([int(x) for x in rng.integers(0, cfg.vocab, n)], 1.1) for n in (24, 40, 9)]
    rows, slots = (2, 0, 1), (1, 2, 0)
    eng, st = P.engine(cfg, w, 3, 128), P.stream()
    out = P.run_pack(eng, st, segs, rows, slots, 4)
    P.check_pack(eng, ref, segs, rows, slots, out, "orpheus width")
    eng.close()


# ---- 7. k = 1 ------------------------------------------------------------------------------
def test_one_segment_pack_equals_prefill():
    cfg, w, ref = _model()
    rng = np.random.default_rng(410)
    s = Seg([int(x) for x in rng.integers(0, cfg.vocab, 19)], 1.2)
    st = P.stream()
    a = P.engine(cfg, w, 2, 64)
    got = P.run_pack(a, st, [s], (1,), (1,), 4)[0]
    a.close()
    b = P.engine(cfg, w, 2, 64)
    b.prefill(1, 1, s.prompt, s.penalty, st)
    want = ([], [])
    for k in range(5):
        if k:
            b.decode(2, st)
        st.synchronize()
        want[1].append(b.read_logits(1, st))
        want[0].append(int(b.hist[1, len(s.prompt) + k]))
    b.close()
    for k in range(5):
        np.testing.assert_allclose(got[1][k], want[1][k], atol=P.LOGIT_TOL, rtol=P.LOGIT_TOL)
        if got[0][k] != want[0][k]:   # a near-tie may resolve differently; then the runs part
            assert abs(want[1][k][got[0][k]] - want[1][k][want[0][k]]) < 1e-2
            break
    P.check_stream(s, got[0], got[1], P.raw_logits(ref, [s], [got[0]])[0], "k = 1")


# ---- 8. refusals ---------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was():
    cfg, w, ref = _model()
    rng = np.random.default_rng(411)
    live = Seg([int(x) for x in rng.integers(0, cfg.vocab, 9)], 1.2)
    eng, st = P.engine(cfg, w, 4, 128, max_pos=128), P.stream()
    eng.prefill(0, 0, live.prompt, live.penalty, st)
    ok = [3, 4, 5]

    def seg(slot=1, row=1, ids=ok, **kw):
        return dict(slot=slot, row=row, ids=ids, penalty=1.1, **kw)

    cases = {
        "no segments": [],
        "more segments than rows": [seg(i % 4, i % 4) for i in range(5)],
        "rows past max_prefill": [seg(1, 1, [1] * 70), seg(2, 2, [2] * 70)],
        "empty prompt": [seg(ids=[])],
        "prompt of max_pos ids": [seg(ids=[1] * 128)],
        "slot past the end": [seg(slot=4)],
        "negative slot": [seg(slot=-1)],
        "row past the end": [seg(row=4)],
        "negative row": [seg(row=-1)],
        "slot twice": [seg(1, 1), seg(1, 2)],
        "row twice": [seg(1, 2), seg(2, 2)],
        "id past the vocabulary": [seg(), seg(2, 2, [1, cfg.vocab])],
        "negative id": [seg(ids=[-1, 2])],
        "penalty 0": [seg(), dict(seg(2, 2), penalty=0.0)],
        "top_p 0": [seg(top_p=0.0)],
        "negative temperature": [seg(temperature=-1.0)],
        "negative top_k": [seg(top_k=-1)],
        "min_p above 1": [seg(min_p=1.5)],
        "min_p NaN": [seg(min_p=float("nan"))],
        "window 256": [seg(penalty_last_n=256)],
        "negative window": [seg(penalty_last_n=-1)],
    }
    toks, logits = [], []

    def step(k):
        st.synchronize()
        logits.append(eng.read_logits(0, st))
        toks.append(int(eng.hist[0, len(live.prompt) + k]))

    step(0)
    for k, (name, segs) in enumerate(cases.items(), start=1):
        before = [eng.row_state(r) for r in range(4)]
        with pytest.raises(_lib.MxError) as e:
            eng.prefill_batch(segs, st)
        assert e.value.rc == _lib.MX_ERR_ARG, name
        assert [eng.row_state(r) for r in range(4)] == before, name
        if k % 3 == 0:            # the live stream decodes on (every third case: 7 steps)
            eng.decode(1, st)
            step(len(toks))
    # the sampling refusals carry mx_llm_prefill_ex's messages
    for kw in (dict(penalty=0.0), dict(top_k=-1)):
        with pytest.raises(_lib.MxError) as one:
            eng.prefill(1, 1, ok, **{"penalty": 1.1, **kw}, stream=st)
        with pytest.raises(_lib.MxError) as pack:
            eng.prefill_batch([dict(seg(), **kw)], st)
        assert str(one.value) == str(pack.value)
    eng.decode(1, st)
    step(len(toks))
    P.check_stream(live, toks, logits, P.raw_logits(ref, [live], [toks])[0], "live stream")
    assert eng.row_state(0) == (True, len(live.prompt) + len(toks) - 1)
    eng.close()


def test_refused_before_finalize():
    lib = _lib.load()
    cfg = _cfg()
    c = _lib.LlmConfig(hidden=cfg.hidden, layers=1, heads=cfg.heads, kv_heads=cfg.kv_heads,
                       head_dim=cfg.head_dim, ffn=cfg.ffn, vocab=cfg.vocab, max_slots=1,
                       max_pos=128, max_batch=1, max_prefill=16, eps=cfg.eps, tied=1, wdtype=0)
    h = ctypes.c_void_p()
    assert lib.mx_llm_create(0, ctypes.byref(c), ctypes.byref(h)) == 0
    ids = (ctypes.c_int32 * 3)(1, 2, 3)
    seg = _lib.PrefillSeg(slot=0, row=0, ids_host=ctypes.addressof(ids), n_ids=3,
                          params=_lib.Sampling(0.0, 1.0, 1.1, 0), ext=_lib.SamplingExt(0, 0.0, 0))
    assert lib.mx_llm_prefill_batch(h, ctypes.byref(seg), 1, None) == _lib.MX_ERR_STATE
    lib.mx_llm_destroy(h)


# ---- 9. reuse ------------------------------------------------------------------------------
def test_pack_onto_used_slots_starts_clean():
    """Every prefill resets the slot's penalty state: slots that held windowed streams (their
    seen bytes are counts, their rings hold ids) take whole-sequence and windowed streams of a
    pack with no residue."""
    cfg, w, ref = _model()
    first = [Seg(p, 1.3, last_n=4) for p in P.disjoint_prompts(cfg.vocab, (9, 14), 412)]
    rows, slots = (0, 1), (1, 0)
    eng, st = P.engine(cfg, w, 2, 64), P.stream()
    left = P.run_pack(eng, st, first, rows, slots, 3)
    for r in rows:
        eng.release_row(r, st)
    assert [eng.row_state(r) for r in rows] == [(False, 0), (False, 0)]
    second = [Seg(p, 1.3, last_n=n) for p, n in zip(P.disjoint_prompts(cfg.vocab, (6, 11), 415),
                                                    (0, 3))]
    out = P.run_pack(eng, st, second, rows, slots, 4)
    P.check_pack(eng, ref, second, rows, slots, out, "reuse")
    # the check above cannot pass with the first streams' window counts left in place: penalising
    # the ids they held at release moves a first logit of the new stream far past the tolerance
    for i, s in enumerate(second):
        stale = (list(first[i].prompt) + left[i][0])[-4:]
        lg = out[i][1][0]
        assert max(abs(float(lg[t])) for t in stale) * (1 - 1 / 1.3) > 10 * P.LOGIT_TOL
    eng.close()
