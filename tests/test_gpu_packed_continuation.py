"""Packed continuation (mx_llm_prefill_pack through LlmEngine.prefill_batch with ``pos0``, and
mx_llm_fork_slots through LlmEngine.fork_slots) against the oracles.

A pack of final chunks puts each entry's ids behind the positions its slot already holds (a
forked template) and runs the layers once over all entries' rows.  The oracle is always LlamaRef
on the WHOLE prompt (prefix + suffix) in one plain pass, teacher-forced with the GPU's tokens;
the checker is tests/_packed.py unchanged (logits atol = rtol = 5e-3, greedy tokens tie-aware
with margin 1e-2, sampled tokens against the restatement's draw from the GPU's own logits,
near-tie 1e-5).  A ``Seg`` here carries the whole prompt; ``pos0`` says where its suffix starts.

Shapes: the narrow model of the packed-prefill tests (hidden 512, 2 layers, 4/2 heads, ffn 1024,
vocab 1000, parity weights std 0.05), max_pos 512, unless a test says otherwise.
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

GRAMMAR = C.CodeGrammar(256, 64, 7, 1, 200)
MAX_POS = 512


def _cfg(**kw):
    return C.OrpheusConfig(**{**dict(hidden=512, layers=2, heads=4, kv_heads=2, ffn=1024,
                                     vocab=1000), **kw})


@functools.lru_cache(maxsize=None)
def _model(seed=401):
    cfg = _cfg()
    w = synthetic_llm_weights(cfg, seed=seed, std=0.05, norm_jitter=0.5)
    return cfg, w, P.ref_of(cfg, w, max_pos=MAX_POS)


def _ids(rng, n, vocab=1000):
    return [int(x) for x in rng.integers(0, vocab, n)]


def _template(eng, st, slot, ids):
    """A template slot: the ids as non-final chunks of at most max_prefill."""
    for off in range(0, len(ids), eng.max_prefill):
        eng.prefill_chunk(slot, ids[off:off + eng.max_prefill], off, st)


def _segments(segs, pos0, rows, slots):
    return [dict(P.segment(s, slots[i], rows[i]), ids=s.prompt[pos0[i]:], pos0=pos0[i])
            for i, s in enumerate(segs)]


def _steps(eng, st, segs, rows, slots, steps, out=None):
    """The first tokens (already committed), then ``steps`` decode steps over the rows."""
    out = out if out is not None else [([], []) for _ in segs]
    st.synchronize()
    P.read_step(eng, st, segs, rows, slots, 0, out)
    for k in range(1, steps + 1):
        eng.decode(max(rows) + 1, st)
        st.synchronize()
        P.read_step(eng, st, segs, rows, slots, k, out)
    return out


def _run(eng, st, segs, pos0, rows, slots, steps):
    eng.prefill_batch(_segments(segs, pos0, rows, slots), st)
    return _steps(eng, st, segs, rows, slots, steps)


# ---- 1. pack behind one forked prefix ------------------------------------------------------
def test_pack_behind_one_forked_prefix():
    """R = 32 rows behind 100 positions each; segment 2 has a single id.  Prefix and suffixes
    over disjoint id sets, different penalties: without the history marks a prefix id's logit
    is off by far more than the tolerance."""
    cfg, w, ref = _model()
    pre, *suf = P.disjoint_prompts(cfg.vocab, (100, 5, 9, 1, 17), 502)
    segs = [Seg(pre + s, pen) for s, pen in zip(suf, (1.3, 1.1, 1.0, 1.2))]
    rows, slots = (2, 0, 3, 1), (3, 1, 0, 2)
    eng, st = P.engine(cfg, w, 5, 64, max_pos=MAX_POS), P.stream()
    _template(eng, st, 4, pre)
    assert eng.slot_len(4) == 100
    eng.fork_slots([(s, 4, 100) for s in slots], st)
    assert [eng.slot_len(s) for s in range(5)] == [100] * 5
    out = _run(eng, st, segs, [100] * 4, rows, slots, 8)
    P.check_pack(eng, ref, segs, rows, slots, out, "forked prefix")
    assert [eng.slot_len(s) for s in slots] == [len(s.prompt) for s in segs]
    raw = P.raw_logits(ref, segs[:1], [out[0][0][:1]])[0][0]
    n0 = len(segs[0].prompt)
    whole = SC.penalise(raw, segs[0].prompt, n0, segs[0].penalty, 0)
    only_suffix = SC.penalise(raw, suf[0], len(suf[0]), segs[0].penalty, 0)
    assert np.abs(whole - only_suffix).max() > 10 * P.LOGIT_TOL
    eng.close()


# ---- 2. mixed pos0 and split counts in one launch ------------------------------------------
@pytest.mark.parametrize("options", [None, {"att_nw_batch": 4, "att_cpw_batch": 1}],
                         ids=["default", "splits128"])
def test_mixed_pos0_and_split_counts(options):
    """pos0 0 / 100 / 230 with 9 / 20 / 30 ids: contexts of 9, 120 and 260 positions in one
    launch; with 128-position splits the rows take 1, 1 and 2-3 splits."""
    cfg, w, ref = _model()
    rng = np.random.default_rng(503)
    t1, t2 = _ids(rng, 100), _ids(rng, 230)
    segs = [Seg(_ids(rng, 9), 1.2), Seg(t1 + _ids(rng, 20), 1.1), Seg(t2 + _ids(rng, 30), 1.3)]
    rows, slots = (1, 2, 0), (2, 0, 1)
    eng, st = P.engine(cfg, w, 5, 64, max_pos=MAX_POS, options=options), P.stream()
    _template(eng, st, 3, t1)
    _template(eng, st, 4, t2)
    eng.fork_slots([(0, 3, 100), (1, 4, 230)], st)
    out = _run(eng, st, segs, [0, 100, 230], rows, slots, 6)
    P.check_pack(eng, ref, segs, rows, slots, out, "mixed pos0")
    eng.close()


# ---- 3. window across the seam -------------------------------------------------------------
def test_window_across_the_seam():
    """penalty_last_n = 4 behind 100 positions: 2 history + 2 suffix positions (a), 3 + 1 (b),
    the window inside the suffix (c), next to a whole-sequence segment (d)."""
    cfg, w, ref = _model()
    rng = np.random.default_rng(504)
    far = 17                                     # in the history only, far outside every window
    pool = [i for i in range(cfg.vocab) if i != far]
    pre = [far, far] + [int(x) for x in rng.choice(pool, 98)]
    suf = [[int(x) for x in rng.choice(pool, n)] for n in (2, 1, 6, 7)]
    segs = [Seg(pre + suf[0], 1.3, last_n=4), Seg(pre + suf[1], 1.3, last_n=4),
            Seg(pre + suf[2], 1.3, last_n=4), Seg(pre + suf[3], 1.3)]
    rows, slots = (3, 1, 0, 2), (0, 1, 2, 3)
    eng, st = P.engine(cfg, w, 5, 64, max_pos=MAX_POS), P.stream()
    _template(eng, st, 4, pre)
    eng.fork_slots([(s, 4, 100) for s in slots], st)
    out = _run(eng, st, segs, [100] * 4, rows, slots, 6)
    P.check_pack(eng, ref, segs, rows, slots, out, "seam window")
    # id 17 lies in the history outside the window: not penalised at the first token
    a = segs[0]
    raw = P.raw_logits(ref, [a], [out[0][0][:1]])[0][0]
    whole = SC.penalise(raw, a.prompt, len(a.prompt), a.penalty, 0)
    assert abs(whole[far] - raw[far]) > 4 * P.LOGIT_TOL
    assert out[0][1][0][far] == pytest.approx(raw[far], abs=P.LOGIT_TOL + P.LOGIT_TOL * abs(raw[far]))
    # ... and it is, for the whole-sequence segment of the same pack
    d = segs[3]
    raw_d = P.raw_logits(ref, [d], [out[3][0][:1]])[0][0]
    want_d = SC.penalise(raw_d, d.prompt, len(d.prompt), d.penalty, 0)[far]
    assert out[3][1][0][far] == pytest.approx(want_d, abs=P.LOGIT_TOL + P.LOGIT_TOL * abs(want_d))
    eng.close()


# ---- 4. sampled and chain rows behind a prefix ---------------------------------------------
def _vetted(ref, s, steps, margin=1e-3):
    """The reference alone: every race and filter margin of the scripted steps >= margin."""
    seq, n0 = list(s.prompt), len(s.prompt)
    ref.free(0)
    lg = ref.forward(seq, [0] * n0, list(range(n0)), last_only=True)[-1].numpy()
    for k in range(steps):
        pen = SC.penalise(lg, seq, n0 + k, s.penalty, s.last_n)
        tok, (race, fm) = SC.sample(pen, s.temperature, s.top_p, s.seed, n0 - 1 + k, s.top_k,
                                    s.min_p, return_margin=True)
        if min(race, fm) < margin:
            return False
        seq.append(int(tok))
        lg = ref.forward([int(tok)], [0], [n0 + k])[0].numpy()
    return True


def test_sampled_and_chain_rows_behind_a_prefix():
    cfg, w, ref = _model()
    rng = np.random.default_rng(505)
    pre = _ids(rng, 100)
    suf = [_ids(rng, 11), _ids(rng, 8)]
    steps = 5                                    # 2 rows x 6 tokens = 12 sampled tokens
    segs = []
    for i, kw in enumerate((dict(temperature=0.6, top_p=0.9),
                            dict(temperature=0.6, top_p=1.0, top_k=5, min_p=0.05))):
        for seed in range(7000 + 100 * i, 7000 + 100 * i + 40):
            s = Seg(pre + suf[i], 1.1, seed=seed, **kw)
            if _vetted(ref, s, steps + 1):
                break
        else:
            pytest.fail("no seed with clear margins among 40")
        segs.append(s)
    rows, slots = (1, 0), (0, 1)
    eng, st = P.engine(cfg, w, 3, 64, max_pos=MAX_POS), P.stream()
    _template(eng, st, 2, pre)
    eng.fork_slots([(0, 2, 100), (1, 2, 100)], st)
    out = _run(eng, st, segs, [100, 100], rows, slots, steps)
    ties = P.check_pack(eng, ref, segs, rows, slots, out, "sampled")
    assert ties <= 1
    eng.close()


# ---- 5. grammar ----------------------------------------------------------------------------
@pytest.mark.parametrize("free_one", [False, True], ids=["all_constrained", "one_free"])
def test_grammar(free_one):
    cfg, w, ref = _model()
    rng = np.random.default_rng(506)
    pre = _ids(rng, 100)
    segs = [Seg(pre + _ids(rng, 7), 1.3, grammar=True),
            Seg(pre + _ids(rng, 12), 1.1, 0.6, 0.9, 99, grammar=not free_one),
            Seg(_ids(rng, 4), 1.1, grammar=True)]
    pos0 = [100, 100, 0]
    rows, slots = (2, 0, 1), (0, 1, 2)
    eng, st = P.engine(cfg, w, 4, 64, max_pos=MAX_POS, grammar=GRAMMAR), P.stream()
    _template(eng, st, 3, pre)
    eng.fork_slots([(0, 3, 100), (1, 3, 100)], st)
    heads0 = eng.grammar_window()[2]
    eng.prefill_batch(_segments(segs, pos0, rows, slots), st)
    # one lm_head launch over the row window for the whole call, or none when a row is free
    assert eng.grammar_window()[2] - heads0 == (0 if free_one else 1)
    out = _steps(eng, st, segs, rows, slots, 3)
    for i, s in enumerate(segs):
        first, lg = out[i][0][0], out[i][1][0]
        if s.grammar:                            # the origin is pos0 + n: phase 0 at the first token
            assert GRAMMAR.allows(0, first)
            assert np.isneginf(lg).sum() == cfg.vocab - 64
        else:
            assert np.all(np.isfinite(lg))
    P.check_pack(eng, ref, segs, rows, slots, out, "grammar", GRAMMAR)
    eng.close()


# ---- 6. e4m3 weights -----------------------------------------------------------------------
def test_fp8_pack_behind_a_prefix():
    cfg = C.OrpheusConfig(hidden=1024, layers=2, heads=8, kv_heads=2, ffn=2048, vocab=1000)
    qw = quantize_fp8(synthetic_llm_weights(cfg, seed=406, std=0.05, norm_jitter=0.5), cfg)
    ref = P.ref_of(cfg, dequantize_fp8(qw), max_pos=MAX_POS)
    rng = np.random.default_rng(507)
    pre = _ids(rng, 70)
    segs = [Seg(pre + _ids(rng, n), 1.1) for n in (18, 33)]
    rows, slots = (1, 0), (0, 1)
    eng, st = P.engine(cfg, qw, 3, 64, max_pos=MAX_POS, wdtype="fp8"), P.stream()
    _template(eng, st, 2, pre)
    eng.fork_slots([(0, 2, 70), (1, 2, 70)], st)
    out = _run(eng, st, segs, [70, 70], rows, slots, 6)
    P.check_pack(eng, ref, segs, rows, slots, out, "fp8")
    eng.close()


# ---- 7. Orpheus width ----------------------------------------------------------------------
def test_orpheus_width_pack_behind_a_prefix():
    """The true-width row classes at R = 73 behind 280 positions (hidden 3072, 24/8 heads)."""
    cfg = C.OrpheusConfig(layers=2, vocab=16384)
    w = synthetic_llm_weights(cfg, seed=408)
    ref = P.ref_of(cfg, w, max_pos=1024)
    rng = np.random.default_rng(508)
    pre = _ids(rng, 280, cfg.vocab)
    segs = [Seg(pre + _ids(rng, n, cfg.vocab), 1.1) for n in (24, 40, 9)]
    rows, slots = (2, 0, 1), (1, 2, 0)
    eng, st = P.engine(cfg, w, 4, 128, max_pos=1024), P.stream()
    _template(eng, st, 3, pre)
    eng.fork_slots([(s, 3, 280) for s in slots], st)
    out = _run(eng, st, segs, [280] * 3, rows, slots, 4)
    P.check_pack(eng, ref, segs, rows, slots, out, "orpheus width")
    eng.close()


# ---- 8. degenerate packs -------------------------------------------------------------------
def test_one_entry_pack_equals_final_chunk():
    cfg, w, ref = _model()
    rng = np.random.default_rng(509)
    pre = _ids(rng, 100)
    s = Seg(pre + _ids(rng, 19), 1.2)
    st = P.stream()
    a = P.engine(cfg, w, 2, 64, max_pos=MAX_POS)
    _template(a, st, 1, pre)
    got = _run(a, st, [s], [100], (1,), (1,), 4)[0]
    a.close()
    b = P.engine(cfg, w, 2, 64, max_pos=MAX_POS)
    _template(b, st, 1, pre)
    b.prefill_chunk(1, s.prompt[100:], 100, st, last=True, row=1, penalty=s.penalty)
    want = _steps(b, st, [s], (1,), (1,), 4)[0]
    b.close()
    for k in range(5):
        np.testing.assert_allclose(got[1][k], want[1][k], atol=P.LOGIT_TOL, rtol=P.LOGIT_TOL)
        if got[0][k] != want[0][k]:   # a near-tie may resolve differently; then the runs part
            assert abs(want[1][k][got[0][k]] - want[1][k][want[0][k]]) < 1e-2
            break
    P.check_stream(s, got[0], got[1], P.raw_logits(ref, [s], [got[0]])[0], "one entry")


def _chunks(entries):
    """ctypes array of mx_prefill_chunk from dicts (slot, row, ids, pos0, last, penalty, ...)."""
    arr = (_lib.PrefillChunk * max(1, len(entries)))()
    keep = []
    for a, e in zip(arr, entries):
        ids = np.ascontiguousarray(np.asarray(e["ids"], dtype=np.int32))
        keep.append(ids)
        a.slot, a.row, a.ids_host, a.n_ids = e["slot"], e["row"], ids.ctypes.data, len(ids)
        a.pos0, a.last = e.get("pos0", 0), e.get("last", 1)
        a.params = _lib.Sampling(temperature=e.get("temperature", 0.0), top_p=e.get("top_p", 1.0),
                                 repetition_penalty=e.get("penalty", 1.1), seed=0)
        a.ext = _lib.SamplingExt(top_k=e.get("top_k", 0), min_p=e.get("min_p", 0.0),
                                 penalty_last_n=e.get("penalty_last_n", 0))
    return arr, keep


def _pack_rc(eng, st, entries):
    arr, keep = _chunks(entries)
    return eng.lib.mx_llm_prefill_pack(eng.h, arr, len(entries),
                                       ctypes.c_void_p(st.cuda_stream))


def test_pack_of_whole_prompts_through_the_entry_point():
    """Every pos0 = 0: mx_llm_prefill_pack itself (LlmEngine.prefill_batch would take
    mx_llm_prefill_batch) against the oracle."""
    cfg, w, ref = _model()
    rng = np.random.default_rng(510)
    segs = [Seg(_ids(rng, n), pen) for n, pen in ((13, 1.3), (1, 1.1), (30, 1.2))]
    rows, slots = (2, 0, 1), (0, 2, 1)
    eng, st = P.engine(cfg, w, 3, 64, max_pos=MAX_POS), P.stream()
    rc = _pack_rc(eng, st, [dict(slot=slots[i], row=rows[i], ids=s.prompt, penalty=s.penalty)
                            for i, s in enumerate(segs)])
    assert rc == 0
    out = _steps(eng, st, segs, rows, slots, 4)
    P.check_pack(eng, ref, segs, rows, slots, out, "whole prompts")
    eng.close()


def test_one_id_pack_behind_a_prefix():
    """R = 1: the one-row kernels, as a one-id final chunk."""
    cfg, w, ref = _model()
    rng = np.random.default_rng(511)
    s = Seg(_ids(rng, 101), 1.3)
    eng, st = P.engine(cfg, w, 2, 64, max_pos=MAX_POS), P.stream()
    _template(eng, st, 1, s.prompt[:100])
    eng.fork_slots([(0, 1, 100)], st)
    out = _run(eng, st, [s], [100], (0,), (0,), 4)
    P.check_pack(eng, ref, [s], (0,), (0,), out, "one id")
    eng.close()


# ---- 9. refusals ---------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was():
    cfg, w, ref = _model()
    rng = np.random.default_rng(512)
    live = Seg(_ids(rng, 9), 1.2)
    eng, st = P.engine(cfg, w, 4, 128, max_pos=128), P.stream()
    eng.prefill(0, 0, live.prompt, live.penalty, st)
    _template(eng, st, 3, _ids(rng, 40))
    eng.fork_slots([(1, 3, 40), (2, 3, 40)], st)
    ok = [3, 4, 5]
    ARG, STATE = _lib.MX_ERR_ARG, _lib.MX_ERR_STATE

    def e(slot=1, row=1, ids=ok, pos0=40, **kw):
        return dict(slot=slot, row=row, ids=ids, pos0=pos0, **kw)

    cases = {
        "last = 0": (ARG, [e(), e(2, 2, last=0)]),
        "pos0 is not the slot's length": (STATE, [e(pos0=39)]),
        "pos0 past the slot's length": (STATE, [e(), e(2, 2, pos0=41)]),
        "slot bound to an active row": (STATE, [e(0, 1, pos0=9)]),
        "negative pos0": (ARG, [e(pos0=-1)]),
        "pos0 + n reaches max_pos": (ARG, [e(ids=[1] * 88)]),
        "rows past max_prefill": (ARG, [e(ids=[1] * 70), e(2, 2, ids=[2] * 70)]),
        "slot twice": (ARG, [e(1, 1), e(1, 2)]),
        "row twice": (ARG, [e(1, 2), e(2, 2)]),
        "id past the vocabulary": (ARG, [e(), e(2, 2, [1, cfg.vocab])]),
        "penalty 0": (ARG, [e(), e(2, 2, penalty=0.0)]),
        "window 256": (ARG, [e(penalty_last_n=256)]),
        "no entries": (ARG, []),
    }
    toks, logits = [], []

    def step(k):
        st.synchronize()
        logits.append(eng.read_logits(0, st))
        toks.append(int(eng.hist[0, len(live.prompt) + k]))

    step(0)
    for k, (name, (code, entries)) in enumerate(cases.items(), start=1):
        rows_before = [eng.row_state(r) for r in range(4)]
        lens_before = [eng.slot_len(s) for s in range(4)]
        assert _pack_rc(eng, st, entries) == code, name
        assert [eng.row_state(r) for r in range(4)] == rows_before, name
        assert [eng.slot_len(s) for s in range(4)] == lens_before, name
        if k % 3 == 0:
            eng.decode(1, st)
            step(len(toks))
    # through the Python surface too, with the error code on the exception
    with pytest.raises(_lib.MxError) as err:
        eng.prefill_batch([dict(slot=1, row=1, ids=ok, penalty=1.1, pos0=39)], st)
    assert err.value.rc == STATE
    eng.decode(1, st)
    step(len(toks))
    P.check_stream(live, toks, logits, P.raw_logits(ref, [live], [toks])[0], "live stream")
    assert eng.row_state(0) == (True, len(live.prompt) + len(toks) - 1)
    eng.close()


# ---- 10. fork_slots ------------------------------------------------------------------------
def test_fork_slots_equals_fork_slot():
    """Two sources, n_pos 33 / 100 / 64: 2, 4 and 2 chunks, an odd number of units.  A one-id
    final chunk behind each fork is bit-identical to the same chunk behind one fork_slot on a
    second engine (whose templates are bit-equal because they too are filled by one-row
    launches: a multi-row chunk sums its residuals in no fixed order)."""
    cfg, w, _ = _model()
    rng = np.random.default_rng(513)
    t0, t1, nxt = _ids(rng, 100), _ids(rng, 70), _ids(rng, 3)
    triples = [(2, 0, 33), (3, 0, 100), (4, 1, 64)]
    st = P.stream()
    got, want = [], []
    for many, res in ((True, got), (False, want)):
        eng = P.engine(cfg, w, 5, 64, max_pos=MAX_POS)
        for slot, ids in ((0, t0), (1, t1)):     # id by id: one-row kernels only, no unordered
            for i, t in enumerate(ids):          # reduction, so both engines hold the same bits
                eng.prefill_chunk(slot, [t], i, st)
        if many:
            eng.fork_slots(triples, st)
        else:
            for d, s, n in triples:
                eng.fork_slot(d, s, n, st)
        assert [eng.slot_len(d) for d, _, _ in triples] == [33, 100, 64]
        for i, (d, _, n) in enumerate(triples):
            eng.prefill_chunk(d, [nxt[i]], n, st, last=True, row=i, penalty=1.2)
            st.synchronize()
            res.append(eng.read_logits(i, st).copy())
        if many:
            lens = [eng.slot_len(s) for s in range(5)]
            eng.release_row(1, st)               # slot 3 is free again, slot 2 stays bound to row 0
            for name, bad in {"dst twice": [(3, 0, 10), (3, 1, 10)],
                              "dst is a src": [(3, 0, 10), (1, 3, 10)],
                              "n_pos above the source's length": [(3, 0, 10), (1, 0, 101)],
                              "dst bound to a row": [(3, 0, 10), (2, 0, 10)]}.items():
                with pytest.raises(_lib.MxError) as err:
                    eng.fork_slots(bad, st)
                assert err.value.rc == _lib.MX_ERR_STATE, name
                assert [eng.slot_len(s) for s in range(5)] == lens, name
            with pytest.raises(_lib.MxError) as err:
                eng.fork_slots([], st)
            assert err.value.rc == _lib.MX_ERR_ARG
        eng.close()
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


# ---- 11. reuse -----------------------------------------------------------------------------
def test_pack_behind_a_prefix_onto_used_slots_starts_clean():
    cfg, w, ref = _model()
    first = [Seg(p, 1.3, last_n=4) for p in P.disjoint_prompts(cfg.vocab, (9, 14), 514)]
    rows, slots = (0, 1), (1, 0)
    eng, st = P.engine(cfg, w, 3, 64, max_pos=MAX_POS), P.stream()
    left = P.run_pack(eng, st, first, rows, slots, 3)
    for r in rows:
        eng.release_row(r, st)
    pre, *suf = P.disjoint_prompts(cfg.vocab, (100, 6, 11), 515)
    second = [Seg(pre + s, 1.3, last_n=n) for s, n in zip(suf, (0, 3))]
    _template(eng, st, 2, pre)
    eng.fork_slots([(s, 2, 100) for s in slots], st)
    out = _run(eng, st, second, [100, 100], rows, slots, 4)
    P.check_pack(eng, ref, second, rows, slots, out, "reuse")
    # the check above cannot pass with the first streams' window counts left in place
    for i, s in enumerate(second):
        stale = (list(first[i].prompt) + left[i][0])[-4:]
        lg = out[i][1][0]
        assert max(abs(float(lg[t])) for t in stale) * (1 - 1 / 1.3) > 10 * P.LOGIT_TOL
    eng.close()
