"""Prompt continuation and KV fork (mx_llm_prefill_chunk / mx_llm_fork_slot / mx_llm_slot_len
through LlmEngine.prefill_chunk / fork_slot / slot_len) against the oracles.

A prompt given as chunks, or as a forked prefix plus chunks, must leave the stream where ONE
prefill of the concatenated ids would.  Every stream is compared, first token included, with
LlamaRef teacher-forced on the GPU's tokens over the CONCATENATED prompt (tests/_packed.py:
logits atol = rtol = 5e-3, greedy tokens tie-aware with margin 1e-2, sampled tokens against
the restatement's draw from the GPU's own logits at RNG counter n0 - 1 + k, n0 the whole
prompt), and followed by 6 decode steps.

Shapes: the narrow model of the packed-prefill tests (hidden 512, 2 layers, 4/2 heads, ffn
1024, vocab 1000, parity weights std 0.05) unless a test says otherwise.
"""
import functools

import numpy as np
import pytest

from oracle import llama_ref as L
from project_morpheus_amd import _lib
from project_morpheus_amd import config as C
from project_morpheus_amd.weights import dequantize_fp8, quantize_fp8, synthetic_llm_weights

import _dispatch as D
import _packed as P
import _sampler_chain as SC
from _packed import Seg

pytestmark = pytest.mark.gpu

STEPS = 6
GRAMMAR = C.CodeGrammar(1024, 256, 7, 1, 1000)    # test_gpu_code_grammar's: vocabulary 5,000


def _cfg(**kw):
    return C.OrpheusConfig(**{**dict(hidden=512, layers=2, heads=4, kv_heads=2, ffn=1024,
                                     vocab=1000), **kw})


@functools.lru_cache(maxsize=None)
def _model(vocab=1000, seed=501):
    cfg = _cfg(vocab=vocab)
    w = synthetic_llm_weights(cfg, seed=seed, std=0.05, norm_jitter=0.5)
    return cfg, w, P.ref_of(cfg, w)


@functools.lru_cache(maxsize=None)
def _fp8_model():
    cfg = C.OrpheusConfig(hidden=1024, layers=2, heads=8, kv_heads=2, ffn=2048, vocab=1000)
    qw = quantize_fp8(synthetic_llm_weights(cfg, seed=506, std=0.05, norm_jitter=0.5), cfg)
    return cfg, qw, P.ref_of(cfg, dequantize_fp8(qw))


def _engine(cfg, w, rows, slots, max_prefill, max_pos=256, wdtype="bf16", grammar=None):
    from project_morpheus_amd.engine import LlmEngine
    eng = LlmEngine(cfg, w, device=0, max_slots=slots, max_pos=max_pos, max_batch=rows,
                    max_prefill=max_prefill, wdtype=wdtype)
    eng.enable_logits()
    if grammar is not None:
        eng.set_grammar(grammar)
    return eng


def _ids(rng, vocab, n):
    return [int(x) for x in rng.integers(0, vocab, n)]


def _params(s):
    return dict(penalty=s.penalty, temperature=s.temperature, top_p=s.top_p, seed=s.seed,
                top_k=s.top_k, min_p=s.min_p, penalty_last_n=s.last_n, grammar=s.grammar)


def _chunks(eng, st, slot, ids, pos0, split, final=None, row=None):
    """``ids`` onto ``slot`` behind ``pos0`` positions in chunks of the lengths ``split``; the
    last one ends the prompt under the parameters of the Seg ``final`` (None: no final chunk)."""
    assert sum(split) == len(ids)
    at = 0
    for j, n in enumerate(split):
        last = final is not None and j == len(split) - 1
        kw = dict(last=True, row=row, **_params(final)) if last else {}
        eng.prefill_chunk(slot, ids[at:at + n], pos0 + at, st, **kw)
        at += n
        assert eng.slot_len(slot) == pos0 + at


def _steps(eng, st, segs, rows, slots, steps, n_rows, out=None):
    """Read the streams' current token, then ``steps`` decode steps over rows [0, n_rows) ->
    per stream (tokens, logits)."""
    out = out if out is not None else [([], []) for _ in segs]
    k0 = [len(o[0]) for o in out]
    for k in range(steps + 1):
        if k:
            eng.decode(n_rows, st)
        st.synchronize()
        for i, s in enumerate(segs):
            out[i][1].append(eng.read_logits(rows[i], st))
            out[i][0].append(int(eng.hist[slots[i], len(s.prompt) + k0[i] + k]))
    return out


def _check(ref, segs, out, what, shared_prefix=0, g=None):
    toks = [o[0] for o in out]
    tr = L.teacher_forced_rows(ref, [list(s.prompt) for s in segs], toks, 1.0,
                               shared_prefix=shared_prefix)
    ties = 0
    for i, s in enumerate(segs):
        raw = [x.numpy() for x in tr[i]]
        ties += P.check_stream(s, toks[i], out[i][1], raw, f"{what} stream {i}", g)
    return ties


# ---- 1. seams ------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [(70, 80), (64, 64, 22), (96, 53, 1), (1, 96, 53),
                                   (96, 96, 10)], ids=lambda s: "+".join(map(str, s)))
def test_seams(split):
    """max_prefill 96, max_pos 256.  70 + 80: a seam off the 32-position chunk grid; 64 + 64 +
    22: the last chunk crosses position 128; 96 + 53 + 1: a one-id final chunk on the one-row
    path (context 150: 2 splits of 96); 1 + 96 + 53: a one-id chunk in front (1 + 149 is
    refused: 149 > 96).  96 + 96 + 10 is the one split of this file where prompt rows take TWO
    attention splits: 10 rows x 2 kv heads = 20 pairs, context 202 -> 6 waves x 1 chunk, 192
    positions per split."""
    cfg, w, ref = _model()
    n = sum(split)
    s = Seg(_ids(np.random.default_rng(502), cfg.vocab, n), 1.2)
    eng, st = _engine(cfg, w, 1, 1, 96), P.stream()
    _chunks(eng, st, 0, s.prompt, 0, split, final=s, row=0)
    assert eng.row_state(0) == (True, n)
    out = _steps(eng, st, [s], (0,), (0,), STEPS, 1)
    _check(ref, [s], out, f"seam {split}")
    assert eng.row_state(0) == (True, n + STEPS) and eng.slot_len(0) == n
    eng.close()
    if split == (96, 96, 10):
        assert D.att_shape(D.SMALL, 10, 202, D.DEFAULTS) == (6, 1, 2)


# ---- 2. fork -------------------------------------------------------------------------------
def _fork_case(model, n_prefix, wdtype="bf16", what="fork"):
    cfg, w, ref = model
    rng = np.random.default_rng(503 + n_prefix)
    prefix = _ids(rng, cfg.vocab, n_prefix)
    segs = [Seg(prefix + _ids(rng, cfg.vocab, 9), 1.3), Seg(prefix + _ids(rng, cfg.vocab, 20), 1.1)]
    eng, st = _engine(cfg, w, 2, 4, 32, wdtype=wdtype), P.stream()
    _chunks(eng, st, 3, prefix, 0, (32, n_prefix - 32))     # non-final chunks: a template slot
    assert eng.row_state(0) == (False, 0) and eng.row_state(1) == (False, 0)
    for i, s in enumerate(segs):
        eng.fork_slot(i, 3, n_prefix, st)
        assert eng.slot_len(i) == n_prefix
        _chunks(eng, st, i, s.prompt[n_prefix:], n_prefix, (len(s.prompt) - n_prefix,),
                final=s, row=i)
    out = _steps(eng, st, segs, (0, 1), (0, 1), STEPS, 2)
    _check(ref, segs, out, what, shared_prefix=n_prefix)
    assert eng.slot_len(3) == n_prefix
    eng.close()


@pytest.mark.parametrize("n_prefix", [45, 64])
def test_fork(n_prefix):
    """A prefix (45: not a multiple of 32, the fork copies the tail of its second chunk; 64: whole
    chunks) prefilled once into slot 3, forked into slots 0 and 1, continued with suffixes of 9
    and 20 ids; the two rows step together."""
    _fork_case(_model(), n_prefix)


def test_fork_is_a_copy():
    """src and dst of a fork take the same one-id final chunk and 6 steps, one after the other
    on row 0: one-row kernels only (no unordered reduction), so the logits are bit-equal."""
    cfg, w, _ = _model()
    rng = np.random.default_rng(510)
    prefix, tail = _ids(rng, cfg.vocab, 45), _ids(rng, cfg.vocab, 1)
    s = Seg(prefix + tail, 1.2)
    eng, st = _engine(cfg, w, 1, 4, 32), P.stream()
    _chunks(eng, st, 3, prefix, 0, (32, 13))
    eng.fork_slot(0, 3, 45, st)
    runs = []
    for slot in (3, 0):
        _chunks(eng, st, slot, tail, 45, (1,), final=s, row=0)
        runs.append(_steps(eng, st, [s], (0,), (slot,), STEPS, 1)[0])
        eng.release_row(0, st)
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(a, b)
    eng.close()


def test_fork_from_a_live_source():
    """The source is a decoding stream (admitted by ``prefill``; n_pos = its prompt length); the
    copy continues with another suffix while the source keeps stepping in the same launches."""
    cfg, w, ref = _model()
    rng = np.random.default_rng(511)
    a = Seg(_ids(rng, cfg.vocab, 40), 1.2)
    b = Seg(a.prompt + _ids(rng, cfg.vocab, 12), 1.1)
    eng, st = _engine(cfg, w, 2, 2, 64), P.stream()
    eng.prefill(0, 0, a.prompt, a.penalty, st)
    assert eng.slot_len(0) == 40
    out_a = _steps(eng, st, [a], (0,), (0,), 2, 1)
    eng.fork_slot(1, 0, 40, st)
    _chunks(eng, st, 1, b.prompt[40:], 40, (12,), final=b, row=1)
    out_b = [([], [])]
    for k in range(STEPS + 1):
        if k:
            eng.decode(2, st)
        st.synchronize()
        out_b[0][1].append(eng.read_logits(1, st))
        out_b[0][0].append(int(eng.hist[1, 52 + k]))
        if k:
            out_a[0][1].append(eng.read_logits(0, st))
            out_a[0][0].append(int(eng.hist[0, 40 + 2 + k]))
    _check(ref, [a], out_a, "live source")
    _check(ref, [b], out_b, "copy of a live source")
    eng.close()


# ---- 3. penalty window across the seam -----------------------------------------------------
def test_penalty_window_across_the_seam():
    """penalty_last_n 16 over chunks 70 + 10: the window [64, 80) holds ids of both chunks; id
    777 occurs at position 5 only, outside it.  A greedy and a sampled row."""
    cfg, w, ref = _model()
    rng = np.random.default_rng(512)
    prompt = _ids(rng, 700, 80)
    prompt[5] = 777
    assert len(set(prompt[64:70])) > 1 and len(set(prompt[70:])) > 1
    segs = [Seg(prompt, 1.3, last_n=16), Seg(prompt, 1.3, 0.6, 0.9, 4242, 40, 0.0, 16)]
    eng, st = _engine(cfg, w, 2, 2, 96), P.stream()
    for i, s in enumerate(segs):
        _chunks(eng, st, i, prompt, 0, (70, 10), final=s, row=i)
    out = _steps(eng, st, segs, (0, 1), (0, 1), STEPS, 2)
    assert _check(ref, segs, out, "window") <= 1
    # the window really differs from the whole sequence at the first token
    raw = P.raw_logits(ref, segs[:1], [out[0][0][:1]])[0][0]
    whole = SC.penalise(raw, prompt, 80, 1.3, 0)
    assert abs(whole[777] - raw[777]) > 4 * P.LOGIT_TOL
    assert out[0][1][0][777] == pytest.approx(raw[777], abs=P.LOGIT_TOL * (1 + abs(raw[777])))
    # ... and the check above is sensitive to the ids of BOTH chunks inside it
    inside = SC.penalise(raw, prompt, 80, 1.3, 16)
    for ids in (prompt[64:70], prompt[70:]):
        assert max(abs(inside[t] - raw[t]) for t in ids) > 4 * P.LOGIT_TOL
    eng.close()


# ---- 4. grammar ----------------------------------------------------------------------------
def test_grammar_over_a_forked_prefix():
    """A constrained slot: the first token has phase 0 at position prefix + suffix, and the
    allowed-set rule holds for 8 tokens (check_stream: -inf outside A(k), token in A(k))."""
    cfg, w, ref = _model(5000, 311)
    rng = np.random.default_rng(513)
    prefix = _ids(rng, cfg.vocab, 45)
    s = Seg(prefix + _ids(rng, cfg.vocab, 9), 1.2, grammar=True)
    eng, st = _engine(cfg, w, 1, 2, 32, grammar=GRAMMAR), P.stream()
    _chunks(eng, st, 1, prefix, 0, (32, 13))
    eng.fork_slot(0, 1, 45, st)
    _chunks(eng, st, 0, s.prompt[45:], 45, (9,), final=s, row=0)
    out = _steps(eng, st, [s], (0,), (0,), 7, 1)
    assert GRAMMAR.allows(0, out[0][0][0]) and not GRAMMAR.allows(1, out[0][0][0])
    assert np.isneginf(out[0][1][0]).sum() == cfg.vocab - 256   # 255 codes + the stop id stay
    _check(ref, [s], out, "grammar", shared_prefix=0, g=GRAMMAR)
    eng.close()


# ---- 5. e4m3 weights -----------------------------------------------------------------------
def test_fp8_seam():
    cfg, qw, ref = _fp8_model()
    s = Seg(_ids(np.random.default_rng(514), cfg.vocab, 150), 1.2)
    eng, st = _engine(cfg, qw, 1, 1, 96, wdtype="fp8"), P.stream()
    _chunks(eng, st, 0, s.prompt, 0, (70, 80), final=s, row=0)
    out = _steps(eng, st, [s], (0,), (0,), STEPS, 1)
    _check(ref, [s], out, "fp8 seam")
    eng.close()


def test_fp8_fork():
    _fork_case(_fp8_model(), 45, wdtype="fp8", what="fp8 fork")


# ---- 6. Orpheus width ----------------------------------------------------------------------
def test_orpheus_width():
    """hidden 3072, 24/8 heads, ffn 8192, 2 layers, vocab 16,384, max_pos 1,024: a 300-id prefix
    in chunks of 128 (128 + 128 + 44), forked; one stream continues with 24 ids, a second with 1.
    Attention shapes (waves, chunks per wave, splits) reached, by tests/_dispatch.att_shape:
    the prefix chunks (8, 1, 1) at contexts 128 and 256 and (8, 2, 1) at 300; the 24-id suffix
    (8, 2, 1) with 24 rows over a context of 324 -- prompt rows over more positions than rows;
    the one-id suffix the one-row (3, 1, 4) over 301 positions right after the fork; the two
    decode rows (6, 1, 2)."""
    o = D.DEFAULTS
    d = D.Dims(3072, 24, 8, 8192, 16384)
    assert [D.att_shape(d, 128, 128, o), D.att_shape(d, 128, 256, o), D.att_shape(d, 44, 300, o),
            D.att_shape(d, 24, 324, o), D.att_shape(d, 1, 301, o), D.att_shape(d, 2, 326, o)] == \
        [(8, 1, 1), (8, 1, 1), (8, 2, 1), (8, 2, 1), (3, 1, 4), (6, 1, 2)]
    cfg = C.OrpheusConfig(layers=2, vocab=16384)
    w = synthetic_llm_weights(cfg, seed=508)
    ref = P.ref_of(cfg, w, max_pos=1024)
    rng = np.random.default_rng(509)
    prefix = _ids(rng, cfg.vocab, 300)
    segs = [Seg(prefix + _ids(rng, cfg.vocab, 24), 1.1), Seg(prefix + _ids(rng, cfg.vocab, 1), 1.1)]
    eng, st = _engine(cfg, w, 2, 3, 128, max_pos=1024), P.stream()
    _chunks(eng, st, 2, prefix, 0, (128, 128, 44))
    for i, s in enumerate(segs):
        eng.fork_slot(i, 2, 300, st)
        _chunks(eng, st, i, s.prompt[300:], 300, (len(s.prompt) - 300,), final=s, row=i)
    out = _steps(eng, st, segs, (0, 1), (0, 1), STEPS, 2)
    _check(ref, segs, out, "orpheus width", shared_prefix=300)
    eng.close()


# ---- 7. refusals ---------------------------------------------------------------------------
def _clean_run(eng, st, prompt):
    eng.prefill(1, 1, prompt, 1.2, st)
    toks = []
    for k in range(4):
        if k:
            eng.decode(2, st)
        st.synchronize()
        toks.append(int(eng.hist[1, len(prompt) + k]))
    eng.release_row(1, st)
    return toks


def test_refusals_leave_the_context_as_it_was():
    cfg, w, _ = _model()
    rng = np.random.default_rng(515)
    live, held, clean = _ids(rng, cfg.vocab, 9), _ids(rng, cfg.vocab, 20), _ids(rng, cfg.vocab, 11)
    eng, st = _engine(cfg, w, 2, 4, 32, max_pos=128), P.stream()
    eng.prefill(0, 0, live, 1.2, st)                 # slot 0 is bound to the active row 0
    eng.prefill_chunk(2, held, 0, st)                # slot 2 holds 20 positions, unbound
    ok = [3, 4, 5]
    ARG, STATE = _lib.MX_ERR_ARG, _lib.MX_ERR_STATE
    cases = {
        "pos0 behind the length": (STATE, lambda: eng.prefill_chunk(2, ok, 19, st)),
        "pos0 past the length": (STATE, lambda: eng.prefill_chunk(2, ok, 21, st)),
        "pos0 on an empty slot": (STATE, lambda: eng.prefill_chunk(3, ok, 4, st)),
        "pos0 + n = max_pos": (ARG, lambda: eng.prefill_chunk(2, [1] * 32, 96, st)),
        "n above max_prefill": (ARG, lambda: eng.prefill_chunk(2, [1] * 33, 20, st)),
        "no ids": (ARG, lambda: eng.prefill_chunk(2, [], 20, st)),
        "id past the vocabulary": (ARG, lambda: eng.prefill_chunk(2, [1, cfg.vocab], 20, st)),
        "chunk onto a bound slot": (STATE, lambda: eng.prefill_chunk(0, ok, 9, st)),
        "fork above the source's length": (STATE, lambda: eng.fork_slot(3, 2, 21, st)),
        "fork of nothing": (STATE, lambda: eng.fork_slot(3, 2, 0, st)),
        "fork from an empty slot": (STATE, lambda: eng.fork_slot(2, 3, 1, st)),
        "dst is src": (STATE, lambda: eng.fork_slot(2, 2, 10, st)),
        "dst bound to an active row": (STATE, lambda: eng.fork_slot(0, 2, 10, st)),
        "slot past the end": (STATE, lambda: eng.fork_slot(4, 2, 10, st)),
        "final chunk, penalty 0": (ARG, lambda: eng.prefill_chunk(2, ok, 20, st, last=True, row=1,
                                                                  penalty=0.0)),
        "final chunk, window 256": (ARG, lambda: eng.prefill_chunk(2, ok, 20, st, last=True, row=1,
                                                                   penalty_last_n=256)),
        "final chunk, row past the end": (ARG, lambda: eng.prefill_chunk(2, ok, 20, st, last=True,
                                                                         row=2)),
    }
    for name, (rc, call) in cases.items():
        before = ([eng.row_state(r) for r in range(2)], [eng.slot_len(s) for s in range(4)])
        with pytest.raises(_lib.MxError) as e:
            call()
        assert e.value.rc == rc, name
        assert ([eng.row_state(r) for r in range(2)], [eng.slot_len(s) for s in range(4)]) == before, name
    assert [eng.slot_len(s) for s in range(4)] == [9, 0, 20, 0]
    # nothing was enqueued: a clean stream now equals a fresh engine's, token for token (the
    # two-row steps run the same launches on both engines)
    got = _clean_run(eng, st, clean)
    eng.close()
    fresh = _engine(cfg, w, 2, 4, 32, max_pos=128)
    fresh.prefill(0, 0, live, 1.2, st)
    want = _clean_run(fresh, st, clean)
    fresh.close()
    assert got == want


# ---- 8. unchanged entry points -------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 40])
def test_first_final_chunk_is_prefill(n):
    """pos0 0, last 1 gives what mx_llm_prefill_ex gives: bit for bit for a one-id prompt (one-row
    kernels), within the tolerance for 40 ids."""
    cfg, w, ref = _model()
    s = Seg(_ids(np.random.default_rng(516), cfg.vocab, n), 1.2)
    st, runs = P.stream(), []
    for chunked in (True, False):
        eng = _engine(cfg, w, 1, 1, 64)
        if chunked:
            eng.prefill_chunk(0, s.prompt, 0, st, last=True, row=0, **_params(s))
        else:
            eng.prefill(0, 0, s.prompt, s.penalty, st)
        runs.append(_steps(eng, st, [s], (0,), (0,), STEPS, 1)[0])
        eng.close()
    for k in range(STEPS + 1):
        if n == 1:
            assert np.array_equal(runs[0][1][k], runs[1][1][k])
        else:
            np.testing.assert_allclose(runs[0][1][k], runs[1][1][k], atol=P.LOGIT_TOL, rtol=P.LOGIT_TOL)
    if n == 1:
        assert runs[0][0] == runs[1][0]
    _check(ref, [s], [runs[0]], f"first final chunk of {n}")


def test_prefill_onto_a_slot_used_by_chunks_starts_clean():
    cfg, w, ref = _model()
    rng = np.random.default_rng(517)
    eng, st = _engine(cfg, w, 1, 2, 64), P.stream()
    old = Seg(_ids(rng, cfg.vocab, 50), 1.3, last_n=8)
    _chunks(eng, st, 0, old.prompt, 0, (30, 20), final=old, row=0)
    _steps(eng, st, [old], (0,), (0,), 2, 1)
    eng.release_row(0, st)
    new = Seg(_ids(rng, cfg.vocab, 13), 1.3)
    eng.prefill(0, 0, new.prompt, new.penalty, st)
    assert eng.slot_len(0) == 13
    out = _steps(eng, st, [new], (0,), (0,), STEPS, 1)
    _check(ref, [new], out, "prefill after chunks")
    eng.close()
