"""Helpers of the packed-prefill GPU tests (TEST INFRASTRUCTURE).

A pack is a list of ``Seg`` with explicit decode rows and KV slots.  ``run_pack`` admits it
through ``LlmEngine.prefill_batch`` and steps the rows together; ``check_stream`` compares one
stream with the oracle: LlamaRef teacher-forced with the GPU's tokens (raw logits), the
(windowed) penalty rule of ``_sampler_chain.penalise``, -inf outside the grammar's allowed set.
Logits within atol = rtol = 5e-3; greedy tokens through ``check_tokens`` (margin 1e-2); sampled
tokens against the restatement's draw from the GPU's own logits at RNG counter n0 - 1 + k, a
mismatch accepted only as a near-tie (race or filter margin below 1e-5).
"""
from collections import namedtuple

import numpy as np
import torch

from oracle import llama_ref as L

import _sampler_chain as SC
from _parity import check_tokens

LOGIT_TOL = 5e-3
NEAR_TIE = 1e-5

Seg = namedtuple("Seg", "prompt penalty temperature top_p seed top_k min_p last_n grammar",
                 defaults=(1.1, 0.0, 1.0, 0, 0, 0.0, 0, False))


def ref_of(cfg, w, max_pos=256):
    rc = L.RefConfig(hidden=cfg.hidden, layers=cfg.layers, heads=cfg.heads,
                     kv_heads=cfg.kv_heads, head_dim=cfg.head_dim, ffn=cfg.ffn, vocab=cfg.vocab,
                     eps=cfg.eps, rope_theta=cfg.rope_theta, rope_scaling=cfg.rope_scaling,
                     tied=cfg.tied)
    return L.LlamaRef(rc, w, max_pos=max_pos)


def engine(cfg, w, B, max_prefill, max_pos=256, wdtype="bf16", grammar=None, options=None):
    from project_morpheus_amd.engine import LlmEngine
    eng = LlmEngine(cfg, w, device=0, max_slots=B, max_pos=max_pos, max_batch=B,
                    max_prefill=max_prefill, wdtype=wdtype)
    for k, v in (options or {}).items():
        eng.set_option(k, v)
    eng.enable_logits()
    if grammar is not None:
        eng.set_grammar(grammar)
    return eng


def segment(s, slot, row):
    return dict(slot=slot, row=row, ids=s.prompt, penalty=s.penalty, temperature=s.temperature,
                top_p=s.top_p, seed=s.seed, top_k=s.top_k, min_p=s.min_p,
                penalty_last_n=s.last_n, grammar=s.grammar)


def read_step(eng, st, segs, rows, slots, k, out):
    for i, s in enumerate(segs):
        out[i][1].append(eng.read_logits(rows[i], st))
        out[i][0].append(int(eng.hist[slots[i], len(s.prompt) + k]))


def run_pack(eng, st, segs, rows, slots, steps):
    """One ``prefill_batch`` of ``segs`` onto (rows, slots), then ``steps`` decode steps over the
    rows -> per segment (tokens, logits), first token included (steps + 1 entries)."""
    out = [([], []) for _ in segs]
    eng.prefill_batch([segment(s, slots[i], rows[i]) for i, s in enumerate(segs)], st)
    st.synchronize()
    read_step(eng, st, segs, rows, slots, 0, out)
    for k in range(1, steps + 1):
        eng.decode(max(rows) + 1, st)
        st.synchronize()
        read_step(eng, st, segs, rows, slots, k, out)
    return out


def raw_logits(ref, segs, toks):
    """The oracle's unpenalised logits [segment][step], every stream on its own slot and
    teacher-forced with the GPU's tokens (one forward per step for all streams)."""
    tr = L.teacher_forced_rows(ref, [list(s.prompt) for s in segs], toks, 1.0)
    return [[x.numpy() for x in row] for row in tr]


def mask(lg, g, phase):
    ids, stop = g.allowed(phase)
    out = np.full_like(np.asarray(lg, dtype=np.float32), -np.inf)
    out[ids.start:ids.stop] = lg[ids.start:ids.stop]
    if stop is not None:
        out[stop] = lg[stop]
    return out


def want_logits(s, toks, raw, g=None):
    seq, n0 = list(s.prompt) + list(toks), len(s.prompt)
    pen = [SC.penalise(raw[k], seq, n0 + k, s.penalty, s.last_n) for k in range(len(toks))]
    if s.grammar:
        pen = [mask(p, g, k % g.phases) for k, p in enumerate(pen)]
    return pen


def check_stream(s, toks, logits, raw, what, g=None):
    """-> near-ties accepted among the sampled steps."""
    want = want_logits(s, toks, raw, g)
    n0, ties = len(s.prompt), 0
    for k in range(len(toks)):
        ok = np.isfinite(want[k])
        assert np.all(np.isneginf(logits[k][~ok])), f"{what} step {k}: not -inf outside A(k)"
        err = float(np.max(np.abs(logits[k][ok] - want[k][ok])))
        print(f"{what} step {k}: max |logit error| {err:.3e}")
        np.testing.assert_allclose(logits[k][ok], want[k][ok], atol=LOGIT_TOL, rtol=LOGIT_TOL,
                                   err_msg=f"{what} step {k}")
        if s.grammar:
            assert g.allows(k % g.phases, toks[k]), f"{what} step {k}: {toks[k]} not allowed"
        if s.temperature > 0:
            tok, (race, fm) = SC.sample(logits[k], s.temperature, s.top_p, s.seed, n0 - 1 + k,
                                        s.top_k, s.min_p, return_margin=True)
            if toks[k] != tok:
                assert min(race, fm) < NEAR_TIE, \
                    f"{what} step {k}: {toks[k]} vs {tok} (race {race:.2e}, filter {fm:.2e})"
                ties += 1
        else:
            assert toks[k] == int(np.argmax(logits[k])), f"{what} step {k}"
    if s.temperature <= 0:
        check_tokens(toks, want, margin=1e-2, what=what)
    return ties


def check_pack(eng, ref, segs, rows, slots, out, what, g=None):
    """Every stream of a pack against the oracle, plus the host views: the history holds the
    tokens read step by step, and every row is live at prompt length + tokens."""
    toks = [o[0] for o in out]
    raw = raw_logits(ref, segs, toks)
    ties = 0
    for i, s in enumerate(segs):
        ties += check_stream(s, toks[i], out[i][1], raw[i], f"{what} segment {i}", g)
        n0, n = len(s.prompt), len(toks[i])
        assert [int(t) for t in eng.hist[slots[i], n0:n0 + n]] == toks[i]
        assert eng.row_state(rows[i]) == (True, n0 + n - 1)   # the last token's position
    return ties


def disjoint_prompts(vocab, lengths, seed):
    """Prompts of the given lengths over disjoint id sets (ids may repeat inside a prompt)."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(vocab)
    out, at = [], 0
    for n in lengths:
        pool = perm[at:at + max(1, min(n, vocab // len(lengths)))]
        at += len(pool)
        out.append([int(x) for x in rng.choice(pool, n)])
    return out


def stream():
    return torch.cuda.Stream()
