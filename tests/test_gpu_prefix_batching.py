"""BatchSynthesizer with long prompts and the prefix cache: a prompt longer than max_prefill is
admitted in chunks between the live streams' steps, requests naming a registered prefix start
as forks of its template slot, the least recently used prefix is evicted, and a cancel in the
middle of a prompt frees the row and the slot.

The narrow model of tests/test_gpu_prompt_continuation.py (hidden 512, 2 layers, 4/2 heads, ffn
1024, vocab 1000, parity weights) with synthetic SNAC weights; token-only streams, greedy, each
compared with LlamaRef teacher-forced on the GPU's tokens over the WHOLE prompt (tie-aware,
margin 1e-2: tests/_parity.check_tokens).
"""
import functools

import numpy as np
import pytest

from oracle import llama_ref as L
from project_morpheus_amd import config as C
from project_morpheus_amd.weights import synthetic_llm_weights, synthetic_snac_weights

import _packed as P
from _parity import check_tokens

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _world():
    cfg = C.OrpheusConfig(hidden=512, layers=2, heads=4, kv_heads=2, ffn=1024, vocab=1000)
    w = synthetic_llm_weights(cfg, seed=521, std=0.05, norm_jitter=0.5)
    return cfg, w, synthetic_snac_weights(seed=8), P.ref_of(cfg, w, max_pos=512)


def _synth(rows, max_prefill, prefix_slots=0):
    from project_morpheus_amd.batching import BatchSynthesizer
    from project_morpheus_amd.engine import LlmEngine, SnacDecoder
    cfg, w, sw, _ = _world()
    llm = LlmEngine(cfg, w, max_slots=rows + prefix_slots, max_pos=512, max_batch=rows,
                    max_prefill=max_prefill)
    return llm, BatchSynthesizer(llm, SnacDecoder(sw, max_frames=7, max_batch=8), depth=2,
                                 prefix_slots=prefix_slots)


def _req(ids, n, **kw):
    from project_morpheus_amd.batching import StreamRequest
    return StreamRequest(prompt_ids=list(ids), max_tokens=n, arrival=0.0, audio=False,
                         stop_ids=(), **kw)


def _ids(rng, n):
    return [int(x) for x in rng.integers(0, 1000, n)]


def _matches_oracle(prompt, req, what, n=None):
    assert req.error is None, f"{what}: {req.error!r}"
    assert len(req.tokens) == (req.max_tokens if n is None else n), what
    ref = _world()[3]
    tr = L.teacher_forced_rows(ref, [list(prompt)], [req.tokens], 1.1)
    check_tokens(req.tokens, tr[0], margin=1e-2, what=what)


def test_long_prompt_under_load():
    """A 200-id prompt at max_prefill 64 (chunks 64 + 64 + 64 + 8) joins while two short streams
    decode: they keep stepping between its chunks, and speak as they do without it."""
    rng = np.random.default_rng(522)
    short, long_ = [_ids(rng, 10), _ids(rng, 14)], _ids(rng, 200)
    llm, syn = _synth(3, 64)
    reqs = [_req(short[0], 24), _req(short[1], 24), _req(long_, 8)]
    syn.run(reqs)
    assert syn.prompt_chunks == 4 and not syn.prefill_packs
    assert syn.row_steps[2] >= 2          # two-row steps while the third row was mid-prompt
    llm.close()
    llm, alone = _synth(3, 64)
    base = [_req(short[0], 24), _req(short[1], 24)]
    alone.run(base)
    assert alone.prompt_chunks == 0
    llm.close()
    for i in range(2):
        assert reqs[i].error is None and reqs[i].tokens == base[i].tokens, f"short stream {i}"
        _matches_oracle(short[i], reqs[i], f"short stream {i}")
    _matches_oracle(long_, reqs[2], "long stream")


def test_many_requests_on_one_prefix():
    """Four requests name one registered prefix of 100 ids (prefilled once, 64 + 36) and carry
    suffixes of 5, 9, 17 and 70 ids (the last one in two chunks itself)."""
    rng = np.random.default_rng(523)
    prefix = _ids(rng, 100)
    suffixes = [_ids(rng, n) for n in (5, 9, 17, 70)]
    llm, syn = _synth(4, 64, prefix_slots=1)
    h = syn.register_prefix("voice", prefix)
    reqs = [_req(s, 8, prefix="voice") for s in suffixes]
    syn.run(reqs)
    assert h.result(timeout=0) == "voice"
    assert dict(syn.prefix_fills) == {"voice": 1} and dict(syn.prefix_forks) == {"voice": 4}
    assert syn.prompt_chunks == 2 + 3 + 2
    assert llm.slot_len(4) == 100                    # the template slot, above the stream slots
    llm.close()
    for i, (s, r) in enumerate(zip(suffixes, reqs)):
        _matches_oracle(prefix + s, r, f"prefixed stream {i}")


def test_eviction_fails_only_the_request_that_names_the_evicted_prefix():
    from project_morpheus_amd.batching import UnknownPrefix
    rng = np.random.default_rng(524)
    first, second, tail = _ids(rng, 40), _ids(rng, 50), _ids(rng, 6)
    llm, syn = _synth(3, 64, prefix_slots=1)
    ha, hb = syn.register_prefix("a", first), syn.register_prefix("b", second)
    syn.run([])                                      # both registrations, in order: b evicts a
    assert ha.result(timeout=0) == "a" and hb.result(timeout=0) == "b"
    reqs = [_req(tail, 6, prefix="a"), _req(tail, 6, prefix="b"), _req(tail, 6)]
    syn.run(reqs)
    assert "a" not in syn.prefixes and "b" in syn.prefixes and not syn.has_prefix("a")
    assert dict(syn.prefix_fills) == {"a": 1, "b": 1}
    llm.close()
    assert isinstance(reqs[0].error, UnknownPrefix) and not reqs[0].tokens
    _matches_oracle(second + tail, reqs[1], "stream on the surviving prefix")
    _matches_oracle(tail, reqs[2], "plain stream")
    # no template slots at all: the registration is refused, nothing reaches the loop
    llm, syn = _synth(1, 64)
    assert isinstance(syn.register_prefix("a", first).error, ValueError)
    llm.close()


def test_cancel_mid_prompt_frees_row_and_slot(monkeypatch):
    """One row, one slot.  The long prompt is cancelled after its second chunk; the request
    behind it gets the row and the slot and speaks."""
    rng = np.random.default_rng(525)
    long_, nxt = _ids(rng, 200), _ids(rng, 12)
    llm, syn = _synth(1, 64)
    reqs = [_req(long_, 8), _req(nxt, 8)]
    real, calls = llm.prefill_chunk, []

    def chunk(slot, ids, pos0, stream, **kw):
        real(slot, ids, pos0, stream, **kw)
        calls.append((slot, pos0, kw.get("last", False)))
        if len(calls) == 2:
            reqs[0].cancel()

    monkeypatch.setattr(llm, "prefill_chunk", chunk)
    syn.run(reqs)
    assert calls == [(0, 0, False), (0, 64, False)]
    assert reqs[0].cancelled and not reqs[0].tokens and reqs[0].error is None
    assert reqs[0].t_done is not None
    assert llm.row_state(0) == (False, 0)
    llm.close()
    _matches_oracle(nxt, reqs[1], "stream after the cancel")
