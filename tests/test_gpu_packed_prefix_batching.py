"""BatchSynthesizer with packed prefill AND the prefix cache: requests naming a ready prefix
whose suffix fits one chunk are admitted as one pack behind one ``fork_slots``; longer suffixes
stay chunked; with packing off nothing changes.

The world of tests/test_gpu_prefix_batching.py (narrow model, token-only greedy streams, each
compared with LlamaRef teacher-forced on the GPU's tokens over the WHOLE prompt, tie-aware with
margin 1e-2).
"""
import numpy as np
import pytest

from project_morpheus_amd import _lib

from test_gpu_prefix_batching import _ids, _matches_oracle, _req, _world

pytestmark = pytest.mark.gpu


def _synth(rows, max_prefill, prefix_slots, packed):
    from project_morpheus_amd.batching import BatchSynthesizer
    from project_morpheus_amd.engine import LlmEngine, SnacDecoder
    cfg, w, sw, _ = _world()
    llm = LlmEngine(cfg, w, max_slots=rows + prefix_slots, max_pos=512, max_batch=rows,
                    max_prefill=max_prefill)
    return llm, BatchSynthesizer(llm, SnacDecoder(sw, max_frames=7, max_batch=8), depth=2,
                                 prefix_slots=prefix_slots, packed_prefill=packed)


def _voice_burst(seed):
    rng = np.random.default_rng(seed)
    return _ids(rng, 100), [_ids(rng, n) for n in (5, 9, 17, 70)]


def test_suffixes_on_one_prefix_share_a_pack():
    prefix, suffixes = _voice_burst(531)
    llm, syn = _synth(4, 64, 1, True)
    syn.register_prefix("voice", prefix)
    reqs = [_req(s, 8, prefix="voice") for s in suffixes]
    syn.run(reqs)
    assert dict(syn.prefix_packs) == {3: 1} and dict(syn.prefill_packs) == {3: 1}
    assert dict(syn.prefix_fills) == {"voice": 1} and dict(syn.prefix_forks) == {"voice": 4}
    assert syn.prompt_chunks == 2 + 2      # the prefix's own chunks and the 70-id suffix's
    llm.close()
    for i, (s, r) in enumerate(zip(suffixes, reqs)):
        _matches_oracle(prefix + s, r, f"prefixed stream {i}")


def test_packing_off_keeps_the_chunked_path():
    prefix, suffixes = _voice_burst(531)
    llm, syn = _synth(4, 64, 1, False)
    syn.register_prefix("voice", prefix)
    reqs = [_req(s, 8, prefix="voice") for s in suffixes]
    syn.run(reqs)
    assert not syn.prefix_packs and not syn.prefill_packs
    assert dict(syn.prefix_forks) == {"voice": 4}
    assert syn.prompt_chunks == 2 + 3 + 2
    llm.close()
    for i, (s, r) in enumerate(zip(suffixes, reqs)):
        _matches_oracle(prefix + s, r, f"chunked stream {i}")


def test_plain_and_prefixed_requests_share_a_pack():
    rng = np.random.default_rng(532)
    prefix, plain, suffixes = _ids(rng, 100), _ids(rng, 12), [_ids(rng, 7), _ids(rng, 15)]
    llm, syn = _synth(3, 64, 1, True)
    syn.register_prefix("voice", prefix)
    reqs = [_req(suffixes[0], 8, prefix="voice"), _req(plain, 8),
            _req(suffixes[1], 8, prefix="voice")]
    syn.run(reqs)
    assert dict(syn.prefill_packs) == {3: 1} and dict(syn.prefix_packs) == {3: 1}
    assert syn.prompt_chunks == 2
    llm.close()
    _matches_oracle(prefix + suffixes[0], reqs[0], "prefixed stream 0")
    _matches_oracle(plain, reqs[1], "plain stream")
    _matches_oracle(prefix + suffixes[1], reqs[2], "prefixed stream 1")


def test_refused_pack_is_admitted_member_by_member(monkeypatch):
    rng = np.random.default_rng(533)
    prefix, plain, suffixes = _ids(rng, 100), _ids(rng, 12), [_ids(rng, 7), _ids(rng, 15)]
    llm, syn = _synth(3, 64, 1, True)
    syn.register_prefix("voice", prefix)
    real, refused = llm.fork_slots, []

    def fork_slots(pairs, stream):
        try:
            real(list(pairs) + [pairs[0]], stream)      # a dst named twice
        except _lib.MxError as e:
            refused.append(e.rc)
            raise

    monkeypatch.setattr(llm, "fork_slots", fork_slots)
    reqs = [_req(suffixes[0], 8, prefix="voice"), _req(plain, 8),
            _req(suffixes[1], 8, prefix="voice")]
    syn.run(reqs)
    assert refused == [_lib.MX_ERR_STATE]
    assert not syn.prefix_packs and not syn.prefill_packs
    assert dict(syn.prefix_forks) == {"voice": 2}
    assert syn.prompt_chunks == 2 + 2      # the prefix's chunks, one final chunk per suffix
    llm.close()
    _matches_oracle(prefix + suffixes[0], reqs[0], "prefixed stream 0")
    _matches_oracle(plain, reqs[1], "plain stream")
    _matches_oracle(prefix + suffixes[1], reqs[2], "prefixed stream 1")
