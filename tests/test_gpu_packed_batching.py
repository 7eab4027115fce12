"""BatchSynthesizer with packed prefill: the requests one iteration admits go through
LlmEngine.prefill_batch, and every stream still speaks its script.

The speaking weights of tests/_speaking.py, four scripts arriving together; token ids must equal
the scripts id for id and the PCM the oracle pipeline's within 1 LSB (as
tests/test_gpu_composed.py, whose oracle helper is restated here).
"""
import numpy as np
import pytest

from _speaking import STARTS, four_scripts, speaking_config, speaking_weights
from oracle import llama_ref as L
from oracle import snac_ref
from oracle import speechpipe_ref as SP
from project_morpheus_amd import config as C
from project_morpheus_amd.batching import window_seed
from project_morpheus_amd.weights import synthetic_snac_weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    cfg = speaking_config()
    scripts = four_scripts()
    w = speaking_weights(cfg, dict(zip(STARTS, scripts)))
    sw = synthetic_snac_weights(seed=8)
    ref = L.LlamaRef(L.RefConfig(hidden=cfg.hidden, layers=cfg.layers, heads=cfg.heads,
                                 kv_heads=cfg.kv_heads, ffn=cfg.ffn, vocab=cfg.vocab,
                                 tied=False), w, max_pos=512)
    # the oracle's greedy decode of the four prompts, computed once for every test below: one
    # forward per step for all four streams, teacher-forced with the scripts; its argmax (after
    # the 1.1 penalty) is the script at every step, so the free-running oracle emits the scripts
    tr = L.teacher_forced_rows(ref, [_prompt(b) for b in range(4)], scripts, 1.1)
    for b in range(4):
        assert [int(np.argmax(x.numpy())) for x in tr[b]] == scripts[b], f"oracle stream {b}"
        assert scripts[b][-1] in C.STOP_IDS
    return cfg, w, sw, scripts, ref


def _strings(toks):
    return [f"<custom_token_{t - C.CUSTOM_TOKEN_BASE}>" if t >= C.CUSTOM_TOKEN_BASE
            else f" text{t}" for t in toks]


def _oracle_pcm(sw, toks, noise_seed_of_window):
    """The oracle pipeline on the oracle's tokens (``world``): token strings -> speechpipe_ref
    -> snac_ref with the device's NoiseBlock noise."""
    j = [0]

    def dec(c0, c1, c2):
        noise = snac_ref.window_noise(noise_seed_of_window(j[0]), len(c0))
        j[0] += 1
        return snac_ref.decode(sw, c0, c1, c2, noise=noise).reshape(-1).numpy()

    return SP.drop_empty(SP.decode_stream(_strings(toks), dec))


def _same_pcm(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} vs {len(want)} chunks"
    for i, (a, b) in enumerate(zip(got, want)):
        x = np.frombuffer(a, dtype=np.int16).astype(np.int32)
        y = np.frombuffer(b, dtype=np.int16).astype(np.int32)
        assert x.shape == y.shape, f"{what} chunk {i}"
        assert np.abs(x - y).max() <= 1, f"{what} chunk {i}"


def _prompt(b):
    return [1001 + b, 1002, 1003 + 5 * b, STARTS[b]][: 2 + b % 3] + [STARTS[b]]


def _synth(world, max_prefill, packed):
    from project_morpheus_amd.batching import BatchSynthesizer
    from project_morpheus_amd.engine import LlmEngine, SnacDecoder
    cfg, w, sw, scripts, ref = world
    llm = LlmEngine(cfg, w, max_slots=4, max_pos=512, max_batch=4, max_prefill=max_prefill)
    return llm, BatchSynthesizer(llm, SnacDecoder(sw, max_frames=7, max_batch=8), depth=2,
                                 packed_prefill=packed)


def test_four_scripts_in_one_pack(world):
    from project_morpheus_amd.batching import StreamRequest
    cfg, w, sw, scripts, ref = world
    llm, syn = _synth(world, 64, True)
    reqs = [StreamRequest(prompt_ids=_prompt(b), max_tokens=len(scripts[b]) + 8, arrival=0.0,
                          noise_seed=777 + b) for b in range(4)]
    chunks = {id(r): [] for r in reqs}
    syn.run(reqs, on_chunk=lambda r, c: chunks[id(r)].append(c))
    assert dict(syn.prefill_packs) == {4: 1}
    for b, r in enumerate(reqs):
        assert r.tokens == scripts[b], f"GPU stream {b}"
        want = _oracle_pcm(sw, scripts[b], lambda j, s=r.noise_seed: window_seed(s, j))
        _same_pcm(chunks[id(r)], want, f"packed stream {b}")
    llm.close()


def test_six_requests_split_into_several_packs(world):
    """Six requests on four rows, max_prefill 12: the first iteration admits four prompts
    (3 + 4 + 5 ids in one pack, 3 in the next), the last two join as rows free up."""
    from project_morpheus_amd.batching import StreamRequest
    cfg, w, sw, scripts, ref = world
    llm, syn = _synth(world, 12, True)
    reqs = [StreamRequest(prompt_ids=_prompt(b % 4), max_tokens=len(scripts[b % 4]) + 8,
                          arrival=0.0, audio=False) for b in range(6)]
    syn.run(reqs)
    assert sum(syn.prefill_packs.values()) >= 3
    assert sum(k * v for k, v in syn.prefill_packs.items()) == 6
    assert max(syn.prefill_packs) < 4          # 15 ids do not fit 12 rows: no pack of four
    for b, r in enumerate(reqs):
        assert r.error is None and r.tokens == scripts[b % 4], f"stream {b}"
    llm.close()


def test_packing_off_makes_no_pack(world):
    from project_morpheus_amd.batching import StreamRequest
    cfg, w, sw, scripts, ref = world
    llm, syn = _synth(world, 64, False)
    reqs = [StreamRequest(prompt_ids=_prompt(b), max_tokens=len(scripts[b]) + 8, arrival=0.0,
                          audio=False) for b in range(4)]
    syn.run(reqs)
    assert not syn.prefill_packs
    for b, r in enumerate(reqs):
        assert r.tokens == scripts[b], f"stream {b}"
    llm.close()


def test_bad_request_fails_alone_next_to_a_pack(world):
    """An id past the vocabulary is refused before the pack forms: that request fails alone, the
    other three are admitted in one pack and speak."""
    from project_morpheus_amd.batching import StreamRequest
    cfg, w, sw, scripts, ref = world
    llm, syn = _synth(world, 64, True)
    reqs = [StreamRequest(prompt_ids=_prompt(b), max_tokens=len(scripts[b]) + 8, arrival=0.0,
                          audio=False) for b in range(4)]
    reqs[1].prompt_ids = [1001, cfg.vocab, STARTS[1]]
    syn.run(reqs)
    assert dict(syn.prefill_packs) == {3: 1}
    assert isinstance(reqs[1].error, ValueError) and not reqs[1].tokens
    for b in (0, 2, 3):
        assert reqs[b].error is None and reqs[b].tokens == scripts[b], f"stream {b}"
    llm.close()


def test_refused_pack_is_retried_request_by_request(world, monkeypatch):
    """A pack the device refuses with MX_ERR_ARG enqueues nothing; the batcher then admits its
    requests one by one.  The refusal is provoked by handing the real entry point a pack of five
    segments on four rows."""
    from project_morpheus_amd.batching import StreamRequest
    cfg, w, sw, scripts, ref = world
    llm, syn = _synth(world, 64, True)
    real, calls = llm.prefill_batch, []

    def twice(segments, stream):
        calls.append(len(segments))
        real(list(segments) + [segments[0]], stream)

    monkeypatch.setattr(llm, "prefill_batch", twice)
    reqs = [StreamRequest(prompt_ids=_prompt(b), max_tokens=len(scripts[b]) + 8, arrival=0.0,
                          audio=False) for b in range(4)]
    syn.run(reqs)
    assert calls == [4] and not syn.prefill_packs
    for b, r in enumerate(reqs):
        assert r.error is None and r.tokens == scripts[b], f"stream {b}"
    llm.close()
