"""Voice registration from audio on the GPU: ``Service.register_voice`` encodes a recording with
the SNAC encoder, frames it with its transcript and registers the ids as a prefix; a request that
names the voice then runs like one behind ``register_prefix`` with those ids.  Small-width model,
one template slot."""
import numpy as np
import pytest
import torch

import _snac_encoder_ref as R
from project_morpheus_amd import config as C
from project_morpheus_amd import inference as I
from project_morpheus_amd.weights import (synthetic_llm_weights, synthetic_snac_encoder_weights,
                                          synthetic_snac_weights)

pytestmark = pytest.mark.gpu

CFG = C.OrpheusConfig(hidden=512, layers=2, heads=4, kv_heads=2, ffn=1024)
TEXT = "this is what I sound like"
MAX_POS = 512


@pytest.fixture(scope="module")
def svc():
    from project_morpheus_amd import service
    w = synthetic_llm_weights(CFG, seed=81, std=0.05, norm_jitter=0.5)
    sw, ew = synthetic_snac_weights(seed=82), synthetic_snac_encoder_weights(seed=83)
    s = service.Service(device=0, cfg=CFG, llm_weights=w, snac_weights=sw, max_pos=MAX_POS,
                        max_prefill=128, max_batch=2, synthetic_audio=True, prefix_slots=1,
                        snac_encoder_weights=ew)
    s.test_weights = (sw, ew)
    saved = (I.TEMPERATURE, I.MAX_TOKENS)
    I.update_generation_params(temperature=0.0, max_tokens=56)
    yield s
    I.update_generation_params(temperature=saved[0], max_tokens=saved[1])
    s.close()


def _drain(h):
    pcm = b"".join(h.chunks())
    assert h.req.error is None, h.req.error
    return list(h.req.tokens), pcm


def test_register_voice_registers_the_framed_encoding(svc):
    from project_morpheus_amd.engine import SnacEncoder
    audio = R.make_audio(5000, seed=3)
    sw, ew = svc.test_weights
    enc = SnacEncoder({**sw, **ew}, device=0, max_frames=3)
    frames = enc.encode(audio)
    torch.cuda.synchronize()
    enc.close()
    want = I.frame_voice_pairs([(svc.tok.encode(TEXT), I.audio_ids_from_frames(frames.cpu()))])
    assert len(want) == len(svc.tok.encode(TEXT)) + 5 + 21 + 2

    h = svc.register_voice("ana", TEXT, audio)
    assert h.result(timeout=60) == "ana"
    entry = svc.batch.prefixes.get("ana", touch=False)
    assert entry.ids == want
    assert svc.encode_audio(audio) == want[len(svc.tok.encode(TEXT)) + 5:-2]
    # int16 PCM of the same samples goes the same way (/ 32768)
    pcm16 = (audio * 32768.0).astype(np.int16)
    assert svc.encode_audio(pcm16) == svc.encode_audio(pcm16.astype(np.float32) / 32768.0)

    # a request that names the voice completes and yields PCM ...
    toks, pcm = _drain(svc.submit("and this is new text", seed=5, prefix="ana"))
    assert len(toks) == 56 and len(pcm) > 0 and len(pcm) % 2 == 0
    assert svc.llm.slot_len(entry.slot) == len(want)
    # ... exactly as behind register_prefix with those ids: same prompt length, same stream
    assert svc.register_prefix("ids", want).result(timeout=60) == "ids"
    by_ids = svc.batch.prefixes.get("ids", touch=False)
    toks2, pcm2 = _drain(svc.submit("and this is new text", seed=5, prefix="ids"))
    assert svc.llm.slot_len(by_ids.slot) == len(want)
    assert toks2 == toks and pcm2 == pcm


def test_refusals_leave_no_prefix(svc):
    audio = R.make_audio(5000, seed=4)
    frames_max = svc.voice_max_frames
    assert frames_max == (MAX_POS - 9) // 7
    cases = {
        "wrong sample rate": dict(audio=audio, sample_rate=16000),
        "empty": dict(audio=audio[:0]),
        "too long": dict(audio=np.zeros((frames_max + 1) * 2048, np.float32)),
        # fits the encoder, but 7 ids a frame plus the transcript do not fit max_pos
        "prompt does not fit": dict(audio=np.zeros(frames_max * 2048, np.float32)),
    }
    for what, kw in cases.items():
        with pytest.raises(ValueError):
            svc.register_voice("bad", TEXT, **kw)
        assert not svc.batch.has_prefix("bad"), what
    with pytest.raises(ValueError):
        svc.register_voice("", TEXT, audio)
    # and a good registration still goes through afterwards
    assert svc.register_voice("good", TEXT, audio).result(timeout=60) == "good"
    assert svc.batch.has_prefix("good")
