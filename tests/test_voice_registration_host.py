"""``POST /v1/voices`` on the host: WAV parsing, the registrar hook, the 400s, and the route's
absence without the hook (the golden server tests build the app without it)."""
import base64
import struct

import numpy as np
import pytest
from starlette.testclient import TestClient

from project_morpheus_amd.server import build_app, parse_voice_wav


def _wav(samples=None, rate=24000, channels=1, bits=16, fmt=1, extra_chunk=True):
    if samples is None:
        samples = (np.arange(5000) % 200 - 100).astype("<i2")
    body = np.asarray(samples).tobytes()
    head = struct.pack("<4sIHHIIHH", b"fmt ", 16, fmt, channels, rate,
                       rate * channels * bits // 8, channels * bits // 8, bits)
    if extra_chunk:  # an odd-sized chunk ahead of the data, as real files carry (LIST, fact)
        head += b"LIST" + struct.pack("<I", 3) + b"abc\x00"
    data = b"data" + struct.pack("<I", len(body)) + body
    return b"RIFF" + struct.pack("<I", 4 + len(head) + len(data)) + b"WAVE" + head + data


class _Registrar:
    def __init__(self):
        self.calls = []

    def __call__(self, name, text, samples, rate):
        if name == "refused":
            raise ValueError("voice prompt does not fit")
        self.calls.append((name, text, np.array(samples), rate))
        return 7 * -(-samples.size // 2048) + 11


def _post(client, **fields):
    return client.post("/v1/voices", json=fields)


def test_parse_voice_wav():
    pcm = (np.arange(4096) - 2048).astype("<i2")
    samples, rate = parse_voice_wav(_wav(pcm))
    assert rate == 24000 and samples.dtype == np.int16 and np.array_equal(samples, pcm)
    # a streamed header (sizes 0xFFFFFFFF, server.riff_header) reads up to the end of the bytes
    from project_morpheus_amd.server import riff_header
    samples, _ = parse_voice_wav(riff_header() + pcm.tobytes())
    assert np.array_equal(samples, pcm)


def test_voices_route_happy_path():
    reg = _Registrar()
    client = TestClient(build_app(voice_registrar=reg))
    pcm = (np.arange(5000) % 200 - 100).astype("<i2")
    r = _post(client, name="ana", text="hello there",
              audio_b64=base64.b64encode(_wav(pcm)).decode())
    assert r.status_code == 200, r.text
    assert r.json() == {"name": "ana", "frames": 3, "prefix_ids": 32}
    (name, text, samples, rate), = reg.calls
    assert (name, text, rate) == ("ana", "hello there", 24000)
    assert samples.dtype == np.int16 and np.array_equal(samples, pcm)


@pytest.mark.parametrize("case,wav", [
    ("not RIFF", b"OggS" + bytes(60)),
    ("stereo", _wav(channels=2)),
    ("16 kHz", _wav(rate=16000)),
    ("8-bit", _wav(samples=np.zeros(100, np.uint8), bits=8)),
    ("float format", _wav(fmt=3)),
    ("no samples", _wav(samples=np.zeros(0, "<i2"))),
])
def test_voices_route_refuses_malformed_audio(case, wav):
    reg = _Registrar()
    client = TestClient(build_app(voice_registrar=reg))
    r = _post(client, name="v", text="t", audio_b64=base64.b64encode(wav).decode())
    assert r.status_code == 400, (case, r.text)
    assert not reg.calls


def test_voices_route_refuses_bad_requests():
    reg = _Registrar()
    client = TestClient(build_app(voice_registrar=reg))
    good = base64.b64encode(_wav()).decode()
    assert _post(client, name="v", audio_b64=good).status_code == 400          # missing field
    assert _post(client, name="", text="t", audio_b64=good).status_code == 400
    assert _post(client, name="v", text="t", audio_b64="***").status_code == 400
    assert _post(client, name="v", text="t", audio_b64=7).status_code == 400
    assert client.post("/v1/voices", content=b"{").status_code == 400
    assert not reg.calls
    # what the registrar refuses (audio too long, prompt does not fit) is a 400 too
    r = _post(client, name="refused", text="t", audio_b64=good)
    assert r.status_code == 400 and "does not fit" in r.text


def test_route_absent_without_the_hook():
    client = TestClient(build_app())
    good = base64.b64encode(_wav()).decode()
    assert _post(client, name="v", text="t", audio_b64=good).status_code == 404
    with_hook = {r.path for r in build_app(voice_registrar=_Registrar()).routes}
    without = {r.path for r in build_app().routes}
    assert with_hook - without == {"/v1/voices"}


# ---- GpuPool: one worker encodes, every worker gets the ids ------------------------------------
from test_prompt_continuation_host import PrefixService, _tokens  # noqa: E402


class VoiceService(PrefixService):
    """Encodes "audio" to ids that name the encoding worker, so the test reads who encoded."""

    def voice_prefix_ids(self, text, audio, sample_rate=24000):
        if sample_rate != 24000:
            raise ValueError("voice audio must be 24000 Hz mono")
        return [1000 * (self.device + 1), len(text), int(audio.size), int(audio.sum())]


def voice_factory(device):
    return VoiceService(device)


def test_pool_encodes_on_one_worker_and_registers_ids_everywhere():
    from project_morpheus_amd.dispatch import GpuPool
    p = GpuPool(2, factory=voice_factory, start_timeout=120, poll_s=0.1)
    try:
        audio = np.arange(10, dtype=np.int16)
        assert p.register_voice("ana", "hello", audio) == [0, 1]
        ids = p.prefixes["ana"]
        assert ids == [1000, 5, 10, 45]                     # encoded once, by worker 0
        a = p.submit_tokens([1], max_tokens=700, prefix="ana")
        b = p.submit_tokens([1], max_tokens=700, prefix="ana")
        assert (a.worker, b.worker) == (0, 1)
        assert _tokens(a) == ids + [100] and _tokens(b) == [t + 1 for t in ids] + [100]
        with pytest.raises(ValueError, match="24000"):
            p.register_voice("bad", "hello", audio, sample_rate=16000)
        assert "bad" not in p.prefixes
        with pytest.raises(ValueError):
            p.register_voice("", "hello", audio)
        assert p.load == [0, 0]
    finally:
        p.close()
