"""Host plumbing of the sampler chain's extras (top_k, min_p, the penalty window), on CPU:
the /v1/completions payload names (llama.cpp server's), their checks, the env defaults and
preset, the request fields and the C ABI struct."""
import ctypes
import json
import os
import queue

import pytest
from starlette.testclient import TestClient

from project_morpheus_amd import _lib
from project_morpheus_amd import config as C
from project_morpheus_amd import inference as I
from project_morpheus_amd.batching import StreamRequest, check_params
from project_morpheus_amd.completions import params_from_payload
from project_morpheus_amd.config import CUSTOM_TOKEN_BASE
from project_morpheus_amd.server import build_app
from project_morpheus_amd.tokenizer import Tokenizer

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "sse_golden.json")))


def test_golden_payload_still_yields_the_four_keys():
    p = GOLDEN["payload"]
    assert params_from_payload(p) == {"max_tokens": p["max_tokens"],
                                      "temperature": p["temperature"], "top_p": p["top_p"],
                                      "penalty": p["repeat_penalty"]}


def test_new_keys_pass_through_only_when_named():
    base = dict(GOLDEN["payload"])
    out = params_from_payload(dict(base, top_k=40))
    assert out["top_k"] == 40 and "min_p" not in out and "penalty_last_n" not in out
    out = params_from_payload(dict(base, min_p=0.05))
    assert out["min_p"] == 0.05 and "top_k" not in out and "penalty_last_n" not in out
    out = params_from_payload(dict(base, top_k=40, min_p=0.05, repeat_last_n=64))
    assert (out["top_k"], out["min_p"], out["penalty_last_n"]) == (40, 0.05, 64)
    assert out["penalty"] == base["repeat_penalty"]
    assert params_from_payload(dict(base, top_k=0, min_p=0))["top_k"] == 0


def test_repeat_last_n_mapping():
    base = dict(GOLDEN["payload"])
    out = params_from_payload(dict(base, repeat_last_n=-1))   # the whole sequence
    assert out["penalty_last_n"] == 0 and out["penalty"] == base["repeat_penalty"]
    out = params_from_payload(dict(base, repeat_last_n=0))    # penalty off
    assert out["penalty_last_n"] == 0 and out["penalty"] == 1.0
    out = params_from_payload(dict(base, repeat_last_n=64))
    assert out["penalty_last_n"] == 64 and out["penalty"] == base["repeat_penalty"]
    assert params_from_payload(dict(base, repeat_last_n=255))["penalty_last_n"] == 255
    for bad in (256, -2, 1.5, "many", None, True):
        with pytest.raises(ValueError):
            params_from_payload(dict(base, repeat_last_n=bad))


class _Handle:
    def __init__(self, toks):
        self.q = queue.Queue()
        for t in toks:
            self.q.put(t)
        self.q.put(None)

    def get(self, timeout=None):
        return self.q.get(timeout=timeout) if timeout else self.q.get_nowait()

    def cancel(self):
        pass


def test_bad_extras_are_a_400_before_the_token_source():
    tok, seen = Tokenizer(None), []

    def source(ids, **params):
        seen.append(params)
        return _Handle([CUSTOM_TOKEN_BASE + 11])
    c = TestClient(build_app(token_source=source, encode=tok.encode))
    base = {"prompt": "<|audio|>tara: hi<|eot_id|>", "max_tokens": 2}
    for bad in ({"top_k": -1}, {"top_k": 2.5}, {"top_k": "forty"}, {"min_p": -0.1},
                {"min_p": 1.5}, {"min_p": "low"}, {"min_p": float("nan")},
                {"repeat_last_n": 256}, {"repeat_last_n": -2}):
        body = json.dumps(dict(base, **bad))  # (json.dumps writes NaN, which starlette reads)
        r = c.post("/v1/completions", content=body, headers={"content-type": "application/json"})
        assert r.status_code == 400, bad
    assert seen == []
    r = c.post("/v1/completions", json=dict(base, top_k=40, min_p=0.05, repeat_last_n=64))
    assert r.status_code == 200
    assert seen == [{"max_tokens": 2, "temperature": I.TEMPERATURE, "top_p": I.TOP_P,
                     "penalty": I.REPETITION_PENALTY, "top_k": 40, "min_p": 0.05,
                     "penalty_last_n": 64}]


def test_check_params_keeps_its_positionals_and_checks_the_extras():
    check_params(1.1, 0.6, 0.9, 10)
    check_params(1.1, 0.6, 0.9, 10, top_k=0, min_p=0.0, penalty_last_n=0)
    check_params(1.1, 0.6, 0.9, 10, top_k=40, min_p=1.0, penalty_last_n=255)
    for bad in ({"top_k": -1}, {"top_k": 1.0}, {"min_p": -1e-3}, {"min_p": 1.001},
                {"min_p": float("nan")}, {"penalty_last_n": 256}, {"penalty_last_n": -1},
                {"penalty_last_n": 3.0}):
        with pytest.raises(ValueError):
            check_params(1.1, 0.6, 0.9, 10, **bad)
    with pytest.raises(TypeError):
        check_params(1.1, 0.6, 0.9, 10, 40)  # the extras are keyword-only


def test_env_defaults_and_preset():
    assert C.sampler_defaults({}) == (0, 0.0, 0)
    assert C.sampler_defaults({"MORPHEUS_MX_SAMPLER": "llama_cpp"}) == (40, 0.05, 64)
    assert C.sampler_defaults({"MORPHEUS_MX_TOP_K": "20", "MORPHEUS_MX_MIN_P": "0.1",
                               "MORPHEUS_MX_REPEAT_LAST_N": "32"}) == (20, 0.1, 32)
    # the individual variables win over the preset, which fills what is unset
    assert C.sampler_defaults({"MORPHEUS_MX_SAMPLER": "llama_cpp",
                               "MORPHEUS_MX_TOP_K": "0"}) == (0, 0.05, 64)
    assert C.sampler_defaults({"MORPHEUS_MX_SAMPLER": "llama_cpp",
                               "MORPHEUS_MX_REPEAT_LAST_N": "128"}) == (40, 0.05, 128)
    # what does not parse or lies out of range counts as unset
    assert C.sampler_defaults({"MORPHEUS_MX_TOP_K": "-3", "MORPHEUS_MX_MIN_P": "2",
                               "MORPHEUS_MX_REPEAT_LAST_N": "256"}) == (0, 0.0, 0)
    assert C.sampler_defaults({"MORPHEUS_MX_SAMPLER": "unknown", "MORPHEUS_MX_MIN_P": "x"}) \
        == (0, 0.0, 0)


def test_inference_defaults_and_update(monkeypatch):
    for name in ("TOP_K", "MIN_P", "REPEAT_LAST_N", "TEMPERATURE", "TOP_P", "MAX_TOKENS"):
        monkeypatch.setattr(I, name, getattr(I, name))  # restored after the test
    I.update_generation_params(temperature=0.5, max_tokens=100)  # the benchmark's call
    assert (I.TEMPERATURE, I.MAX_TOKENS) == (0.5, 100)
    I.update_generation_params(top_k=40, min_p=0.05, repeat_last_n=64)
    assert (I.TOP_K, I.MIN_P, I.REPEAT_LAST_N) == (40, 0.05, 64)
    assert (I.TEMPERATURE, I.MAX_TOKENS) == (0.5, 100)


def test_request_fields_and_abi_struct():
    r = StreamRequest(prompt_ids=[1, 2], max_tokens=4)
    assert (r.top_k, r.min_p, r.penalty_last_n) == (0, 0.0, 0)
    r = StreamRequest(prompt_ids=[1, 2], max_tokens=4, top_k=5, min_p=0.1, penalty_last_n=3)
    assert (r.top_k, r.min_p, r.penalty_last_n) == (5, 0.1, 3)
    ext = _lib.SamplingExt(top_k=40, min_p=0.05, penalty_last_n=64)
    assert ctypes.sizeof(ext) == 12
    assert [f[0] for f in _lib.SamplingExt._fields_] == ["top_k", "min_p", "penalty_last_n"]
    assert ctypes.sizeof(_lib.Sampling) == 24  # mx_sampling did not grow
    assert "mx_llm_prefill_ex" in _lib._SIGS and "mx_llm_debug_sample" in _lib._SIGS
