"""Host side of code-grammar decoding (Code grammar), no GPU.

The grammar's allowed sets against the reference's token -> code rule (schedule.code_of_id),
the ABI struct, the environment default, the request field and the completions parameter.
"""
import ctypes
import queue

import pytest
from starlette.testclient import TestClient

from project_morpheus_amd import _lib
from project_morpheus_amd import config as C
from project_morpheus_amd.batching import StreamRequest
from project_morpheus_amd.completions import params_from_payload
from project_morpheus_amd.schedule import code_of_id
from project_morpheus_amd.server import build_app
from project_morpheus_amd.tokenizer import Tokenizer


def test_env_default():
    assert C.grammar_default({}) is False
    for v in ("1", "true", "YES", " on "):
        assert C.grammar_default({"MORPHEUS_MX_GRAMMAR": v}) is True
    for v in ("0", "", "off", "2", "no"):
        assert C.grammar_default({"MORPHEUS_MX_GRAMMAR": v}) is False
    # the sampler defaults keep their three-tuple
    assert C.sampler_defaults({"MORPHEUS_MX_GRAMMAR": "1"}) == (0, 0.0, 0)


def test_request_field_and_default():
    r = StreamRequest(prompt_ids=[1, 2], max_tokens=3)
    assert r.grammar is False
    assert StreamRequest(prompt_ids=[1], max_tokens=1, grammar=True).grammar is True


def test_ctypes_struct_layout():
    assert ctypes.sizeof(_lib.CodeGrammar) == 20
    assert [n for n, _ in _lib.CodeGrammar._fields_] == [
        "code_base", "codes", "phases", "code_min", "stop_id"]
    assert all(t is ctypes.c_int32 for _, t in _lib.CodeGrammar._fields_)
    g = _lib.CodeGrammar(1, 2, 3, 4, 5)
    assert list((ctypes.c_int32 * 5).from_buffer_copy(g)) == [1, 2, 3, 4, 5]
    assert {"mx_llm_set_grammar", "mx_llm_set_slot_grammar"} <= set(_lib.EXPORTS)


def test_orpheus_preset():
    g = C.ORPHEUS_GRAMMAR
    assert (g.code_base, g.codes, g.phases, g.code_min, g.stop_id) == (128266, 4096, 7, 1, 128258)
    assert g.code_base + g.phases * g.codes <= C.OrpheusConfig().vocab


def test_allowed_sets_against_code_of_id():
    """Every id of A(k) maps to a code in [1, 4096) at index k, and no other id >=
    CUSTOM_TOKEN_BASE does, except the stop id (allowed at phase 0 only)."""
    g, V = C.ORPHEUS_GRAMMAR, C.OrpheusConfig().vocab
    for k in range(g.phases):
        ids, stop = g.allowed(k)
        assert len(ids) == 4095
        assert stop == (C.END_OF_SPEECH if k == 0 else None)
        good = {t for t in range(C.CUSTOM_TOKEN_BASE, V) if 1 <= code_of_id(t, k) < 4096}
        assert good == set(ids)
        # the index may be any with the same phase
        assert all(1 <= code_of_id(t, k + 7 * 3) < 4096 for t in (ids[0], ids[-1]))
        assert g.allows(k, ids[0]) and g.allows(k, ids[-1])
        assert not g.allows(k, ids[0] - 1) and not g.allows(k, ids[-1] + 1)
        assert g.allows(k, C.END_OF_SPEECH) == (k == 0)
        assert not g.allows(k, 0) and not g.allows(k, C.START_OF_SPEECH)
    # a grammar without a stop id
    assert C.CodeGrammar(10, 4, 2, 0, -1).allowed(0) == (range(10, 14), None)


class _Handle:
    def __init__(self, toks):
        self.q = queue.Queue()
        for t in list(toks) + [None]:
            self.q.put(t)

    def get(self, timeout=None):
        return self.q.get(timeout=timeout) if timeout else self.q.get_nowait()

    def cancel(self):
        pass


def test_completions_parameter():
    assert "grammar" not in params_from_payload({"prompt": "x"})
    assert params_from_payload({"code_grammar": True})["grammar"] is True
    assert params_from_payload({"code_grammar": False})["grammar"] is False
    for bad in (1, 0, "true", None, [True]):
        with pytest.raises(ValueError):
            params_from_payload({"code_grammar": bad})
    seen = []
    tok = Tokenizer(None)

    def source(ids, **params):
        seen.append(params)
        return _Handle([C.AUDIO_CODE_BASE + 5])
    client = TestClient(build_app(token_source=source, encode=tok.encode))
    r = client.post("/v1/completions", json={"prompt": "<|audio|>tara: hi<|eot_id|>",
                                             "code_grammar": True, "max_tokens": 4})
    assert r.status_code == 200 and seen[-1]["grammar"] is True
    r = client.post("/v1/completions", json={"prompt": "<|audio|>tara: hi<|eot_id|>",
                                             "max_tokens": 4})
    assert r.status_code == 200 and "grammar" not in seen[-1]
    r = client.post("/v1/completions", json={"prompt": "hi", "code_grammar": "yes"})
    assert r.status_code == 400 and len(seen) == 2


def test_adapter_passes_the_choice_only_when_made():
    from project_morpheus_amd.adapter import MxTTSAdapter
    calls = []

    class A(MxTTSAdapter):
        @staticmethod
        def source(prompt, voice, use_batching, max_batch_chars, cancel, **kw):
            calls.append(kw)
            return iter(())
    A("hello")._start()
    A("hello", grammar=True)._start()
    assert calls == [{}, {"grammar": True}]
