"""Host side of prompt continuation and the prefix cache, on CPU: the chunk plan, the prefix
registry's LRU, the validation of ``prefix`` / ``prompt_prefix`` (HTTP 400s through the server
app), the voice-pair framing, and GpuPool's registration fan-out and replay."""
import itertools
import queue
import time

import pytest
from starlette.testclient import TestClient

from _fakes import FakeHandle, FakeService
from _server_fake import GoldenAdapter
from project_morpheus_amd import inference as I
from project_morpheus_amd.batching import (PrefixRegistry, StreamRequest, UnknownPrefix,
                                           check_prefix, plan_prompt_chunks)
from project_morpheus_amd.completions import params_from_payload
from project_morpheus_amd.dispatch import GpuPool
from project_morpheus_amd.server import build_app
from project_morpheus_amd.tokenizer import Tokenizer


# ---- plan_prompt_chunks --------------------------------------------------------------------
def test_chunk_plan_covers_the_prompt_once_in_order():
    for n, pos0, mp in itertools.product(range(1, 41), (0, 1, 31, 32, 45), range(1, 10)):
        plan = plan_prompt_chunks(n, pos0, mp)
        at = pos0
        for off, length, last in plan:
            assert pos0 + off == at and 1 <= length <= mp
            at += length
        assert at == pos0 + n
        assert [last for _, _, last in plan] == [False] * (len(plan) - 1) + [True]
        assert len(plan) == -(-n // mp)


def test_chunk_plan_refuses_nonsense():
    for args in ((0, 0, 8), (5, -1, 8), (5, 0, 0)):
        with pytest.raises(ValueError):
            plan_prompt_chunks(*args)


# ---- prefix registry -----------------------------------------------------------------------
def _ready(reg, name, ids=(1, 2, 3)):
    p, old = reg.place(name, ids)
    p.ready = True
    return p, old


def test_registry_lru_eviction():
    reg = PrefixRegistry([8, 9])
    a, _ = _ready(reg, "a")
    b, _ = _ready(reg, "b")
    assert (a.slot, b.slot) == (8, 9) and not reg.free
    assert reg.get("a") is a                       # touch: b is now the least recently used
    c, old = _ready(reg, "c")
    assert old is b and c.slot == 9 and "b" not in reg and reg.get("b") is None
    d, old = _ready(reg, "d")                      # a was used before c was placed
    assert old is a and d.slot == 8
    assert list(reg.entries) == ["c", "d"]


def test_registry_skips_pinned_and_unfinished_prefixes():
    reg = PrefixRegistry([4, 5])
    a, _ = _ready(reg, "a")
    b, _ = reg.place("b", [7])                     # still being prefilled
    a.pins = 1                                     # a request in admission names it
    with pytest.raises(RuntimeError):
        reg.place("c", [9])
    assert list(reg.entries) == ["a", "b"]         # a refused placement changes nothing
    a.pins = 0
    c, old = reg.place("c", [9])
    assert old is a and c.slot == 4


def test_registry_replaces_a_name_in_its_own_slot_and_frees_on_remove():
    reg = PrefixRegistry([2, 3])
    a, _ = _ready(reg, "a", [1])
    a2, old = reg.place("a", [5, 6])
    assert old is a and a2.slot == a.slot and a2.ids == [5, 6] and not a2.ready
    assert reg.free == [3]
    assert reg.remove("a") is a2 and reg.free == [2, 3] and len(reg) == 0
    assert reg.remove("a") is None


def test_no_template_slots():
    with pytest.raises(RuntimeError):
        PrefixRegistry([]).place("a", [1])


# ---- validation ----------------------------------------------------------------------------
def test_check_prefix():
    check_prefix(None)
    check_prefix("voice-1")
    for bad in ("", 3, ["a"], b"a", True):
        with pytest.raises(ValueError):
            check_prefix(bad)
    assert StreamRequest(prompt_ids=[1], max_tokens=1).prefix is None
    assert issubclass(UnknownPrefix, ValueError)


def test_params_from_payload_prompt_prefix():
    assert params_from_payload({"prompt_prefix": "tara-ref"})["prefix"] == "tara-ref"
    assert "prefix" not in params_from_payload({})
    for bad in (7, None, "", ["x"], {"name": "x"}):
        with pytest.raises(ValueError):
            params_from_payload({"prompt_prefix": bad})


class _Tokens:
    def __init__(self, toks):
        self.q = queue.Queue()
        for t in list(toks) + [None]:
            self.q.put(t)

    def get(self, timeout=None):
        return self.q.get(timeout=timeout) if timeout else self.q.get_nowait()

    def cancel(self):
        pass


def test_completions_prompt_prefix_400s():
    tok, seen, known = Tokenizer(None), [], {"tara-ref"}

    def source(ids, **params):
        if params.get("prefix") is not None and params["prefix"] not in known:
            raise UnknownPrefix(f"unknown prefix {params['prefix']!r}")
        seen.append(params)
        return _Tokens([128266 + 11])

    client = TestClient(build_app(adapter_cls=GoldenAdapter, token_source=source,
                                  encode=tok.encode))
    ok = client.post("/v1/completions", json={"prompt": "hi", "prompt_prefix": "tara-ref"})
    assert ok.status_code == 200 and seen[-1]["prefix"] == "tara-ref"
    plain = client.post("/v1/completions", json={"prompt": "hi"})
    assert plain.status_code == 200 and "prefix" not in seen[-1]
    n = len(seen)
    for bad in (5, None, "", ["tara-ref"]):
        r = client.post("/v1/completions", json={"prompt": "hi", "prompt_prefix": bad})
        assert r.status_code == 400 and "prompt_prefix" in r.json()["error"]
    r = client.post("/v1/completions", json={"prompt": "hi", "prompt_prefix": "nobody"})
    assert r.status_code == 400 and "unknown prefix" in r.json()["error"]
    assert len(seen) == n                          # none of them reached the token source


def test_adapter_voice_prompt_reaches_the_source():
    from project_morpheus_amd.adapter import MxTTSAdapter
    calls = []

    class A(MxTTSAdapter):
        @staticmethod
        def source(prompt, voice, use_batching, max_batch_chars, cancel, **kw):
            calls.append(kw)
            return iter(())

    A("hello", voice_prompt="tara-ref")._start()
    A("hello")._start()
    assert calls == [{"prefix": "tara-ref"}, {}]
    for bad in ("", 4):
        with pytest.raises(ValueError):
            MxTTSAdapter("hello", voice_prompt=bad)


# ---- voice-pair framing --------------------------------------------------------------------
def test_frame_voice_pairs():
    a = I.frame_voice_pairs([([11, 12], [128266 + 5, 128266 + 4096 + 6])])
    assert a == [128259, 11, 12, 128009, 128260, 128261, 128257,
                 128271, 132368, 128258, 128262]
    two = I.frame_voice_pairs([([1], [128300]), ([2, 3], [128301, 128302])])
    assert two == [128259, 1, 128009, 128260, 128261, 128257, 128300, 128258, 128262,
                   128259, 2, 3, 128009, 128260, 128261, 128257, 128301, 128302, 128258, 128262]
    assert I.frame_voice_pairs([]) == []
    # the new text goes behind it in the ordinary prompt framing
    assert I.prompt_ids([9])[0] == two[0] and I.prompt_ids([9])[-4:] == two[2:6]
    for bad in ([([], [1])], [([1], [])]):
        with pytest.raises(ValueError):
            I.frame_voice_pairs(bad)


# ---- GpuPool -------------------------------------------------------------------------------
class PrefixService(FakeService):
    """FakeService with a prefix registry: a token stream that names a prefix echoes the
    prefix's ids (plus the device), so the test reads which registry the worker holds."""

    def __init__(self, device):
        super().__init__(device)
        self.reg = PrefixRegistry(range(100, 104))

    def register_prefix(self, name, ids):
        p, _ = self.reg.place(name, ids)
        p.ready = True
        return p

    def unregister_prefix(self, name):
        self.reg.remove(name)

    def submit_tokens(self, prompt_ids, max_tokens=None, prefix=None, **kw):
        if prefix is None:
            return super().submit_tokens(prompt_ids, max_tokens=max_tokens, **kw)
        p = self.reg.get(prefix)
        if p is None:
            raise UnknownPrefix(f"unknown prefix {prefix!r}")
        return FakeHandle([t + self.device for t in p.ids] + [p.slot])


def prefix_factory(device):
    return PrefixService(device)


def _tokens(h):
    out = []
    while True:
        t = h.get(timeout=60)
        if t is None:
            return out
        out.append(t)


def test_pool_registers_on_every_worker_and_replays_to_a_respawn():
    p = GpuPool(2, factory=prefix_factory, start_timeout=120, poll_s=0.1)
    try:
        assert p.register_prefix("ref", [10, 20]) == [0, 1]
        with pytest.raises(ValueError):
            p.submit_tokens([1], max_tokens=1, prefix="nobody")
        with pytest.raises(ValueError):
            p.register_prefix("", [1])
        # two streams on two workers (least loaded): both know the prefix
        a = p.submit_tokens([1], max_tokens=700, prefix="ref")
        b = p.submit_tokens([1], max_tokens=700, prefix="ref")
        assert (a.worker, b.worker) == (0, 1)
        assert _tokens(a) == [10, 20, 100] and _tokens(b) == [11, 21, 100]
        # worker 0 dies; its replacement is given the registry before it takes requests
        h = p.submit("die soon", "tara", max_tokens=7000)
        assert h.worker == 0
        with pytest.raises(RuntimeError, match="died"):
            while h.get(timeout=60) is not None:
                pass
        deadline = time.time() + 120
        while not p.alive[0] and time.time() < deadline:
            time.sleep(0.05)
        assert p.alive[0]
        c = p.submit_tokens([1], max_tokens=7, prefix="ref")
        assert c.worker == 0 and _tokens(c) == [10, 20, 100]
        assert not p.prefix_errors
        p.unregister_prefix("ref")
        with pytest.raises(ValueError):
            p.submit_tokens([1], max_tokens=1, prefix="ref")
    finally:
        p.close()
