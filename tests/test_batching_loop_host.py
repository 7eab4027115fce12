"""``BatchSynthesizer``'s loop against recording fakes (tests/_fake_engine.py): the calls it makes
on the engine and the SNAC decoder, in order, and what every request ends with, are pinned by
``tests/golden/batching_loop_trace.json``.  No GPU and no built library are needed: the loop
creates its streams, events and staging through ``torch.cuda.Stream``, ``torch.cuda.Event`` and
``batching._BatchRing``, and those three names are replaced."""
import json
import os

import pytest

import _fake_engine as F
from project_morpheus_amd import _lib
from project_morpheus_amd import batching as B

with open(os.path.join(os.path.dirname(__file__), "golden", "batching_loop_trace.json")) as _fh:
    GOLDEN = json.load(_fh)
SCENARIOS = F.scenarios()


@pytest.fixture(autouse=True)
def fakes(monkeypatch):
    F.patch(monkeypatch)


def test_fixture_and_scenarios_name_the_same_cases():
    assert sorted(GOLDEN) == sorted(SCENARIOS)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_loop_trace(name):
    got = json.loads(json.dumps(SCENARIOS[name]()))
    want = GOLDEN[name]
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"{name}: call {i} differs"
    assert len(got["calls"]) == len(want["calls"])
    assert got == want


def test_trace_is_repeatable():
    name = "burst_packed"
    assert SCENARIOS[name]() == SCENARIOS[name]()


def test_the_scenarios_reach_what_they_are_for():
    """The fixture itself: each branch a scenario exists for shows in its recorded trace."""
    def names(case):
        return [c[0] for c in GOLDEN[case]["calls"]]

    def errors(case):
        return [r["error"] for r in GOLDEN[case]["requests"]]
    assert errors("burst_plain") == ["NoneType"] * 4 + ["MxError", "UnknownPrefix", "NoneType"]
    assert errors("burst_packed") == ["NoneType"] * 4 + ["ValueError", "UnknownPrefix", "NoneType"]
    assert "fork_slots" in names("burst_packed") and "fork_slots" not in names("burst_plain")
    one = names("one_prefixed_in_pack")
    assert "fork_slot" in one and "fork_slots" not in one and "prefill_batch" in one
    ref = names("pack_refused")
    assert ref.index("prefill_batch") < ref.index("prefill") and "fork_slot" in ref
    assert errors("pack_refused") == ["NoneType"] * 2 + ["MxError"] + ["NoneType"] * 2
    assert names("grammar_wait").count("set_grammar") == 1
    assert errors("grammar_refused_plain") == ["MxError", "NoneType"]
    for t in ("plain", "packed"):
        assert errors(f"bad_params_{t}") == ["ValueError"] * 5 + ["NoneType", "ValueError"]
        for m in ("chunk", "decode"):
            assert GOLDEN[f"device_failure_{m}_{t}"]["raised"] == "MxError"
    for m in ("prefill", "prefill_batch", "fork_slot"):
        assert GOLDEN[f"device_failure_{m}"]["raised"] == "MxError"
    assert "move_row" in names("compact_on") and "move_row" not in names("compact_off")
    assert [r["samples"] > 0 for r in GOLDEN["audio_streams"]["requests"]] == [True] * 3
    assert [h[1] for h in GOLDEN["prefix_requeue"]["handles"]] == ["NoneType", "NoneType"]
    stop = GOLDEN["clip_and_stop"]["requests"]
    assert [len(r["tokens"]) for r in stop] == [9, 5, 2, 1, 0, 0]


# ---------------------------------------------------------------------------------------------
# the online driver (start / submit / stop) is paced by a thread: outcomes only

def _tokens(slot_of, reqs):
    return [[F.hist_token(slot_of[i], len(r.prompt_ids) + k) for k in range(r.max_tokens)]
            for i, r in enumerate(reqs)]


def test_online_handles_complete_with_their_tokens():
    llm, syn = F.make(dict(max_batch=2, max_slots=2))
    reqs = [F.req(F.ids(3 + i), 4 + i) for i in range(5)]
    try:
        handles = [syn.submit(r) for r in reqs]
        got = []
        for h in handles:
            toks = []
            while True:
                t = h.get(timeout=30)
                if t is None:
                    break
                toks.append(t)
            got.append(toks)
    finally:
        syn.stop()
    for r, toks in zip(reqs, got):
        assert r.error is None and toks == r.tokens and len(toks) == r.max_tokens
        # (which slot a stream got depends on the thread's pacing; its tokens are that slot's)
        assert toks in ([F.hist_token(s, len(r.prompt_ids) + k) for k in range(r.max_tokens)]
                        for s in range(2))
    assert syn.outstanding_tokens == 0
    assert syn._live == []


def test_online_audio_stream_and_prefix():
    llm, syn = F.make(dict(max_pos=256), prefix_slots=1, snac_min_batch=2)
    try:
        syn.start()
        assert syn.register_prefix("v", F.ids(11, 20)).result(timeout=30) == "v"
        a = syn.submit(F.req(F.ids(4), 30, audio=True, inject_ids=F.audio_ids(30, 1)))
        t = syn.submit(F.req(F.ids(3, 2), 5, prefix="v"))
        n = sum(len(c) for c in a.chunks())
        toks = list(iter(lambda: t.get(timeout=30), None))
    finally:
        syn.stop()
    assert n == 2 * a.req.samples > 0 and a.req.windows > 0
    assert len(toks) == 5 and t.req.error is None
    assert syn.prefix_forks["v"] == 1 and syn.outstanding_tokens == 0


def test_online_device_failure_fails_every_handle():
    llm, syn = F.make(dict(max_batch=2, max_slots=3, max_pos=1 << 20), prefix_slots=1)
    # (the loop thread ends with the device's error, as it should: keep it out of the report)
    B.threading.excepthook, hook = (lambda a: None), B.threading.excepthook
    try:
        handles = [syn.submit(F.req(F.ids(3 + i), 1 << 19)) for i in range(2)]
        ph = syn.register_prefix("v", F.ids(30, 2))
        llm.fail = {"decode": (None, _lib.MX_ERR_HIP)}  # both streams are still decoding
        for h in handles:
            with pytest.raises(_lib.MxError):
                while h.get(timeout=30) is not None:
                    pass
        assert ph.wait(timeout=30)
        with pytest.raises(RuntimeError):
            syn.submit(F.req(F.ids(2)))
        late = syn.register_prefix("w", F.ids(3))
    finally:
        syn.stop()
        B.threading.excepthook = hook
    assert ph.done and (ph.error is None or isinstance(ph.error, _lib.MxError))
    assert all(isinstance(h.req.error, _lib.MxError) for h in handles)
    assert not late.done or late.error is not None
