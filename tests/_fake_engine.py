"""Recording fakes for ``BatchSynthesizer``'s loop (tests/test_batching_loop_host.py): an engine,
a SNAC decoder, streams, events and the staging ring, none of which needs a GPU or the built
library.  Every engine and SNAC call lands in one ordered log, so two versions of the loop can
be compared call for call.  ``scenarios()`` is the set the fixture
``tests/golden/batching_loop_trace.json`` was recorded from (tests/golden/
make_batching_loop_trace.py)."""
from __future__ import annotations

import dataclasses
import math
import types

import numpy as np

from project_morpheus_amd import _lib
from project_morpheus_amd import batching as B
from project_morpheus_amd.config import CUSTOM_TOKEN_BASE
from project_morpheus_amd.engine import SLICE_HI, SLICE_LO

DEFAULTS = dict(penalty=1.1, temperature=0.0, top_p=1.0, seed=0, top_k=0, min_p=0.0,
                penalty_last_n=0, grammar=False)


def hist_token(slot: int, pos: int) -> int:
    """The token the fake engine "generates" for ``slot`` at ``pos``."""
    return (slot * 37 + pos * 11 + 3) % 97


class _Hist:
    def __getitem__(self, key):
        slot, pos = key
        return hist_token(int(slot), int(pos))


class FakeStream:
    cuda_stream = 0

    def __init__(self, device=None):
        self.device = device

    def synchronize(self):
        pass


class FakeEvent:
    def record(self, stream=None):
        pass

    def query(self):
        return True

    def synchronize(self):
        pass


class FakeRing:
    """``_BatchRing`` with plain arrays; the ``*_dev`` pointers are the ring index + 1."""
    last = None

    def __init__(self, n: int, max_batch: int, max_frames: int):
        self.n, self.max_batch = n, max_batch
        self.codes = [np.zeros(max_batch * 7 * max_frames, np.int32) for _ in range(n)]
        self.seeds = [np.zeros(max_batch, np.uint64) for _ in range(n)]
        self.pcm = [np.zeros(max_batch * (SLICE_HI - SLICE_LO), np.int16) for _ in range(n)]
        self.codes_dev = self.seeds_dev = self.pcm_dev = [i + 1 for i in range(n)]
        FakeRing.last = self


class FakeSnac:
    def __init__(self, log, max_batch=4, max_frames=7):
        self.log, self.max_batch, self.max_frames = log, max_batch, max_frames

    def decode_ptr(self, frames_ptr, n_frames, batch, noise_ptr, seed, pcm_ptr, audio_ptr, lo, hi,
                   stream, seeds_ptr=0):
        ring, i = FakeRing.last, frames_ptr - 1
        self.log.append(["snac", n_frames, batch, lo, hi,
                         [int(s) for s in ring.seeds[i][:batch]],
                         int(ring.codes[i][:7 * n_frames * batch].sum())])


def _arg(what):
    return _lib.MxError(f"morpheus_mx error {_lib.MX_ERR_ARG}: {what}", _lib.MX_ERR_ARG)


class FakeEngine:
    """The attributes and methods the loop uses.  ``fail``: {method name: (k, rc)} makes the
    k-th call (from 0) of that method, or with k None every call, raise ``MxError(rc)`` after
    logging it.  ``POISON`` is an
    id the host checks pass and every prefill refuses: what only the device can see."""

    POISON = 95

    def __init__(self, max_slots=6, max_pos=64, max_batch=4, max_prefill=8, vocab=100,
                 fail=None):
        self.max_slots, self.max_pos, self.max_batch = max_slots, max_pos, max_batch
        self.max_prefill, self.device = max_prefill, 0
        self.cfg = types.SimpleNamespace(vocab=vocab)
        self.grammar = None
        self.hist = _Hist()
        self.log = []
        self.fail = dict(fail or {})
        self.calls = {}

    def _call(self, name, *args):
        self.log.append([name, *args])
        k = self.calls.get(name, 0)
        self.calls[name] = k + 1
        if name in self.fail and self.fail[name][0] in (k, None):
            rc = self.fail[name][1]
            raise _lib.MxError(f"morpheus_mx error {rc}: injected", rc)

    def _check_ids(self, slot, ids, pos0):
        if not 0 <= slot < self.max_slots:
            raise _arg("slot")
        if not 1 <= len(ids) <= self.max_prefill or pos0 < 0 or pos0 + len(ids) >= self.max_pos:
            raise _arg("length")
        if min(ids) < 0 or max(ids) >= self.cfg.vocab or self.POISON in ids:
            raise _arg("id out of vocab")

    def _check_params(self, row, p):
        ok = (0 <= row < self.max_batch
              and math.isfinite(p["penalty"]) and p["penalty"] > 0
              and math.isfinite(p["temperature"]) and p["temperature"] >= 0
              and 0 < p["top_p"] <= 1 and p["top_k"] >= 0 and 0 <= p["min_p"] <= 1
              and 0 <= p["penalty_last_n"] <= 255)
        if not ok:
            raise _arg("generation parameter")
        if p["grammar"] and self.grammar is None:
            raise _lib.MxError("no grammar", _lib.MX_ERR_STATE)

    @staticmethod
    def _params(kw):
        p = dict(DEFAULTS)
        p.update(kw)
        p["grammar"] = bool(p["grammar"])
        return p

    def prefill(self, slot, row, ids, penalty, stream, **kw):
        ids, p = [int(t) for t in ids], self._params(dict(kw, penalty=penalty))
        self._call("prefill", dict(slot=slot, row=row, ids=ids, **p))
        self._check_ids(slot, ids, 0)
        self._check_params(row, p)

    def prefill_batch(self, segments, stream):
        segs = []
        for s in segments:
            d = dataclasses.asdict(s) if dataclasses.is_dataclass(s) else dict(s)
            d = dict(self._params(d), ids=[int(t) for t in d["ids"]])
            d.setdefault("pos0", 0)
            segs.append(d)
        self._call("prefill_batch", segs)
        if not segs:
            raise _arg("empty pack")
        for d in segs:  # the whole pack is refused: nothing was enqueued
            self._check_ids(d["slot"], d["ids"], d["pos0"])
            self._check_params(d["row"], d)
        if sum(len(d["ids"]) for d in segs) > self.max_prefill:
            raise _arg("pack too long")

    def prefill_chunk(self, slot, ids, pos0, stream, *, last=False, row=None, **kw):
        ids = [int(t) for t in ids]
        if last:
            if row is None:
                raise ValueError("the final chunk needs a decode row")
            p = self._params(kw)
            self._call("prefill_chunk", dict(slot=slot, ids=ids, pos0=pos0, last=True, row=row, **p))
        else:
            self._call("prefill_chunk", dict(slot=slot, ids=ids, pos0=pos0, last=False))
        self._check_ids(slot, ids, pos0)
        if last:
            self._check_params(row, p)

    def fork_slot(self, dst, src, n_pos, stream):
        self._call("fork_slot", dst, src, n_pos)

    def fork_slots(self, pairs, stream):
        self._call("fork_slots", [[int(v) for v in p] for p in pairs])

    def decode(self, n_rows, stream):
        self._call("decode", n_rows)

    def check(self, stream):
        self._call("check")

    def release_row(self, row, stream):
        self._call("release_row", row)

    def move_row(self, dst, src, stream):
        self._call("move_row", dst, src)

    def set_grammar(self, grammar=None):
        self._call("set_grammar")
        if self.cfg.vocab < CUSTOM_TOKEN_BASE:  # the preset's ids do not fit this vocabulary
            raise _arg("grammar does not fit the vocabulary")
        self.grammar = grammar


def patch(monkeypatch):
    """The three names the loop creates its streams, events and staging through."""
    monkeypatch.setattr(B.torch.cuda, "Stream", FakeStream)
    monkeypatch.setattr(B.torch.cuda, "Event", FakeEvent)
    monkeypatch.setattr(B, "_BatchRing", FakeRing)


def make(llm_kw=None, **syn_kw):
    llm = FakeEngine(**(llm_kw or {}))
    syn_kw.setdefault("depth", 2)
    syn = B.BatchSynthesizer(llm, FakeSnac(llm.log), **syn_kw)
    return llm, syn


def req(ids, max_tokens=3, **kw):
    kw.setdefault("audio", False)
    kw.setdefault("stop_ids", ())
    return B.StreamRequest(prompt_ids=list(ids), max_tokens=max_tokens, arrival=0.0, **kw)


def ids(n, base=1):
    return [(base + 3 * i) % 90 for i in range(n)]


def audio_ids(n, salt):
    """Valid Orpheus audio ids (code in [1, 4095] at every phase)."""
    return [CUSTOM_TOKEN_BASE + 10 + 4096 * (i % 7) + 1 + (i * 131 + salt * 17) % 4095
            for i in range(n)]


def outcome(llm, syn, reqs, handles=(), raised=None):
    return {
        "calls": llm.log,
        "requests": [{"tokens": r.tokens, "error": type(r.error).__name__,
                      "samples": r.samples, "windows": r.windows} for r in reqs],
        "handles": [[h.done, type(h.error).__name__] for h in handles],
        "raised": type(raised).__name__,
        "counters": {k: sorted([str(a), b] for a, b in getattr(syn, k).items())
                     for k in ("prefill_packs", "prefix_packs", "prefix_forks", "prefix_fills",
                               "row_steps")},
        "prompt_chunks": syn.prompt_chunks,
    }


def run(llm, syn, reqs, handles=()):
    raised = None
    try:
        syn.run(reqs)
    except _lib.MxError as e:
        raised = e
    return outcome(llm, syn, reqs, handles, raised)


# ----------------------------------------------------------------------------------------------
def burst(packed):
    llm, syn = make(packed_prefill=packed, prefix_slots=2)
    h = syn.register_prefix("v", ids(5, 40))
    reqs = [req(ids(3)), req(ids(19, 2)), req(ids(3, 5), prefix="v"), req(ids(2, 7), prefix="v"),
            req([1, 100, 2]), req(ids(3), prefix="nobody"), req(ids(6, 9), max_tokens=5)]
    return run(llm, syn, reqs, [h])


def one_prefixed_in_pack():
    llm, syn = make(packed_prefill=True, prefix_slots=1)
    h = syn.register_prefix("v", ids(4, 30))
    return run(llm, syn, [req(ids(2)), req(ids(3, 4), prefix="v"), req(ids(2, 8))], [h])


def pack_refused():
    llm, syn = make(packed_prefill=True, prefix_slots=1)
    h = syn.register_prefix("v", ids(4, 30))
    reqs = [req(ids(2)), req(ids(2, 4), prefix="v"), req([3, FakeEngine.POISON]),
            req(ids(1, 6), prefix="v"), req(ids(2, 5), max_tokens=2)]
    return run(llm, syn, reqs, [h])


def pack_refused_by_state():
    """MX_ERR_STATE refuses a pack as MX_ERR_ARG does; every member then passes alone."""
    llm, syn = make(dict(fail={"prefill_batch": (0, _lib.MX_ERR_STATE)}), packed_prefill=True)
    return run(llm, syn, [req(ids(2)), req(ids(3, 4)), req(ids(2, 6))])


def long_suffix(packed):
    llm, syn = make(packed_prefill=packed, prefix_slots=1)
    h = syn.register_prefix("v", ids(11, 20))
    return run(llm, syn, [req(ids(13, 2), prefix="v"), req(ids(3))], [h])


def prefix_requeue():
    llm, syn = make(prefix_slots=1)
    hs = [syn.register_prefix("a", ids(17, 10)), syn.register_prefix("b", ids(3, 50))]
    reqs = [req(ids(2), prefix="a"), req(ids(2, 3), prefix="b"), req(ids(2, 6), prefix="a")]
    return run(llm, syn, reqs, hs)


def prefix_replace_unregister():
    llm, syn = make(prefix_slots=2)
    hs = [syn.register_prefix("a", ids(9, 10)), syn.register_prefix("a", ids(3, 60)),
          syn.register_prefix("c", ids(2, 70)), syn.register_prefix("", [1]),
          syn.register_prefix("big", ids(70))]
    reqs = [req(ids(2), prefix="a", max_tokens=6), req(ids(2, 3), prefix="c", max_tokens=4)]

    def gone(r, tok):  # from the loop thread, while both decode
        if len(r.tokens) == 2:
            hs.append(syn.unregister_prefix("c"))
            hs.append(syn.unregister_prefix("zz"))
    reqs[0].on_token = gone
    return run(llm, syn, reqs, hs)


def unregister_waiting():
    """More requests than rows: the one still waiting names a prefix that goes away."""
    llm, syn = make(dict(max_batch=2, max_slots=3), prefix_slots=1)
    hs = [syn.register_prefix("c", ids(2, 70))]
    reqs = [req(ids(2), max_tokens=4), req(ids(2, 3), prefix="c", max_tokens=4),
            req(ids(3, 5), prefix="c")]

    def gone(r, tok):
        if len(r.tokens) == 1:
            hs.append(syn.unregister_prefix("c"))
    reqs[0].on_token = gone
    return run(llm, syn, reqs, hs)


def cancel_in_callback(packed):
    llm, syn = make(packed_prefill=packed)
    reqs = [req(ids(3), max_tokens=9), req(ids(12, 2), max_tokens=9), req(ids(2, 4), max_tokens=4)]

    def barge(r, tok):
        if len(r.tokens) == 3:
            r.cancel()
            reqs[1].cancel()   # (mid-prompt or decoding, as the iteration has it)
    reqs[0].on_token = barge
    late = req(ids(2, 9))
    late.cancelled = True      # cancelled before admission
    return run(llm, syn, reqs + [late])


def clip_and_stop():
    llm, syn = make(dict(max_pos=16), depth=2)
    a = req(ids(7), max_tokens=40)                    # 16 - 7 = 9 tokens
    b = req(ids(3, 4), max_tokens=12, stop_ids=(hist_token(1, 3 + 4),))   # stops at its 5th token
    c = req(ids(14, 2), max_tokens=5)                 # chunked, limit 2
    d = req(ids(15, 1), max_tokens=5)                 # limit 1: parked as it is bound
    e = req(ids(16, 1), max_tokens=5)                 # does not fit
    return run(llm, syn, [a, b, c, d, e, req([])])


def grammar_wait():
    llm, syn = make(dict(vocab=CUSTOM_TOKEN_BASE + 7 * 4096 + 16))
    reqs = [req(ids(3), max_tokens=4), req(ids(2, 5), max_tokens=3, grammar=True),
            req(ids(2, 7), max_tokens=2), req(ids(9, 1), max_tokens=2, grammar=True)]
    return run(llm, syn, reqs)


def grammar_refused(packed):
    llm, syn = make(packed_prefill=packed)  # vocabulary 100: the preset cannot fit
    return run(llm, syn, [req(ids(3), grammar=True), req(ids(2, 5))])


def bad_params(packed):
    llm, syn = make(packed_prefill=packed, prefix_slots=1)
    h = syn.register_prefix("v", ids(3, 30))
    reqs = [req(ids(3), top_p=-1.0), req(ids(10, 2), top_k=-2), req(ids(2, 5), min_p=1.5),
            req(ids(2, 6), prefix="v", penalty=0.0), req(ids(2, 8), penalty_last_n=300),
            req(ids(3, 7), temperature=0.7, top_p=0.9, seed=2 ** 64 + 5, top_k=40, min_p=0.05,
                penalty_last_n=64, penalty=1.3), req(ids(3, 9), max_tokens=0)]
    return run(llm, syn, reqs, [h])


def device_failure(method, packed, k=0):
    llm, syn = make(dict(fail={method: (k, _lib.MX_ERR_HIP)}), packed_prefill=packed,
                    prefix_slots=1)
    h = syn.register_prefix("v", ids(3, 30)) if method == "fork_slot" else None
    reqs = [req(ids(3), 6), req(ids(11, 2), 6), req(ids(2, 5), 6, prefix="v" if h else None)]
    return run(llm, syn, reqs, [h] if h else [])


def audio_streams():
    llm, syn = make(dict(max_pos=256), snac_min_batch=3, snac_max_hold=4)
    reqs = [req(ids(4 + i), n, audio=True, inject_ids=audio_ids(n, i))
            for i, n in enumerate((60, 35, 9))]
    return run(llm, syn, reqs)


def audio_cancelled():
    llm, syn = make(dict(max_pos=256), snac_min_batch=2, snac_max_hold=2)
    reqs = [req(ids(4 + i), n, audio=True, inject_ids=audio_ids(n, 5 + i), noise_seed=77 * i or None)
            for i, n in enumerate((30, 44))]

    def barge(r, tok):
        if len(r.tokens) == 17:
            r.cancel()
    reqs[1].on_token = barge
    return run(llm, syn, reqs)


def compaction(compact):
    llm, syn = make(compact=compact)
    reqs = [req(ids(2), 2), req(ids(2, 3), 3), req(ids(2, 5), 12), req(ids(2, 7), 9),
            req(ids(2, 9), 4)]
    return run(llm, syn, reqs)


def scenarios():
    s = {}
    for p in (False, True):
        t = "packed" if p else "plain"
        s[f"burst_{t}"] = lambda p=p: burst(p)
        s[f"long_suffix_{t}"] = lambda p=p: long_suffix(p)
        s[f"cancel_in_callback_{t}"] = lambda p=p: cancel_in_callback(p)
        s[f"grammar_refused_{t}"] = lambda p=p: grammar_refused(p)
        s[f"bad_params_{t}"] = lambda p=p: bad_params(p)
        s[f"device_failure_chunk_{t}"] = lambda p=p: device_failure("prefill_chunk", p, 1)
        s[f"device_failure_decode_{t}"] = lambda p=p: device_failure("decode", p, 2)
    s["device_failure_prefill"] = lambda: device_failure("prefill", False)
    s["device_failure_prefill_batch"] = lambda: device_failure("prefill_batch", True)
    s["device_failure_fork_slot"] = lambda: device_failure("fork_slot", False)
    s["one_prefixed_in_pack"] = one_prefixed_in_pack
    s["pack_refused"] = pack_refused
    s["pack_refused_by_state"] = pack_refused_by_state
    s["prefix_requeue"] = prefix_requeue
    s["prefix_replace_unregister"] = prefix_replace_unregister
    s["unregister_waiting"] = unregister_waiting
    s["clip_and_stop"] = clip_and_stop
    s["grammar_wait"] = grammar_wait
    s["audio_streams"] = audio_streams
    s["audio_cancelled"] = audio_cancelled
    s["compact_on"] = lambda: compaction(True)
    s["compact_off"] = lambda: compaction(False)
    return s
