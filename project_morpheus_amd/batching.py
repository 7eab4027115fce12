"""Continuous batching of concurrent utterance streams on one GPU (BASELINE configs 3-5, and
the serving path behind every adapter).

The reference serves concurrent requests by handing them to vLLM's continuous-batching
engine, one request per thread (Orpheus-TTS/orpheus_tts_pypi/orpheus_tts/engine_class.py:
114-134), and decodes each stream's SNAC windows independently (speechpipe.py:191-293).
``BatchSynthesizer`` is that loop for the MI355X engine:

* every stream owns one KV slot and one decode row; a step decodes rows [0, n_rows) at once
  (``mx_llm_decode(n_rows)``: one hipGraph per row count, the one-launch step for one row),
  rows without a stream are parked on the scratch slot; each row decodes under its own
  generation parameters (penalty and its window, temperature, top-k, min-p, top-p, seed:
  per-slot state set at prefill);
* rows are compacted: when a stream ends, the highest live row moves into the lowest free
  one (``mx_llm_move_row``: same KV slot, stream-ordered between steps), so a step runs the
  row class of the live stream count, not of the highest row index ever used;
* a stream is admitted as soon as it has arrived and a row is free: its prefill is enqueued
  between steps (ordered on the same HIP stream, nothing drains);
* ``depth`` steps stay queued on the GPU; tokens are read from the host-mapped history when
  a step's event completes, never by a per-token copy;
* a stream that has issued all its tokens is parked at once (its position never runs past
  ``max_pos``); a cancelled stream (``StreamRequest.cancel``, the adapter's ``reset``) frees
  its row at the next iteration and its undelivered audio is dropped;
* each stream keeps the reference window schedule (``schedule.WindowScheduler``); the
  windows that become due in one host iteration are grouped by frame count and decoded by
  ONE batched SNAC call per group on a second HIP stream, PCM read from host-mapped memory.
  NoiseBlock noise of window j of a stream is drawn from (stream noise seed, j) only, so a
  stream's audio does not depend on what it was batched with.

Two drivers share the loop: ``run(requests)`` (offline: arrival times, bench / long-form
jobs) and ``start()`` + ``submit(request) -> StreamHandle`` (online: the per-GPU service the
adapters use; a background thread owns the GPU).  One run of it is a ``_Loop``: the run's state
and, as methods, the steps ``iterate`` calls in order: poll, cancellations, control,
advance_prefixes, admit, advance_prompts, compact, issue, collect, windows, drain, announce.  A
request passes admission as an ``_Admission`` and reaches the engine as ``request_segment`` of it.
"""
from __future__ import annotations

import collections
import queue
import threading
import time
from collections import deque
from dataclasses import dataclass, field
from typing import Callable, Deque, Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .config import (BATCH_DEPTH, ORPHEUS_GRAMMAR, SNAC_MAX_HOLD, SNAC_MIN_BATCH, STOP_IDS,
                     packed_prefill_default)
from .engine import (SAMPLES_PER_FRAME, SLICE_HI, SLICE_LO, LlmEngine, PrefillSegment,
                     SnacDecoder)
from .schedule import WindowScheduler, code_of_id, frames_for_slice, window_seed


@dataclass(eq=False)
class StreamRequest:
    prompt_ids: Sequence[int]
    max_tokens: int
    arrival: float = 0.0                    # seconds after run start (offline driver)
    inject_ids: Optional[Sequence[int]] = None  # synthetic audio ids (bench, random weights)
    stop_ids: Sequence[int] = STOP_IDS
    penalty: float = 1.1
    temperature: float = 0.0                # <= 0: greedy (the parity mode)
    top_p: float = 1.0
    seed: int = 0                           # sampling stream (Philox key)
    top_k: int = 0                          # 0: no limit
    min_p: float = 0.0                      # 0: off
    penalty_last_n: int = 0                 # 0: penalty over the whole sequence; N <= 255
    grammar: bool = False                   # decode under the Orpheus code grammar
    noise_seed: Optional[int] = None        # SNAC noise stream (None: assigned at admission)
    on_chunk: Optional[Callable[["StreamRequest", bytes], None]] = None
    on_done: Optional[Callable[["StreamRequest"], None]] = None
    on_token: Optional[Callable[["StreamRequest", int], None]] = None
    audio: bool = True                      # False: token stream only (no SNAC windows)
    prefix: Optional[str] = None            # a registered prefix (register_prefix): prompt_ids
                                            # is then the suffix behind it
    # filled in by the synthesizer
    tokens: List[int] = field(default_factory=list)
    pcm: List[bytes] = field(default_factory=list)  # for callers that collect chunks here
    samples: int = 0
    windows: int = 0
    cancelled: bool = False
    error: Optional[BaseException] = None
    t_admit: Optional[float] = None
    t_first_audio: Optional[float] = None
    t_done: Optional[float] = None

    @property
    def audio_seconds(self) -> float:
        return self.samples / 24000.0

    @property
    def first_audio_ms(self) -> Optional[float]:
        if self.t_first_audio is None:
            return None
        return 1e3 * (self.t_first_audio - self.arrival)

    def cancel(self) -> None:
        """Barge-in: the loop frees the row at its next iteration, nothing more is emitted."""
        self.cancelled = True


def check_params(penalty: float, temperature: float, top_p: float, max_tokens: int, *,
                 top_k: Optional[int] = None, min_p: Optional[float] = None,
                 penalty_last_n: Optional[int] = None) -> None:
    """Reject generation parameters the device cannot run (mx_llm_prefill_ex returns
    MX_ERR_ARG for them): a bad request must fail alone, at submit time, never inside the GPU
    loop."""
    import math
    if top_k is not None and (isinstance(top_k, bool) or not isinstance(top_k, int)
                              or not 0 <= top_k < 2 ** 31):
        raise ValueError(f"top_k must be an integer >= 0, got {top_k!r}")
    if min_p is not None and (isinstance(min_p, bool) or not isinstance(min_p, (int, float))
                              or not 0 <= min_p <= 1):  # (NaN fails the comparison)
        raise ValueError(f"min_p must be in [0, 1], got {min_p!r}")
    if penalty_last_n is not None and (isinstance(penalty_last_n, bool)
                                       or not isinstance(penalty_last_n, int)
                                       or not 0 <= penalty_last_n <= 255):
        raise ValueError(f"penalty_last_n must be an integer in [0, 255], got {penalty_last_n!r}")
    for name, v in (("repetition_penalty", penalty), ("temperature", temperature),
                    ("top_p", top_p)):
        if not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
    if penalty <= 0:
        raise ValueError(f"repetition_penalty must be > 0, got {penalty}")
    if temperature < 0:
        raise ValueError(f"temperature must be >= 0, got {temperature}")
    if not 0 < top_p <= 1:
        raise ValueError(f"top_p must be in (0, 1], got {top_p}")
    if not isinstance(max_tokens, int) or max_tokens < 1:
        raise ValueError(f"max_tokens must be a positive integer, got {max_tokens!r}")


class UnknownPrefix(ValueError):
    """A request names a prefix nobody registered (HTTP 400 on the completions surface)."""


def check_prefix(prefix) -> None:
    """A request's ``prefix`` is None or the non-empty name of a registered prefix (whether it
    is registered is the loop's to say: an unknown name fails that request alone)."""
    if prefix is not None and (not isinstance(prefix, str) or not prefix):
        raise ValueError(f"prefix must be a non-empty string, got {prefix!r}")


def request_segment(req: StreamRequest, slot: int, row: int, pos0: int = 0) -> PrefillSegment:
    """``req``'s prompt and generation parameters as the engine takes them (spelt out here only)."""
    return PrefillSegment(slot=slot, row=row, ids=req.prompt_ids, penalty=req.penalty,
                          temperature=req.temperature, top_p=req.top_p, seed=req.seed,
                          top_k=req.top_k, min_p=req.min_p, penalty_last_n=req.penalty_last_n,
                          grammar=bool(req.grammar), pos0=pos0)


def check_request(req: StreamRequest, vocab: Optional[int] = None) -> None:
    """ValueError for what the device would refuse: ``check_params`` of the request and, given
    ``vocab``, the range of its prompt ids (without it the device checks them)."""
    kw = request_segment(req, -1, -1).keywords()
    del kw["seed"], kw["grammar"]  # (nothing to check on the host)
    check_params(max_tokens=req.max_tokens, **kw)
    if vocab is not None:
        ids = np.asarray(req.prompt_ids, dtype=np.int64)
        if ids.min() < 0 or ids.max() >= vocab:
            raise ValueError("prompt id out of vocab")


class _Row:
    """One stream's decode state; ``idx`` is the device row it decodes in (rows are compacted,
    so it can change), ``slot`` its KV slot (fixed for the stream's life)."""

    def __init__(self, idx: int):
        self.idx = idx
        self.slot = -1
        self.req: Optional[StreamRequest] = None
        self.sched: Optional[WindowScheduler] = None
        self.n0 = 0          # prompt length (position of generated token 0)
        self.issued = 0      # generated tokens whose step has been enqueued
        self.limit = 0       # tokens this row may issue (max_tokens clipped to max_pos)
        self.parked = False  # released on the device (all tokens issued / stopped)
        self.stopped = False
        # mid-prompt (a long or prefixed prompt): [positions the slot holds before prompt_ids,
        # the chunks still to enqueue]; the row is reserved and stays parked until the final one
        self.prompt: Optional[list] = None

    def reserve(self, req: StreamRequest, slot: int, n0: int) -> None:
        """Mid-prompt: the row is taken and stays parked on the device until the final chunk."""
        self.slot, self.req, self.sched, self.n0 = slot, req, None, n0
        self.stopped, self.parked = False, True

    def bind(self, req: StreamRequest, slot: int, n0: int, max_pos: int) -> None:
        """The prompt is on the device: the row decodes from the next step on."""
        self.slot, self.req, self.sched, self.n0 = slot, req, WindowScheduler(), n0
        self.limit = max(1, min(req.max_tokens, max_pos - n0))
        self.issued, self.stopped, self.parked, self.prompt = 1, False, False, None

    def clear(self) -> None:
        """The stream is gone (ended, cancelled or refused): the row is free."""
        self.req, self.sched, self.slot, self.prompt = None, None, -1, None
        self.stopped, self.parked = False, False


def plan_compaction(rows: List[_Row]) -> List[Tuple[int, int]]:
    """Row compaction plan, applied to ``rows`` in place: while a free row (no stream) sits
    below the highest row still decoding, that row's stream moves into the lowest free row.
    Returns the device moves (dst, src) in order (``mx_llm_move_row``).  ``rows[i].idx == i``
    holds before and after; a stream keeps its KV slot, so host reads by slot are unaffected,
    and the steps already queued for the old row index run before the move on the stream.
    Rows that are parked (all tokens issued) or stopped stay where they are: they decode no
    more steps, so they never set the row class."""
    moves = []
    while True:
        free = [r for r in rows if r.req is None]
        live = [r for r in rows if r.req is not None and not r.stopped and not r.parked]
        if not free or not live:
            return moves
        lo, hi = free[0], live[-1]
        if lo.idx > hi.idx:
            return moves
        i, j = lo.idx, hi.idx
        moves.append((i, j))
        rows[i], rows[j] = hi, lo
        hi.idx, lo.idx = i, j


# Packed continuation: a pack takes its prefixed members (one ``fork_slots``, their suffixes in
# the pack's ``prefill_batch``) only from this many of them; fewer take the chunked path
# (``fork_slot`` + ``prefill_chunk`` each).  Set from profiles/packed_continuation_time.log:
# the smallest k at which the packed arm's total beats the chunked arm's by more than the
# chunked arm's own spread (DESIGN.md §7 "Packed continuation").
PREFIX_PACK_MIN = 2


def plan_prefill_packs(lengths: Sequence[int], max_prefill: int, max_k: int) -> List[List[int]]:
    """Packs of a burst of prompts for ``LlmEngine.prefill_batch``: indices into ``lengths`` in
    arrival order, never reordered.  A pack is filled greedily and closed by the first prompt
    that would take it past ``max_prefill`` rows or ``max_k`` streams.  (A prompt longer than
    ``max_prefill`` lands in a pack of its own: refusing it is the caller's business.)"""
    packs: List[List[int]] = []
    cur: List[int] = []
    rows = 0
    for i, n in enumerate(lengths):
        if cur and (rows + n > max_prefill or len(cur) >= max_k):
            packs.append(cur)
            cur, rows = [], 0
        cur.append(i)
        rows += n
    if cur:
        packs.append(cur)
    return packs


def plan_prompt_chunks(n: int, pos0: int, max_prefill: int) -> List[Tuple[int, int, bool]]:
    """Chunks of ``n`` prompt ids that go behind the ``pos0`` positions a slot already holds, for
    ``LlmEngine.prefill_chunk``: ``(offset, length, last)`` in order, ``offset`` into the ids (the
    chunk's ``pos0`` is ``pos0 + offset``).  Every chunk but the last is ``max_prefill`` long;
    only the last is marked."""
    if n < 1 or pos0 < 0 or max_prefill < 1:
        raise ValueError(f"bad chunk plan: n {n}, pos0 {pos0}, max_prefill {max_prefill}")
    out = []
    for off in range(0, n, max_prefill):
        length = min(max_prefill, n - off)
        out.append((off, length, off + length == n))
    return out


class PrefixHandle:
    """Outcome of ``register_prefix`` / ``unregister_prefix``: completes once the loop thread has
    enqueued the prefix (every later request is ordered behind it) or refused it."""

    def __init__(self, name: str):
        self.name = name
        self.error: Optional[BaseException] = None
        self._ev = threading.Event()

    def _finish(self, error: Optional[BaseException] = None) -> None:
        self.error = error
        self._ev.set()

    @property
    def done(self) -> bool:
        return self._ev.is_set()

    def wait(self, timeout: Optional[float] = None) -> bool:
        return self._ev.wait(timeout)

    def result(self, timeout: Optional[float] = None) -> str:
        """The prefix's name once it is registered; raises what refused it."""
        if not self._ev.wait(timeout):
            raise TimeoutError(f"prefix {self.name!r} not registered yet")
        if self.error is not None:
            raise self.error
        return self.name


class _Prefix:
    def __init__(self, name: str, slot: int, ids: Sequence[int]):
        self.name, self.slot, self.ids, self.n = name, slot, list(ids), len(ids)
        self.ready = False        # every chunk enqueued: requests may fork it
        self.pins = 0             # requests in admission that named it
        self.plan: Deque = deque()
        self.handle: Optional[PrefixHandle] = None


@dataclass
class _Admission:
    """A request on its way into ``row``: its KV slot is taken, its prefix (if any) pinned."""
    row: _Row
    req: StreamRequest
    slot: int
    n0: int                      # prompt length, the prefix's included
    prefix: Optional[_Prefix] = None


_HOLD = object()  # (admission) the request went back first in line


class PrefixRegistry:
    """Names -> template KV slots, least recently used first.  Pure host bookkeeping: the caller
    prefills and forks."""

    def __init__(self, slots: Sequence[int]):
        self.free: List[int] = sorted(slots)
        self.entries: "collections.OrderedDict[str, _Prefix]" = collections.OrderedDict()

    def __contains__(self, name) -> bool:
        return name in self.entries

    def __len__(self) -> int:
        return len(self.entries)

    def get(self, name, touch: bool = True) -> Optional[_Prefix]:
        p = self.entries.get(name)
        if p is not None and touch:
            self.entries.move_to_end(name)
        return p

    def place(self, name: str, ids: Sequence[int]) -> Tuple[_Prefix, Optional[_Prefix]]:
        """A template slot for ``name`` -> (its new entry, the entry it displaced or None): the
        name's own slot if it is registered already, else a free one, else that of the least
        recently used prefix that is ready and that no request in admission names.  RuntimeError
        when there is none."""
        old = self.entries.pop(name, None)
        if old is not None:
            slot = old.slot
        elif self.free:
            slot = self.free.pop(0)
        else:
            old = next((p for p in self.entries.values() if p.ready and p.pins == 0), None)
            if old is None:
                raise RuntimeError("no template slot for a prefix "
                                   f"({len(self.entries)} registered, none can be evicted)")
            del self.entries[old.name]
            slot = old.slot
        p = _Prefix(name, slot, ids)
        self.entries[name] = p
        return p, old

    def remove(self, name: str) -> Optional[_Prefix]:
        p = self.entries.pop(name, None)
        if p is not None:
            self.free.append(p.slot)
            self.free.sort()
        return p


class _BatchRing:
    """Host-mapped staging for batched SNAC calls: codes and noise seeds in, PCM16 out."""

    def __init__(self, n: int, max_batch: int, max_frames: int):
        self.n, self.max_batch = n, max_batch
        self.cbytes = max_batch * 7 * max_frames * 4
        self.sbytes = max_batch * 8
        self.pbytes = max_batch * (SLICE_HI - SLICE_LO) * 2
        per = (self.cbytes + self.sbytes + self.pbytes + 255) // 256 * 256
        self.buf = _lib.HostBuffer(n * per)
        self.codes = [self.buf.view(np.int32, max_batch * 7 * max_frames, i * per)
                      for i in range(n)]
        self.seeds = [self.buf.view(np.uint64, max_batch, i * per + self.cbytes)
                      for i in range(n)]
        self.pcm = [self.buf.view(np.int16, max_batch * (SLICE_HI - SLICE_LO),
                                  i * per + self.cbytes + self.sbytes) for i in range(n)]
        self.codes_dev = [self.buf.dev_ptr(i * per) for i in range(n)]
        self.seeds_dev = [self.buf.dev_ptr(i * per + self.cbytes) for i in range(n)]
        self.pcm_dev = [self.buf.dev_ptr(i * per + self.cbytes + self.sbytes) for i in range(n)]


class StreamHandle:
    """Online stream: PCM chunks arrive through a queue filled by the loop thread (never
    blocks the loop: the queue is unbounded, one utterance is at most ~1 MB of PCM)."""

    _END = object()

    def __init__(self, req: StreamRequest):
        self.req = req
        self._q: "queue.Queue" = queue.Queue()

    def _chunk(self, req, data: bytes) -> None:
        self._q.put(data)

    def _done(self, req) -> None:
        self._q.put(self._END)

    def get(self, timeout: Optional[float] = None):
        """Next PCM chunk, or None at the end of the stream; re-raises a loop failure."""
        item = self._q.get(timeout=timeout)
        if item is self._END:
            self._q.put(self._END)  # the end stays visible to later calls
            if self.req.error is not None:
                raise self.req.error
            return None
        return item

    def chunks(self) -> Iterator[bytes]:
        while True:
            c = self.get()
            if c is None:
                return
            yield c

    def cancel(self) -> None:
        self.req.cancel()


class TokenHandle(StreamHandle):
    """Online token-only stream (the /v1/completions surface): ``get`` -> token id | None."""

    def _token(self, req, tok: int) -> None:
        self._q.put(tok)


class BatchSynthesizer:
    def __init__(self, llm: LlmEngine, snac: SnacDecoder, depth: Optional[int] = None, seed: int = 0,
                 snac_min_batch: Optional[int] = None, snac_max_hold: Optional[int] = None,
                 compact: bool = True, packed_prefill: Optional[bool] = None,
                 prefix_slots: int = 0):
        if llm.max_slots - prefix_slots < llm.max_batch or prefix_slots < 0:
            raise ValueError("BatchSynthesizer needs one KV slot per decode row"
                             + (f" below its {prefix_slots} template slots" if prefix_slots else ""))
        self.llm, self.snac, self.seed = llm, snac, seed
        # prefix cache: the engine's last `prefix_slots` KV slots hold registered prefixes
        # (templates); a request naming one starts as a fork of it
        self.prefix_slots = prefix_slots
        self.prefixes = PrefixRegistry(range(llm.max_slots - prefix_slots, llm.max_slots))
        self.prefix_fills = collections.Counter()   # times a name's prefix was prefilled
        self.prefix_forks = collections.Counter()   # requests started from a name's prefix
        self.prompt_chunks = 0                      # prefill_chunk calls of long / prefixed prompts
        self._ctl: Deque = deque()                  # (op, name, ids, handle) for the loop thread
        self.compact = compact  # row compaction (mx_llm_move_row) when streams end
        self.row_steps = collections.Counter()  # decode steps issued per row count (stats)
        # packed prefill: the requests one iteration admits go through LlmEngine.prefill_batch,
        # one pass over the weights per pack (None: MORPHEUS_MX_PACKED_PREFILL, off when unset)
        self.packed_prefill = packed_prefill_default() if packed_prefill is None \
            else bool(packed_prefill)
        self.prefill_packs = collections.Counter()  # prefill_batch calls per stream count
        self.prefix_packs = collections.Counter()   # ... of them, with a member behind a prefix
        self.depth = max(1, BATCH_DEPTH if depth is None else depth)
        # SNAC window coalescing: due windows are held until `snac_min_batch` of them are
        # ready or the oldest has waited `snac_max_hold` decode steps (a stream's first window
        # and closing streams' windows go at once).  Staggered streams make ~streams / 7
        # windows due per step; a bigger SNAC batch costs less per window.
        self.snac_min_batch = max(1, SNAC_MIN_BATCH if snac_min_batch is None else snac_min_batch)
        self.snac_max_hold = max(0, SNAC_MAX_HOLD if snac_max_hold is None else snac_max_hold)
        self.stream = torch.cuda.Stream(llm.device)
        self.snac_stream = torch.cuda.Stream(llm.device)
        self.ring = _BatchRing(16, snac.max_batch, snac.max_frames)
        self._calls = 0
        self._admitted = 0
        self._live: List[StreamRequest] = []
        # online driver
        self._inbox: Deque[StreamRequest] = deque()
        self._cv = threading.Condition()
        self._thread: Optional[threading.Thread] = None
        self._stop = False
        self._t0 = time.perf_counter()
        self.outstanding_tokens = 0  # tokens still owed to submitted streams (dispatch load)

    def run(self, requests: List[StreamRequest], on_chunk=None) -> float:
        """Serve ``requests`` (admitted in arrival order) to completion; returns wall seconds.
        ``on_chunk(request, pcm_bytes)`` is called for every non-empty PCM chunk in order."""
        waiting: Deque[StreamRequest] = deque(sorted(requests, key=lambda r: r.arrival))
        if on_chunk is not None:
            for r in waiting:
                r.on_chunk = r.on_chunk or on_chunk
        n, done = len(waiting), []   # (done: the requests that have ended)
        t0 = time.perf_counter()

        def poll(now):
            out = []
            while waiting and waiting[0].arrival <= now:
                out.append(waiting.popleft())
            return out

        def idle(now):
            if waiting:
                time.sleep(max(0.0, min(0.001, waiting[0].arrival - now)))

        self._loop(t0, poll, idle, lambda: len(done) >= n and not waiting, done.append)
        return time.perf_counter() - t0

    def start(self) -> "BatchSynthesizer":
        """Online mode: a daemon thread owns the GPU and serves ``submit``-ted streams."""
        if self._thread is None:
            self._t0 = time.perf_counter()
            self._stop = False
            self._thread = threading.Thread(target=self._serve, name="mx-batch", daemon=True)
            self._thread.start()
        return self

    def submit(self, req: StreamRequest) -> StreamHandle:
        check_request(req)
        check_prefix(req.prefix)
        if self._thread is None:
            self.start()
        h = StreamHandle(req) if req.audio else TokenHandle(req)
        req.on_chunk, req.on_done = h._chunk, h._done
        if not req.audio:
            req.on_token = h._token
        req.arrival = time.perf_counter() - self._t0
        with self._cv:
            if self._stop:
                raise RuntimeError("BatchSynthesizer stopped")
            self._inbox.append(req)
            self.outstanding_tokens += req.max_tokens
            self._cv.notify()
        return h

    def register_prefix(self, name: str, ids: Sequence[int]) -> PrefixHandle:
        """Prefill ``ids`` once into a template slot under ``name`` (replacing an earlier prefix
        of that name); requests with ``StreamRequest.prefix == name`` then start as a fork of it.
        Goes through the loop thread like a request, chunked like a long prompt; with no free
        template slot the least recently used prefix is evicted.  The handle completes, or
        carries the error."""
        h = PrefixHandle(name)
        try:
            if not isinstance(name, str) or not name:
                raise ValueError(f"prefix name must be a non-empty string, got {name!r}")
            ids = [int(t) for t in ids]
            if self.prefix_slots < 1:
                raise ValueError("no template slots (prefix_slots is 0)")
            if not 1 <= len(ids) < self.llm.max_pos - 1:
                raise ValueError(f"prefix of {len(ids)} ids does not fit (max_pos "
                                 f"{self.llm.max_pos}: it needs room for a suffix and a token)")
            if min(ids) < 0 or max(ids) >= self.llm.cfg.vocab:
                raise ValueError("prefix id out of vocab")
        except (TypeError, ValueError) as e:
            h._finish(e)
            return h
        with self._cv:
            self._ctl.append(("register", name, ids, h))
            self._cv.notify()
        return h

    def has_prefix(self, name) -> bool:
        """``name`` is registered, or its registration is on its way to the loop thread."""
        with self._cv:
            return name in self.prefixes or any(op == "register" and n == name
                                                for op, n, _, _ in self._ctl)

    def unregister_prefix(self, name: str) -> PrefixHandle:
        h = PrefixHandle(name)
        with self._cv:
            self._ctl.append(("unregister", name, None, h))
            self._cv.notify()
        return h

    def stop(self) -> None:
        with self._cv:
            self._stop = True
            self._cv.notify()
        if self._thread is not None:
            self._thread.join()
            self._thread = None

    def _serve(self) -> None:
        def poll(now):
            with self._cv:
                out = list(self._inbox)
                self._inbox.clear()
            return out

        def idle(now):
            with self._cv:
                if not self._inbox and not self._ctl and not self._stop:
                    self._cv.wait(timeout=0.05)

        def done_cb(req):
            with self._cv:
                self.outstanding_tokens -= req.max_tokens

        try:
            self._loop(self._t0, poll, idle, lambda: self._stop, done_cb)
        except BaseException as e:  # fail every stream loudly, never hang a consumer
            with self._cv:
                self._stop = True
                orphans = list(self._inbox) + list(self._live)
                self._inbox.clear()
                ctl = list(self._ctl)
                self._ctl.clear()
            for _, _, _, h in ctl:
                h._finish(e)
            for p in self.prefixes.entries.values():
                if p.handle is not None and not p.handle.done:
                    p.handle._finish(e)
            for req in orphans:
                req.error = e
                if req.on_done is not None:
                    req.on_done(req)
            raise

    def _loop(self, t0: float, poll, idle, finished, done_cb) -> None:
        _Loop(self, t0, poll, idle, finished, done_cb).run()


class _Loop:
    """One run of ``BatchSynthesizer``'s loop: its state, and the steps of ``iterate`` as methods.
    ``syn`` keeps what outlives a run: engine, streams, staging, prefixes and the counters."""

    def __init__(self, syn: BatchSynthesizer, t0: float, poll, idle, finished, done_cb):
        self.syn, self.llm, self.stream = syn, syn.llm, syn.stream
        self.t0, self.poll_fn, self.idle = t0, poll, idle
        self.finished, self.done_cb = finished, done_cb
        self.rows = [_Row(i) for i in range(syn.llm.max_batch)]
        self.free_slots = set(range(syn.llm.max_slots - syn.prefix_slots))  # (templates sit above)
        self.waiting: Deque[StreamRequest] = deque()
        self.inflight: Deque = deque()   # (event, [(row, req, k)])
        self.pending: Deque = deque()    # (event, ring index, [(req, nbytes)])
        self.closing: Deque = deque()    # streams whose end waits for their last SNAC call
        self.held: List = []             # due SNAC windows not launched yet (coalescing)
        self.held_age = 0                # decode steps the oldest held window has waited

    def now(self) -> float:
        return time.perf_counter() - self.t0

    def run(self) -> None:
        while self.iterate():
            pass
        for e, _ in self.inflight:
            e.synchronize()

    def iterate(self) -> bool:
        """One iteration; False once the driver has finished and nothing is left to serve."""
        self.poll()
        self.cancellations()
        self.control()
        busy = self.advance_prefixes()
        self.admit()
        busy = self.advance_prompts() or busy
        self.compact()
        self.issue()
        stepped = bool(self.inflight)
        if stepped:
            self.windows(self.collect())
        self.drain(block=not stepped and bool(self.pending) and not self.waiting)
        self.announce()
        if stepped or self.pending or self.closing or busy:
            return True
        if self.finished() and not self.waiting and not self.syn._ctl and \
                all(r.req is None for r in self.rows):
            return False
        self.idle(self.now())
        return True

    def poll(self) -> None:
        self.waiting.extend(self.poll_fn(self.now()))

    def complete(self, req: StreamRequest, error: Optional[BaseException] = None) -> None:
        if error is not None:
            req.error = error
        req.t_done = self.now()
        if any(q is req for q in self.syn._live):
            self.syn._live.remove(req)
        self.done_cb(req)
        if req.on_done is not None:
            req.on_done(req)

    def park(self, r: _Row) -> None:
        if not r.parked:
            self.llm.release_row(r.idx, self.stream)
            r.parked = True

    def cancellations(self) -> None:
        for r in self.rows:  # barge-in: free cancelled rows now
            if r.req is not None and r.req.cancelled:
                self.finish(r, [])

    def finish(self, r: _Row, due: List) -> None:
        req = r.req
        if not req.cancelled and req.audio and r.sched is not None:
            for win in r.sched.flush():
                due.append((req, req.windows, win))
                req.windows += 1
        self.park(r)
        self.closing.append(req)
        self.free_slots.add(r.slot)
        r.clear()

    def compact(self) -> None:
        """Live rows to a prefix: a lone stream in row 31 no longer costs a 32-row step."""
        if self.syn.compact:
            for dst, src in plan_compaction(self.rows):
                self.llm.move_row(dst, src, self.stream)

    def refused(self, e: BaseException) -> None:
        """Only what the device refused for its arguments fails its owner alone."""
        if isinstance(e, _lib.MxError) and e.rc != _lib.MX_ERR_ARG:
            raise e

    def fail(self, a: _Admission, e: BaseException) -> None:
        if a.row.req is a.req:  # (mid-prompt: the row was reserved)
            a.row.clear()
        self.free_slots.add(a.slot)
        self.complete(a.req, e)

    def enqueued(self, adms: List[_Admission]) -> None:
        """The prompts of ``adms`` are enqueued: their rows decode on, one event for their tokens."""
        for a in adms:
            a.row.bind(a.req, a.slot, a.n0, self.llm.max_pos)
            a.req.t_admit = self.now()
            if not any(q is a.req for q in self.syn._live):
                self.syn._live.append(a.req)
        ev = torch.cuda.Event()
        ev.record(self.stream)
        self.inflight.append((ev, [(a.row, a.req, 0) for a in adms]))
        for a in adms:
            if a.row.issued >= a.row.limit:
                self.park(a.row)

    def control(self) -> None:
        """Prefix registrations and removals handed to the loop thread."""
        syn = self.syn
        while True:
            with syn._cv:
                if not syn._ctl:
                    return
                op, name, ids, h = syn._ctl.popleft()
                p, old, err = None, None, None
                if op == "unregister":
                    p = syn.prefixes.remove(name)
                else:  # (under the lock: has_prefix never sees the name in neither place)
                    try:
                        p, old = syn.prefixes.place(name, ids)
                    except RuntimeError as e:
                        err = e
                        if any(not q.ready for q in syn.prefixes.entries.values()):
                            # a slot frees up once the prefix being prefilled is ready
                            syn._ctl.appendleft((op, name, ids, h))
                            return
            if op == "unregister":
                if p is not None and p.handle is not None and not p.handle.done:
                    p.handle._finish(KeyError(f"prefix {name!r} was unregistered"))
                h._finish(None if p is not None else KeyError(f"unknown prefix {name!r}"))
                continue
            if err is not None:
                h._finish(err)
                continue
            if old is not None and old.handle is not None and not old.handle.done:
                old.handle._finish(KeyError(f"prefix {old.name!r} was replaced"))
            p.handle = h
            p.plan = deque(plan_prompt_chunks(p.n, 0, self.llm.max_prefill))

    def advance_prefixes(self) -> bool:
        """One chunk of every prefix still being prefilled; True while one is unfinished."""
        syn, busy = self.syn, False
        for p in [q for q in syn.prefixes.entries.values() if not q.ready]:
            off, n, _ = p.plan.popleft()
            try:  # every chunk of a template is non-final: layers and KV only
                self.llm.prefill_chunk(p.slot, p.ids[off:off + n], off, self.stream)
            except (ValueError, _lib.MxError) as e:
                self.refused(e)
                syn.prefixes.remove(p.name)
                p.handle._finish(e)
                continue
            syn.prompt_chunks += 1
            if p.plan:
                busy = True
                continue
            p.ready = True
            syn.prefix_fills[p.name] += 1
            p.handle._finish(None)
        return busy

    def admit(self) -> None:
        """Waiting requests into the free rows, one per row, each validated on the host (the plain
        unpacked path leaves its ids to the device).  Those that fit a pack wait for
        ``admit_packs``; a prefix stays pinned until the iteration's forks are enqueued."""
        llm, formed, cands = self.llm, [], []
        try:
            for r in self.rows:
                if not self.waiting:
                    break
                if r.req is not None:
                    continue
                a = self.candidate(r, idle=not cands and all(q.req is None for q in self.rows))
                if a is _HOLD:
                    break
                if a is None:
                    continue
                formed.append(a)
                # a pack takes the prompts that fit one chunk and, behind a ready prefix, the
                # suffixes that do; everything longer goes chunk by chunk
                pack = self.syn.packed_prefill and len(a.req.prompt_ids) <= llm.max_prefill
                try:
                    check_request(a.req, llm.cfg.vocab if pack or self.chunked(a) else None)
                except ValueError as e:
                    self.fail(a, e)
                    continue
                if pack:
                    cands.append(a)
                else:
                    self.single(a)
            self.admit_packs(cands)
        finally:
            for a in formed:
                if a.prefix is not None:
                    a.prefix.pins -= 1

    def candidate(self, r: _Row, idle: bool):
        """The next waiting request as a candidate for row ``r`` (slot taken, prefix pinned);
        None when it ended here, ``_HOLD`` when it went back first in line, where it holds
        later arrivals.  ``idle``: no stream is live and none was formed in this iteration."""
        syn, llm = self.syn, self.llm
        req = self.waiting.popleft()
        if req.cancelled:
            return self.complete(req)
        pre = None
        if req.prefix is not None:
            named = isinstance(req.prefix, str)
            pre = syn.prefixes.get(req.prefix) if named else None
            # still being prefilled, or its registration has not reached the loop yet
            coming = named and syn.has_prefix(req.prefix) if pre is None else not pre.ready
            if coming:
                self.waiting.appendleft(req)
                return _HOLD
            if pre is None:  # an unknown (or evicted) name fails this request alone
                return self.complete(req, UnknownPrefix(f"unknown prefix {req.prefix!r}"))
        # n0, limit, the window scheduler and the grammar count from the whole prompt
        n0 = len(req.prompt_ids) + (pre.n if pre is not None else 0)
        if len(req.prompt_ids) < 1 or n0 >= llm.max_pos:
            return self.complete(req, ValueError(f"prompt of {n0} ids does not fit (max_pos "
                                                 f"{llm.max_pos})"))
        if req.grammar and llm.grammar is None:
            if not idle:  # the context takes its grammar while idle: wait for the live streams
                self.waiting.appendleft(req)
                return _HOLD
            for q in self.rows:
                self.park(q)
            try:  # a vocabulary that cannot hold the preset fails this request alone
                llm.set_grammar(ORPHEUS_GRAMMAR)
            except _lib.MxError as e:
                self.refused(e)
                return self.complete(req, e)
        if req.noise_seed is None:
            req.noise_seed = window_seed(syn.seed, syn._admitted)
        syn._admitted += 1
        slot = min(self.free_slots)
        self.free_slots.discard(slot)
        if pre is not None:
            pre.pins += 1
        return _Admission(r, req, slot, n0, pre)

    def chunked(self, a: _Admission) -> bool:
        return a.prefix is not None or a.n0 > self.llm.max_prefill

    def single(self, a: _Admission) -> None:
        """Admit ``a`` alone: a prefixed or long prompt chunk by chunk, any other by one prefill."""
        if self.chunked(a):
            return self.start_prompt(a)
        try:  # a request the device rejects fails alone; the loop serves on
            seg = request_segment(a.req, a.slot, a.row.idx)
            self.llm.prefill(seg.slot, seg.row, seg.ids, stream=self.stream, **seg.keywords())
        except (ValueError, _lib.MxError) as e:
            self.refused(e)
            return self.fail(a, e)
        self.enqueued([a])

    def admit_packs(self, cands: List[_Admission]) -> None:
        """``cands`` in admission order: per pack of the plan one ``fork_slots`` for its prefixed
        members, then one ``prefill_batch`` (their suffixes at ``pos0`` = the prefix's length)."""
        syn, llm = self.syn, self.llm
        plan = plan_prefill_packs([len(a.req.prompt_ids) for a in cands], llm.max_prefill,
                                  llm.max_batch)
        for pack in plan:
            items = [cands[i] for i in pack]
            prefixed = [a for a in items if a.prefix is not None]
            if 0 < len(prefixed) < PREFIX_PACK_MIN:
                # too few for the pack to pay: they take the chunked path as ever
                for a in prefixed:
                    self.single(a)
                items, prefixed = [a for a in items if a.prefix is None], []
                if not items:
                    continue
            segs = [request_segment(a.req, a.slot, a.row.idx,
                                    pos0=a.prefix.n if a.prefix is not None else 0) for a in items]
            try:
                if prefixed:
                    llm.fork_slots([(a.slot, a.prefix.slot, a.prefix.n) for a in prefixed],
                                   self.stream)
                llm.prefill_batch(segs, self.stream)
            except _lib.MxError as e:
                if e.rc not in (_lib.MX_ERR_ARG, _lib.MX_ERR_STATE):
                    raise
                for a in items:  # refused as a whole, nothing enqueued: the bad one fails alone
                    self.single(a)
                continue
            syn.prefill_packs[len(items)] += 1
            if prefixed:
                syn.prefix_packs[len(items)] += 1
            for a in prefixed:
                syn.prefix_forks[a.prefix.name] += 1
            self.enqueued(items)

    def start_prompt(self, a: _Admission) -> None:
        """Reserve the row for a long or prefixed prompt: the fork of its prefix now, its chunks
        from ``advance_prompts`` on."""
        r, req, pre = a.row, a.req, a.prefix
        r.reserve(req, a.slot, a.n0)
        self.syn._live.append(req)
        pos0 = 0
        if pre is not None:
            try:
                self.llm.fork_slot(a.slot, pre.slot, pre.n, self.stream)
            except _lib.MxError as e:
                self.refused(e)
                return self.fail(a, e)
            self.syn.prefix_forks[pre.name] += 1
            pos0 = pre.n
        r.prompt = [pos0, deque(plan_prompt_chunks(len(req.prompt_ids), pos0,
                                                   self.llm.max_prefill))]

    def advance_prompts(self) -> bool:
        """Every mid-prompt row one step on; True while a row is still mid-prompt."""
        return any([self.advance_prompt(r) for r in self.rows  # (a list: every row advances)
                    if r.req is not None and r.prompt is not None])

    def advance_prompt(self, r: _Row) -> bool:
        """``r``'s next chunks up to and including ONE non-final chunk (the live streams step
        between chunks); the final chunk binds the row as a plain prefill does.  True while the
        row is still mid-prompt."""
        a, (pos0, plan), last = _Admission(r, r.req, r.slot, r.n0), r.prompt, False
        while not last:
            off, n, last = plan.popleft()
            kw = dict(request_segment(a.req, r.slot, r.idx).keywords(), last=True, row=r.idx) \
                if last else {}
            try:
                self.llm.prefill_chunk(r.slot, a.req.prompt_ids[off:off + n], pos0 + off,
                                       self.stream, **kw)
            except (ValueError, _lib.MxError) as e:
                self.refused(e)
                self.fail(a, e)
                return False
            self.syn.prompt_chunks += 1
            if not last:
                return True
        self.enqueued([a])
        return False

    def issue(self) -> None:
        """Keep ``depth`` steps queued for the rows that still need tokens."""
        act = [r for r in self.rows if r.req is not None and not r.stopped and not r.parked]
        while act and len(self.inflight) < self.syn.depth:
            n_rows = max(r.idx for r in act) + 1
            self.llm.decode(n_rows, self.stream)
            self.syn.row_steps[n_rows] += 1
            ev = torch.cuda.Event()
            ev.record(self.stream)
            entries = [(r, r.req, r.issued) for r in act]
            for r in act:
                r.issued += 1
                if r.issued >= r.limit:
                    self.park(r)
            self.inflight.append((ev, entries))
            act = [r for r in act if not r.parked]

    def collect(self) -> List:
        """The oldest queued step's tokens, read from the history; streams that ended free their
        rows.  Returns the SNAC windows that fell due: [(req, window index, codes)]."""
        ev, entries = self.inflight.popleft()
        ev.synchronize()
        self.llm.check(self.stream)
        due: List = []
        for r, req, k in entries:
            if r.req is not req or r.stopped or req.cancelled:
                continue  # speculative step of a stream that already ended
            tok = int(self.llm.hist[r.slot, r.n0 + k])
            req.tokens.append(tok)
            if req.on_token is not None:
                req.on_token(req, tok)
            if req.audio:
                feed = int(req.inject_ids[k]) if req.inject_ids is not None else tok
                for win in r.sched.push(code_of_id(feed, r.sched.count)):
                    due.append((req, req.windows, win))
                    req.windows += 1
            if tok in req.stop_ids or len(req.tokens) >= r.limit:
                r.stopped = True
        for r in self.rows:
            if r.req is not None and r.stopped:
                self.finish(r, due)
        return due

    def windows(self, due: List) -> None:
        """Coalescing: hold the due windows until enough are ready or the oldest has waited."""
        syn, held = self.syn, self.held
        if held:
            self.held_age += 1
        held.extend(due)
        if held and (len(held) >= syn.snac_min_batch or self.held_age >= syn.snac_max_hold or
                     self.closing or any(w == 0 for _, w, _ in held) or not self.inflight):
            self.launch_windows(held)
            held.clear()
            self.held_age = 0

    def launch_windows(self, due: List) -> None:
        """due: [(req, window index, codes)] -> one SNAC call per frame-count group."""
        syn, ring = self.syn, self.syn.ring
        groups: Dict[int, List] = {}
        for item in due:  # grouped by the frames the kept slice depends on (7 -> 5)
            n = len(item[2]) // 7
            groups.setdefault(frames_for_slice(n, min(SLICE_HI, SAMPLES_PER_FRAME * n)),
                              []).append(item)
        for nf, items in groups.items():
            for s in range(0, len(items), ring.max_batch):
                chunk = items[s:s + ring.max_batch]
                i = syn._calls % ring.n
                while len(self.pending) >= ring.n:
                    self.drain(block=True, upto=1)
                codes, seeds = ring.codes[i], ring.seeds[i]
                for j, (req, widx, win) in enumerate(chunk):
                    codes[j * 7 * nf:(j + 1) * 7 * nf] = win[:7 * nf]
                    seeds[j] = window_seed(req.noise_seed, widx)
                lo, hi = SLICE_LO, max(SLICE_LO, min(SLICE_HI, SAMPLES_PER_FRAME * nf))
                syn.snac.decode_ptr(ring.codes_dev[i], nf, len(chunk), 0, 0,
                                    ring.pcm_dev[i] if hi > lo else 0, 0, lo, hi,
                                    syn.snac_stream, seeds_ptr=ring.seeds_dev[i])
                e = torch.cuda.Event()
                e.record(syn.snac_stream)
                self.pending.append((e, i, [(req, (hi - lo) * 2) for req, _, _ in chunk]))
                syn._calls += 1

    def drain(self, block: bool, upto: Optional[int] = None) -> None:
        k = 0
        while self.pending and (upto is None or k < upto):
            e, i, items = self.pending[0]
            if not block and not e.query():
                return
            e.synchronize()
            self.pending.popleft()
            k += 1
            pcm = self.syn.ring.pcm[i]
            for j, (req, nbytes) in enumerate(items):
                if not nbytes or req.cancelled:
                    continue
                n = nbytes // 2
                data = pcm[j * n:(j + 1) * n].tobytes()
                req.samples += n
                if req.t_first_audio is None:
                    req.t_first_audio = self.now()
                if req.on_chunk is not None:
                    req.on_chunk(req, data)

    def announce(self) -> None:
        """A closing stream's windows were all launched when it closed: once no pending SNAC call
        holds one of them, its end is announced (in close order)."""
        while self.closing:
            req = self.closing[0]
            if any(q is req for _, _, items in self.pending for q, _ in items):
                return
            self.closing.popleft()
            self.complete(req)
