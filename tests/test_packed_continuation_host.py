"""Host side of packed continuation: the ctypes view of mx_prefill_chunk, the ``pos0`` field of
``PrefillSegment``, the entry point ``LlmEngine.prefill_batch`` selects, the ``fork_slots``
marshalling and the pack plan over mixed plain and prefixed candidates.  No GPU."""
import ctypes
import os
import re
import types

import numpy as np

from project_morpheus_amd import _lib
from project_morpheus_amd.batching import PREFIX_PACK_MIN, plan_prefill_packs
from project_morpheus_amd.engine import LlmEngine, PrefillSegment

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "morpheus_mx.h")


def test_prefill_chunk_layout_matches_the_header():
    hdr = open(HEADER).read()
    doc = hdr[hdr.index("Layout (64-bit ABI): offset 0 slot, 4 row, 8 ids_host, 16 n_ids, 20 pos0"):]
    doc = doc[:doc.index("*/")]
    size = int(re.search(r"sizeof (\d+)", doc).group(1))
    offs = {n: int(o) for o, n in re.findall(r"(\d+) (\w+)", doc.split(";")[0].split("offset")[1])
            if n != "bytes"}
    S = _lib.PrefillChunk
    assert ctypes.sizeof(S) == size == 72
    assert offs == {"slot": 0, "row": 4, "ids_host": 8, "n_ids": 16, "pos0": 20, "last": 24,
                    "params": 32, "ext": 56}
    for name, off in offs.items():
        assert getattr(S, name).offset == off, name
    sa = hdr[hdr.index("(sizeof(mx_prefill_chunk) == 72"):hdr.index('"mx_prefill_chunk layout"')]
    for name in ("ids_host", "n_ids", "pos0", "last", "params", "ext"):
        assert f"offsetof(mx_prefill_chunk, {name}) == {offs[name]}" in sa
    assert {"mx_llm_prefill_pack", "mx_llm_fork_slots"} <= set(_lib.EXPORTS)
    for fn in ("mx_llm_prefill_pack", "mx_llm_fork_slots"):
        assert re.search(r"\bint %s\(mx_llm\* ctx" % fn, hdr), fn


def test_segment_pos0_defaults_to_zero():
    assert PrefillSegment(slot=0, row=0, ids=[1]).pos0 == 0
    assert PrefillSegment(slot=0, row=0, ids=[1], pos0=7).pos0 == 7


class _Lib:
    """Records the calls of the entry points ``prefill_batch`` and ``fork_slots`` may take."""

    def __init__(self):
        self.calls = []

    def mx_llm_set_slot_grammar(self, h, slot, on):
        self.calls.append(("grammar", slot, on))
        return 0

    def mx_llm_prefill_batch(self, h, arr, n, stream):
        assert isinstance(arr[0], _lib.PrefillSeg)
        self.calls.append(("batch", [(arr[i].slot, arr[i].row, arr[i].n_ids) for i in range(n)]))
        return 0

    def mx_llm_prefill_pack(self, h, arr, n, stream):
        assert isinstance(arr[0], _lib.PrefillChunk)
        self.calls.append(("pack", [(arr[i].slot, arr[i].row, arr[i].n_ids, arr[i].pos0,
                                     arr[i].last, arr[i].ext.penalty_last_n) for i in range(n)]))
        return 0

    def mx_llm_fork_slots(self, h, dst, src, n_pos, n, stream):
        self.calls.append(("forks", [(dst[i], src[i], n_pos[i]) for i in range(n)]))
        return 0

    def mx_llm_last_error(self, h):
        return b""


def _engine():
    eng = LlmEngine.__new__(LlmEngine)      # the methods under test touch these fields only
    eng.lib, eng.h, eng.max_slots, eng._slot_grammar = _Lib(), None, 8, {}
    return eng


def test_prefill_batch_selects_the_entry_point_by_pos0():
    st = types.SimpleNamespace(cuda_stream=0)
    eng = _engine()
    eng.prefill_batch([dict(slot=1, row=0, ids=[1, 2, 3], penalty=1.1),
                       PrefillSegment(slot=2, row=1, ids=[4], pos0=0)], st)
    assert eng.lib.calls == [("batch", [(1, 0, 3), (2, 1, 1)])]
    eng = _engine()
    eng.prefill_batch([dict(slot=1, row=0, ids=[1, 2, 3], penalty=1.1, grammar=True),
                       dict(slot=2, row=1, ids=[4, 5], penalty=1.1, pos0=100, penalty_last_n=4)],
                      st)
    assert eng.lib.calls == [("grammar", 1, 1),
                             ("pack", [(1, 0, 3, 0, 1, 0), (2, 1, 2, 100, 1, 4)])]


def test_fork_slots_marshals_three_arrays():
    eng = _engine()
    eng.fork_slots([(2, 0, 33), (3, 0, 100), (4, 1, 64)], types.SimpleNamespace(cuda_stream=0))
    assert eng.lib.calls == [("forks", [(2, 0, 33), (3, 0, 100), (4, 1, 64)])]


def test_pack_plan_counts_suffix_rows_in_arrival_order():
    """Candidates (whole prompt length, prefix length): the plan sees the rows a candidate
    adds, i.e. its suffix; whole prompts of 1,000+ ids would each close a pack."""
    cands = [(1024 + 24, 1024), (30, 0), (1024 + 20, 1024), (2048 + 40, 2048), (50, 0)]
    rows = [n0 - pre for n0, pre in cands]
    assert rows == [24, 30, 20, 40, 50]
    assert plan_prefill_packs(rows, 128, 8) == [[0, 1, 2, 3], [4]]
    assert plan_prefill_packs(rows, 128, 3) == [[0, 1, 2], [3, 4]]
    assert plan_prefill_packs([n0 for n0, _ in cands], 128, 8) == [[0], [1], [2], [3], [4]]
    assert PREFIX_PACK_MIN >= 2             # one prefixed request runs the chunked launches
