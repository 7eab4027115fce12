"""Host side of the packed prefill: the pack planner, the environment default, the export and
the ctypes layout of mx_prefill_seg (no GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _plan(lengths, max_prefill, max_k):
    from project_morpheus_amd.batching import plan_prefill_packs
    packs = plan_prefill_packs(lengths, max_prefill, max_k)
    # never reorders, never drops: the packs concatenate to 0 .. n-1
    assert [i for p in packs for i in p] == list(range(len(lengths)))
    assert all(p for p in packs)
    return packs


def test_plan_keeps_order_and_both_caps():
    lengths = [24, 24, 24, 24, 60, 3, 3, 3, 3, 3, 40, 30]
    packs = _plan(lengths, 64, 4)
    assert packs == [[0, 1], [2, 3], [4, 5], [6, 7, 8, 9], [10], [11]]
    for p in packs:
        assert len(p) <= 4 and sum(lengths[i] for i in p) <= 64
    # greedy: a pack closes only when the next prompt does not fit
    for a, b in zip(packs, packs[1:]):
        assert len(a) == 4 or sum(lengths[i] for i in a) + lengths[b[0]] > 64


def test_plan_stream_cap_alone():
    assert _plan([1] * 9, 1000, 4) == [[0, 1, 2, 3], [4, 5, 6, 7], [8]]
    assert _plan([5, 6], 64, 1) == [[0], [1]]


def test_plan_prompt_of_exactly_max_prefill_is_alone():
    assert _plan([10, 64, 10], 64, 8) == [[0], [1], [2]]
    assert _plan([64], 64, 8) == [[0]]
    assert _plan([32, 32, 1], 64, 8) == [[0, 1], [2]]


def test_plan_empty_input():
    assert _plan([], 64, 4) == []


def test_plan_does_not_judge_an_oversized_prompt():
    assert _plan([3, 100, 3], 64, 4) == [[0], [1], [2]]


@pytest.mark.parametrize("value,want", [("1", True), ("true", True), (" Yes ", True), ("ON", True),
                                        ("0", False), ("", False), ("off", False), ("2", False)])
def test_packed_prefill_default_parses_like_grammar_default(value, want):
    from project_morpheus_amd import config as C
    assert C.packed_prefill_default({"MORPHEUS_MX_PACKED_PREFILL": value}) is want
    assert C.grammar_default({"MORPHEUS_MX_GRAMMAR": value}) is want


def test_packed_prefill_default_unset_is_off(monkeypatch):
    from project_morpheus_amd import config as C
    assert C.packed_prefill_default({}) is False
    monkeypatch.delenv("MORPHEUS_MX_PACKED_PREFILL", raising=False)
    assert C.packed_prefill_default() is False
    monkeypatch.setenv("MORPHEUS_MX_PACKED_PREFILL", "1")
    assert C.packed_prefill_default() is True


def test_entry_point_is_exported():
    from project_morpheus_amd import _lib, build
    assert "mx_llm_prefill_batch" in _lib.EXPORTS
    import torch  # noqa: F401  (the library binds torch's HIP runtime)
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "mx_llm_prefill_batch")


def test_ctypes_struct_matches_the_header_layout():
    """include/morpheus_mx.h states mx_prefill_seg's offsets in its comment and static_asserts
    the same numbers; the ctypes mirror must agree with both."""
    from project_morpheus_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "morpheus_mx.h")).read()
    doc = hdr[hdr.index("Layout (64-bit ABI"):hdr.index("typedef struct mx_prefill_seg")]
    stated = {name: int(off) for off, name in re.findall(r"(\d+) ([a-z_]+)", doc)
              if name in ("slot", "row", "ids_host", "n_ids", "params", "ext")}
    size = int(re.search(r"sizeof (\d+)", doc).group(1))
    assert set(stated) == {"slot", "row", "ids_host", "n_ids", "params", "ext"}
    S = _lib.PrefillSeg
    assert ctypes.sizeof(S) == size == 64
    for name, off in stated.items():
        assert getattr(S, name).offset == off, name
    # ... and the static_assert carries the same numbers
    sa = hdr[hdr.index("static_assert(sizeof(void*) != 8"):hdr.index('"mx_prefill_seg layout"')]
    assert f"sizeof(mx_prefill_seg) == {size}" in sa
    for name, off in stated.items():
        if name != "slot":
            assert f"offsetof(mx_prefill_seg, {name}) == {off}" in sa, name
    assert ctypes.sizeof(_lib.Sampling) == 24 and ctypes.sizeof(_lib.SamplingExt) == 12


def test_batcher_flag_default_and_counter():
    """The flag resolves without a GPU: BatchSynthesizer reads it from the environment only
    when the caller does not say."""
    import inspect

    from project_morpheus_amd.batching import BatchSynthesizer
    from project_morpheus_amd.service import Service
    assert inspect.signature(BatchSynthesizer.__init__).parameters["packed_prefill"].default is None
    assert inspect.signature(Service.__init__).parameters["packed_prefill"].default is None
