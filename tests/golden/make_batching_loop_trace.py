"""Record ``tests/golden/batching_loop_trace.json``: what ``BatchSynthesizer``'s loop asks of the
engine and the SNAC decoder, and what each request ends with, for the scenarios of
``tests/_fake_engine.py`` (recording fakes: no GPU, no built library).

    python tests/golden/make_batching_loop_trace.py

The fixture pins the loop's behaviour call for call; it is re-recorded only by a change that
means to alter what is enqueued on the device.  Nothing in it depends on time: every request
arrives at 0.0 and the fake events are always complete.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "batching_loop_trace.json")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    import pytest
    import _fake_engine as F
    with pytest.MonkeyPatch.context() as mp:
        F.patch(mp)
        trace = {name: fn() for name, fn in F.scenarios().items()}
    with open(OUT, "w") as f:
        json.dump(trace, f, separators=(",", ":"))
        f.write("\n")
    n = sum(len(t["calls"]) for t in trace.values())
    print(f"wrote {OUT}: {len(trace)} scenarios, {n} calls, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
