"""bench.py's plain run, ``--full`` and ``--dump-outputs``: a plain run carries the headline
keys only, ``--full`` is off by default, and the dumped arrays are float .npy files holding
what the last timed utterance handed its caller."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps",
            "warmup", "n_gpus"}
FULL_ONLY = {"http_level", "configs_2_batched", "configs_3_long_read", "configs_4_fp8",
             "roofline", "step_roofline", "eager_step_us_by_kernel", "cpu_baseline"}


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_options_probe",
                                                  os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_full_is_off_by_default(monkeypatch):
    b = _bench_module()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1"])
    a = b.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "somewhere"])
    a = b.parse()
    assert a.full is True and a.dump_outputs == "somewhere"


def test_dump_outputs_writes_exact_float_arrays(tmp_path):
    b = _bench_module()
    pcm = np.array([0, 1, -1, 32767, -32768, 12345], dtype=np.int16)
    chunks = [pcm[:2].tobytes(), pcm[2:].tobytes()]
    ids = [128266, 156933, 7, 0]
    out = tmp_path / "new" / "dir"
    b.dump_outputs(str(out), 0, chunks, ids)
    b.dump_outputs(str(out), 3, chunks, ids)
    assert sorted(os.listdir(out)) == ["pcm.npy", "pcm.rank3.npy", "token_ids.npy",
                                       "token_ids.rank3.npy"]
    got = np.load(out / "pcm.npy")
    assert got.dtype == np.float32 and got.tolist() == pcm.tolist()
    got = np.load(out / "token_ids.npy")
    assert got.dtype == np.float64 and got.tolist() == ids


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """One short plain run (2 timed utterances of 56 tokens): headline keys only, ms_per_step
    consistent with the value, and the dump = the last utterance's PCM and token ids."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", "2", "--warmup", "0", "--max-tokens", "56",
                        "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert HEADLINE <= set(d) and not (FULL_ONLY & set(d)), sorted(d)
    assert d["steps"] == 2 and d["warmup"] == 0 and d["dtype"] == "bf16"
    assert d["unit"] == "audio-sec/wall-sec" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0
    # value = audio of the timed steps / their wall time (the line rounds audio_seconds to
    # 1 ms of a few hundred and ms_per_step to 0.01 ms of about a hundred: within 1 %)
    assert d["value"] == pytest.approx(d["audio_seconds"] / (2 * d["ms_per_step"] / 1e3),
                                       rel=1e-2)
    pcm, ids = np.load(tmp_path / "pcm.npy"), np.load(tmp_path / "token_ids.npy")
    assert pcm.dtype == np.float32 and ids.dtype == np.float64
    assert ids.shape == (56,) and np.all(ids == np.round(ids)) and np.all(ids >= 0)
    # both timed utterances are the same request, so the last one holds half the audio
    # (audio_seconds is rounded to 1 ms = 24 samples)
    assert pcm.size > 0 and abs(pcm.size - d["audio_seconds"] * 24000 / 2) <= 12
    assert np.all(pcm == np.round(pcm)) and np.abs(pcm).max() <= 32768 and np.any(pcm != 0)
