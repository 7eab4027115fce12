"""SNAC encoder timing: SnacEncoder.encode (HIP) against the same arithmetic as eager torch ops on
the GPU -- the only thing a user without this encoder could run (tests/_snac_encoder_ref.py moved
to the device; the third-party snac package is that plus module plumbing).

    python scripts/snac_encode_time.py [--rounds 7] [--inner 3]
    python scripts/snac_encode_time.py --trace-case        (under rocprofv3, in a run of its own)

2 s / 12 s / 24 s of audio (24 / 144 / 288 frames), synthetic weights.  The two variants
alternate round by round after one warm call of each; a round times `--inner` back-to-back calls
between two device events; per variant the median over rounds and the spread (max - min).
Target: HIP no slower than eager torch beyond that spread.  If the eager convolutions cannot run
on the machine the HIP time is reported alone, with its activation traffic.  --trace-case runs
one 24 s encode after a device-wide wait, for a kernel trace."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def activation_bytes(n_frames: int) -> int:
    """Bytes the encoder's launches read and write per encode: with F_k the floats of block k's
    input (98,304 a frame at the two full-rate levels), stem F_0; a residual unit 5 F (depthwise
    2, 1x1 conv with its residual 3), + F for the third unit's Snake output; down-conv F_k + F_k+1."""
    f = [2048 * 48, 1024 * 96, 256 * 192, 32 * 384, 4 * 768]
    floats = f[0] + sum(17 * f[k] + f[k + 1] for k in range(4)) + 2 * f[4]
    return 4 * floats * n_frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--trace-case", action="store_true")
    args = ap.parse_args()
    import torch
    import _snac_encoder_ref as R
    from project_morpheus_amd.engine import SnacEncoder
    from project_morpheus_amd.weights import synthetic_snac_encoder_weights, synthetic_snac_weights
    w = {**synthetic_snac_weights(seed=3), **synthetic_snac_encoder_weights(seed=5)}
    enc = SnacEncoder(w, device=0, max_frames=288)
    st = torch.cuda.Stream()
    frames_of = {"2s": 24, "12s": 144, "24s": 288}
    audio = {k: torch.from_numpy(R.make_audio(n * 2048, seed=n)).cuda() for k, n in frames_of.items()}
    if args.trace_case:
        enc.encode(audio["24s"], stream=st)          # warm (module load)
        torch.cuda.synchronize()
        enc.encode(audio["24s"], stream=st)
        torch.cuda.synchronize()
        print(json.dumps({"case": "one 24 s encode (the second of two)"}))
        return
    wd = {k: v.cuda() for k, v in w.items()}

    def eager(a):
        with torch.no_grad():
            z = R.encoder(wd, a.reshape(1, 1, -1))
            codes, _ = R.quantize(wd, z)
        return codes

    eager_ok, why = True, None
    try:
        with torch.cuda.stream(st):
            got = eager(audio["2s"])
        st.synchronize()
        ours = enc.encode(audio["2s"], stream=st)
        st.synchronize()
        agree = int((R.interleave(*[c.cpu() for c in got]) == ours.cpu()).sum())
        print(json.dumps({"check": "eager torch vs HIP codes at 2 s", "agree": agree, "of": 168}))
    except Exception as e:  # MIOpen cannot run the convs here
        eager_ok, why = False, repr(e)[:300]
        print(json.dumps({"eager_torch": "unavailable", "error": why}))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(args.inner):
            fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.inner

    for tag, n in frames_of.items():
        a = audio[tag]
        variants = {"hip": lambda: enc.encode(a, stream=st)}
        if eager_ok:
            def run_eager():
                with torch.cuda.stream(st):
                    eager(a)
            variants["eager_torch"] = run_eager
        ms = {k: [] for k in variants}
        for fn in variants.values():
            fn()
        st.synchronize()
        for _ in range(args.rounds):
            for k, fn in variants.items():
                ms[k].append(timed(fn))
        out = {"audio": tag, "frames": n}
        for k, v in ms.items():
            out[k + "_ms"] = round(statistics.median(v), 3)
            out[k + "_spread_ms"] = round(max(v) - min(v), 3)
        gb = activation_bytes(n) / 1e9
        out["hip_activation_GB"] = round(gb, 3)
        out["hip_TBps"] = round(gb / out["hip_ms"], 3)
        out["hip_x_realtime"] = round(n * 2048 / 24000.0 / (out["hip_ms"] / 1e3))
        if eager_ok:
            out["hip_over_eager"] = round(out["hip_ms"] / out["eager_torch_ms"], 3)
            out["target_met"] = out["hip_ms"] <= out["eager_torch_ms"] + out["eager_torch_spread_ms"]
        print(json.dumps(out))
    enc.close()


if __name__ == "__main__":
    main()
