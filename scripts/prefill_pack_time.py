"""Packed prefill timing at the full Orpheus-3B shape (synthetic weights, bf16 or --fp8).

    python scripts/prefill_pack_time.py [--fp8] [--ks 1,2,4,8] [--ns 24,48] [--rounds 7]

For every (k, n) three variants are timed in one process, alternating round by round after one
warm call of each:
  pack    one prefill_batch of k prompts of n ids,
  seq     k sequential prefill calls of n ids,
  single  one prefill of k * n ids (the same rows as ONE stream: the floor of the pack).
Each round times `--inner` back-to-back calls between two device events on the stream.  Per
variant: the median over rounds and the spread (max - min).  The k-row lm_head's excess over
the one-row head comes from mx_llm_bench_gemv in the same process.  Targets:
pack < seq for k >= 2; pack <= single + (single's spread + the head's excess)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--ns", default="24,48")
    ap.add_argument("--fp8", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    args = ap.parse_args()
    import torch
    from project_morpheus_amd import config as C
    from project_morpheus_amd.engine import LlmEngine
    from project_morpheus_amd.weights import synthetic_llm_weights
    cfg = C.OrpheusConfig()
    w = synthetic_llm_weights(cfg, seed=0, device="cuda:0")
    if args.fp8:
        from project_morpheus_amd.weights import quantize_fp8
        w = quantize_fp8(w, cfg)
    ks = [int(s) for s in args.ks.split(",")]
    ns = [int(s) for s in args.ns.split(",")]
    K = max(ks)
    wd = "fp8" if args.fp8 else "bf16"
    llm = LlmEngine(cfg, w, device=0, max_slots=K, max_pos=2048, max_batch=K,
                    max_prefill=K * max(ns), wdtype=wd)
    del w
    torch.cuda.empty_cache()
    st = torch.cuda.Stream()

    def ids(j, n):
        return [1000 + ((j * 131 + i) * 7919) % 120000 for i in range(n)]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(args.inner):
            fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.inner

    head_us = {}
    for k, n in [(k, n) for n in ns for k in ks]:
        prompts = [ids(j, n) for j in range(k)]
        one = [t for p in prompts for t in p]
        variants = {
            "pack": lambda: llm.prefill_batch(
                [dict(slot=j, row=j, ids=p, penalty=1.1) for j, p in enumerate(prompts)], st),
            "seq": lambda: [llm.prefill(j, j, p, 1.1, st) for j, p in enumerate(prompts)],
            "single": lambda: llm.prefill(0, 0, one, 1.1, st),
        }
        for fn in variants.values():   # warm every shape of the timed window
            fn()
        st.synchronize()
        ms = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                ms[name].append(timed(fn))
        med = {name: statistics.median(v) for name, v in ms.items()}
        spread = {name: max(v) - min(v) for name, v in ms.items()}
        for j in range(K):
            llm.release_row(j, st)
        st.synchronize()
        for r in (1, k):               # idle context: the head probe clobbers row state
            if r not in head_us:
                head_us[r] = min(llm.bench_gemv("lm_head", reps=4, n_rows=r)[0] for _ in range(3))
        excess = max(0.0, head_us[k] - head_us[1]) * 1e-3
        margin = spread["single"] + excess
        rec = {"wdtype": wd, "k": k, "n": n,
               "pack_ms": round(med["pack"], 3), "seq_ms": round(med["seq"], 3),
               "single_ms": round(med["single"], 3),
               "spread_ms": {a: round(b, 3) for a, b in spread.items()},
               "pack_over_seq": round(med["pack"] / med["seq"], 3),
               "pack_over_single": round(med["pack"] / med["single"], 3),
               "head_us": {"1": round(head_us[1], 1), str(k): round(head_us[k], 1)},
               "margin_ms": round(margin, 3),
               "faster_than_seq": bool(k < 2 or med["pack"] < med["seq"]),
               "within_margin_of_single": bool(med["pack"] <= med["single"] + margin)}
        print(json.dumps(rec), flush=True)
    llm.close()


if __name__ == "__main__":
    main()
