"""First audio of a burst with and without packed prefill (full Orpheus-3B shape, synthetic
weights and SNAC, synthetic audio ids).

    python scripts/prefill_burst.py [--bursts 8,32] [--rounds 3] [--ids 24] [--tokens 84]

Every stream of a burst arrives at t = 0.  Per burst size, BatchSynthesizer runs alternate
packing off / on for `--rounds` rounds after one warm run of each (the warm runs capture the
step graphs of every row count).  Per run: first-audio p50 / p95 over the streams (ms after
arrival) and the wall time; per mode the median over rounds."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bursts", default="8,32")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ids", type=int, default=24)
    ap.add_argument("--tokens", type=int, default=84)
    ap.add_argument("--fp8", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from project_morpheus_amd import config as C
    from project_morpheus_amd.batching import BatchSynthesizer, StreamRequest
    from project_morpheus_amd.engine import LlmEngine, SnacDecoder
    from project_morpheus_amd.weights import synthetic_llm_weights, synthetic_snac_weights
    cfg = C.OrpheusConfig()
    w = synthetic_llm_weights(cfg, seed=0, device="cuda:0")
    wd = "fp8" if args.fp8 else "bf16"
    if args.fp8:
        from project_morpheus_amd.weights import quantize_fp8
        w = quantize_fp8(w, cfg)
    bursts = [int(s) for s in args.bursts.split(",")]
    B = max(bursts)
    llm = LlmEngine(cfg, w, device=0, max_slots=B, max_pos=1024, max_batch=B, max_prefill=512,
                    wdtype=wd)
    del w
    torch.cuda.empty_cache()
    snac = SnacDecoder(synthetic_snac_weights(), device=0, max_batch=B)

    def run(n, packed):
        syn = BatchSynthesizer(llm, snac, packed_prefill=packed)
        reqs = []
        for j in range(n):
            ids = [1000 + ((j * 131 + i) * 7919) % 120000 for i in range(args.ids)]
            reqs.append(StreamRequest(prompt_ids=ids, max_tokens=args.tokens, arrival=0.0,
                                      stop_ids=(), seed=j, noise_seed=j,
                                      inject_ids=C.synthetic_audio_ids(args.tokens, seed=j)))
        wall = syn.run(reqs)
        fa = [r.first_audio_ms for r in reqs]
        assert all(r.error is None for r in reqs) and all(f is not None for f in fa)
        return {"p50": float(np.percentile(fa, 50)), "p95": float(np.percentile(fa, 95)),
                "wall_ms": 1e3 * wall, "packs": dict(syn.prefill_packs)}

    for n in bursts:
        for packed in (False, True):
            run(n, packed)   # warm
        res = {False: [], True: []}
        for _ in range(args.rounds):
            for packed in (False, True):
                r = run(n, packed)
                res[packed].append(r)
                print(json.dumps({"wdtype": wd, "burst": n, "packed": packed,
                                  **{k: (round(v, 2) if isinstance(v, float) else v)
                                     for k, v in r.items()}}), flush=True)
        for packed in (False, True):
            print(json.dumps({"wdtype": wd, "burst": n, "packed": packed, "median_of": args.rounds,
                              **{k: round(statistics.median(x[k] for x in res[packed]), 2)
                                 for k in ("p50", "p95", "wall_ms")}}), flush=True)
    llm.close()


if __name__ == "__main__":
    main()
