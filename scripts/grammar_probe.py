"""Decode steps for a per-launch kernel trace of the lm_head and the samplers, with and without
the code grammar (DESIGN.md §7 "Code grammar"):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- \
        python3 scripts/grammar_probe.py [--grammar]

One layer at the Orpheus width and vocabulary (the head and sampler launches do not depend on
the depth), bf16 then e4m3; for each, one sampled row (T 0.6, top-p 0.9: sample_kernel) for
``--steps`` steps, then eight rows with top-k 40 / min-p 0.05 (sample_chain_kernel).  The
kernel names tell the cases apart: head1::head_b1_kernel<6, 2, false> / <3, 4, true> at one
row, gemm_rows_kernel / gemm_rows_gram_kernel <.., F8, ..> at eight.  Prints the engine's
device memory before and after the grammar is set.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from project_morpheus_amd import config as C
from project_morpheus_amd.engine import LlmEngine
from project_morpheus_amd.weights import quantize_fp8, synthetic_llm_weights


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grammar", action="store_true")
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    cfg = C.OrpheusConfig(layers=1)
    w16 = synthetic_llm_weights(cfg, seed=0)
    rng = np.random.default_rng(5)
    for wdtype in ("bf16", "fp8"):
        w = quantize_fp8(w16, cfg) if wdtype == "fp8" else w16
        free0 = torch.cuda.mem_get_info(0)[0]
        eng = LlmEngine(cfg, w, device=0, max_slots=8, max_pos=512, max_batch=8, max_prefill=64,
                        wdtype=wdtype)
        free1 = torch.cuda.mem_get_info(0)[0]
        if args.grammar:
            eng.set_grammar(C.ORPHEUS_GRAMMAR)
        free2 = torch.cuda.mem_get_info(0)[0]
        print(f"{wdtype}: engine {free0 - free1} bytes, after set_grammar +{free1 - free2} bytes",
              flush=True)
        st = torch.cuda.Stream()
        for B, top_k, min_p in ((1, 0, 0.0), (8, 40, 0.05)):
            for i in range(B):
                p = [int(x) for x in rng.integers(0, 128000, 8 + i)] + [C.START_OF_SPEECH]
                eng.prefill(i, i, p, 1.1, st, temperature=0.6, top_p=0.9, seed=100 + i,
                            top_k=top_k, min_p=min_p, grammar=args.grammar)
            for _ in range(args.steps):
                eng.decode(B, st)
            st.synchronize()
            toks = [int(eng.hist[0, 9 + k]) for k in range(8)]
            print(f"{wdtype} {B} rows: first tokens of row 0 {toks}", flush=True)
            for i in range(B):
                eng.release_row(i, st)
            st.synchronize()
        if args.grammar:
            print(f"{wdtype}: grammar window {eng.grammar_window()}", flush=True)
        eng.close()


if __name__ == "__main__":
    main()
