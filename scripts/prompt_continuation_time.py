"""Prompt continuation timing at the full Orpheus-3B shape (synthetic weights, bf16).

    python scripts/prompt_continuation_time.py [--rounds 7] [--inner 3]
    python scripts/prompt_continuation_time.py --trace-case          (under rocprofv3, own run)
    python scripts/prompt_continuation_time.py --analyze <kernel_trace.csv>

One engine (max_pos 4096, max_prefill 2072, 3 slots, 1 row) serves every variant; the variants
of a comparison alternate round by round after one warm call of each, a round times `--inner`
back-to-back calls between two device events; per variant the median over rounds and the spread
(max - min).  Lines (DESIGN.md §7 "Prompt continuation"):
  fork        kv_fork_kernel (LlmEngine.fork_slot) at n_pos 256 / 1,024 / 2,048 against the same
              bytes moved by the runtime's own device-to-device copies: one hipMemcpy2DAsync per
              (layer, K | V) over a buffer of the cache's geometry.  Target: kernel <= copies +
              the copies' spread.  Both as TB/s (bytes read + bytes written).
  cached      fork of P positions + a 24-id final chunk against ONE prefill of P + 24 ids (what an
              engine without continuation has to do), P = 1,024 / 2,048.
  chunked     2,048 ids as 4 chunks of 512 against one prefill of 2,048 ids (reported, no target).
--trace-case runs one fork + 48-id suffix at P = 2,048 after a device-wide wait, for a kernel
trace; --analyze sums that trace's kernel times from the fork on and prints attn_kernel's share
of the suffix prefill."""
import argparse
import csv
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def analyze(path):
    rows = list(csv.DictReader(open(path)))
    name = next(k for k in rows[0] if k.lower() in ("kernel_name", "name"))
    t0 = next(k for k in rows[0] if k.lower() in ("start_timestamp", "start"))
    t1 = next(k for k in rows[0] if k.lower() in ("end_timestamp", "end"))
    rows.sort(key=lambda r: int(r[t0]))
    forks = [i for i, r in enumerate(rows) if "kv_fork_kernel" in r[name]]
    tail = rows[forks[-1]:]
    by = {}
    for r in tail[1:]:
        key = r[name].split("(")[0].split("<")[0].split()[-1].split("::")[-1]
        by[key] = by.get(key, 0) + int(r[t1]) - int(r[t0])
    total = sum(by.values())
    print(json.dumps({"case": "fork 2048 + 48-id suffix", "fork_us": round(
        (int(tail[0][t1]) - int(tail[0][t0])) / 1e3, 1), "suffix_kernel_us": round(total / 1e3, 1),
        "attn_share": round(by.get("attn_kernel", 0) / total, 3),
        "by_kernel_us": {k: round(v / 1e3, 1) for k, v in sorted(by.items(), key=lambda x: -x[1])}}))


def hip_runtime():
    """The HIP runtime this process already runs on (the mapping torch loaded)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime mapped")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--trace-case", action="store_true")
    ap.add_argument("--analyze")
    args = ap.parse_args()
    if args.analyze:
        return analyze(args.analyze)
    import torch
    from project_morpheus_amd import config as C
    from project_morpheus_amd.engine import LlmEngine
    from project_morpheus_amd.weights import synthetic_llm_weights
    cfg = C.OrpheusConfig()
    w = synthetic_llm_weights(cfg, seed=0, device="cuda:0")
    MAX_POS, CHUNK = 4096, 512
    llm = LlmEngine(cfg, w, device=0, max_slots=3, max_pos=MAX_POS, max_batch=1, max_prefill=2072)
    del w
    torch.cuda.empty_cache()
    st = torch.cuda.Stream()

    def ids(n, j=0):
        return [1000 + ((j * 131 + i) * 7919) % 120000 for i in range(n)]

    def chunks(slot, toks, final):
        for off in range(0, len(toks), CHUNK):
            part = toks[off:off + CHUNK]
            last = final and off + CHUNK >= len(toks)
            llm.prefill_chunk(slot, part, off, st, **(dict(last=True, row=0) if last else {}))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(args.inner):
            fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.inner

    def compare(variants):
        for fn in variants.values():
            fn()
        st.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                ms[k].append(timed(fn))
        return ({k: statistics.median(v) for k, v in ms.items()},
                {k: max(v) - min(v) for k, v in ms.items()})

    prefix = ids(2048)
    chunks(2, prefix, final=False)          # the template: slot 2 holds 2,048 positions
    st.synchronize()

    if args.trace_case:
        torch.cuda.synchronize()
        llm.fork_slot(0, 2, 2048, st)
        llm.prefill_chunk(0, ids(48, 5), 2048, st, last=True, row=0)
        st.synchronize()
        llm.close()
        return

    # ---- fork against the runtime's copies ---------------------------------------------
    hip = hip_runtime()
    hip.hipMemcpy2DAsync.restype = ctypes.c_int
    hip.hipMemcpy2DAsync.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                     ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                     ctypes.c_int, ctypes.c_void_p]
    pitch = MAX_POS * 128 * 2                                   # one (slot, kv head) block
    layer = 2 * cfg.kv_heads * pitch                            # two slots of one layer
    mirror = torch.empty(2 * cfg.layers * layer, dtype=torch.uint8, device="cuda:0")

    def runtime_copies(n_pos):
        width = (n_pos + 31) // 32 * 8192
        for i in range(2 * cfg.layers):                         # (layer, K | V)
            base = mirror.data_ptr() + i * layer
            rc = hip.hipMemcpy2DAsync(base + cfg.kv_heads * pitch, pitch, base, pitch, width,
                                      cfg.kv_heads, 3, st.cuda_stream)   # 3: device to device
            assert rc == 0, rc

    for n_pos in (256, 1024, 2048):
        nbytes = 2 * ((n_pos + 31) // 32 * 8192) * 2 * cfg.layers * cfg.kv_heads   # read + write
        med, spread = compare({"kernel": lambda: llm.fork_slot(0, 2, n_pos, st),
                               "copies": lambda: runtime_copies(n_pos)})
        print(json.dumps({
            "line": "fork", "n_pos": n_pos, "mb_each_way": round(nbytes / 2e6, 1),
            "kernel_us": round(1e3 * med["kernel"], 1), "copies_us": round(1e3 * med["copies"], 1),
            "spread_us": {k: round(1e3 * v, 1) for k, v in spread.items()},
            "kernel_tb_s": round(nbytes / med["kernel"] / 1e9, 2),
            "copies_tb_s": round(nbytes / med["copies"] / 1e9, 2),
            "kernel_not_slower": bool(med["kernel"] <= med["copies"] + spread["copies"])}),
            flush=True)
    del mirror

    # ---- cached-voice first token ------------------------------------------------------
    tail = ids(24, 9)
    for P in (1024, 2048):
        whole = prefix[:P] + tail

        def cached():
            llm.fork_slot(0, 2, P, st)
            llm.prefill_chunk(0, tail, P, st, last=True, row=0)
            llm.release_row(0, st)

        def one_prefill():
            llm.prefill(0, 0, whole, 1.1, st)
            llm.release_row(0, st)

        med, spread = compare({"cached": cached, "prefill": one_prefill})
        print(json.dumps({
            "line": "cached", "P": P, "suffix": 24, "cached_ms": round(med["cached"], 3),
            "prefill_ms": round(med["prefill"], 3),
            "spread_ms": {k: round(v, 3) for k, v in spread.items()},
            "prefill_over_cached": round(med["prefill"] / med["cached"], 2)}), flush=True)

    # ---- chunked long prompt -----------------------------------------------------------
    def chunked():
        chunks(0, prefix, final=True)
        llm.release_row(0, st)

    def one_shot():
        llm.prefill(0, 0, prefix, 1.1, st)
        llm.release_row(0, st)

    med, spread = compare({"chunked": chunked, "one_shot": one_shot})
    print(json.dumps({
        "line": "chunked", "ids": 2048, "chunk": CHUNK, "chunked_ms": round(med["chunked"], 3),
        "one_shot_ms": round(med["one_shot"], 3),
        "spread_ms": {k: round(v, 3) for k, v in spread.items()},
        "chunked_over_one_shot": round(med["chunked"] / med["one_shot"], 3)}), flush=True)
    llm.close()


if __name__ == "__main__":
    main()
