"""Packed continuation timing at the full Orpheus-3B shape (synthetic weights, bf16).

    python scripts/packed_continuation_time.py [--rounds 7]

One engine (max_pos 4096, max_prefill 512, 32 rows, 32 stream slots + 1 template slot).  A burst
is k requests of 24 new ids each behind one template of P ids (P = 2,048 and 1,024):
  arm A  the chunked path: k x (fork_slot + prefill_chunk(last));
  arm B  packed continuation: per pack of the plan (plan_prefill_packs over the suffix rows) one
         fork_slots + one prefill_batch with pos0 = P.
The arms alternate round by round after one warm call of each.  A round is timed between device
events: from the first fork to the last first-token commit (total) and to the first stream's
first-token commit (first).  Per arm the median over rounds and the spread (max - min).  Lines
(DESIGN.md §7 "Packed continuation"):
  burst      both arms per (P, k), and whether B's total beats A's by more than A's spread
  threshold  the smallest such k per P (what batching.PREFIX_PACK_MIN is set from)
  fanout     fork_slots of k forks of 2,048 positions from one source against k fork_slot calls,
             in GB/s written."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch
    from project_morpheus_amd import config as C
    from project_morpheus_amd.batching import plan_prefill_packs
    from project_morpheus_amd.engine import LlmEngine, PrefillSegment
    from project_morpheus_amd.weights import synthetic_llm_weights
    cfg = C.OrpheusConfig()
    w = synthetic_llm_weights(cfg, seed=0, device="cuda:0")
    MAX_POS, CHUNK, B, SUFFIX = 4096, 512, 32, 24
    T = B                                              # the template slot
    llm = LlmEngine(cfg, w, device=0, max_slots=B + 1, max_pos=MAX_POS, max_batch=B,
                    max_prefill=CHUNK)
    del w
    torch.cuda.empty_cache()
    st = torch.cuda.Stream()

    def ids(n, j=0):
        return [1000 + ((j * 131 + i) * 7919) % 120000 for i in range(n)]

    def event():
        return torch.cuda.Event(enable_timing=True)

    prefix = ids(2048)
    for off in range(0, 2048, CHUNK):                  # the template: 2,048 positions
        llm.prefill_chunk(T, prefix[off:off + CHUNK], off, st)
    st.synchronize()
    tails = [ids(SUFFIX, 9 + i) for i in range(B)]

    def arm_a(k, P):
        e0, ef, e1 = event(), event(), event()
        e0.record(st)
        for i in range(k):
            llm.fork_slot(i, T, P, st)
            llm.prefill_chunk(i, tails[i], P, st, last=True, row=i)
            if i == 0:
                ef.record(st)
        e1.record(st)
        return e0, ef, e1

    def arm_b(k, P):
        e0, ef, e1 = event(), event(), event()
        e0.record(st)
        for j, pack in enumerate(plan_prefill_packs([SUFFIX] * k, CHUNK, B)):
            llm.fork_slots([(i, T, P) for i in pack], st)
            llm.prefill_batch([PrefillSegment(slot=i, row=i, ids=tails[i], pos0=P) for i in pack],
                              st)
            if j == 0:
                ef.record(st)
        e1.record(st)
        return e0, ef, e1

    def run(arm, k, P):
        e0, ef, e1 = arm(k, P)
        for i in range(k):
            llm.release_row(i, st)
        e1.synchronize()
        st.synchronize()
        return e0.elapsed_time(e1), e0.elapsed_time(ef)

    def stats(v):
        return round(statistics.median(v), 3), round(max(v) - min(v), 3)

    for P in (2048, 1024):
        threshold = None
        for k in (1, 2, 4, 8, 16, 32):
            run(arm_a, k, P), run(arm_b, k, P)          # warm
            t = {"A": ([], []), "B": ([], [])}
            for _ in range(args.rounds):
                for name, arm in (("A", arm_a), ("B", arm_b)):
                    total, first = run(arm, k, P)
                    t[name][0].append(total)
                    t[name][1].append(first)
            a, a_sp = stats(t["A"][0])
            b, b_sp = stats(t["B"][0])
            af, af_sp = stats(t["A"][1])
            bf, bf_sp = stats(t["B"][1])
            wins = bool(a - b > a_sp)
            if wins and threshold is None:
                threshold = k
            print(json.dumps({
                "line": "burst", "P": P, "k": k, "suffix": SUFFIX,
                "A_total_ms": a, "A_spread_ms": a_sp, "B_total_ms": b, "B_spread_ms": b_sp,
                "A_first_ms": af, "A_first_spread_ms": af_sp, "B_first_ms": bf,
                "B_first_spread_ms": bf_sp, "first_token_delay_ms": round(bf - af, 3),
                "A_over_B": round(a / b, 2), "B_beats_A_beyond_A_spread": wins}), flush=True)
        print(json.dumps({"line": "threshold", "P": P, "smallest_k_B_wins": threshold}),
              flush=True)

    # ---- fork fan-out ------------------------------------------------------------------
    per_fork = (2048 // 32) * 8192 * 2 * cfg.layers * cfg.kv_heads      # bytes written per fork
    for k in (2, 8, 32):
        def many():
            llm.fork_slots([(i, T, 2048) for i in range(k)], st)

        def singles():
            for i in range(k):
                llm.fork_slot(i, T, 2048, st)

        ms = {"many": [], "singles": []}
        many(), singles()
        st.synchronize()
        for _ in range(args.rounds):
            for name, fn in (("many", many), ("singles", singles)):
                e0, e1 = event(), event()
                e0.record(st)
                fn()
                e1.record(st)
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        m, m_sp = stats(ms["many"])
        s, s_sp = stats(ms["singles"])
        print(json.dumps({
            "line": "fanout", "k": k, "n_pos": 2048, "mb_written": round(k * per_fork / 1e6, 1),
            "fork_slots_ms": m, "fork_slots_spread_ms": m_sp, "fork_slot_x_k_ms": s,
            "fork_slot_x_k_spread_ms": s_sp,
            "fork_slots_gb_s": round(k * per_fork / m / 1e6, 1),
            "fork_slot_x_k_gb_s": round(k * per_fork / s / 1e6, 1),
            "fork_slots_not_slower": bool(m <= s + s_sp)}), flush=True)
    llm.close()


if __name__ == "__main__":
    main()
