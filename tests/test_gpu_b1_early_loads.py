"""One-row decode kernels with their dependent loads issued up front (llm_kernels.hip
gemv1_kernel / attn_kernel): what the hoisting could break, against the fp32 CPU oracle.

* The merging o-projection reads a group's split slots (up to the host's bound) before it
  knows how many are live and masks the dead ones afterwards.  Option debug_poison_att_partials turns every
  partial into quiet NaNs; the steps after it rewrite the live slots only, so a dead slot that
  reaches the result makes the logits NaN.
* The attention prologue takes the row's position and slot together at the top of the kernel,
  and the merging o-projection requests the position beside its partial loads.  A second
  utterance on the same engine, at a smaller position and on another slot, replays the graph
  captured for the first: stale values would give it the first utterance's position or slot
  (and a qkv epilogue that hoisted them, its RoPE row).

Tolerances as tests/test_gpu_llm.py (teacher-forced; every step's logits within 5e-3 of the
oracle, tokens tie-aware); the e4m3 cases run the config and tolerance of tests/test_gpu_fp8.py.
"""
import numpy as np
import pytest
import torch

from oracle import llama_ref as L
from project_morpheus_amd import config as C
from project_morpheus_amd.weights import dequantize_fp8, quantize_fp8, synthetic_llm_weights

pytestmark = pytest.mark.gpu

LOGIT_TOL = 5e-3
TIE_MARGIN = 1e-2
PENALTY = 1.1
MAX_POS = 512
POISON = "debug_poison_att_partials"


def _small():
    return C.OrpheusConfig(hidden=512, layers=2, heads=4, kv_heads=2, ffn=1024, vocab=1000)


def _small_fp8():
    return C.OrpheusConfig(hidden=1024, layers=2, heads=8, kv_heads=2, ffn=2048, vocab=1000)


def _engine(cfg, w, wdtype=None):
    from project_morpheus_amd.engine import LlmEngine
    kw = {"wdtype": wdtype} if wdtype else {}
    eng = LlmEngine(cfg, w, device=0, max_slots=2, max_pos=MAX_POS, max_batch=1,
                    max_prefill=256, **kw)
    eng.enable_logits()
    return eng


def _utterance(eng, st, slot, prompt, steps, poison_before=()):
    """Prefill ``prompt`` on (slot, row 0), then ``steps`` decode steps; the partials are
    poisoned before each decode step listed in ``poison_before`` (1 = the first).  Returns the
    tokens and logits of the prefill and of every step."""
    eng.prefill(slot, 0, prompt, PENALTY, st)
    toks, logits = [], []
    for k in range(steps + 1):
        if k > 0:
            if k in poison_before:
                st.synchronize()
                eng.set_option(POISON, 1)
            eng.decode(1, st)
        logits.append(eng.read_logits(0, st))
        toks.append(int(eng.hist[slot, len(prompt) + k]))
    return toks, logits


def _against_oracle(cfg, ref_w, prompt, toks, logits, what):
    rc = L.RefConfig(hidden=cfg.hidden, layers=cfg.layers, heads=cfg.heads,
                     kv_heads=cfg.kv_heads, head_dim=cfg.head_dim, ffn=cfg.ffn, vocab=cfg.vocab,
                     eps=cfg.eps, rope_theta=cfg.rope_theta, rope_scaling=cfg.rope_scaling)
    ref = L.LlamaRef(rc, ref_w, max_pos=MAX_POS)
    _, r_logits = L.greedy_generate(ref, prompt, len(toks), PENALTY, return_logits=True,
                                    forced=toks)
    for k, (g, r) in enumerate(zip(logits, r_logits)):
        r = r.numpy()
        print(f"{what} step {k}: max |logit diff| {np.abs(g - r).max():.3e}")
        assert np.isfinite(g).all(), f"{what}: non-finite logits at step {k}"
        np.testing.assert_allclose(g, r, atol=LOGIT_TOL, rtol=LOGIT_TOL,
                                   err_msg=f"{what}: logits step {k}")
        assert toks[k] == int(np.argmax(g))
        if toks[k] != int(np.argmax(r)):
            top2 = np.sort(r)[-2:]
            assert top2[1] - top2[0] < TIE_MARGIN, \
                f"{what}: token mismatch at step {k} (margin {top2[1] - top2[0]})"


def _prompt(seed, n, vocab):
    return [int(x) for x in np.random.default_rng(seed).integers(0, vocab, n)]


# (prompt ids, decode steps, poison before these steps); the one-row attention of these
# contexts splits every 96 positions
DEAD_SLOT_CASES = {
    "1_live_of_2": (13, 8, (1,)),          # 1 live split under the NSM = 2 merge
    "1_to_2_splits": (90, 12, (1,)),       # L crosses 96
    "2_to_3_of_4": (188, 10, (1, 6)),      # L crosses 192 under NSM = 4: two, then one dead slot
}


@pytest.mark.parametrize("case", list(DEAD_SLOT_CASES))
def test_dead_split_slots_never_reach_the_result(case):
    n, steps, poison = DEAD_SLOT_CASES[case]
    cfg = _small()
    w = synthetic_llm_weights(cfg, seed=21, std=0.05, norm_jitter=0.5)
    prompt = _prompt(31 + n, n, cfg.vocab)
    eng = _engine(cfg, w)
    st = torch.cuda.Stream()
    toks, logits = _utterance(eng, st, 1, prompt, steps, poison_before=poison)
    eng.close()
    _against_oracle(cfg, w, prompt, toks, logits, case)


def _two_utterances(cfg, w, ref_w, wdtype=None):
    """40 ids on slot 1, then -- same engine, same row, same captured graph -- 9 other ids on
    slot 0: a smaller position and another slot."""
    first, second = _prompt(41, 40, cfg.vocab), _prompt(42, 9, cfg.vocab)
    eng = _engine(cfg, w, wdtype)
    st = torch.cuda.Stream()
    t1, l1 = _utterance(eng, st, 1, first, 6)
    eng.release_row(0, st)
    t2, l2 = _utterance(eng, st, 0, second, 6)
    eng.close()
    _against_oracle(cfg, ref_w, first, t1, l1, "first utterance")
    _against_oracle(cfg, ref_w, second, t2, l2, "second utterance")


def test_hoisted_position_and_slot_are_the_current_steps():
    cfg = _small()
    w = synthetic_llm_weights(cfg, seed=22, std=0.05, norm_jitter=0.5)
    _two_utterances(cfg, w, w)


def test_e4m3_dead_split_slots_never_reach_the_result():
    n, steps, poison = DEAD_SLOT_CASES["2_to_3_of_4"]
    cfg = _small_fp8()
    qw = quantize_fp8(synthetic_llm_weights(cfg, seed=23, std=0.05, norm_jitter=0.5), cfg)
    prompt = _prompt(33 + n, n, cfg.vocab)
    eng = _engine(cfg, qw, "fp8")
    st = torch.cuda.Stream()
    toks, logits = _utterance(eng, st, 1, prompt, steps, poison_before=poison)
    eng.close()
    _against_oracle(cfg, dequantize_fp8(qw), prompt, toks, logits, "e4m3 2_to_3_of_4")


def test_e4m3_hoisted_position_and_slot_are_the_current_steps():
    cfg = _small_fp8()
    qw = quantize_fp8(synthetic_llm_weights(cfg, seed=24, std=0.05, norm_jitter=0.5), cfg)
    _two_utterances(cfg, qw, dequantize_fp8(qw), "fp8")
