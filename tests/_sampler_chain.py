"""Numpy restatement of the extended sampler chain (TEST INFRASTRUCTURE).

Extends oracle/sampling_ref.py (which it reduces to exactly at neutral values) by the two
filters in front of the nucleus and by the penalty window; stated independently of the GPU's
radix selects (csrc/sample_kernels.hip sample_chain_kernel), by sorting and counting:

  e_i, f_i as in the oracle;
  F = {i : f_i > 0, e_i >= min_p (fp32), #{j : e_j > e_i} < top_k}   (top_k = 0: no limit);
  Z = sum_{i in F} f_i, thr = max(1, floor(float64(Z) * top_p))  (Z when top_p >= 1);
  keep i in F iff sum_{j : e_j > e_i} f_j < thr   (F is an upper set in e-order, so the mass
                                                   above a member lies inside F);
  token = argmax over the kept set of e_i / -log(u_i), Philox counter (i, pos), smallest
          index on ties.

Order: temperature, then top-k and min-p, then top-p (vLLM's order).

Penalty window: choosing the token of position p with ``penalty_last_n`` = N > 0 penalises
exactly the ids at positions max(0, p - N) .. p - 1 (prompt included); N = 0 the whole
sequence.  Rule: v > 0 ? v / pen : v * pen.
"""
from __future__ import annotations

import numpy as np

from oracle import sampling_ref as S


def window_ids(ids, p: int, last_n: int):
    """The set of ids penalised when the token of position ``p`` is chosen (ids[:p] known)."""
    lo = max(0, p - last_n) if last_n > 0 else 0
    return set(int(t) for t in ids[lo:p])


def penalise(raw, ids, p: int, penalty: float, last_n: int) -> np.ndarray:
    """fp32 logits of position ``p`` after the (windowed) repetition penalty."""
    lg = np.array(raw, dtype=np.float32)
    idx = np.fromiter(window_ids(ids, p, last_n), dtype=np.int64)
    if len(idx):
        v = lg[idx]
        lg[idx] = np.where(v > 0, v / np.float32(penalty), v * np.float32(penalty))
    return lg


def chain(logits, temperature: float, top_p: float, top_k: int = 0, min_p: float = 0.0):
    """-> (e float32 [V], kept bool [V], in_f bool [V], f uint64 [V], thr, filter_margin).

    ``filter_margin``: relative gap between the smallest e inside F and the largest e outside
    it (inf when no filter is set or nothing with f > 0 lies outside)."""
    lg = np.asarray(logits, dtype=np.float32)
    m = lg.max()
    e = np.exp((lg - m) / np.float32(temperature)).astype(np.float32)
    f = np.floor(e.astype(np.float64) * 2.0 ** 40).astype(np.uint64)
    asc = np.sort(e)
    n_above = len(e) - np.searchsorted(asc, e, side="right")   # #{j : e_j > e_i}
    in_f = f > 0
    if min_p > 0:
        in_f &= e >= np.float32(min_p)
    if top_k > 0:
        in_f &= n_above < top_k
    margin = np.inf
    out = (f > 0) & ~in_f
    if out.any():
        lo_in, hi_out = float(e[in_f].min()), float(e[out].max())
        margin = (lo_in - hi_out) / lo_in
    fz = np.where(in_f, f, np.uint64(0))
    Z = int(fz.sum(dtype=np.uint64))
    thr = Z if top_p >= 1.0 else max(1, int(np.float64(Z) * np.float64(np.float32(top_p))))
    # mass strictly above each value, counted over F
    order = np.argsort(e, kind="stable")
    suffix = np.concatenate([np.cumsum(fz[order][::-1], dtype=np.uint64)[::-1],
                             np.zeros(1, dtype=np.uint64)])
    above = suffix[np.searchsorted(asc, e, side="right")]
    kept = in_f & (above < np.uint64(thr))
    return e, kept, in_f, f, thr, margin


def sample(logits, temperature: float, top_p: float, seed: int, pos: int, top_k: int = 0,
           min_p: float = 0.0, return_margin: bool = False):
    """One token at RNG counter ``pos``; with ``return_margin`` also (race margin, filter
    margin): a GPU token that differs is a near-tie when either is tiny."""
    lg = np.asarray(logits, dtype=np.float32)
    if temperature <= 0:
        tok = int(np.argmax(lg))
        return (tok, (np.inf, np.inf)) if return_margin else tok
    e, kept, _, _, _, fmargin = chain(lg, temperature, top_p, top_k, min_p)
    idx = np.nonzero(kept)[0]
    x = S.philox_x0(idx, pos, seed)
    u = ((x >> 9).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    s = e[idx] / -np.log(u)
    tok = int(idx[int(np.argmax(s))])
    if not return_margin:
        return tok
    srt = np.sort(s)
    race = float((srt[-1] - srt[-2]) / srt[-1]) if len(srt) > 1 else np.inf
    return tok, (race, float(fmargin))


def min_p_distance(logits, temperature: float, min_p: float) -> float:
    """Smallest relative distance of an e to the min-p bound (seed vetting: a step whose
    bound sits within an expf ulp of some e could go either way on the device)."""
    if not min_p > 0:
        return np.inf
    lg = np.asarray(logits, dtype=np.float32)
    e = np.exp((lg - lg.max()) / np.float32(temperature)).astype(np.float64)
    return float(np.min(np.abs(e - np.float64(np.float32(min_p)))) / np.float64(np.float32(min_p)))
