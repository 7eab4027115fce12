"""CPU checks of the extended sampler-chain restatement (tests/_sampler_chain.py): it reduces
to oracle/sampling_ref.py at neutral values, its filters match brute force, the draw follows
the renormalised kept distribution, and the penalty window covers the right ids."""
import numpy as np

from oracle import sampling_ref as S

import _sampler_chain as SC


def test_neutral_values_reduce_to_the_oracle():
    rng = np.random.default_rng(5)
    for trial in range(24):
        n = int(rng.integers(2, 400))
        lg = rng.normal(0, float(rng.choice([0.2, 1, 6])), n).astype(np.float32)
        if trial % 3 == 0:
            lg = np.round(lg, 1)  # ties
        if trial % 5 == 0:
            lg[: n // 2] -= 60.0  # f = 0 tail
        for t in (0.6, 1.0):
            for p in (0.9, 1.0):
                e0, kept0, f0, thr0 = S.nucleus(lg, t, p)
                e, kept, in_f, f, thr, fm = SC.chain(lg, t, p)
                np.testing.assert_array_equal(e, e0)
                np.testing.assert_array_equal(f, f0)
                np.testing.assert_array_equal(kept, kept0)
                np.testing.assert_array_equal(in_f, f0 > 0)
                assert thr == thr0 and fm == np.inf
                for pos in (0, 3, 77):
                    want, wm = S.sample(lg, t, p, 1234 + trial, pos, return_margin=True)
                    got, (race, _) = SC.sample(lg, t, p, 1234 + trial, pos, return_margin=True)
                    assert got == want and race == wm
    assert SC.sample(np.array([0.1, 3.0, 3.0, -1.0], np.float32), 0.0, 0.9, 1, 5) == 1


def _brute(e, f, top_p, top_k, min_p):
    n = len(e)
    in_f = np.array([f[i] > 0 and e[i] >= np.float32(min_p)
                     and (top_k == 0 or int((e > e[i]).sum()) < top_k) for i in range(n)])
    Z = int(sum(int(f[i]) for i in range(n) if in_f[i]))
    thr = Z if top_p >= 1.0 else max(1, int(np.float64(Z) * np.float64(np.float32(top_p))))
    kept = np.array([in_f[i] and sum(int(f[j]) for j in range(n) if in_f[j] and e[j] > e[i]) < thr
                     for i in range(n)])
    return in_f, kept, thr


def test_filters_match_brute_force():
    rng = np.random.default_rng(6)
    for trial in range(40):
        n = int(rng.integers(2, 120))
        lg = rng.normal(0, float(rng.choice([0.3, 1, 4])), n).astype(np.float32)
        if trial % 2 == 0:
            lg = np.round(lg, 1)  # tie groups, some straddling the k-th place
        if trial % 7 == 0:
            lg[: n // 3] -= 80.0
        t = float(rng.choice([0.6, 1.0]))
        p = float(rng.choice([0.3, 0.8, 1.0]))
        k = int(rng.choice([0, 1, 3, 10, 500]))
        mp = float(rng.choice([0.0, 0.01, 0.2, 1.0]))
        e, kept, in_f, f, thr, _ = SC.chain(lg, t, p, k, mp)
        b_in, b_kept, b_thr = _brute(e, f, p, k, mp)
        np.testing.assert_array_equal(in_f, b_in)
        np.testing.assert_array_equal(kept, b_kept)
        assert thr == b_thr
        assert kept[np.argmax(lg)]


def test_draw_follows_the_renormalised_kept_distribution():
    pr = np.array([0.30, 0.20, 0.15, 0.15, 0.05, 0.04, 0.03, 0.03, 0.02, 0.01, 0.01, 0.01],
                  dtype=np.float64)
    lg = np.log(pr).astype(np.float32)
    # T = 1.  top_k = 3 keeps ids 0-3 (ids 2 and 3 tie at the third place), min_p = 0.2 of the
    # top probability (0.06) agrees; over F the masses are 0.30 0.20 0.15 0.15 of Z = 0.80 and
    # top_p = 0.8 gives thr = 0.64: the mass above the tie group is 0.50 < 0.64, so all four stay
    e, kept, in_f, *_ = SC.chain(lg, 1.0, 0.8, 3, 0.2)
    assert np.nonzero(in_f)[0].tolist() == [0, 1, 2, 3]
    assert np.nonzero(kept)[0].tolist() == [0, 1, 2, 3]
    counts = np.zeros(12)
    for pos in range(6000):
        counts[SC.sample(lg, 1.0, 0.8, 11, pos, top_k=3, min_p=0.2)] += 1
    np.testing.assert_allclose(counts[:4] / counts.sum(), pr[:4] / pr[:4].sum(), atol=0.02)
    assert counts[4:].sum() == 0
    # Z is taken over F.  top_p 0.7 unfiltered: thr = 0.70 of Z = 1, the tie group stays
    # (0.50 above it).  Over F = {0, 1} (top_k 2) Z = 0.50: thr = 0.35 keeps id 1 (0.30 above
    # it), and top_p 0.5 (thr = 0.25) drops it
    assert np.nonzero(SC.chain(lg, 1.0, 0.7)[1])[0].tolist() == [0, 1, 2, 3]
    assert np.nonzero(SC.chain(lg, 1.0, 0.7, 2)[1])[0].tolist() == [0, 1]
    assert np.nonzero(SC.chain(lg, 1.0, 0.5, 2)[1])[0].tolist() == [0]


def test_filter_margin_is_the_gap_at_the_boundary():
    lg = np.log(np.array([0.5, 0.25, 0.125, 0.125], dtype=np.float64)).astype(np.float32)
    *_, fm = SC.chain(lg, 1.0, 1.0, 2)
    assert abs(fm - 0.5) < 1e-6          # inside down to 0.5 (of the top), outside from 0.25
    *_, fm = SC.chain(lg, 1.0, 1.0, 3)   # the tie at the third place is kept whole
    assert fm == np.inf


def test_window_rule():
    ids = [9, 4, 4, 7, 5, 4, 2]
    # whole sequence
    assert SC.window_ids(ids, 4, 0) == {9, 4, 7}
    # N = 3: positions p-3 .. p-1
    assert SC.window_ids(ids, 4, 3) == {4, 7}       # positions 1, 2, 3: id 4 counted twice
    assert SC.window_ids(ids, 5, 3) == {4, 7, 5}    # one 4 evicted, the other still inside
    assert SC.window_ids(ids, 6, 3) == {7, 5, 4}    # ... and 4 came back at position 5
    assert SC.window_ids(ids, 7, 3) == {5, 4, 2}
    assert SC.window_ids(ids, 2, 3) == {9, 4}       # window longer than the sequence
    assert SC.window_ids(ids, 5, 1) == {5}
    ids2 = [1, 8, 8, 3, 6, 6, 6]
    assert 8 in SC.window_ids(ids2, 4, 3) and 8 in SC.window_ids(ids2, 5, 3)
    assert 8 not in SC.window_ids(ids2, 6, 3)       # penalised for exactly one more step
    raw = np.array([2.0, -2.0, 1.0, -1.0, 0.5, 4.0, 0.0, 3.0, -3.0, 1.5], dtype=np.float32)
    got = SC.penalise(raw, ids, 5, 2.0, 3)
    want = raw.copy()
    want[4], want[7], want[5] = 0.25, 1.5, 2.0
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(SC.penalise(raw, ids, 5, 1.0, 3), raw)
