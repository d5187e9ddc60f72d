"""CPU: the numpy restatement of the best-path CTC alignment (tests/ctc_align_restatement.py) against path enumeration and against
ln p, and the conditions on the INPUTS that the bars of tests/test_gpu_ctc_align.py rely on.

Why bar_s = 64 * 2^-24 * |score64_s|.  A path's score is n sequential fp32 additions; their worst-case rounding bound is
(n+1) * 2^-24 relative (1.7e-4 at n = 2900), far above what random rounding does.  What the fp32 restatement shows over the cases
below is at most 5.8e-7 relative, with the fp32 path equal to the fp64 path in every utterance; 64 * 2^-24 = 3.8e-6 is 6.6 times
that.  The smallest runner-up gap outside long_U2047 is 3.9e-3 nats on a score of about 200 (bar 7.6e-4); long_U2047 has gaps of
6e-4 and 8e-3 nats on scores of several thousand, below its bars, and is the one case whose positions the GPU test may not demand.
peaky_class0 has gap 0 in two utterances: a label that names class 0 and the blank beside it emit the same class, the two paths
have bit-identical scores in either precision, and the tie rule decides.  These are conditions on the inputs: a case that fails
one gets another seed, the bar stays.
"""
import itertools

import numpy as np
import pytest

from tests import ctc_align_restatement as R
from tests import ctc_cases as cc


def _softmax(x):
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def _all_paths(L, T, sk):
    """Every position sequence that starts in {0, 1}, ends in {L-2, L-1} and moves legally."""
    def grow(path):
        if len(path) == T:
            if path[-1] >= L - 2:
                yield path
            return
        j = path[-1]
        for b in (j, j + 1, j + 2):
            if b < L and (b != j + 2 or sk[b]):
                yield from grow(path + [b])
    for j0 in (0, 1):
        yield from grow([j0])


@pytest.mark.parametrize("T,K,label", [(4, 3, [1]), (5, 3, [1, 2]), (5, 3, [1, 1]), (6, 3, [2, 1, 2])])
def test_score_is_the_maximum_over_all_enumerated_paths(T, K, label):
    rng = np.random.default_rng(T * 10 + K)
    lp = np.log(_softmax(rng.standard_normal((T, K))))
    lab = R.expand(label)
    paths = list(_all_paths(lab.size, T, R._skip(lab)))
    assert paths and all(R.path_is_valid(np.array(p), label, T) for p in paths)
    # the enumeration is the set of valid paths: every class sequence that collapses to the label is one of them
    n_cls = sum(1 for c in itertools.product(range(K), repeat=T)
                if [k for k, _ in itertools.groupby(c) if k != 0] == list(label))
    assert len({tuple(lab[list(p)]) for p in paths}) == n_cls
    best = max(sum(lp[t, lab[j]] for t, j in enumerate(p)) for p in paths)
    for dt, tol in ((np.float64, 1e-12), (np.float32, 1e-5)):
        pos, cls, score = R.viterbi(lp, label, dt)
        assert R.path_is_valid(pos, label, T) and np.array_equal(cls, lab[pos])
        assert abs(float(score) - best) < tol
        assert abs(float(R.path_score(lp, label, pos)) - best) < tol


def test_tie_rule_and_infeasible_convention():
    lens, probs, labels, T, S = R.uniform_case()
    for s in range(S):
        lp = R.log64(R.utterance(probs, s, S, T))
        pos64, _, sc64 = R.viterbi(lp, labels[s], np.float64)
        pos32, _, sc32 = R.viterbi(R.log32(R.utterance(probs, s, S, T)), labels[s], np.float32)
        assert R.path_is_valid(pos64, labels[s], T) and np.array_equal(pos64, pos32)
        # stay wins every tie on the way back and the final blank wins at the end: the labels sit on the FIRST frames
        # (walking backwards the path stays on a position as long as it can), adjacent repeats with their blank between
        L = 2 * len(labels[s]) + 1
        assert pos64[-1] == L - 1 and pos64[0] in (0, 1)
        assert R.runner_up_gap(lp, labels[s]) < 1e-9
    # infeasible: one frame fewer than labels + adjacent repeats; no frames
    lp = np.log(_softmax(np.random.default_rng(0).standard_normal((3, 4))))
    pos, cls, score = R.viterbi(lp[:2], [1, 1], np.float32)
    assert score == np.float32(-1e30) and np.all(pos == -1) and np.all(cls == -1)
    assert R.viterbi(lp[:0], [1], np.float64)[2] == -1e30
    # the shortest feasible length has exactly one path, ending on the last label
    pos, cls, score = R.viterbi(lp, [1, 2, 1], np.float64)
    assert list(pos) == [1, 3, 5] and abs(score - (lp[0, 1] + lp[1, 2] + lp[2, 1])) < 1e-12
    assert R.runner_up_gap(lp, [1, 2, 1]) == float("inf")


def test_best_path_score_is_below_ln_p():
    lens, probs, labels, T, S, ref = R.case("dense_3x12x7")
    _, o64 = cc.oracle_pair(lens, probs, labels, T, S)
    for s in range(S):
        assert ref[s]["score64"] <= o64["pzx"][s] + 1e-12
        assert ref[s]["score64"] > o64["pzx"][s] - lens[s] * np.log(2 * len(labels[s]) + 1)   # at most L'^n paths


@pytest.mark.parametrize("name", R.DISPATCH_CASES + R.FEASIBILITY_CASES + R.TIE_CASES)
def test_case_list_condition(name):
    lens, probs, labels, T, S, ref = R.case(name)
    for s in range(S):
        r = ref[s]
        where = f"{name} utterance {s}: score64 {r['score64']:.6g} score32 {r['score32']:.6g} gap {r['gap']:.3g} bar {r['bar']:.3g}"
        assert r["score64"] > -1e29 and R.path_is_valid(r["pos64"], labels[s], int(lens[s])), where
        assert np.array_equal(r["pos32"], r["pos64"]), where
        assert abs(r["score32"] - r["score64"]) <= r["bar"], where
        if name in R.TIE_CASES:
            assert r["gap"] >= r["bar"] or abs(r["gap"]) <= 1e-9 * abs(r["score64"]), where      # an exact tie or a clear winner
        elif name not in R.GAP_EXEMPT:
            assert r["gap"] >= r["bar"], where
