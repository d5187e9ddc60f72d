"""CPU: the numpy restatement of the CTC prefix beam search (tests/ctc_beam_restatement.py) against path enumeration and against the
exact ln p of a labelling, and the conditions on the INPUTS that the checks of tests/test_gpu_ctc_decode.py rely on.

The bar of every comparison with the fp64 restatement, per utterance s of n_s frames:

  bar_s = 64 * 2^-24 * |score64_s| + 4e-7 * sqrt(n_s)

The first term is the alignment's bar (tests/test_ctc_align_restatement.py): a score is a chain of n fp32 additions of log-scores, each
rounded to 2^-24 of the running magnitude, with the fp32 logarithm's own rounding on every term; 64 of them leave room for the
chain's length.  The second is csrc/ctc.hip's documented bound of the hardware log-add (4e-7 absolute on log(1 + e^d)), once per
frame, accumulated as a random walk: scores of confident posteriors sit near 0, where a relative bar means nothing.

What is held here, without a GPU:
  * without pruning the restatement IS the sum over paths: on the exhaustive case every labelling of non-zero probability comes back
    with its enumerated ln p;
  * beam search never over-counts: score <= lnp64(hyp) + bar for every entry of every final beam;
  * the fp32 restatement agrees with the fp64 one wherever the GPU test demands agreement (stable utterances: same 1-best, scores
    within the bar; measured: within 0.06 of the bar);
  * at most one eighth (rounded down) of a case's utterances is unstable under the selection jitter.
The restatement takes under ten seconds on every case, so no results travel as fixtures.
"""
import numpy as np
import pytest

from tests import ctc_beam_restatement as R
from tests import ctc_decode_cases as dc

CONFIGS = [(name, B, C) for name, cfgs in dc.CONFIGS.items() for B, C in cfgs]


def test_exhaustive_equals_path_enumeration():
    lens, probs, T, S, ref = R.case("exhaustive", 64, 2)
    for s in range(S):
        n = int(lens[s])
        lp = R.log64(R.utterance(probs, s, S, n))
        want = R.enumerate_paths(lp)
        got = dict(ref[s]["beam64"])
        assert len(got) == len(ref[s]["beam64"]) and set(got) == set(want), s
        assert len(want) <= 2 ** (n + 1) - 1
        for hyp, v in want.items():
            assert abs(got[hyp] - v) <= 1e-9 * max(1.0, abs(v)), (s, hyp)
            assert abs(R.lnp64(lp, hyp) - v) <= 1e-9 * max(1.0, abs(v)), (s, hyp)
        assert ref[s]["beam64"][0][0] == max(want, key=want.get)
        scores = [v for _, v in ref[s]["beam64"]]
        assert scores == sorted(scores, reverse=True)


def test_lnp64_conventions():
    lp = R.log64(np.array([[0.5, 0.25, 0.25]], np.float32))
    assert R.lnp64(lp[:0], ()) == 0.0 and R.lnp64(lp[:0], (1,)) == R.NEG
    assert abs(R.lnp64(lp, ()) - np.log(0.5)) < 1e-12 and abs(R.lnp64(lp, (2,)) - np.log(0.25)) < 1e-12
    assert R.lnp64(np.concatenate([lp, lp]), (1, 1)) <= -1e29          # a repeat needs a blank between: three frames


@pytest.mark.parametrize("name,B,C", CONFIGS)
def test_conditions_the_gpu_checks_rely_on(name, B, C):
    lens, probs, T, S, ref = R.case(name, B, C)
    unstable, worst = [], 0.0
    for s in range(S):
        r, n = ref[s], int(lens[s])
        where = f"{name} ({B}, {C}) utterance {s} (n {n})"
        lp = R.log64(R.utterance(probs, s, S, n))
        hyps = [h for h, _ in r["beam64"]]
        assert 1 <= len(hyps) <= B and len(set(hyps)) == len(hyps), where
        for hyp, v in r["beam64"]:
            assert v <= R.lnp64(lp, hyp) + r["bar"], (where, hyp)
            assert len(hyp) <= n and all(1 <= c < probs.shape[1] for c in hyp), (where, hyp)
        if not r["stable"]:
            unstable.append(s)
            continue
        assert r["beam32"][0][0] == r["beam64"][0][0], where
        fig = abs(r["beam32"][0][1] - r["score64"]) / r["bar"]
        worst = max(worst, fig)
        assert fig <= 1.0, where
    print(f"{name} ({B}, {C}): unstable {unstable} of {S}; worst fp32 |score - score64| / bar = {worst:.3g}")
    assert len(unstable) <= S // 8, unstable


def test_candidates_tie_to_the_smaller_id_in_ascending_order():
    row = np.array([9, 1, 3, 3, 0, 3, 2], np.float32)        # blank 9 never a candidate; three classes tie at 3
    assert R.candidates(row, 2).tolist() == [2, 3]
    assert R.candidates(row, 4).tolist() == [2, 3, 5, 6]
    assert R.candidates(row, 64).tolist() == [1, 2, 3, 4, 5, 6]
