"""-m gpu: the best-path CTC alignment (csrc/ctc.hip: ctc_best_path_kernel + ctc_traceback_kernel, through api.Ctc.AlignParallel) held
per utterance against the fp64 restatement of the recurrence (tests/ctc_align_restatement.py) on the same float32 probabilities.

A result is a path, and a path is optimal or it is not.  Per utterance s, with bar_s = 64 * 2^-24 * |score64_s|
(tests/test_ctc_align_restatement.py derives it and holds, without a GPU, the conditions on these inputs that the checks rely on):

  the path is valid (starts in {0, 1}, ends in {L'-2, L'-1}, legal moves, collapses to the labels)
  |score - score64| <= bar_s
  the fp64 score summed along the RETURNED path >= score64 - bar_s
  the positions equal the fp64 restatement's exactly wherever the runner-up gap_s >= bar_s (everywhere but long_U2047)
  rows t >= len_s read -1, and the class ids are the labels at the positions

Legs: (1) both sides of every dispatch step of the sweep -- L' = 63, 65, 255, 257, 1023, 4095 -- ragged dense minibatches and peaky
posteriors down to denormals; (2) the edge of feasibility; (3) exact ties; (4) the conventions of the interface; (5) the statistics
and a following EvalParallel are untouched.
"""
import numpy as np
import pytest

from tests import ctc_align_restatement as R
from tests import ctc_cases as cc

pytestmark = pytest.mark.gpu


def _align(ctc, lens, probs, labels, is_log=False):
    from eesen_amd.api import CuMatrix
    return ctc.AlignParallel(lens, CuMatrix.from_numpy(probs), labels, is_log=is_log)


def _hold(name, lens, probs, labels, T, S, ref, got, exact="gap"):
    ali, pos, score = got
    assert ali.shape == pos.shape == (T, S) and score.shape == (S,)
    worst, same = 0.0, 0
    for s in range(S):
        n, r = int(lens[s]), ref[s]
        where = f"{name} utterance {s} (n {n}, U {len(labels[s])})"
        p = pos[:n, s]
        assert np.all(pos[n:, s] == -1) and np.all(ali[n:, s] == -1), where
        assert R.path_is_valid(p, labels[s], n), where
        assert np.array_equal(ali[:n, s], R.expand(labels[s])[p]), where
        err = abs(float(score[s]) - r["score64"])
        worst = max(worst, err / abs(r["score64"]))
        along = float(R.path_score(R.log64(R.utterance(probs, s, S, n)), labels[s], p))
        equal = np.array_equal(p, r["pos64"])
        same += equal
        print(f"{where}: score {score[s]:.7g} score64 {r['score64']:.10g} |err| {err:.3g} bar {r['bar']:.3g} along-path deficit "
              f"{r['score64'] - along:.3g} gap {r['gap']} path equal {equal}")
        assert err <= r["bar"], where
        assert along >= r["score64"] - r["bar"], where
        if exact == "all" or r["gap"] >= r["bar"]:
            assert equal, where
    print(f"{name}: worst |score - score64| / |score64| = {worst:.3g}; exact paths {same}/{S}")


@pytest.fixture(scope="module")
def ctc(gpu):
    from eesen_amd.api import Ctc
    return Ctc()


@pytest.mark.parametrize("name", R.DISPATCH_CASES)
def test_dispatch_edges(ctc, name):
    lens, probs, labels, T, S, ref = R.case(name)
    _hold(name, lens, probs, labels, T, S, ref, _align(ctc, lens, probs, labels))


@pytest.mark.parametrize("name", R.FEASIBILITY_CASES)
def test_edge_of_feasibility(ctc, name):
    """One spare frame, and none: one_short_* has exactly one path per utterance (it ends on the last label, the final blank is
    unreachable), which the ln p formula of EvalParallel cannot handle and this call must simply return, with its score."""
    lens, probs, labels, T, S, ref = R.case(name)
    got = _align(ctc, lens, probs, labels)
    _hold(name, lens, probs, labels, T, S, ref, got, exact="all")
    if name.startswith("one_short"):
        for s in range(S):
            assert ref[s]["gap"] == float("inf") and got[1][int(lens[s]) - 1, s] == 2 * len(labels[s]) - 1


def test_ties_class0(ctc):
    """A label that names class 0 and the blanks beside it emit the same class: bit-identical scores, the tie rule decides."""
    lens, probs, labels, T, S, ref = R.case("peaky_class0")
    _hold("peaky_class0", lens, probs, labels, T, S, ref, _align(ctc, lens, probs, labels), exact="all")


def test_ties_uniform_rows(ctc):
    """Every row uniform: every reachable cell ties and the path is the tie rule's alone."""
    lens, probs, labels, T, S = R.uniform_case()
    ref = R.reference_of(lens, probs, labels, S)
    _hold("uniform", lens, probs, labels, T, S, ref, _align(ctc, lens, probs, labels), exact="all")


def test_conventions(ctc):
    from eesen_amd.api import CuMatrix, EesenError
    S, T, K = 4, 12, 6
    rng = np.random.default_rng(77)
    probs = cc.softmax32(rng.standard_normal((T * S, K)).astype(np.float32) * np.float32(2))
    labels = [np.array(l, np.int32) for l in ([2, 3], [4, 4, 1, 5], [3, 1, 1, 2], [5])]
    lens = np.array([0, 4, T, 1], np.int32)     # empty; U + repeats - 1 = 4 (infeasible); full length; one label on one frame
    ld = K + 3
    buf = rng.standard_normal((T * S, ld)).astype(np.float32) * np.float32(1e6)    # garbage in the pad columns
    buf[:, :K] = probs
    own = CuMatrix.from_numpy(buf.reshape(1, -1))
    assert own.stride == T * S * ld
    m = CuMatrix.view(own.ptr, T * S, K, ld, keepalive=own)
    ali, pos, score = ctc.AlignParallel(lens, m, labels)
    for s in (0, 1):
        assert score[s] == np.float32(-1e30) and np.all(ali[:, s] == -1) and np.all(pos[:, s] == -1)
    ref = R.reference_of(lens, probs, labels, S, with_gap=False)
    for s in (2, 3):
        n = int(lens[s])
        one = ctc.AlignParallel([n], CuMatrix.from_numpy(np.ascontiguousarray(probs[s::S][:T])), [labels[s]])   # the neighbour alone, S = 1
        assert one[2][0] == score[s] and np.array_equal(one[1][:, 0], pos[:, s]) and np.array_equal(one[0][:, 0], ali[:, s])
        assert np.all(pos[n:, s] == -1) and np.all(ali[n:, s] == -1)
        assert R.path_is_valid(pos[:n, s], labels[s], n) and np.array_equal(pos[:n, s], ref[s]["pos64"])
        assert abs(float(score[s]) - ref[s]["score64"]) <= ref[s]["bar"]
    assert pos[0, 3] == 1 and ali[0, 3] == 5
    # is_log: the logarithm taken by the test
    logm = buf.copy()
    logm[:, :K] = R.log32(probs)
    own2 = CuMatrix.from_numpy(logm.reshape(1, -1))
    ali2, pos2, score2 = ctc.AlignParallel(lens, CuMatrix.view(own2.ptr, T * S, K, ld, keepalive=own2), labels, is_log=True)
    assert np.array_equal(pos2, pos) and np.array_equal(ali2, ali)
    for s in range(S):
        assert abs(float(score2[s]) - float(score[s])) <= (ref[s]["bar"] if s >= 2 else 0.0)
    # refused: a label outside [0, K), an empty label sequence
    for bad in ([labels[0], labels[1], np.array([1, K], np.int32), labels[3]], [labels[0], np.array([], np.int32), labels[2], labels[3]]):
        with pytest.raises(EesenError) as e:
            ctc.AlignParallel(lens, m, bad)
        assert e.value.code == -1      # EESEN_ERR_INVALID


def test_guard_word_set_returns_nan_and_minus_one(gpu):
    """Aligned from a timed-out forward pass (the guarded Net's error word raised): -1 and NaN, never garbage with status OK."""
    from eesen_amd import synth
    from eesen_amd.api import Net, Ctc
    lens, probs, labels, T, S, _ = R.case("dense_3x12x7")
    net = Net.from_layers(synth.make_model(**synth.config("tiny_bi")))
    ctc = Ctc()
    ctc.SetGuard(net)
    ok = _align(ctc, lens, probs, labels)
    for s in range(S):
        assert np.all(ok[0][:int(lens[s]), s] >= 0) and np.all(ok[1][:int(lens[s]), s] >= 0)
    assert np.all(np.isfinite(ok[2]))
    net._raise_error_word(2)
    ali, pos, score = _align(ctc, lens, probs, labels)
    assert np.all(ali == -1) and np.all(pos == -1) and np.all(np.isnan(score))
    net._raise_error_word(0)
    again = _align(ctc, lens, probs, labels)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, ok))
    ctc.SetGuard(None)


def test_statistics_and_eval_parallel_untouched(gpu):
    from eesen_amd.api import Ctc, CuMatrix
    lens, probs, labels, T, S, _ = R.case("dense_3x12x7")
    lens2, probs2, labels2, T2, S2, _ = R.case("boundary_U32")
    net_out = CuMatrix.from_numpy(probs)
    plain = Ctc()
    want_diff = plain.EvalParallel(lens, net_out, labels).numpy()
    want_pzx = plain.pzx.copy()
    ctc = Ctc()
    ctc.EvalParallel(lens, net_out, labels)
    ctc.ErrorRateMSeq(lens, net_out, labels)
    before = ctc.stats()
    ctc.AlignParallel(lens2, CuMatrix.from_numpy(probs2), labels2)      # another shape: borrows and regrows alpha / logp
    ctc.AlignParallel(lens, net_out, labels)
    assert ctc.stats() == before
    diff = ctc.EvalParallel(lens, net_out, labels).numpy()
    assert np.array_equal(diff, want_diff) and np.array_equal(ctc.pzx, want_pzx)
    after = ctc.stats()
    assert after["sequences"] == before["sequences"] + S and after["frames"] == before["frames"] + int(lens.sum())
