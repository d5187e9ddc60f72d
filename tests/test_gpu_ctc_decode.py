"""-m gpu: the CTC prefix beam search (csrc/ctc_decode.hip: ctc_row_topc_kernel + ctc_prefix_beam_kernel<false> + ctc_hyp_kernel, through
api.Ctc.DecodeParallel) held per utterance against the fp64 restatement of the computation (tests/ctc_beam_restatement.py) and
against the exact ln p of every returned labelling, on the same float32 posteriors.

Every test holds, per utterance s (bar_s = 64 * 2^-24 * |score64_s| + 4e-7 * sqrt(n_s); tests/test_ctc_beam_restatement.py derives
it and holds, without a GPU, the conditions on these inputs that the checks rely on):

  count, lengths, -1 / -1e30 padding, scores descending, labellings pairwise distinct, no blank and no id >= K, length <= n_s
  every returned entry i:  score_i <= lnp64(hyp_i) + bar_s            (beam search never over-counts)
  stable utterances:       the 1-best labelling is the restatement's, and |score - score64| <= bar_s

Each case prints `worst |score - score64| / bar` (recorded in profiles/ctc_decode.md).

The exhaustive case as the issue words it ("each of the 2^(n+1) - 1 labellings is returned") overlooks that a labelling with adjacent
repeats needs a blank between them: with n = 5 the labelling 1 1 1 1 1 has no path.  The test asks for what the wording means: the
returned set IS the set of labellings path enumeration gives a non-zero probability, each with its enumerated ln p.
"""
import numpy as np
import pytest

from tests import ctc_beam_restatement as R
from tests import ctc_cases as cc
from tests import ctc_decode_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctc(gpu):
    from eesen_amd.api import Ctc
    return Ctc()


def _decode(ctc, lens, m, B, C, N, is_log=False):
    """(hyps, scores [S, N], raw labels [S, N, T], lengths [S, N]); m: numpy matrix or CuMatrix."""
    from eesen_amd.api import CuMatrix
    if isinstance(m, np.ndarray):
        m = CuMatrix.from_numpy(m)
    hyps, scores = ctc.DecodeParallel(lens, m, beam=B, max_classes=C, nbest=N, is_log=is_log)
    return hyps, scores, ctc.hyp.copy(), ctc.hyp_len.copy()


def _invariants(name, lens, logp64_of, K, got, N, bars, counts=None):
    """What holds whatever the pruning decided.  logp64_of(s): the utterance's fp64 log-scores [n x K]."""
    hyps, scores, raw, hlen = got
    S = len(lens)
    assert scores.shape == hlen.shape == (S, N) and raw.shape[:2] == (S, N)
    for s in range(S):
        n = int(lens[s])
        where = f"{name} utterance {s} (n {n})"
        count = len(hyps[s])
        assert count <= N and np.all(hlen[s, :count] >= 0) and np.all(hlen[s, count:] == -1), where
        assert np.all(scores[s, count:] == np.float32(-1e30)) and np.all(raw[s, count:] == -1), where
        if counts is not None:
            assert count == counts[s], (where, count, counts[s])
        assert np.all(np.diff(scores[s, :count]) <= 0), where
        assert len(set(map(tuple, hyps[s]))) == count, where
        lp = logp64_of(s)
        for i, h in enumerate(hyps[s]):
            assert len(h) == hlen[s, i] <= n and np.all(raw[s, i, len(h):] == -1) and all(1 <= c < K for c in h), (where, i)
            assert float(scores[s, i]) <= R.lnp64(lp, h) + bars[s], (where, i, float(scores[s, i]), R.lnp64(lp, h), bars[s])


def _hold(name, lens, probs, S, ref, got, N, is_log=False):
    K = probs.shape[1]
    as64 = (lambda p: np.maximum(np.asarray(p, np.float64), R.NEG)) if is_log else R.log64
    _invariants(name, lens, lambda s: as64(R.utterance(probs, s, S, int(lens[s]))), K, got, N, [r["bar"] for r in ref],
                counts=[min(N, len(r["beam64"])) for r in ref])
    hyps, scores = got[0], got[1]
    worst, same, unstable = 0.0, 0, []
    for s in range(S):
        r = ref[s]
        where = f"{name} utterance {s} (n {int(lens[s])})"
        if not r["beam64"]:
            continue
        equal = tuple(hyps[s][0]) == r["beam64"][0][0]
        same += equal
        err = abs(float(scores[s, 0]) - r["score64"])
        print(f"{where}: score {scores[s, 0]:.7g} score64 {r['score64']:.10g} |err| {err:.3g} bar {r['bar']:.3g} stable {r['stable']} 1-best equal {equal}")
        if not r["stable"]:
            unstable.append(s)
            continue
        worst = max(worst, err / r["bar"] if r["bar"] > 0 else 0.0)
        assert equal, (where, hyps[s][0], r["beam64"][0][0])
        assert err <= r["bar"], where
    print(f"{name}: worst |score - score64| / bar = {worst:.3g}; 1-best equal {same}/{S}; unstable {unstable}")


@pytest.mark.parametrize("name,B,C", [(n, B, C) for n, cfgs in dc.CONFIGS.items() if n != "exhaustive" for B, C in cfgs])
def test_cases(ctc, name, B, C):
    lens, probs, T, S, ref = R.case(name, B, C)
    N = min(B, 4)
    _hold(f"{name} ({B}, {C})", lens, probs, S, ref, _decode(ctc, lens, probs, B, C, N), N)


def test_exhaustive(ctc):
    """Nothing is ever pruned: the result is the sum over paths, labelling by labelling."""
    B, C, N = 64, 2, 63
    lens, probs, T, S, ref = R.case("exhaustive", B, C)
    got = _decode(ctc, lens, probs, B, C, N)
    _hold("exhaustive", lens, probs, S, ref, got, N)
    hyps, scores = got[0], got[1]
    for s in range(S):
        n, bar = int(lens[s]), ref[s]["bar"]
        want = R.enumerate_paths(R.log64(R.utterance(probs, s, S, n)))
        assert set(map(tuple, hyps[s])) == set(want), s
        for i, h in enumerate(hyps[s]):
            assert abs(float(scores[s, i]) - want[tuple(h)]) <= bar, (s, h)
        order = sorted(want, key=want.get, reverse=True)
        assert tuple(hyps[s][0]) == order[0], s
        for i, h in enumerate(order):       # the order is exact wherever the neighbouring scores are 2 bars away
            lo = want[order[i - 1]] - want[h] if i else np.inf
            hi = want[h] - want[order[i + 1]] if i + 1 < len(order) else np.inf
            if min(lo, hi) >= 2 * bar:
                assert tuple(hyps[s][i]) == h, (s, i)


@pytest.mark.parametrize("name,B,C", [("wide_K4100", 8, 64), ("dense_33x40x100", 32, 64), ("dense_8x60x46", 16, 20)])
def test_candidate_classes_are_numpys(ctc, name, B, C):
    """The candidate ids and scores of every frame, exactly: many values per lane (K = 4100), two per lane in registers (K = 100),
    less than a wave (K = 46).  On log-domain input, so that both sides compare the very same floats."""
    lens, probs, T, S = dc.build(name)
    logs = R.log32(probs)
    got = _decode(ctc, lens, logs, B, C, 1, is_log=True)
    ids, sc, bl = ctc.DecodeCandidates(T * S, C)
    Cc = min(C, logs.shape[1] - 1)
    assert ids.shape == sc.shape == (T * S, Cc)
    for r in range(T * S):
        if r // S >= lens[r % S]:
            assert np.all(ids[r] == -1) and bl[r] == np.float32(-1e30)
            continue
        want = R.candidates(logs[r], C)
        assert np.array_equal(ids[r], want), (r, ids[r], want)
        assert np.array_equal(sc[r], logs[r, want]) and bl[r] == logs[r, 0], r
    ref = R.reference_of(lens, logs, S, B, C, is_log=True)
    _hold(f"{name} log ({B}, {C})", lens, logs, S, ref, got, 1, is_log=True)


def test_one_hot_rows_decode_to_the_greedy_collapse_with_score_0(ctc):
    S, T, K = 2, 14, 6
    paths = [[0, 2, 2, 0, 2, 3, 3, 0, 0, 5, 1, 1, 0, 0], [4, 4, 0, 4, 1, 0, 0, 0, 2, 2, 2, 3, 0, 5]]
    lens = np.array([T, T - 1], np.int32)
    probs = np.zeros((T * S, K), np.float32)
    for s, p in enumerate(paths):
        probs[np.arange(T) * S + s, p] = 1
    hyps, scores, _, hlen = _decode(ctc, lens, probs, 16, 5, 2)
    for s in range(S):
        assert tuple(hyps[s][0]) == R.collapse(paths[s][:int(lens[s])]) and len(hyps[s]) == 1 and hlen[s, 1] == -1
        assert abs(float(scores[s, 0])) <= 4e-7 * np.sqrt(T)


@pytest.mark.parametrize("name", dc.TIE_CASES)
def test_ties_are_deterministic(ctc, name):
    """Exact ties between classes and between prefixes: the order is the tie rule's, the same on every call."""
    lens, probs, T, S = dc.build(name)
    B, C, N = 8, 4, 8
    a = _decode(ctc, lens, probs, B, C, N)
    b = _decode(ctc, lens, probs, B, C, N)
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    ref = R.reference_of(lens, probs, S, B, C)
    _invariants(name, lens, lambda s: R.log64(R.utterance(probs, s, S, int(lens[s]))), probs.shape[1], a, N, [r["bar"] for r in ref])
    if name == "uniform":        # every class ties: the candidates are classes 1 .. C, and the first extension is class 1
        ids, _, _ = ctc.DecodeCandidates(T * S, C)
        assert np.all(ids[:S] == np.arange(1, C + 1))


def test_conventions(ctc):
    from eesen_amd.api import CuMatrix, EesenError
    from eesen_amd import _lib
    import ctypes as C
    S, T, K = 4, 12, 6
    rng = np.random.default_rng(78)
    probs = cc.softmax32(rng.standard_normal((T * S, K)).astype(np.float32) * np.float32(2))
    lens = np.array([0, 5, T, 1], np.int32)          # no frames beside ordinary utterances
    B, Cm, N = 8, 3, 3
    ref = R.reference_of(lens, probs, S, B, Cm)
    # ld > K, garbage in the pad columns
    ld = K + 3
    buf = rng.standard_normal((T * S, ld)).astype(np.float32) * np.float32(1e6)
    buf[:, :K] = probs
    own = CuMatrix.from_numpy(buf.reshape(1, -1))
    m = CuMatrix.view(own.ptr, T * S, K, ld, keepalive=own)
    got = _decode(ctc, lens, m, B, Cm, N)
    _hold("conventions", lens, probs, S, ref, got, N)
    assert got[0][0] == [[]] and got[1][0, 0] == 0.0 and got[3][0].tolist() == [0, -1, -1]
    plain = _decode(ctc, lens, probs, B, Cm, N)
    for x, y in zip(got[1:], plain[1:]):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    # is_log on what eesen_op_log_sub_prior leaves (log-posteriors minus scaled log-priors: scores above 0 occur)
    pri = np.log(np.array([0.6, 0.1, 0.05, 0.1, 0.05, 0.1], np.float32))
    dev = CuMatrix.from_numpy(probs)
    _lib.check(_lib.load().eesen_op_log_sub_prior(0, None, C.c_void_p(dev.ptr), dev.rows, dev.cols, dev.stride, 1,
                                                  pri.ctypes.data_as(C.c_void_p), C.c_float(0.8)))
    llk = dev.numpy()
    assert llk.max() > 0
    _hold("log_sub_prior", lens, llk, S, R.reference_of(lens, llk, S, B, Cm, is_log=True), _decode(ctc, lens, dev, B, Cm, N, is_log=True), N, is_log=True)
    # an all -inf row under is_log: that utterance's beam dies, the others are untouched
    logs = R.log32(probs)
    base = _decode(ctc, lens, logs, B, Cm, N, is_log=True)
    dead = logs.copy()
    dead[3 * S + 2] = -np.inf                        # frame 3 of utterance 2
    hyps, scores, raw, hlen = _decode(ctc, lens, dead, B, Cm, N, is_log=True)
    assert hyps[2] == [] and np.all(hlen[2] == -1) and np.all(scores[2] == np.float32(-1e30)) and np.all(raw[2] == -1)
    for s in (0, 1, 3):
        assert hyps[s] == base[0][s] and np.array_equal(scores[s], base[1][s])
    # each limit, violated once
    for kw, word in ((dict(beam=0), "beam"), (dict(beam=65), "beam"), (dict(max_classes=0), "max_classes"), (dict(max_classes=65), "max_classes"),
                     (dict(beam=64, max_classes=33), "beam * max_classes"), (dict(nbest=0), "nbest"), (dict(beam=4, nbest=5), "nbest")):
        with pytest.raises(EesenError) as e:
            ctc.DecodeParallel(lens, dev, **kw)
        assert e.value.code == -1 and word in str(e.value), kw      # EESEN_ERR_INVALID
    with pytest.raises(EesenError) as e:
        ctc.DecodeParallel(lens, CuMatrix.from_numpy(np.ones((T * S, 1), np.float32)))
    assert e.value.code == -1


def test_guard_word_set_returns_nan_and_minus_one(gpu):
    from eesen_amd import synth
    from eesen_amd.api import Net, Ctc
    lens, probs, T, S = dc.build("dense_3x12x7")
    net = Net.from_layers(synth.make_model(**synth.config("tiny_bi")))
    ctc = Ctc()
    ctc.SetGuard(net)
    ok = _decode(ctc, lens, probs, 4, 3, 2)
    assert np.all(np.isfinite(ok[1])) and np.all(ok[3][:, 0] >= 0)
    net._raise_error_word(2)
    hyps, scores, raw, hlen = _decode(ctc, lens, probs, 4, 3, 2)
    assert np.all(np.isnan(scores)) and np.all(hlen == -1) and np.all(raw == -1) and all(h == [] for h in hyps)
    net._raise_error_word(0)
    again = _decode(ctc, lens, probs, 4, 3, 2)
    assert np.array_equal(again[1], ok[1]) and again[0] == ok[0]
    ctc.SetGuard(None)


def test_statistics_and_eval_parallel_untouched(gpu):
    from eesen_amd.api import Ctc, CuMatrix
    lens, probs, labels, T, S = cc.build("dense_3x12x7")
    lens2, probs2, T2, S2 = dc.build("dense_8x60x46")
    net_out = CuMatrix.from_numpy(probs)

    def run(with_decode):
        ctc = Ctc()
        diff = ctc.EvalParallel(lens, net_out, labels).numpy()
        first = ctc.ErrorRateMSeq(lens, net_out, labels)
        if with_decode:
            ctc.DecodeParallel(lens2, CuMatrix.from_numpy(probs2), beam=16, max_classes=20)      # another shape: regrows logp
            ctc.DecodeParallel(lens, net_out, nbest=3)
        diff2 = ctc.EvalParallel(lens, net_out, labels).numpy()
        second = ctc.ErrorRateMSeq(lens, net_out, labels)
        return diff, diff2, ctc.pzx.copy(), first, second, ctc.stats()

    a, b = run(False), run(True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[3:] == b[3:]


def test_decode_times(gpu):
    from eesen_amd.api import Ctc
    lens, probs, T, S = dc.build("dense_3x12x7")
    ctc = Ctc()
    _decode(ctc, lens, probs, 4, 3, 1)
    t = ctc.DecodeTimes()
    assert set(t) == {"topc", "beam", "hyp"} and all(0 <= v < 1 for v in t.values()) and t["beam"] > 0
