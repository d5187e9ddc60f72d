"""-m gpu: the CTC prefix beam search with a token n-gram LM fused in (csrc/ctc_decode.hip: ctc_prefix_beam_kernel<true>, csrc/lm.cpp,
through api.Ctc.DecodeParallel(lm=...)) held per utterance against the fp64 restatement (tests/ctc_lm_restatement.py: the textbook ARPA
definition on dictionaries, no automaton) and against the exact fused score of every returned labelling.

Per utterance s, with bar_s = bar_of(score64_s, n_s) + |alpha| * (len + order + 1) * 2^-23 * sum|terms| of the 1-best's LM walk
(tests/test_ctc_lm_restatement.py holds, without a GPU, the conditions on these inputs that the checks rely on):

  count, lengths, -1 / -1e30 padding, scores descending, labellings pairwise distinct, no blank and no id >= K, length <= n_s
  every returned entry i:  score_i <= lnp64(hyp_i) + alpha * lm64(hyp_i [, </s>]) + beta * len_i + bar_s
                           |lm_score_i - eesen_lm_score(hyp_i)| <= (len_i + order + 1) * 2^-23 * sum|terms|_i
  stable utterances:       the 1-best labelling is the restatement's, and |score - score64| <= bar_s

Each case prints `worst |score - score64| / bar` (recorded in profiles/ctc_decode_lm.md).
"""
import numpy as np
import pytest

from tests import ctc_beam_restatement as R
from tests import ctc_cases as cc
from tests import ctc_decode_cases as dc
from tests import ctc_lm_cases as lc
from tests import ctc_lm_restatement as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctc(gpu):
    from eesen_amd.api import Ctc
    return Ctc()


@pytest.fixture(scope="module")
def lm_of(gpu, tmp_path_factory):
    """name of tests/ctc_lm_cases.py: MODELS -> (restatement model, api.TokenLm built from its ARPA text), each made once."""
    from eesen_amd.api import TokenLm
    d = tmp_path_factory.mktemp("lm")
    made = {}

    def get(name):
        if name not in made:
            m = L.model_of(name)
            arpa, units = m.write(d, name)
            made[name] = (m, TokenLm(arpa, units, K=m.K))
        return made[name]
    return get


def _decode(ctc, lens, m, B, C, N, lm=None, alpha=1.0, beta=0.0, eos=False, is_log=False):
    """(hyps, scores [S, N], raw labels [S, N, T], lengths [S, N], lm scores [S, N] or None)"""
    from eesen_amd.api import CuMatrix
    if isinstance(m, np.ndarray):
        m = CuMatrix.from_numpy(m)
    hyps, scores = ctc.DecodeParallel(lens, m, beam=B, max_classes=C, nbest=N, is_log=is_log, lm=lm, lm_weight=alpha, insertion_bonus=beta, lm_eos=eos)
    return hyps, scores, ctc.hyp.copy(), ctc.hyp_len.copy(), None if ctc.lm_score is None else ctc.lm_score.copy()


def _invariants(name, lens, probs, S, got, N, bars, model, lm, alpha, beta, eos, counts=None):
    hyps, scores, raw, hlen, lms = got
    K = probs.shape[1]
    assert scores.shape == hlen.shape == lms.shape == (S, N) and raw.shape[:2] == (S, N)
    for s in range(S):
        n = int(lens[s])
        where = f"{name} utterance {s} (n {n})"
        count = len(hyps[s])
        assert count <= N and np.all(hlen[s, :count] >= 0) and np.all(hlen[s, count:] == -1), where
        assert np.all(scores[s, count:] == np.float32(-1e30)) and np.all(raw[s, count:] == -1) and np.all(lms[s, count:] == np.float32(-1e30)), where
        if counts is not None:
            assert count == counts[s], (where, count, counts[s])
        assert np.all(np.diff(scores[s, :count]) <= 0), where
        assert len(set(map(tuple, hyps[s]))) == count, where
        lp = R.log64(R.utterance(probs, s, S, n))
        for i, h in enumerate(hyps[s]):
            assert len(h) == hlen[s, i] <= n and np.all(raw[s, i, len(h):] == -1) and all(1 <= c < K for c in h), (where, i)
            lm64, _ = model.lm64(h, eos)
            exact = R.lnp64(lp, h) + alpha * lm64 + beta * len(h)
            assert float(scores[s, i]) <= exact + bars[s], (where, i, float(scores[s, i]), exact, bars[s])
            want, absum = lm.Score(h, eos=eos, with_abs=True)
            bound = (len(h) + model.order + 1) * 2.0 ** -23 * absum
            assert abs(float(lms[s, i]) - want) <= bound, (where, i, float(lms[s, i]), want, bound)


def _hold(name, lens, probs, S, ref, got, N, model, lm, alpha, beta, eos):
    _invariants(name, lens, probs, S, got, N, [r["bar"] for r in ref], model, lm, alpha, beta, eos, counts=[min(N, len(r["beam64"])) for r in ref])
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


@pytest.mark.parametrize("key", list(lc.CASES))
def test_cases(ctc, lm_of, key):
    lens, probs, T, S, model, cfg, ref = L.case(key)
    _, lm = lm_of(cfg["model"])
    B, C = cfg["B"], cfg["C"]
    N = min(B, 4)
    got = _decode(ctc, lens, probs, B, C, N, lm, cfg["alpha"], cfg["beta"], cfg["eos"])
    _hold(f"{key} ({B}, {C}) order {model.order}", lens, probs, S, ref, got, N, model, lm, cfg["alpha"], cfg["beta"], cfg["eos"])


def test_exhaustive(ctc, lm_of):
    """Nothing is ever pruned: every labelling with a path comes back with ln p + alpha * (ln P_lm + final) + beta * len."""
    cfg = lc.EXHAUSTIVE
    B, C, N, alpha, beta = cfg["B"], cfg["C"], 63, cfg["alpha"], cfg["beta"]
    model, lm = lm_of(cfg["model"])
    lens, probs, T, S = dc.build(cfg["case"])
    ref = L.reference_of(lens, probs, S, B, C, model, alpha, beta, True)
    got = _decode(ctc, lens, probs, B, C, N, lm, alpha, beta, True)
    _hold("exhaustive", lens, probs, S, ref, got, N, model, lm, alpha, beta, True)
    hyps, scores = got[0], got[1]
    for s in range(S):
        n = int(lens[s])
        lp = R.log64(R.utterance(probs, s, S, n))
        want = {h: v + alpha * model.lm64(h, True)[0] + beta * len(h) for h, v in R.enumerate_paths(lp).items()}
        assert set(map(tuple, hyps[s])) == set(want), s
        for i, h in enumerate(hyps[s]):
            bar = R.bar_of(want[tuple(h)], n) + L.lm_term(model, alpha, h, True)[0]
            assert abs(float(scores[s, i]) - want[tuple(h)]) <= bar, (s, h, float(scores[s, i]), want[tuple(h)], bar)
        assert tuple(hyps[s][0]) == max(want, key=want.get), s


@pytest.mark.parametrize("key", list(lc.CASES))
def test_zero_weights_are_the_unfused_bits(ctc, lm_of, key):
    """alpha = 0, beta = 0, no eos, on every posterior case at its (beam, max_classes) with its model: hyps, lengths and scores are
    DecodeParallel's without an LM, bit for bit; and a plain call after a fused one is the plain call before it."""
    cfg = lc.CASES[key]
    lens, probs, T, S = dc.build(cfg["case"])
    _, lm = lm_of(cfg["model"])
    B, C = cfg["B"], cfg["C"]
    N = min(B, 4)
    before = _decode(ctc, lens, probs, B, C, N)
    fused = _decode(ctc, lens, probs, B, C, N, lm, 0.0, 0.0, False)
    after = _decode(ctc, lens, probs, B, C, N)
    assert before[4] is None and after[4] is None
    for x, y, z in zip(before[1:4], fused[1:4], after[1:4]):
        assert np.array_equal(x.view(np.int32), y.view(np.int32)) and np.array_equal(x.view(np.int32), z.view(np.int32))
    assert before[0] == fused[0] == after[0]


def test_insertion_bonus_alone_shifts_by_beta_per_label(ctc, lm_of):
    """alpha = 0, beta != 0 where nothing is pruned (the exhaustive case): every labelling's score moves by beta * len."""
    lens, probs, T, S = dc.build("exhaustive")
    _, lm = lm_of("k3_o3")
    B, C, N, beta = 64, 2, 63, 0.75
    plain = _decode(ctc, lens, probs, B, C, N)
    fused = _decode(ctc, lens, probs, B, C, N, lm, 0.0, beta, False)
    for s in range(S):
        base = {tuple(h): float(plain[1][s, i]) for i, h in enumerate(plain[0][s])}
        assert set(base) == set(map(tuple, fused[0][s]))
        for i, h in enumerate(fused[0][s]):
            want = base[tuple(h)] + beta * len(h)
            assert abs(float(fused[1][s, i]) - want) <= R.bar_of(want, int(lens[s])), (s, h)


def test_eos_rerank(ctc, tmp_path):
    """Two frames, two classes: labelling (1) wins acoustically and still wins with the LM's label weights (they are equal), and loses to
    (2) only through ln P(</s> | 1) against ln P(</s> | 2)."""
    from eesen_amd.api import TokenLm
    arpa = tmp_path / "eos.arpa"
    arpa.write_text("\\data\\\nngram 1=4\nngram 2=2\n\n\\1-grams:\n-99 <s> 0\n-1 </s>\n-0.5 1 0\n-0.5 2 0\n\n"
                    "\\2-grams:\n-2.0 1 </s>\n-0.1 2 </s>\n\n\\end\\\n")
    lm = TokenLm(str(arpa), None, K=3)
    probs = np.array([[0.1, 0.5, 0.4], [0.1, 0.5, 0.4]], np.float32)
    lens = np.array([2], np.int32)
    no = _decode(ctc, lens, probs, 8, 2, 5, lm, 1.0, 0.0, False)
    yes = _decode(ctc, lens, probs, 8, 2, 5, lm, 1.0, 0.0, True)
    assert no[0][0][:2] == [[1], [2]], no[0]
    assert yes[0][0][0] == [2] and yes[0][0].index([1]) > 0, yes[0]
    assert sorted(no[0][0]) == sorted(yes[0][0]) == [[], [1], [1, 2], [2], [2, 1]]
    ln10 = np.log(10.0)
    for h, fin in (([1], -2.0), ([2], -0.1)):
        i, j = no[0][0].index(h), yes[0][0].index(h)
        assert abs(float(yes[1][0, j]) - (float(no[1][0, i]) + fin * ln10)) <= 1e-5
        assert abs(float(yes[4][0, j]) - (float(no[4][0, i]) + fin * ln10)) <= 1e-5
        assert abs(float(yes[4][0, j]) - lm.Score(h, eos=True)) <= 1e-5


@pytest.mark.parametrize("eos", [True, False])
def test_lm_scores_come_out_of_the_hypothesis_walk(ctc, lm_of, eos):
    """ctc_hyp_kernel's lane of (utterance, rank) hands out the entry's LM sum: more ranks asked for than an utterance has entries
    (no frames: only the empty prefix lives) beside an ordinary utterance; the plain call writes no LM sum at all."""
    S, T, K, B, C, N, alpha, beta = 2, 2, 3, 4, 2, 3, 0.5, 0.1
    model, lm = lm_of("k3_o3")
    probs = cc.softmax32(np.random.default_rng(211).standard_normal((T * S, K)).astype(np.float32))
    lens = np.array([0, T], np.int32)
    got = _decode(ctc, lens, probs, B, C, N, lm, alpha, beta, eos)
    hyps, scores, raw, hlen, lms = got
    assert hyps[0] == [[]] and hlen[0].tolist() == [0, -1, -1]
    want = lm.Score([], eos=eos)
    assert abs(float(lms[0, 0]) - want) <= L.lm_term(model, alpha, [], eos)[1], (float(lms[0, 0]), want)
    assert np.all(scores[0, 1:] == np.float32(-1e30)) and np.all(lms[0, 1:] == np.float32(-1e30))
    ref = L.reference_of(lens, probs, S, B, C, model, alpha, beta, eos)
    assert len(hyps[1]) == N
    _invariants(f"lm sums, eos {eos}", lens, probs, S, got, N, [r["bar"] for r in ref], model, lm, alpha, beta, eos)   # every entry's lm_score
    plain = _decode(ctc, lens, probs, B, C, N)
    assert plain[4] is None and plain[0][0] == [[]]
    assert plain[3][0].tolist() == [0, -1, -1] and np.all(plain[1][0, 1:] == np.float32(-1e30))


@pytest.mark.parametrize("name", dc.TIE_CASES)
def test_ties_are_deterministic(ctc, lm_of, name):
    lens, probs, T, S = dc.build(name)
    model, lm = lm_of(lc.TIE_MODELS[name])
    B, C, N, alpha, beta, eos = 8, 4, 8, 0.7, 0.25, model.has_eos
    a = _decode(ctc, lens, probs, B, C, N, lm, alpha, beta, eos)
    b = _decode(ctc, lens, probs, B, C, N, lm, alpha, beta, eos)
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    ref = L.reference_of(lens, probs, S, B, C, model, alpha, beta, eos)
    _invariants(name, lens, probs, S, a, N, [r["bar"] for r in ref], model, lm, alpha, beta, eos)


def test_conventions(ctc, lm_of, tmp_path):
    from eesen_amd.api import EesenError, TokenLm
    model, lm = lm_of("k7_o4_unk")
    S, T, K = 3, 6, 7
    rng = np.random.default_rng(79)
    probs = cc.softmax32(rng.standard_normal((T * S, K)).astype(np.float32))
    lens = np.array([0, T, 2], np.int32)          # no frames beside ordinary utterances
    alpha = 0.8
    with_eos = _decode(ctc, lens, probs, 8, 3, 2, lm, alpha, 0.3, True)
    without = _decode(ctc, lens, probs, 8, 3, 2, lm, alpha, 0.3, False)
    fin = lm.Final(lm.Start())
    assert with_eos[0][0] == [[]] and without[0][0] == [[]]
    assert with_eos[1][0, 0] == np.float32(alpha) * np.float32(fin) and with_eos[4][0, 0] == np.float32(fin)
    assert without[1][0, 0] == 0.0 and without[4][0, 0] == 0.0
    assert with_eos[3][0].tolist() == [0, -1] and with_eos[1][0, 1] == np.float32(-1e30) and with_eos[4][0, 1] == np.float32(-1e30)
    ref = L.reference_of(lens, probs, S, 8, 3, model, alpha, 0.3, True)
    _hold("conventions", lens, probs, S, ref, with_eos, 2, model, lm, alpha, 0.3, True)
    # an LM for another K; use_eos without </s>; non-finite weights
    _, other = lm_of("k5_o3")
    _, noeos = lm_of("k12_o3_noeos")
    from eesen_amd.api import CuMatrix
    dev = CuMatrix.from_numpy(probs)
    dev12 = CuMatrix.from_numpy(cc.softmax32(rng.standard_normal((T * S, 12)).astype(np.float32)))
    for m, kw, word in ((dev, dict(lm=other), "another class count"), (dev12, dict(lm=noeos, lm_eos=True), "</s>"),
                        (dev, dict(lm=lm, lm_weight=float("nan")), "finite"), (dev, dict(lm=lm, insertion_bonus=float("inf")), "finite"),
                        (dev, dict(lm=lm, beam=65), "beam")):
        with pytest.raises(EesenError) as e:
            ctc.DecodeParallel(lens, m, **kw)
        assert e.value.code == -1 and word in str(e.value), kw
    ok = ctc.DecodeParallel(lens, dev12, lm=noeos)          # the same model without eos is fine
    assert len(ok[0]) == S
    with pytest.raises(EesenError):
        noeos.Score([1, 2], eos=True)


def test_guard_word_set_returns_nan_and_minus_one(gpu, lm_of):
    from eesen_amd import synth
    from eesen_amd.api import Net, Ctc
    lens, probs, T, S = dc.build("dense_3x12x7")
    _, lm = lm_of("k7_o2")
    net = Net.from_layers(synth.make_model(**synth.config("tiny_bi")))
    ctc = Ctc()
    ctc.SetGuard(net)
    ok = _decode(ctc, lens, probs, 4, 3, 2, lm, 0.5, 0.1, True)
    assert np.all(np.isfinite(ok[1])) and np.all(ok[3][:, 0] >= 0)
    net._raise_error_word(2)
    hyps, scores, raw, hlen, lms = _decode(ctc, lens, probs, 4, 3, 2, lm, 0.5, 0.1, True)
    assert np.all(np.isnan(scores)) and np.all(np.isnan(lms)) and np.all(hlen == -1) and np.all(raw == -1) and all(h == [] for h in hyps)
    net._raise_error_word(0)
    again = _decode(ctc, lens, probs, 4, 3, 2, lm, 0.5, 0.1, True)
    assert np.array_equal(again[1], ok[1]) and again[0] == ok[0] and np.array_equal(again[4], ok[4])
    ctc.SetGuard(None)


def test_statistics_untouched_and_times_populated(gpu, lm_of):
    from eesen_amd.api import Ctc, CuMatrix
    lens, probs, labels, T, S = cc.build("dense_3x12x7")
    _, lm = lm_of("k7_o2")
    net_out = CuMatrix.from_numpy(probs)

    def run(with_decode):
        ctc = Ctc()
        diff = ctc.EvalParallel(lens, net_out, labels).numpy()
        first = ctc.ErrorRateMSeq(lens, net_out, labels)
        if with_decode:
            ctc.DecodeParallel(lens, net_out, nbest=3, lm=lm, lm_weight=0.5, lm_eos=True)
            t = ctc.DecodeTimes()
            assert set(t) == {"topc", "beam", "hyp"} and all(0 <= v < 1 for v in t.values()) and t["beam"] > 0
            ids, sc, bl = ctc.DecodeCandidates(T * S, 20)
            assert ids.shape == (T * S, 6) and np.array_equal(ids[0], np.arange(1, 7))
        diff2 = ctc.EvalParallel(lens, net_out, labels).numpy()
        second = ctc.ErrorRateMSeq(lens, net_out, labels)
        return diff, diff2, ctc.pzx.copy(), first, second, ctc.stats()

    a, b = run(False), run(True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[3:] == b[3:]
