"""-m gpu: the CTC word beam search along a lexicon without a boundary unit (csrc/ctc_decode.hip: ctc_word_beam_kernel,
ctc_word_hyp_kernel; csrc/lex.cpp's unspaced kind; through api.Ctc.DecodeParallel(lexicon=Lexicon(space=None))), per utterance
against the fp64 restatement (tests/ctc_words_restatement.py: dictionaries of augmented sequences, no trie, no fingerprint) and
against the exact score of every returned hypothesis.

Per utterance s, with bar_s = bar_of(score64_s, n_s) + |alpha| * (|words| + order + 1) * 2^-23 * sum|terms| of the 1-best's LM walk
(tests/test_ctc_words_restatement.py holds, without a GPU, the conditions on these inputs that the checks rely on):

  count, lengths, -1 / -1e30 padding of labels, words, ends, scores and LM sums; scores descending; entries pairwise distinct as
  (labels, words, ends)
  every returned entry i:  its labels are the concatenation of spellings of its words, cut at its ends
                           score_i <= lnp64(labels_i) + alpha * lm64(words_i [, </s>]) + beta * |words_i| + bar_s
                           |lm_score_i - eesen_lm_score(words_i)| <= (|words_i| + order + 1) * 2^-23 * sum|terms|_i   (0 without an LM)
  stable utterances:       the 1-best (labels, words, ends) is the restatement's, and |score - score64| <= bar_s

Each case prints `worst |score - score64| / bar` (recorded in profiles/ctc_decode_words.md).
"""
import ctypes as C

import numpy as np
import pytest

from tests import ctc_beam_restatement as R
from tests import ctc_cases as cc
from tests import ctc_decode_cases as dc
from tests import ctc_lex_cases as xc
from tests import ctc_lex_restatement as X
from tests import ctc_lm_cases as lc
from tests import ctc_lm_restatement as L
from tests import ctc_words_cases as wc
from tests import ctc_words_restatement as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctc(gpu):
    from eesen_amd.api import Ctc
    return Ctc()


def _compile(d, tag, rl, model):
    """(api.Lexicon, api.TokenLm or None) of a restatement lexicon and a word model over its ids (the ARPA text names the words as
    the lexicon does and is read through Lexicon.WriteWords' table)."""
    from eesen_amd.api import Lexicon, TokenLm
    trie = Lexicon(rl.write(d, tag), None, K=rl.K, space=None)
    if model is None:
        return trie, None
    table = str(d / (tag + ".words.txt"))
    trie.WriteWords(table)
    by_id = {w: n for n, w in rl.ids.items()}
    arpa, _ = L.Model(model.K, model.order, model.grams, [None] + [by_id[w] for w in range(1, rl.V + 1)]).write(d, tag)
    return trie, TokenLm(arpa, table, K=rl.V + 1)


@pytest.fixture(scope="module")
def made(gpu, tmp_path_factory):
    """(restatement WLex or its name, word model name or None) -> (WLex, Model or None, api.Lexicon, api.TokenLm or None), made once."""
    d = tmp_path_factory.mktemp("wlex")
    done = {}

    def get(lex, model_name=None, tag=None):
        tag = (tag or lex) + "." + str(model_name)
        if tag not in done:
            rl = W.lex_of(lex) if isinstance(lex, str) else lex
            m = W.model_of(model_name)
            done[tag] = (rl, m) + _compile(d, tag, rl, m)
        return done[tag]
    return get


def _decode(ctc, lens, m, B, C, N, trie, lm=None, alpha=1.0, beta=0.0, eos=False, is_log=False):
    """(hyps, scores [S, N], raw labels [S, N, T], lengths [S, N], lm scores [S, N], words [S, N, T], word counts [S, N], ends [S, N, T])"""
    from eesen_amd.api import CuMatrix
    if isinstance(m, np.ndarray):
        m = CuMatrix.from_numpy(m)
    hyps, scores = ctc.DecodeParallel(lens, m, beam=B, max_classes=C, nbest=N, is_log=is_log, lm=lm, lm_weight=alpha, lm_eos=eos, lexicon=trie, word_bonus=beta)
    return hyps, scores, ctc.hyp.copy(), ctc.hyp_len.copy(), ctc.lm_score.copy(), ctc.words.copy(), ctc.words_len.copy(), ctc.word_ends.copy()


def _entry(got, s, i):
    """(labels, words, ends) of returned entry i of utterance s."""
    nw = int(got[6][s, i])
    return tuple(got[0][s][i]), tuple(got[5][s, i, :nw].tolist()), tuple(got[7][s, i, :nw].tolist())


def _invariants(name, lens, probs, S, got, N, bars, lex, model, lm, alpha, beta, eos, is_log=False):
    hyps, scores, raw, hlen, lms, words, wlen, ends = got
    assert scores.shape == hlen.shape == lms.shape == wlen.shape == (S, N) and raw.shape == words.shape == ends.shape and raw.shape[:2] == (S, N)
    for s in range(S):
        n = int(lens[s])
        where = f"{name} utterance {s} (n {n})"
        count = len(hyps[s])
        assert count <= N and np.all(hlen[s, :count] >= 0) and np.all(hlen[s, count:] == -1) and np.all(wlen[s, count:] == -1), where
        assert np.all(scores[s, count:] == np.float32(-1e30)) and np.all(raw[s, count:] == -1) and np.all(lms[s, count:] == np.float32(-1e30)), where
        assert np.all(words[s, count:] == -1) and np.all(ends[s, count:] == -1), where
        assert np.all(np.diff(scores[s, :count]) <= 0), where
        assert len({_entry(got, s, i) for i in range(count)}) == count, where
        u = R.utterance(probs, s, S, n)
        lp = np.maximum(np.asarray(u, np.float64), R.NEG) if is_log else R.log64(u)
        for i, h in enumerate(hyps[s]):
            assert len(h) == hlen[s, i] <= n and np.all(raw[s, i, len(h):] == -1) and all(1 <= c < lex.K for c in h), (where, i)
            labels, ws, es = _entry(got, s, i)
            assert 0 <= wlen[s, i] <= len(h) and np.all(words[s, i, len(ws):] == -1) and np.all(ends[s, i, len(ws):] == -1), (where, i)
            assert lex.consistent(labels, ws, es), (where, i, labels, ws, es)
            lm64, _ = W.lm64(model, ws, eos)
            exact = R.lnp64(lp, h) + alpha * lm64 + beta * len(ws)
            # (an utterance whose restatement holds no entry has no bar of its own: the entry's, as the exhaustive test forms it)
            bar = bars[s] if bars[s] is not None else R.bar_of(exact, n) + W.lm_term(model, alpha, ws, eos)[0]
            assert float(scores[s, i]) <= exact + bar, (where, i, float(scores[s, i]), exact, bar)
            if lm is None:
                assert lms[s, i] == 0.0, (where, i)
            else:
                want, absum = lm.Score(list(ws), eos=eos, with_abs=True)
                bound = (len(ws) + model.order + 1) * 2.0 ** -23 * absum
                assert abs(float(lms[s, i]) - want) <= bound, (where, i, float(lms[s, i]), want, bound)


def _hold(name, lens, probs, S, ref, got, N, lex, model, lm, alpha, beta, eos, is_log=False):
    _invariants(name, lens, probs, S, got, N, [r["bar"] if r["beam64"] else None for r in ref], lex, model, lm, alpha, beta, eos, is_log)
    hyps, scores = got[0], got[1]
    worst, same, unstable, held = 0.0, 0, [], 0
    for s in range(S):
        r = ref[s]
        where = f"{name} utterance {s} (n {int(lens[s])})"
        if not r["beam64"]:          # no complete entry: the dead-beam convention, where the jittered restatements agree that there is none
            print(f"{where}: the restatement holds no complete entry (stable {r['stable']}); returned {len(hyps[s])}")
            if r["stable"]:
                assert len(hyps[s]) == 0 and np.all(scores[s] == np.float32(-1e30)) and np.all(got[3][s] == -1), (where, hyps[s])
            continue
        equal = bool(hyps[s]) and _entry(got, s, 0) == W.split(r["beam64"][0][0])
        same += equal
        err = abs(float(scores[s, 0]) - r["score64"])
        print(f"{where}: score {scores[s, 0]:.7g} score64 {r['score64']:.10g} |err| {err:.3g} bar {r['bar']:.3g} stable {r['stable']} 1-best equal {equal}")
        if not r["stable"]:
            unstable.append(s)
            continue
        held += 1
        worst = max(worst, err / r["bar"] if r["bar"] > 0 else 0.0)
        assert equal, (where, _entry(got, s, 0) if hyps[s] else None, W.split(r["beam64"][0][0]))
        assert err <= r["bar"], where
    print(f"{name}: worst |score - score64| / bar = {worst:.3g}; 1-best equal {same}/{S}; unstable {unstable}; held {held}")


@pytest.mark.parametrize("key", list(wc.CASES))
def test_cases(ctc, made, key):
    lens, probs, T, S, lex, model, cfg, ref = W.case(key)
    _, _, trie, lm = made(cfg["lex"], cfg["model"])
    B, C = cfg["B"], cfg["C"]
    N = min(B, 4)
    got = _decode(ctc, lens, probs, B, C, N, trie, lm, cfg["alpha"], cfg["beta"], cfg["eos"])
    _hold(f"{key} ({B}, {C}) V {lex.V} H {lex.H}", lens, probs, S, ref, got, N, lex, model, lm, cfg["alpha"], cfg["beta"], cfg["eos"])


def test_exhaustive(ctc, made):
    """Nothing is ever pruned: every hypothesis with a path comes back -- every segmentation and every homophone of every labelling,
    the final fan-out included -- with ln p + alpha * ln P_lm(words, </s>) + beta * |words|, and nothing else does."""
    cfg = wc.EXHAUSTIVE
    B, C, N, alpha, beta = cfg["B"], cfg["C"], 64, cfg["alpha"], cfg["beta"]
    lex, model, trie, lm = made(cfg["lex"], cfg["model"])
    lens, probs, T, S = wc.build_exhaustive()
    ref = W.reference_of(lens, probs, S, B, C, lex, model, alpha, beta, True)
    got = _decode(ctc, lens, probs, B, C, N, trie, lm, alpha, beta, True)
    _hold("exhaustive", lens, probs, S, ref, got, N, lex, model, lm, alpha, beta, True)
    hyps, scores = got[0], got[1]
    for s in range(S):
        n = int(lens[s])
        lp = R.log64(R.utterance(probs, s, S, n))
        want = {W.split(h): W.exact_of(model, alpha, beta, True, lp, *W.split(h)[:2]) for h in W.enumerate_hypotheses(lex, lp)}
        have = [_entry(got, s, i) for i in range(len(hyps[s]))]
        assert set(have) == set(want) and len(have) == len(want), s
        for i, e in enumerate(have):
            bar = R.bar_of(want[e], n) + W.lm_term(model, alpha, e[1], True)[0]
            assert abs(float(scores[s, i]) - want[e]) <= bar, (s, e, float(scores[s, i]), want[e], bar)
        assert have[0] == max(want, key=want.get), s


def _small(tmp_path, entries, K, grams=None, order=2, tag="s"):
    rl = W.WLex(K, entries)
    model = None if grams is None else L.Model(rl.V + 1, order, grams)
    return (rl, model) + _compile(tmp_path, tag, rl, model)


def _spell(path, K, peak=0.94):
    """One utterance whose frame t puts `peak` on class path[t] and shares the rest."""
    probs = np.full((len(path), K), (1.0 - peak) / (K - 1), np.float32)
    probs[np.arange(len(path)), list(path)] = peak
    return np.array([len(path)], np.int32), probs


def test_homophone_is_decided_by_the_following_word(ctc, tmp_path):
    """to / two share the spelling (t u); P(two | <s>) > P(to | <s>) but P(x | to) >> P(x | two): the frames spell `t u x` and the
    1-best must be `to x` -- both homophones have to survive the close for the next word to choose."""
    t, u, x = 1, 2, 3
    grams = {(1,): (-1.0, -0.2), (2,): (-0.3, -0.2), (3,): (-1.0, 0.0), (L.BOS,): (-99.0, 0.0), (L.EOS,): (-1.0, None),
             (1, 3): (-0.1, None), (2, 3): (-3.0, None)}
    lex, model, trie, lm = _small(tmp_path, [("to", (t, u)), ("two", (t, u)), ("x", (x,))], 4, grams)
    assert lm.Score([2]) > lm.Score([1]) and lm.Score([1, 3]) > lm.Score([2, 3]) + 3.0
    lens, probs = _spell((t, u, 0, x, 0), 4)
    ref = W.reference_of(lens, probs, 1, 8, 3, lex, model, 1.0, 0.0, False)
    assert W.split(ref[0]["beam64"][0][0]) == ((t, u, x), (1, 3), (2, 3)) and ref[0]["stable"]
    got = _decode(ctc, lens, probs, 8, 3, 4, trie, lm, 1.0, 0.0, False)
    _hold("homophone", lens, probs, 1, ref, got, 4, lex, model, lm, 1.0, 0.0, False)
    entries = [_entry(got, 0, i) for i in range(len(got[0][0]))]
    assert entries[0] == ((t, u, x), (1, 3), (2, 3)) and entries.index(((t, u, x), (2, 3), (2, 3))) > 0, entries


def test_prefix_word_and_its_split_are_both_returned(ctc, tmp_path):
    """Lexicon a, b, ab; the frames spell `a b`: `ab` and `a b` come back with the same labels, and their scores differ by the LM and
    bonus terms alone."""
    model = L.random_model(seed=6601, K=4, order=2)
    lex, model, trie, lm = _small(tmp_path, [("a", (1,)), ("b", (2,)), ("ab", (1, 2))], 3, model.grams)
    alpha, beta = 0.3, 0.3
    lens, probs = _spell((1, 0, 2, 0), 3, peak=0.99)
    ref = W.reference_of(lens, probs, 1, 8, 2, lex, model, alpha, beta, True)
    got = _decode(ctc, lens, probs, 8, 2, 2, trie, lm, alpha, beta, True)
    _hold("prefix word", lens, probs, 1, ref, got, 2, lex, model, lm, alpha, beta, True)
    e = [_entry(got, 0, i) for i in range(2)]
    assert sorted(e) == sorted([((1, 2), (3,), (2,)), ((1, 2), (1, 2), (1, 2))]), e
    lp = R.log64(probs)
    exact = [W.exact_of(model, alpha, beta, True, lp, en[0], en[1]) for en in e]
    bars = [R.bar_of(v, 4) + W.lm_term(model, alpha, en[1], True)[0] for v, en in zip(exact, e)]
    diff = float(got[1][0, 0]) - float(got[1][0, 1])
    assert abs(diff - (exact[0] - exact[1])) <= bars[0] + bars[1], (diff, exact, bars)


def test_repeat_rule_applies_across_a_word_boundary(ctc, tmp_path):
    """Words xa, ay and xay; the frames are x a a y with no blank between the two a: they are one label, so the labels are x a y -- the
    word xay -- and not `xa ay` with a doubled a, which needs a blank the frames do not have."""
    lex, _, trie, _ = _small(tmp_path, [("xa", (1, 2)), ("ay", (2, 3)), ("xay", (1, 2, 3))], 4)
    lens, probs = _spell((1, 2, 2, 3, 0), 4)
    ref = W.reference_of(lens, probs, 1, 8, 3, lex, None, 1.0, 0.2, False)
    assert W.split(ref[0]["beam64"][0][0]) == ((1, 2, 3), (3,), (3,)) and ref[0]["stable"]
    got = _decode(ctc, lens, probs, 8, 3, 4, trie, None, 1.0, 0.2, False)
    _hold("repeat across a boundary", lens, probs, 1, ref, got, 4, lex, None, None, 1.0, 0.2, False)
    want = [W.split(h) for h, _, _ in ref[0]["beam64"]][:len(got[0][0])]
    assert [_entry(got, 0, i) for i in range(len(got[0][0]))] == want
    assert ((1, 2, 2, 3), (1, 2), (2, 4)) not in want[:1]          # (`xa ay` has a path -- a blank on an a frame -- and cannot win)


@pytest.mark.parametrize("name", dc.TIE_CASES)
def test_ties_follow_the_selection_order(ctc, made, name):
    """Homophones without a model and uniform posteriors tie exactly: labels, words, ends and their order are the fp32 restatement's,
    and two runs are bit-identical."""
    lens, probs, T, S = dc.build(name)
    lex = wc.lexicon(name, wc.TIE_LEXICONS)
    assert lex.K == probs.shape[1] and lex.H >= 2
    _, _, trie, _ = made(lex, None, tag="tie_" + name)
    B, C, N, beta = 8, 4, 8, 0.25
    a = _decode(ctc, lens, probs, B, C, N, trie, None, 1.0, beta)
    b = _decode(ctc, lens, probs, B, C, N, trie, None, 1.0, beta)
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    ref = W.reference_of(lens, probs, S, B, C, lex, None, 1.0, beta, False)
    _invariants(name, lens, probs, S, a, N, [r["bar"] if r["beam64"] else None for r in ref], lex, None, None, 1.0, beta, False)
    for s in range(S):
        want = [W.split(h) for h, _, _ in ref[s]["beam32"]][:N]
        assert [_entry(a, s, i) for i in range(len(a[0][s]))] == want, (name, s)


def test_mid_word_utterance_returns_nothing_and_its_neighbours_are_untouched(ctc, tmp_path):
    """Lexicon {ab}: utterance 1 hears only `a`, so at beam 1 its one live entry ends mid-word: count 0, score -1e30; utterances 0 and
    2 hear `a b` and return it, exactly as they do when decoded without the middle one."""
    lex, _, trie, _ = _small(tmp_path, [("ab", (2, 3))], 4)
    S, T = 3, 4
    probs = np.full((T * S, 4), 0.02, np.float32)
    for s, path in enumerate(((2, 3, 0, 0), (2, 2, 0, 0), (2, 0, 3, 0))):
        for t, c in enumerate(path):
            probs[t * S + s, c] = 0.94
    lens = np.array([T, T, T], np.int32)
    got = _decode(ctc, lens, probs, 1, 3, 1, trie, None, 1.0, 0.3)
    assert got[0] == [[[2, 3]], [], [[2, 3]]] and got[3][:, 0].tolist() == [2, -1, 2] and got[6][:, 0].tolist() == [1, -1, 1]
    assert got[5][:, 0, 0].tolist() == [1, -1, 1] and got[7][:, 0, 0].tolist() == [2, -1, 2]
    assert got[1][1, 0] == np.float32(-1e30) and got[4][1, 0] == np.float32(-1e30) and np.all(got[2][1] == -1) and np.all(got[5][1] == -1) and np.all(got[7][1] == -1)
    alone = _decode(ctc, lens[[0, 2]], np.ascontiguousarray(probs.reshape(T, S, 4)[:, [0, 2]].reshape(-1, 4)), 1, 3, 1, trie, None, 1.0, 0.3)
    assert np.array_equal(alone[1].view(np.int32), got[1][[0, 2]].view(np.int32)) and alone[0] == [got[0][0], got[0][2]]
    ref = W.reference_of(lens, probs, S, 1, 3, lex, None, 1.0, 0.3, False)
    assert [len(r["beam64"]) for r in ref] == [1, 0, 1]
    _hold("mid-word", lens, probs, S, ref, got, 1, lex, None, None, 1.0, 0.3, False)


def test_a_beam_that_dies_with_is_log_input(ctc, tmp_path):
    """Log-scores at the sentinel on every class of a frame: no candidate survives it, the utterance returns nothing, and its
    neighbour is what it is alone."""
    lex, _, trie, _ = _small(tmp_path, [("a", (1,)), ("b", (2,))], 3)
    S, T = 2, 3
    logs = np.log(np.full((T * S, 3), 1.0 / 3, np.float32))
    logs[1 * S + 0, :] = -1e30          # utterance 0, frame 1
    lens = np.array([T, T], np.int32)
    got = _decode(ctc, lens, logs, 4, 2, 2, trie, None, 1.0, 0.1, is_log=True)
    assert got[0][0] == [] and np.all(got[1][0] == np.float32(-1e30)) and np.all(got[3][0] == -1) and np.all(got[6][0] == -1)
    alone = _decode(ctc, lens[[1]], np.ascontiguousarray(logs[1::S]), 4, 2, 2, trie, None, 1.0, 0.1, is_log=True)
    assert len(got[0][1]) == 2 and alone[0][0] == got[0][1] and np.array_equal(alone[1][0].view(np.int32), got[1][1].view(np.int32))
    ref = W.reference_of(lens, logs, S, 4, 2, lex, None, 1.0, 0.1, False, is_log=True)
    assert not ref[0]["beam64"]
    _hold("dead beam", lens, logs, S, ref, got, 2, lex, None, None, 1.0, 0.1, False, is_log=True)


def test_limits_and_wrong_kind(ctc, made, tmp_path):
    from eesen_amd.api import CuMatrix, EesenError, Lexicon
    lex, model, trie, lm = made("k7", "v12_o3_unk")
    S, T, K = 3, 6, 7
    rng = np.random.default_rng(79)
    probs = cc.softmax32(rng.standard_normal((T * S, K)).astype(np.float32))
    lens = np.array([0, T, 2], np.int32)          # no frames beside ordinary utterances
    alpha = 0.8
    with_eos = _decode(ctc, lens, probs, 8, 3, 2, trie, lm, alpha, 0.3, True)
    without = _decode(ctc, lens, probs, 8, 3, 2, trie, lm, alpha, 0.3, False)
    fin = lm.Final(lm.Start())
    assert with_eos[0][0] == [[]] and without[0][0] == [[]]
    assert with_eos[1][0, 0] == np.float32(alpha) * np.float32(fin) and with_eos[4][0, 0] == np.float32(fin)
    assert without[1][0, 0] == 0.0 and without[4][0, 0] == 0.0
    assert with_eos[3][0].tolist() == [0, -1] and with_eos[6][0].tolist() == [0, -1] and with_eos[1][0, 1] == np.float32(-1e30)
    ref = W.reference_of(lens, probs, S, 8, 3, lex, model, alpha, 0.3, True)
    _hold("conventions", lens, probs, S, ref, with_eos, 2, lex, model, lm, alpha, 0.3, True)
    _, _, other, other_lm = made("k8", "v20_o4")
    _, _, h8, _ = made("k40", None)
    dev = CuMatrix.from_numpy(probs)
    dev40 = CuMatrix.from_numpy(cc.softmax32(rng.standard_normal((T * S, 40)).astype(np.float32)))
    spaced = Lexicon(X.lex_of("k7_sp3").write(tmp_path, "spaced"), None, K=7, space=3)
    # the unspaced lexicon's own file through the spaced call and the other way round; every limit, by name
    for m, kw, word in ((dev, dict(lexicon=other), "another class count"), (dev, dict(lexicon=trie, lm=other_lm), "word count + 1"),
                        (dev, dict(lexicon=trie, lm_eos=True), "use_eos"), (dev, dict(lexicon=trie, lm=lm, lm_weight=float("nan")), "finite"),
                        (dev, dict(lexicon=trie, word_bonus=float("inf")), "finite"), (dev, dict(lexicon=trie, beam=65), "beam"),
                        (dev, dict(lexicon=trie, max_classes=65), "max_classes"), (dev, dict(lexicon=trie, beam=4, nbest=5), "nbest"),
                        (dev40, dict(lexicon=h8, beam=32, max_classes=20), "beam * (1 + max_classes * (1 + H))"),
                        (dev40, dict(lexicon=h8, beam=23, max_classes=20), "beam * (1 + max_classes * (1 + H))")):
        with pytest.raises(EesenError) as e:
            ctc.DecodeParallel(lens, m, **kw)
        assert e.value.code == -1 and word in str(e.value), kw
    ok = ctc.DecodeParallel(lens, dev40, lexicon=h8, beam=22, max_classes=20)          # 22 * 181 = 3982 <= 4096
    assert len(ok[0]) == S
    fn = np.ascontiguousarray(lens, np.int32)
    hyp, hl, sc = np.empty((S, 1, T), np.int32), np.empty((S, 1), np.int32), np.empty((S, 1), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    args = (vp(fn), S, C.c_void_p(dev.ptr), dev.rows, dev.cols, dev.stride, 0, 4, 3, 1)
    rc = ctc.lib.eesen_ctc_decode_parallel_words(ctc.h, *args, None, None, 1.0, 0.0, 0, vp(hyp), vp(hl), vp(sc), None, None, None, None)
    assert rc == -1 and b"lexicon handle is null" in ctc.lib.eesen_last_error()
    rc = ctc.lib.eesen_ctc_decode_parallel_words(ctc.h, *args, spaced.h, None, 1.0, 0.0, 0, vp(hyp), vp(hl), vp(sc), None, None, None, None)
    assert rc == -1 and b"eesen_ctc_decode_parallel_lex" in ctc.lib.eesen_last_error()
    rc = ctc.lib.eesen_ctc_decode_parallel_lex(ctc.h, *args, trie.h, None, 1.0, 0.0, 0, vp(hyp), vp(hl), vp(sc), None, None, None)
    assert rc == -1 and b"eesen_ctc_decode_parallel_words" in ctc.lib.eesen_last_error()
    # the optional outputs may all be null
    rc = ctc.lib.eesen_ctc_decode_parallel_words(ctc.h, *args, trie.h, None, 1.0, 0.0, 0, vp(hyp), vp(hl), vp(sc), None, None, None, None)
    assert rc == 0 and hl[0, 0] == 0


def test_guard_word_set_returns_nan_and_minus_one(gpu, made):
    from eesen_amd import synth
    from eesen_amd.api import Net, Ctc
    lens, probs, T, S, lex, model, cfg, _ = W.case("k7_c3")
    _, _, trie, lm = made(cfg["lex"], cfg["model"])
    net = Net.from_layers(synth.make_model(**synth.config("tiny_bi")))
    ctc = Ctc()
    ctc.SetGuard(net)
    ok = _decode(ctc, lens, probs, 4, 3, 2, trie, lm, 0.5, 0.1, True)
    assert np.all(np.isfinite(ok[1])) and np.all(ok[3][:, 0] >= 0)
    net._raise_error_word(2)
    hyps, scores, raw, hlen, lms, words, wlen, ends = _decode(ctc, lens, probs, 4, 3, 2, trie, lm, 0.5, 0.1, True)
    assert np.all(np.isnan(scores)) and np.all(np.isnan(lms)) and np.all(hlen == -1) and np.all(raw == -1) and all(h == [] for h in hyps)
    assert np.all(words == -1) and np.all(wlen == -1) and np.all(ends == -1)
    net._raise_error_word(0)
    again = _decode(ctc, lens, probs, 4, 3, 2, trie, lm, 0.5, 0.1, True)
    assert again[0] == ok[0] and all(np.array_equal(p, q) for p, q in zip(again[1:], ok[1:]))
    ctc.SetGuard(None)


def test_statistics_untouched_and_times_populated(gpu, made):
    from eesen_amd.api import Ctc, CuMatrix
    lens, probs, labels, T, S = cc.build("dense_3x12x7")
    _, _, trie, lm = made("k7", "v12_o3_unk")
    net_out = CuMatrix.from_numpy(probs)

    def run(with_decode):
        ctc = Ctc()
        diff = ctc.EvalParallel(lens, net_out, labels).numpy()
        first = ctc.ErrorRateMSeq(lens, net_out, labels)
        if with_decode:
            ctc.DecodeParallel(lens, net_out, nbest=3, lexicon=trie, lm=lm, lm_weight=0.5, lm_eos=True, word_bonus=0.2)
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


def test_other_modes_are_untouched_by_a_words_call(gpu, made, tmp_path):
    """On one Ctc: the plain, the token-LM and the spaced-lexicon call return the same arrays before and after a words call with a
    word LM -- the table caches (the token LM's, the word LM's, the two lexicons' shared buffer) do not leak between the modes."""
    from eesen_amd.api import Ctc, CuMatrix, Lexicon, TokenLm
    key = next(iter(lc.CASES))
    cfg = lc.CASES[key]
    lens, probs, T, S = dc.build(cfg["case"])
    m = L.model_of(cfg["model"])
    arpa, units = m.write(tmp_path, "tok")
    tok = TokenLm(arpa, units, K=m.K)
    B, C = cfg["B"], cfg["C"]
    N = min(B, 4)
    ctc = Ctc()
    dev = CuMatrix.from_numpy(probs)
    xcfg = xc.CASES["k7_c3"]
    xlens, xprobs, _, _, xlex, _, _, _ = X.case("k7_c3")
    xdev = CuMatrix.from_numpy(xprobs)
    spaced = Lexicon(xlex.write(tmp_path, "spaced"), None, K=xlex.K, space=xlex.space)

    def others():
        out = []
        for d, l, kw in ((dev, lens, dict()), (dev, lens, dict(lm=tok, lm_weight=cfg["alpha"], insertion_bonus=cfg["beta"], lm_eos=cfg["eos"])),
                         (xdev, xlens, dict(lexicon=spaced, word_bonus=xcfg["beta"]))):
            hyps, scores = ctc.DecodeParallel(l, d, beam=B, max_classes=C, nbest=N, **kw)
            out.append((hyps, scores.copy(), ctc.hyp.copy(), ctc.hyp_len.copy(), None if ctc.lm_score is None else ctc.lm_score.copy(),
                        None if ctc.words is None else ctc.words.copy()))
            assert ctc.word_ends is None
        return out
    before = others()
    wcfg = wc.CASES["k7_c3"]
    wlens, wprobs, _, _, _, _, _, _ = W.case("k7_c3")
    _, _, trie, wlm = made(wcfg["lex"], wcfg["model"])
    first = _decode(ctc, wlens, wprobs, wcfg["B"], wcfg["C"], 2, trie, wlm, wcfg["alpha"], wcfg["beta"], wcfg["eos"])
    after = others()
    again = _decode(ctc, wlens, wprobs, wcfg["B"], wcfg["C"], 2, trie, wlm, wcfg["alpha"], wcfg["beta"], wcfg["eos"])
    for x, y in zip(before, after):
        assert x[0] == y[0]
        for p, q in zip(x[1:], y[1:]):
            assert (p is None and q is None) or np.array_equal(p.view(np.int32), q.view(np.int32))
    assert first[0] == again[0]
    for p, q in zip(first[1:], again[1:]):
        assert np.array_equal(p.view(np.int32), q.view(np.int32))
