"""-m gpu: the CTC prefix beam search held to a lexicon, with or without a word n-gram LM (csrc/ctc_decode.hip:
ctc_prefix_beam_lex_kernel, csrc/lex.cpp, through api.Ctc.DecodeParallel(lexicon=...)), per utterance against the fp64 restatement
(tests/ctc_lex_restatement.py: sets of spellings, no trie) and against the exact score of every returned labelling.

Per utterance s, with bar_s = bar_of(score64_s, n_s) + |alpha| * (|words| + order + 1) * 2^-23 * sum|terms| of the 1-best's LM walk over
its words (tests/test_ctc_lex_restatement.py holds, without a GPU, the conditions on these inputs that the checks rely on):

  count, lengths, -1 / -1e30 padding of labels, words, scores and LM sums; scores descending; labellings pairwise distinct
  every returned entry i:  hyp_i is in L and complete, words_i is its segmentation
                           score_i <= lnp64(hyp_i) + alpha * lm64(words_i [, </s>]) + beta * |words_i| + bar_s
                           |lm_score_i - eesen_lm_score(words_i)| <= (|words_i| + order + 1) * 2^-23 * sum|terms|_i   (0 without an LM)
  stable utterances:       the 1-best labelling is the restatement's, and |score - score64| <= bar_s

Each case prints `worst |score - score64| / bar` (recorded in profiles/ctc_decode_lex.md).
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

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctc(gpu):
    from eesen_amd.api import Ctc
    return Ctc()


@pytest.fixture(scope="module")
def made(gpu, tmp_path_factory):
    """(restatement Lex or its name, word model name or None) -> (Lex, Model or None, api.Lexicon, api.TokenLm or None), each made once.
    The word model's ARPA text names the words as the lexicon does and is read through Lexicon.WriteWords' table."""
    from eesen_amd.api import Lexicon, TokenLm
    d = tmp_path_factory.mktemp("lex")
    tries, lms = {}, {}

    def get(lex, model_name=None, tag=None):
        tag = tag or lex
        if tag not in tries:
            rl = X.lex_of(lex) if isinstance(lex, str) else lex
            trie = Lexicon(rl.write(d, tag), None, K=rl.K, space=rl.space)
            table = str(d / (tag + ".words.txt"))
            trie.WriteWords(table)
            tries[tag] = (rl, trie, table)
        rl, trie, table = tries[tag]
        if model_name is None:
            return rl, None, trie, None
        if (tag, model_name) not in lms:
            m = X.model_of(model_name)
            by_id = {w: n for n, w in rl.ids.items()}
            arpa, _ = L.Model(m.K, m.order, m.grams, [None] + [by_id[w] for w in range(1, rl.V + 1)]).write(d, tag + "." + model_name)
            lms[(tag, model_name)] = (m, TokenLm(arpa, table, K=rl.V + 1))
        m, lm = lms[(tag, model_name)]
        return rl, m, trie, lm
    return get


def _decode(ctc, lens, m, B, C, N, trie, lm=None, alpha=1.0, beta=0.0, eos=False, is_log=False):
    """(hyps, scores [S, N], raw labels [S, N, T], lengths [S, N], lm scores [S, N], words [S, N, T], word counts [S, N])"""
    from eesen_amd.api import CuMatrix
    if isinstance(m, np.ndarray):
        m = CuMatrix.from_numpy(m)
    hyps, scores = ctc.DecodeParallel(lens, m, beam=B, max_classes=C, nbest=N, is_log=is_log, lm=lm, lm_weight=alpha, lm_eos=eos, lexicon=trie, word_bonus=beta)
    return hyps, scores, ctc.hyp.copy(), ctc.hyp_len.copy(), ctc.lm_score.copy(), ctc.words.copy(), ctc.words_len.copy()


def _invariants(name, lens, probs, S, got, N, bars, lex, model, lm, alpha, beta, eos):
    hyps, scores, raw, hlen, lms, words, wlen = got
    assert scores.shape == hlen.shape == lms.shape == wlen.shape == (S, N) and raw.shape == words.shape and raw.shape[:2] == (S, N)
    for s in range(S):
        n = int(lens[s])
        where = f"{name} utterance {s} (n {n})"
        count = len(hyps[s])
        assert count <= N and np.all(hlen[s, :count] >= 0) and np.all(hlen[s, count:] == -1) and np.all(wlen[s, count:] == -1), where
        assert np.all(scores[s, count:] == np.float32(-1e30)) and np.all(raw[s, count:] == -1) and np.all(lms[s, count:] == np.float32(-1e30)), where
        assert np.all(words[s, count:] == -1), where
        assert np.all(np.diff(scores[s, :count]) <= 0), where
        assert len(set(map(tuple, hyps[s]))) == count, where
        lp = R.log64(R.utterance(probs, s, S, n))
        for i, h in enumerate(hyps[s]):
            assert len(h) == hlen[s, i] <= n and np.all(raw[s, i, len(h):] == -1) and all(1 <= c < lex.K for c in h), (where, i)
            seg = lex.segment(h)
            assert seg is not None, (where, i, h)                    # in L and complete
            assert wlen[s, i] == len(seg) and tuple(words[s, i, :len(seg)]) == seg and np.all(words[s, i, len(seg):] == -1), (where, i, h)
            lm64, _ = X.lm64(model, seg, eos)
            exact = R.lnp64(lp, h) + alpha * lm64 + beta * len(seg)
            # (an utterance whose restatement holds no entry has no bar of its own: the entry's, as the exhaustive test forms it)
            bar = bars[s] if bars[s] is not None else R.bar_of(exact, n) + X.lm_term(model, alpha, seg, eos)[0]
            assert float(scores[s, i]) <= exact + bar, (where, i, float(scores[s, i]), exact, bar)
            if lm is None:
                assert lms[s, i] == 0.0, (where, i)
            else:
                want, absum = lm.Score(list(seg), eos=eos, with_abs=True)
                bound = (len(seg) + model.order + 1) * 2.0 ** -23 * absum
                assert abs(float(lms[s, i]) - want) <= bound, (where, i, float(lms[s, i]), want, bound)


def _hold(name, lens, probs, S, ref, got, N, lex, model, lm, alpha, beta, eos):
    _invariants(name, lens, probs, S, got, N, [r["bar"] if r["beam64"] else None for r in ref], lex, model, lm, alpha, beta, eos)
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
        equal = bool(hyps[s]) and tuple(hyps[s][0]) == r["beam64"][0][0]
        same += equal
        err = abs(float(scores[s, 0]) - r["score64"])
        print(f"{where}: score {scores[s, 0]:.7g} score64 {r['score64']:.10g} |err| {err:.3g} bar {r['bar']:.3g} stable {r['stable']} 1-best equal {equal}")
        if not r["stable"]:
            unstable.append(s)
            continue
        held += 1
        worst = max(worst, err / r["bar"] if r["bar"] > 0 else 0.0)
        assert equal, (where, hyps[s][:1], r["beam64"][0][0])
        assert err <= r["bar"], where
    print(f"{name}: worst |score - score64| / bar = {worst:.3g}; 1-best equal {same}/{S}; unstable {unstable}; held {held}")


@pytest.mark.parametrize("key", list(xc.CASES))
def test_cases(ctc, made, key):
    lens, probs, T, S, lex, model, cfg, ref = X.case(key)
    _, _, trie, lm = made(cfg["lex"], cfg["model"])
    B, C = cfg["B"], cfg["C"]
    N = min(B, 4)
    got = _decode(ctc, lens, probs, B, C, N, trie, lm, cfg["alpha"], cfg["beta"], cfg["eos"])
    _hold(f"{key} ({B}, {C}) V {lex.V}", lens, probs, S, ref, got, N, lex, model, lm, cfg["alpha"], cfg["beta"], cfg["eos"])


def test_exhaustive(ctc, made):
    """Nothing is ever pruned: every complete labelling with a path comes back with ln p + alpha * ln P_lm(words, </s>) + beta * |words|,
    and nothing outside the language does."""
    cfg = xc.EXHAUSTIVE
    B, C, N, alpha, beta = cfg["B"], cfg["C"], 64, cfg["alpha"], cfg["beta"]
    lex, model, trie, lm = made(cfg["lex"], cfg["model"])
    lens, probs, T, S = xc.build_exhaustive()
    ref = X.reference_of(lens, probs, S, B, C, lex, model, alpha, beta, True)
    got = _decode(ctc, lens, probs, B, C, N, trie, lm, alpha, beta, True)
    _hold("exhaustive", lens, probs, S, ref, got, N, lex, model, lm, alpha, beta, True)
    hyps, scores = got[0], got[1]
    for s in range(S):
        n = int(lens[s])
        lp = R.log64(R.utterance(probs, s, S, n))
        want = {h: X.exact_of(lex, model, alpha, beta, True, lp, h) for h in X.enumerate_language(lex, lp)}
        assert set(map(tuple, hyps[s])) == set(want), s
        for i, h in enumerate(hyps[s]):
            bar = R.bar_of(want[tuple(h)], n) + X.lm_term(model, alpha, lex.segment(h), True)[0]
            assert abs(float(scores[s, i]) - want[tuple(h)]) <= bar, (s, h, float(scores[s, i]), want[tuple(h)], bar)
        assert tuple(hyps[s][0]) == max(want, key=want.get), s


def test_word_bonus_alone_shifts_by_beta_per_word(ctc, made):
    """No LM, where nothing is pruned: every labelling's score moves by beta * |words| against beta = 0, and beta = 0 without an LM is
    ln p of the plain search on the labellings both return."""
    cfg = xc.EXHAUSTIVE
    lex, _, trie, _ = made(cfg["lex"])
    lens, probs, T, S = xc.build_exhaustive()
    beta = 0.75
    zero = _decode(ctc, lens, probs, 64, 3, 64, trie, None, 1.0, 0.0)
    plus = _decode(ctc, lens, probs, 64, 3, 64, trie, None, 1.0, beta)
    for s in range(S):
        n = int(lens[s])
        lp = R.log64(R.utterance(probs, s, S, n))
        base = {tuple(h): float(zero[1][s, i]) for i, h in enumerate(zero[0][s])}
        assert set(base) == set(map(tuple, plus[0][s])) == set(X.enumerate_language(lex, lp))
        for h, v in base.items():
            want = R.lnp64(lp, h)
            assert abs(v - want) <= R.bar_of(want, n), (s, h)
        for i, h in enumerate(plus[0][s]):
            want = base[tuple(h)] + beta * len(lex.segment(h))
            assert abs(float(plus[1][s, i]) - want) <= R.bar_of(want, n), (s, h)


def _small(tmp_path, text, K, space, arpa=None):
    from eesen_amd.api import Lexicon, TokenLm
    (tmp_path / "l.txt").write_text(text)
    trie = Lexicon(str(tmp_path / "l.txt"), None, K=K, space=space)
    lm = None
    if arpa is not None:
        trie.WriteWords(str(tmp_path / "w.txt"))
        (tmp_path / "w.arpa").write_text(arpa)
        lm = TokenLm(str(tmp_path / "w.arpa"), str(tmp_path / "w.txt"), K=trie.Info()["words"] + 1)
    entries = [(l.split()[0], tuple(map(int, l.split()[1:]))) for l in text.splitlines()]
    return X.Lex(K, space, entries), trie, lm


def test_mid_word_utterance_returns_nothing_and_its_neighbours_are_untouched(ctc, tmp_path):
    """Lexicon {ab}: utterance 1 hears only `a`, so at beam 1 its one live entry ends mid-word: count 0, score -1e30; utterances 0 and
    2 hear `a b` and return it, exactly as they do when decoded without the middle one."""
    lex, trie, _ = _small(tmp_path, "ab 2 3\n", 4, 1)
    S, T = 3, 4
    probs = np.full((T * S, 4), 0.02, np.float32)
    for s, path in enumerate(((2, 3, 0, 0), (2, 2, 0, 0), (2, 0, 3, 0))):
        for t, c in enumerate(path):
            probs[t * S + s, c] = 0.94
    lens = np.array([T, T, T], np.int32)
    got = _decode(ctc, lens, probs, 1, 3, 1, trie, None, 1.0, 0.3)
    assert got[0] == [[[2, 3]], [], [[2, 3]]] and got[3][:, 0].tolist() == [2, -1, 2] and got[6][:, 0].tolist() == [1, -1, 1]
    assert got[1][1, 0] == np.float32(-1e30) and got[4][1, 0] == np.float32(-1e30) and np.all(got[2][1] == -1) and np.all(got[5][1] == -1)
    alone = _decode(ctc, lens[[0, 2]], np.ascontiguousarray(probs.reshape(T, S, 4)[:, [0, 2]].reshape(-1, 4)), 1, 3, 1, trie, None, 1.0, 0.3)
    assert np.array_equal(alone[1].view(np.int32), got[1][[0, 2]].view(np.int32)) and alone[0] == [got[0][0], got[0][2]]
    ref = X.reference_of(lens, probs, S, 1, 3, lex, None, 1.0, 0.3, False)
    assert [len(r["beam64"]) for r in ref] == [1, 0, 1]
    _hold("mid-word", lens, probs, S, ref, got, 1, lex, None, None, 1.0, 0.3, False)
    # a wider beam keeps the empty prefix alive, which is complete: the utterance returns the empty labelling
    wide = _decode(ctc, lens, probs, 8, 3, 2, trie, None, 1.0, 0.3)
    assert [] in wide[0][1] and wide[6][1].tolist()[wide[0][1].index([])] == 0


def test_trailing_space_is_dropped_for_the_next_complete_entry(ctc, tmp_path):
    """Lexicon {a}: the frames say `a <space>`, so the best live entry ends in a space -- it stands on the root, which ends no word --
    and the runner-up (a) is what comes back, first."""
    lex, trie, _ = _small(tmp_path, "a 2\n", 3, 1)
    probs = np.array([[0.05, 0.05, 0.9], [0.05, 0.9, 0.05]], np.float32)
    lens = np.array([2], np.int32)
    ref = X.reference_of(lens, probs, 1, 4, 2, lex, None, 1.0, -0.2, False)
    assert ref[0]["beam64"][0][0] == (2,) and R.lnp64(R.log64(probs), (2, 1)) > R.lnp64(R.log64(probs), (2,))
    got = _decode(ctc, lens, probs, 4, 2, 4, trie, None, 1.0, -0.2)
    assert got[0][0][0] == [2] and [2, 1] not in got[0][0] and sorted(got[0][0]) == [[], [2]]
    _hold("trailing space", lens, probs, 1, ref, got, 4, lex, None, None, 1.0, -0.2, False)


def test_eos_rerank(ctc, tmp_path):
    """Two words of one unit each: (a) wins acoustically and with the LM's word weights (they are equal), and loses to (b) only through
    ln P(</s> | a) against ln P(</s> | b)."""
    arpa = ("\\data\\\nngram 1=4\nngram 2=2\n\n\\1-grams:\n-99 <s> 0\n-1 </s>\n-0.5 a 0\n-0.5 b 0\n\n"
            "\\2-grams:\n-2.0 a </s>\n-0.1 b </s>\n\n\\end\\\n")
    lex, trie, lm = _small(tmp_path, "a 2\nb 3\n", 4, 1, arpa)
    probs = np.array([[0.1, 0.02, 0.48, 0.4], [0.1, 0.02, 0.48, 0.4]], np.float32)
    lens = np.array([2], np.int32)
    no = _decode(ctc, lens, probs, 16, 3, 8, trie, lm, 1.0, 0.0, False)
    yes = _decode(ctc, lens, probs, 16, 3, 8, trie, lm, 1.0, 0.0, True)
    assert no[0][0][:2] == [[2], [3]], no[0]
    assert yes[0][0][0] == [3] and yes[0][0].index([2]) > 0, yes[0]
    assert sorted(no[0][0]) == sorted(yes[0][0]) == [[], [2], [3]]          # (2 1 3) needs three frames
    ln10 = np.log(10.0)
    for h, w, fin in (([2], 1, -2.0), ([3], 2, -0.1)):
        i, j = no[0][0].index(h), yes[0][0].index(h)
        assert no[5][0, i, 0] == w and yes[5][0, j, 0] == w
        assert abs(float(yes[1][0, j]) - (float(no[1][0, i]) + fin * ln10)) <= 1e-5
        assert abs(float(yes[4][0, j]) - (float(no[4][0, i]) + fin * ln10)) <= 1e-5
        assert abs(float(yes[4][0, j]) - lm.Score([w], eos=True)) <= 1e-5
    i = yes[0][0].index([])
    assert abs(float(yes[1][0, i]) - (R.lnp64(R.log64(probs), ()) + lm.Final(lm.Start()))) <= 1e-5


@pytest.mark.parametrize("name", dc.TIE_CASES)
def test_ties_are_deterministic(ctc, made, name):
    lens, probs, T, S = dc.build(name)
    lex = xc.lexicon(name, xc.TIE_LEXICONS)
    assert lex.K == probs.shape[1]
    _, _, trie, _ = made(lex, None, tag="tie_" + name)
    B, C, N, beta = 8, 4, 8, 0.25
    a = _decode(ctc, lens, probs, B, C, N, trie, None, 1.0, beta)
    b = _decode(ctc, lens, probs, B, C, N, trie, None, 1.0, beta)
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    ref = X.reference_of(lens, probs, S, B, C, lex, None, 1.0, beta, False)
    _invariants(name, lens, probs, S, a, N, [r["bar"] if r["beam64"] else None for r in ref], lex, None, None, 1.0, beta, False)


def test_conventions(ctc, made):
    from eesen_amd.api import CuMatrix, EesenError
    lex, model, trie, lm = made("k7_sp3", "v12_o3_unk")
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
    ref = X.reference_of(lens, probs, S, 8, 3, lex, model, alpha, 0.3, True)
    _hold("conventions", lens, probs, S, ref, with_eos, 2, lex, model, lm, alpha, 0.3, True)
    # a lexicon for another K; an LM whose K is not V + 1; use_eos without an LM or without </s>; non-finite weights; the limits
    _, _, other, other_lm = made("k8_sp7", "v20_o4")
    _, _, big, noeos = made("k30_sp1", "v1000_o2_noeos")
    dev = CuMatrix.from_numpy(probs)
    dev30 = CuMatrix.from_numpy(cc.softmax32(rng.standard_normal((T * S, 30)).astype(np.float32)))
    for m, kw, word in ((dev, dict(lexicon=other), "another class count"), (dev, dict(lexicon=trie, lm=other_lm), "word count + 1"),
                        (dev, dict(lexicon=trie, lm_eos=True), "use_eos"), (dev30, dict(lexicon=big, lm=noeos, lm_eos=True), "</s>"),
                        (dev, dict(lexicon=trie, lm=lm, lm_weight=float("nan")), "finite"), (dev, dict(lexicon=trie, word_bonus=float("inf")), "finite"),
                        (dev, dict(lexicon=trie, beam=65), "beam")):
        with pytest.raises(EesenError) as e:
            ctc.DecodeParallel(lens, m, **kw)
        assert e.value.code == -1 and word in str(e.value), kw
    ok = ctc.DecodeParallel(lens, dev30, lexicon=big, lm=noeos)          # the same model without eos is fine
    assert len(ok[0]) == S
    # lex == NULL through the C-ABI
    fn = np.ascontiguousarray(lens, np.int32)
    hyp, hl, sc = np.empty((S, 1, T), np.int32), np.empty((S, 1), np.int32), np.empty((S, 1), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = ctc.lib.eesen_ctc_decode_parallel_lex(ctc.h, vp(fn), S, C.c_void_p(dev.ptr), dev.rows, dev.cols, dev.stride, 0, 4, 3, 1, None, None, 1.0, 0.0, 0,
                                               vp(hyp), vp(hl), vp(sc), None, None, None)
    assert rc == -1 and b"lexicon handle is null" in ctc.lib.eesen_last_error()


def test_guard_word_set_returns_nan_and_minus_one(gpu, made):
    from eesen_amd import synth
    from eesen_amd.api import Net, Ctc
    lens, probs, T, S, lex, model, cfg, _ = X.case("k7_c3")
    _, _, trie, lm = made(cfg["lex"], cfg["model"])
    net = Net.from_layers(synth.make_model(**synth.config("tiny_bi")))
    ctc = Ctc()
    ctc.SetGuard(net)
    ok = _decode(ctc, lens, probs, 4, 3, 2, trie, lm, 0.5, 0.1, True)
    assert np.all(np.isfinite(ok[1])) and np.all(ok[3][:, 0] >= 0)
    net._raise_error_word(2)
    hyps, scores, raw, hlen, lms, words, wlen = _decode(ctc, lens, probs, 4, 3, 2, trie, lm, 0.5, 0.1, True)
    assert np.all(np.isnan(scores)) and np.all(np.isnan(lms)) and np.all(hlen == -1) and np.all(raw == -1) and all(h == [] for h in hyps)
    assert np.all(words == -1) and np.all(wlen == -1)
    net._raise_error_word(0)
    again = _decode(ctc, lens, probs, 4, 3, 2, trie, lm, 0.5, 0.1, True)
    assert np.array_equal(again[1], ok[1]) and again[0] == ok[0] and np.array_equal(again[4], ok[4]) and np.array_equal(again[5], ok[5])
    ctc.SetGuard(None)


def test_statistics_untouched_and_times_populated(gpu, made):
    from eesen_amd.api import Ctc, CuMatrix
    lens, probs, labels, T, S = cc.build("dense_3x12x7")
    _, _, trie, lm = made("k7_sp3", "v12_o3_unk")
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


@pytest.mark.parametrize("key", list(lc.CASES))
def test_other_modes_are_untouched_by_a_lexicon_call(gpu, made, tmp_path, key):
    """On one Ctc: the plain and the token-LM call return the same arrays before and after a lexicon call with a word LM -- the table
    caches (the token LM's, the word LM's, the lexicon's) do not leak between the modes."""
    from eesen_amd.api import Ctc, CuMatrix, TokenLm
    cfg = lc.CASES[key]
    lens, probs, T, S = dc.build(cfg["case"])
    m = L.model_of(cfg["model"])
    arpa, units = m.write(tmp_path, "tok")
    tok = TokenLm(arpa, units, K=m.K)
    B, C = cfg["B"], cfg["C"]
    N = min(B, 4)
    ctc = Ctc()
    dev = CuMatrix.from_numpy(probs)

    def both():
        out = []
        for kw in (dict(), dict(lm=tok, lm_weight=cfg["alpha"], insertion_bonus=cfg["beta"], lm_eos=cfg["eos"])):
            hyps, scores = ctc.DecodeParallel(lens, dev, beam=B, max_classes=C, nbest=N, **kw)
            out.append((hyps, scores.copy(), ctc.hyp.copy(), ctc.hyp_len.copy(), None if ctc.lm_score is None else ctc.lm_score.copy()))
            assert ctc.words is None and ctc.words_len is None
        return out
    before = both()
    xcfg = xc.CASES["k7_c3"]
    xlens, xprobs, _, _, _, _, _, _ = X.case("k7_c3")
    _, _, trie, wlm = made(xcfg["lex"], xcfg["model"])
    first = _decode(ctc, xlens, xprobs, xcfg["B"], xcfg["C"], 2, trie, wlm, xcfg["alpha"], xcfg["beta"], xcfg["eos"])
    after = both()
    again = _decode(ctc, xlens, xprobs, xcfg["B"], xcfg["C"], 2, trie, wlm, xcfg["alpha"], xcfg["beta"], xcfg["eos"])
    for x, y in zip(before, after):
        assert x[0] == y[0]
        for p, q in zip(x[1:], y[1:]):
            assert (p is None and q is None) or np.array_equal(p.view(np.int32), q.view(np.int32))
    assert first[0] == again[0]
    for p, q in zip(first[1:], again[1:]):
        assert np.array_equal(p.view(np.int32), q.view(np.int32))
