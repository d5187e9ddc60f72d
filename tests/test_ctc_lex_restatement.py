"""CPU: what tests/test_gpu_ctc_decode_lex.py relies on, held with the restatement alone (tests/ctc_lex_restatement.py).

  the restatement against enumeration: on the exhaustive case (K = 4: blank, space, two units; lexicon {a, ab, ba, aa}; at most 64
      prefixes the search can hold exist, so nothing is pruned at beam 64) every labelling of the language that has a path comes back
      with enumerate_paths' ln p + alpha * lm64(words, </s>) + beta * |words|, and nothing else does
  the language: every returned labelling is in L with `segment` its words; the empty one takes only alpha * fin
  over-counting: score <= exact + bar for every entry of every case
  the conditions of the shapes: the space is no candidate on some frames of the C' < K - 1 case, the <unk> fallback is taken, the
      word models have the orders the cases name, the lexicons hold a prefix word and a word with two spellings
  the stability cap: at most S // 8 utterances per case whose 1-best moves under the eight jitter seeds -- a condition on the cases
      (tests/ctc_lex_cases.py records the seeds), not a measurement
  fp32: the restatement run in float32 is within the bar of the fp64 one on the stable utterances, 1-best equal

The bar: bar_of(score64, n) of tests/ctc_beam_restatement.py on the score, plus tests/ctc_lm_restatement.py's LM term with one label
per word.
"""
import numpy as np
import pytest

from tests import ctc_beam_restatement as R
from tests import ctc_lex_cases as xc
from tests import ctc_lex_restatement as X


def test_exhaustive_case_never_prunes():
    cfg = xc.EXHAUSTIVE
    lex = X.lex_of(cfg["lex"])
    assert lex.K == 4 and set(lex.spell) == {(2,), (2, 3), (3, 2), (2, 2)} and cfg["B"] == 64 and cfg["C"] == lex.K - 1
    assert len(X.valid_prefixes(lex, max(cfg["lens"]))) <= 64 < len(X.valid_prefixes(lex, max(cfg["lens"]) + 1))


def test_restatement_is_the_enumeration():
    cfg = xc.EXHAUSTIVE
    lex, model = X.lex_of(cfg["lex"]), X.model_of(cfg["model"])
    alpha, beta = cfg["alpha"], cfg["beta"]
    assert (alpha, beta, cfg["eos"]) == (0.8, 0.5, True) and model.K == lex.V + 1
    lens, probs, T, S = xc.build_exhaustive()
    for s in range(S):
        n = int(lens[s])
        lp = R.log64(R.utterance(probs, s, S, n))
        got = X.beam_search(lp, R.log32(R.utterance(probs, s, S, n)), cfg["B"], cfg["C"], lex, model, alpha, beta, True)
        want = {h: v + alpha * model.lm64(list(lex.segment(h)), True)[0] + beta * len(lex.segment(h)) for h, v in X.enumerate_language(lex, lp).items()}
        assert () in want and len(want) > 1 or n == 0
        assert {h for h, _, _ in got} == set(want), s
        for h, score, lmsum in got:
            assert abs(score - want[h]) <= 1e-12 * max(1.0, abs(want[h])), (s, h)
            assert abs(lmsum - model.lm64(list(lex.segment(h)), True)[0]) <= 1e-12 * max(1.0, abs(lmsum)), (s, h)
        assert [h for h, _, _ in got] == sorted(want, key=want.get, reverse=True)
    # the beta is per word and the space is what pays it: (a Sp a) has two words, (a a) one
    assert lex.segment((2, 1, 2)) == (1, 1) and lex.segment((2, 2)) == (4,) and lex.segment((2, 1)) is None and lex.segment((1, 2)) is None


def test_lexicons_hold_what_the_cases_name():
    for name in xc.LEXICONS:
        lex = X.lex_of(name)
        assert 1 <= lex.space < lex.K and () in lex.prefixes
    for name in ("k7_sp3", "k30_sp1", "k40_sp39"):
        lex = X.lex_of(name)
        words_of = {}
        for sp, w in lex.spell.items():
            words_of.setdefault(w, []).append(sp)
        assert any(len(v) > 1 for v in words_of.values()), name                                   # a word with two spellings
        assert any(sp[:i] in lex.spell for sp in lex.spell for i in range(1, len(sp))), name      # a word that is a prefix of another
    assert X.lex_of("k30_sp1").V == X.lex_of("k40_sp39").V == 1000
    assert X.lex_of("k3_sp1").space == 1 and X.lex_of("k3_sp2").space == 2 and X.lex_of("k40_sp39").space == 39
    assert X.model_of("v1000_o3_unk").order == 3 and (5,) not in X.model_of("v1000_o3_unk").grams
    for name, cfg in xc.TIE_LEXICONS.items():
        assert xc.lexicon(name, xc.TIE_LEXICONS).V == cfg["V"]


@pytest.mark.parametrize("key", list(xc.CASES))
def test_cases_hold_their_conditions(key):
    lens, probs, T, S, lex, model, cfg, ref = X.case(key)
    alpha, beta, eos = cfg["alpha"], cfg["beta"], cfg["eos"]
    unstable = [s for s in range(S) if not ref[s]["stable"]]
    assert len(unstable) <= S // 8, (key, unstable)
    assert sum(1 for r in ref if r["beam64"]) >= S - S // 8, key          # the lexicon finds something almost everywhere
    worst, nwords = 0.0, 0
    for s in range(S):
        r = ref[s]
        n = int(lens[s])
        lp = R.log64(R.utterance(probs, s, S, n))
        for h, score, lmsum in r["beam64"]:
            words = lex.segment(h)
            assert words is not None, (key, s, h)
            lm, absum = X.lm64(model, words, eos)
            exact = R.lnp64(lp, h) + alpha * lm + beta * len(words)
            assert score <= exact + r["bar"], (key, s, h, score, exact)
            assert abs(lmsum - lm) <= 1e-12 * max(1.0, absum), (key, s, h)
        if not r["beam64"] or not r["stable"]:
            continue
        nwords += len(lex.segment(r["beam64"][0][0]))
        assert r["beam32"] and r["beam32"][0][0] == r["beam64"][0][0], (key, s)
        err = abs(r["beam32"][0][1] - r["score64"])
        assert err <= r["bar"], (key, s, err, r["bar"])
        assert abs(r["beam32"][0][2] - r["beam64"][0][2]) <= X.lm_term(model, alpha, lex.segment(r["beam64"][0][0]), eos)[1] + 0.0, (key, s)
        worst = max(worst, err / r["bar"])
    assert nwords >= S, key          # words do close inside the utterances: the space and lm_step are exercised
    print(f"{key}: unstable {unstable} (cap {S // 8}); fp32 |score - score64| / bar <= {worst:.3g}; {nwords} words in the stable 1-bests")


def test_the_space_is_no_candidate_on_some_frames():
    lens, probs, T, S, lex, model, cfg, ref = X.case("k7_c3")
    assert cfg["C"] < lex.K - 1
    with_space = [lex.space in R.candidates(R.log32(probs[r]), cfg["C"]) for r in range(T * S) if r // S < lens[r % S]]
    assert 0 < sum(with_space) < len(with_space)


def test_unk_fallback_is_taken():
    """A 1-best of the V = 1000 case, or one of its runners-up, holds a word without a unigram of its own."""
    model = X.model_of("v1000_o3_unk")
    v, _ = model.cond(5, ())
    assert float(v) == model.p[("<unk>",)]
    lex = X.lex_of("k40_sp39")
    h = lex.spelling_of((3, 5, 17))
    assert lex.segment(h) == (3, 5, 17)
    assert np.isfinite(X.lm64(model, lex.segment(h), True)[0])
