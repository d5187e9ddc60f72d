"""CPU: the conditions that tests/test_gpu_ctc_decode_words.py relies on, held on the restatement (tests/ctc_words_restatement.py) and
the inputs of tests/ctc_words_cases.py alone.

  exhaustive   at K = 4, T <= 5, beam 64 the restatement returns exactly the hypotheses brute-force enumeration finds -- every
               segmentation and every homophone of every labelling with a path -- each with lnp64 + alpha * lm64 + beta * |words|;
               at most 64 hypotheses are live at any frame and at most 64 are final, so nothing is pruned (the inputs give way, never
               the 64); the lexicon has a prefix word, a homophone pair and a repeated unit
  cases        at most S // 8 unstable utterances each (a seed that misses the cap is replaced in the cases file, never the cap);
               homophones stand only beside a word model; every lexicon fits the admitted limit at its (beam, max_classes)
  fp32         on stable utterances the fp32 restatement's 1-best is the fp64 one's, its score within the bar
"""
import numpy as np
import pytest

from tests import ctc_beam_restatement as R
from tests import ctc_words_cases as wc
from tests import ctc_words_restatement as W


def test_exhaustive_is_the_enumeration_and_nothing_is_pruned():
    cfg = wc.EXHAUSTIVE
    lex, model = W.lex_of(cfg["lex"]), W.model_of(cfg["model"])
    assert cfg["B"] == 64 and lex.K == 4 and max(cfg["lens"]) <= 5
    spell = lex.spell
    assert any(sp[:i] in spell for sp in spell for i in range(1, len(sp)))          # a word that is a prefix of another
    assert lex.H == 2 and any(len(set(sp)) < len(sp) for sp in spell)               # a homophone pair, a repeated unit
    lens, probs, T, S = wc.build_exhaustive()
    alpha, beta = cfg["alpha"], cfg["beta"]
    total = 0
    for s in range(S):
        n = int(lens[s])
        u = R.utterance(probs, s, S, n)
        lp, l32 = R.log64(u), R.log32(u)
        live = []
        out = W.beam_search(lp, l32, 64, cfg["C"], lex, model, alpha, beta, cfg["eos"], live_count=live)
        assert max(live) <= 64 and len(out) <= 64, (s, live, len(out))
        want = {h: W.exact_of(model, alpha, beta, cfg["eos"], lp, *W.split(h)[:2]) for h in W.enumerate_hypotheses(lex, lp)}
        assert {h for h, _, _ in out} == set(want) and len(out) == len(want), s
        for h, score, lmsum in out:
            labels, words, ends = W.split(h)
            assert lex.consistent(labels, words, ends)
            assert abs(score - want[h]) <= R.bar_of(want[h], n) + W.lm_term(model, alpha, words, cfg["eos"])[0], (s, h)
            assert abs(lmsum - W.lm64(model, words, cfg["eos"])[0]) <= 1e-9, (s, h)
        assert out[0][0] == max(want, key=want.get)
        total += len(out)
        if n == 5:          # homophones and both segmentations of a prefix word are among them, as hypotheses of their own
            by_labels = {}
            for h in want:
                by_labels.setdefault(W.split(h)[0], []).append(h)
            assert max(map(len, by_labels.values())) >= 4
    assert total > 40


@pytest.mark.parametrize("key", list(wc.CASES))
def test_cases_are_stable_enough(key):
    lens, probs, T, S, lex, model, cfg, ref = W.case(key)
    unstable = [s for s in range(S) if not ref[s]["stable"]]
    print(f"{key}: S {S} H {lex.H} unstable {unstable}; without a complete entry {[s for s in range(S) if not ref[s]['beam64']]}")
    assert len(unstable) <= S // 8, (key, unstable)
    assert model is not None or lex.H == 1, key                                     # homophones only beside a model
    assert cfg["B"] * (1 + min(cfg["C"], lex.K - 1) * (1 + lex.H)) <= 4096
    assert sum(1 for r in ref if r["beam64"]) >= (S + 1) // 2                       # the checks have something to hold
    for s in range(S):
        r = ref[s]
        if r["stable"] and r["beam64"]:
            assert r["beam32"] and r["beam32"][0][0] == r["beam64"][0][0] and abs(r["beam32"][0][1] - r["score64"]) <= r["bar"], (key, s)


def test_the_cases_reach_what_they_are_for():
    assert W.lex_of("k8").H >= 3 and W.lex_of("k40").H == 8 and W.lex_of("k40").V == 1000
    c = wc.CASES["k40_16x20_h8"]
    assert (c["B"], c["C"]) == (16, 20) and 16 * (1 + 20 * 9) == 2896
    lens = wc.build("k30_33x40")[0]
    assert lens.size == 33 and (lens == 0).sum() == 1 and len(set(lens.tolist())) > 4
    # a close and a merge across it happen: some stable 1-best of the homophone case holds a homophone
    lens, probs, T, S, lex, model, cfg, ref = W.case("k8_h3")
    homophones = {w for ws in lex.spell.values() if len(ws) > 1 for w in ws}
    assert any(set(W.split(r["beam64"][0][0])[1]) & homophones for r in ref if r["beam64"])


def test_split_and_segmentations():
    lex = W.lex_of("exhaustive")
    h = (1, W.mark(1), 1, 1, W.mark(2), 2, 3, W.mark(4))
    assert W.split(h) == ((1, 1, 1, 2, 3), (1, 2, 4), (1, 3, 5)) and W.partial(h) == () and W.partial(h[:-1]) == (2, 3)
    segs = W.segmentations(lex, (1, 1, 2, 3))
    assert sorted(W.split(x)[1] for x in segs) == [(1, 1, 3), (1, 1, 4), (2, 3), (2, 4)]
    assert W.segmentations(lex, (2,)) == [] and W.segmentations(lex, ()) == [()]
    assert lex.consistent((1, 1), (2,), (2,)) and lex.consistent((1, 1), (1, 1), (1, 2)) and not lex.consistent((1, 1), (1,), (2,))
    assert not lex.consistent((1, 1), (1, 1), (1, 1)) and not lex.consistent((1,), (), ()) and lex.consistent((), (), ())
