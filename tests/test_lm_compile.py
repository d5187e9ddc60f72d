"""CPU: csrc/lm.cpp -- ARPA text -> backoff automaton -- against the textbook ARPA definition on dictionaries of n-gram tuples
(tests/ctc_lm_restatement.py: Model.cond / Model.lm64, which has no automaton).  eesen_lm_* do no device work, so nothing here needs a GPU.

  for every generated model, every history of length <= order over a small alphabet (2000 random ones for the larger models), every
  class:   the eesen_lm_step chain, eesen_lm_final and eesen_lm_score equal the textbook value within 1e-6 of sum|terms| (the weights
           are stored in fp32); the state after a history depends on its last order - 1 symbols only
  every malformed-file case of INTEGRATION.md "LM fusion" is an error with a message; words resolve through the units table first;
  a fully specified model gives the same scores whatever its lower orders' backoff weights are
"""
import itertools

import numpy as np
import pytest

from tests import ctc_lm_cases as lc
from tests import ctc_lm_restatement as L

REL = 1e-6


def _lm(model, directory, stem="lm"):
    from eesen_amd.api import TokenLm
    arpa, units = model.write(directory, stem)
    return TokenLm(arpa, units, K=model.K)


def _walk(lm, labels):
    """(state after the labels, fp64 sum of the fp32 step weights)"""
    st, tot = lm.Start(), 0.0
    for c in labels:
        w, st = lm.Step(st, int(c))
        tot += w
    return st, tot


def _histories(model, rng):
    K, N = model.K, model.order
    if (K - 1) ** N <= 3000:
        return [h for n in range(N + 1) for h in itertools.product(range(1, K), repeat=n)]
    return [tuple(rng.integers(1, K, size=int(rng.integers(0, N + 3))).tolist()) for _ in range(2000)]


@pytest.mark.parametrize("name", list(lc.MODELS))
def test_automaton_is_the_textbook_definition(name, tmp_path):
    model = L.model_of(name)
    lm = _lm(model, tmp_path)
    info = lm.Info()
    assert info["order"] == model.order and info["has_eos"] == model.has_eos
    listed = sum(1 for g in model.grams if len(g) < model.order and g[-1] not in (L.EOS, L.UNK))
    assert info["states"] == 1 + listed
    rng = np.random.default_rng(5)
    classes = range(1, model.K)
    by_tail = {}
    for h in _histories(model, rng):
        st, tot = _walk(lm, h)
        want, absum = model.lm64(h, False)
        assert abs(tot - want) <= REL * absum, (h, tot, want)
        score, sabs = lm.Score(h, eos=False, with_abs=True)
        assert abs(score - want) <= REL * absum and abs(sabs - absum) <= REL * absum, (h, score, want)
        tail = model.history(h)
        assert by_tail.setdefault(tail, st) == st, (h, tail)          # the state is a function of the last order - 1 symbols
        for c in classes:
            w, _ = lm.Step(st, int(c))
            v, a = model.cond(int(c), tail)
            assert abs(w - float(v)) <= REL * a, (h, c, w, float(v))
            assert np.float32(w) == model.cond(int(c), tail, np.float32)[0], (h, c)          # and the fp32 order of additions, exactly
        if model.has_eos:
            v, a = model.cond(L.EOS, tail)
            assert abs(lm.Final(st) - float(v)) <= REL * a, (h, lm.Final(st), float(v))
            se, sa = lm.Score(h, eos=True, with_abs=True)
            we, wa = model.lm64(h, True)
            assert abs(se - we) <= REL * wa and abs(sa - wa) <= REL * wa, h
        else:
            assert lm.Final(st) == 0.0


def test_the_generated_models_cover_what_they_must():
    """N-grams missing at every depth, positive backoffs, unlisted suffixes, <s> contexts, </s> successors -- and a class on <unk>,
    a units table with a unit spelled <UNK>."""
    feats = {name: L.features(L.model_of(name)) for name in lc.MODELS}
    for name in ("k7_o4_unk", "k46_o3", "k40_o3", "k30_o4", "k100_o3"):
        assert all(feats[name].values()), (name, feats[name])
    m = L.model_of("k7_o4_unk")
    assert (5,) not in m.grams and (L.UNK,) in m.grams and "<UNK>" in m.names
    assert not L.model_of("k12_o3_noeos").has_eos and (L.BOS,) not in L.model_of("k12_o3_noeos").grams


def test_class_without_unigram_takes_unk_or_fails(tmp_path):
    from eesen_amd.api import EesenError
    with_unk = L.random_model(seed=11, K=6, order=3, missing=(2, 4), unk=True)
    lm = _lm(with_unk, tmp_path, "a")
    unk = with_unk.p[(L.UNK,)]
    for c in (2, 4):
        assert lm.Step(0, c) == (np.float32(unk), 0)          # <unk>'s weight, and no state of its own
    without = L.random_model(seed=11, K=6, order=3, missing=(2, 4), unk=False)
    with pytest.raises(EesenError, match="class 2 has no unigram") as e:
        _lm(without, tmp_path, "b")
    assert e.value.code == -1


ARPA = """
\\data\\
ngram 1=5
ngram 2=3
ngram 3=1

\\1-grams:
-99 <s> -0.3
-1.1 </s>
-0.4 a -0.2
-0.6 b 0.1
-0.9 <UNK> -0.5

\\2-grams:
-0.25 <s> a -0.15
-0.7 a b
-0.35 b </s>

\\3-grams:
-0.05 <s> a b

\\end\\
"""
UNITS = "a 1\nb 2\n<UNK> 3\n"


def _files(tmp_path, arpa=ARPA, units=UNITS):
    a = tmp_path / "x.arpa"
    a.write_text(arpa)
    u = None
    if units is not None:
        u = tmp_path / "units.txt"
        u.write_text(units)
    return str(a), None if u is None else str(u)


def test_hand_made_model_and_units_first_resolution(tmp_path):
    from eesen_amd.api import TokenLm
    lm = TokenLm(*_files(tmp_path), K=4)
    ln10 = np.log(10.0)
    assert lm.Info() == dict(order=3, states=7, arcs=6, has_eos=True)          # states: empty, <s>, a, b, <UNK>, <s> a, a b
    # <UNK> is a unit (class 3), not the LM's unknown word: it has a unigram and a state of its own
    w, st = lm.Step(0, 3)
    assert abs(w - (-0.9 * ln10)) < 1e-6 and st != 0
    # <s> a b: the trigram; then b </s> through the state of `a b` -> `b`
    v = lm.Score([1, 2], eos=True)
    assert abs(v - (-0.25 - 0.05 - 0.35) * ln10) < 1e-5
    # a after <s> a: no `<s> a a`, no `a a`: bo(<s> a) + bo(a) + P(a)
    v = lm.Score([1, 1])
    assert abs(v - (-0.25 + (-0.15 - 0.2 - 0.4)) * ln10) < 1e-5
    # the same file without a units table: its words are no class ids
    from eesen_amd.api import EesenError
    a, _ = _files(tmp_path, units=None)
    with pytest.raises(EesenError, match="word a "):
        TokenLm(a, None, K=4)
    # decimal words without a units table; <unk> is the LM's unknown word there and fills class 3
    dec = ARPA.replace(" a", " 1").replace(" b", " 2").replace("<UNK>", "<unk>")
    a, _ = _files(tmp_path, arpa=dec, units=None)
    lm2 = TokenLm(a, None, K=4)
    assert lm2.Info()["states"] == 6 and lm2.Step(0, 3) == (np.float32(-0.9 * ln10), 0)
    assert abs(lm2.Score([1, 2], eos=True) - lm.Score([1, 2], eos=True)) < 1e-12


@pytest.mark.parametrize("what,arpa,units,word", [
    ("no data section", ARPA.replace("\\data\\", "\\dat\\"), UNITS, "no \\data\\ section"),
    ("a count that disagrees", ARPA.replace("ngram 2=3", "ngram 2=4"), UNITS, "the header says 4"),
    ("a count that disagrees (last section)", ARPA.replace("ngram 3=1", "ngram 3=2"), UNITS, "the header says 2"),
    ("a word too many", ARPA.replace("-0.7 a b", "-0.7 a b a 0.1"), UNITS, "2 words"),
    ("a word too few", ARPA.replace("-0.05 <s> a b", "-0.05 <s> a"), UNITS, "3 words"),
    ("a backoff weight at the top order", ARPA.replace("-0.05 <s> a b", "-0.05 <s> a b -0.1"), UNITS, "3 words"),
    ("a non-numeric value", ARPA.replace("-0.7 a b", "-0.7x a b"), UNITS, "not a finite number"),
    ("a non-numeric backoff", ARPA.replace("-0.4 a -0.2", "-0.4 a zero"), UNITS, "not a finite number"),
    ("an infinite value", ARPA.replace("-0.7 a b", "-inf a b"), UNITS, "not a finite number"),
    ("an absent prefix", ARPA.replace("-0.05 <s> a b", "-0.05 a a b"), UNITS, "prefix"),
    ("an unknown word", ARPA.replace("-0.7 a b", "-0.7 a c"), UNITS, "word c "),
    ("a unit id outside [1, K)", ARPA, "a 1\nb 2\n<UNK> 4\n", "outside [1, K)"),
    ("a class id outside [1, K)", ARPA.replace(" a", " 1").replace(" b", " 9").replace("<UNK>", "3"), None, "word 9 "),
    ("2^31 n-grams", ARPA.replace("ngram 3=1", "ngram 3=2147483648"), UNITS, "below 2^31"),
    ("order 9", "\\data\\\n" + "".join(f"ngram {n}=1\n" for n in range(1, 10)) + "\n\\1-grams:\n-1 1\n\\end\\\n", None, "order 1..8"),
])
def test_malformed_files_are_errors(tmp_path, what, arpa, units, word):
    from eesen_amd.api import EesenError, TokenLm
    a, u = _files(tmp_path, arpa, units)
    with pytest.raises(EesenError) as e:
        TokenLm(a, u, K=4)
    assert e.value.code == -1 and word in str(e.value), (what, str(e.value))


def test_missing_file_and_bad_arguments(tmp_path):
    from eesen_amd.api import EesenError, TokenLm
    with pytest.raises(EesenError, match="cannot open"):
        TokenLm(str(tmp_path / "none.arpa"), None, K=4)
    lm = TokenLm(*_files(tmp_path), K=4)
    for call in (lambda: lm.Step(99, 1), lambda: lm.Step(0, 0), lambda: lm.Step(0, 4), lambda: lm.Final(-1), lambda: lm.Score([4])):
        with pytest.raises(EesenError):
            call()


def test_fully_specified_model_ignores_lower_order_backoffs(tmp_path):
    """Every n-gram listed at the top order (every context, every successor, the shorter contexts that begin with <s> included): no
    lookup ever backs off, so the lower orders' backoff weights do not matter."""
    K, N = 4, 3
    rng = np.random.default_rng(21)
    syms = list(range(1, K))

    def build(bo_seed):
        brng = np.random.default_rng(bo_seed)
        vr = np.random.default_rng(22)
        val = lambda: round(float(vr.uniform(-2.0, -0.1)), 4)
        bow = lambda: round(float(brng.uniform(-1.0, 0.5)), 4)
        g = {(L.BOS,): (-99.0, bow()), (L.EOS,): (val(), None)}
        for c in syms:
            g[(c,)] = (val(), bow())
        for h in [(L.BOS,)] + [(c,) for c in syms]:
            for w in syms + [L.EOS]:
                g[h + (w,)] = (val(), bow() if w != L.EOS else None)
        for h in [(L.BOS, c) for c in syms] + [(a, b) for a in syms for b in syms]:
            for w in syms + [L.EOS]:
                g[h + (w,)] = (val(), None)
        return L.Model(K, N, g)

    a, b = _lm(build(1), tmp_path, "a"), _lm(build(2), tmp_path, "b")
    for _ in range(200):
        lab = rng.integers(1, K, size=int(rng.integers(0, 7))).tolist()
        assert a.Score(lab, eos=True) == b.Score(lab, eos=True) == pytest.approx(build(1).lm64(lab, True)[0], abs=1e-5)
