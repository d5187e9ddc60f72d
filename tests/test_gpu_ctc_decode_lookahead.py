"""-m gpu: the unigram LM look-ahead in the two lexicon searches (csrc/ctc_decode.hip: ctc_prefix_beam_lex_la_kernel,
ctc_word_beam_la_kernel; csrc/lex.cpp: Lexicon::lookahead; through api.Ctc.DecodeParallel(lm_lookahead=True)), per utterance against
the fp64 restatement (tests/ctc_lookahead_restatement.py: dictionaries of spelling prefixes, no trie) and against the exact score of
every returned entry -- the checks of tests/test_gpu_ctc_decode_lex.py and tests/test_gpu_ctc_decode_words.py, whose _hold this file
calls: a returned score keeps its meaning under the look-ahead, only the pruning changes.

tests/test_ctc_lookahead_cases.py holds, without a GPU, the conditions on these inputs that the checks rely on.  Each case prints
`worst |score - score64| / bar` (recorded in profiles/ctc_decode_lookahead.md).
"""
import ctypes as C

import numpy as np
import pytest

from tests import ctc_beam_restatement as R
from tests import ctc_lex_cases as xc
from tests import ctc_lex_restatement as X
from tests import ctc_lm_restatement as L
from tests import ctc_lookahead_cases as kc
from tests import ctc_lookahead_restatement as A
from tests import ctc_words_cases as wc
from tests import ctc_words_restatement as W
from tests import test_gpu_ctc_decode_lex as TX
from tests import test_gpu_ctc_decode_words as TW
from tests import test_gpu_ctc_stamps as TS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctc(gpu):
    from eesen_amd.api import Ctc
    return Ctc()


@pytest.fixture(scope="module")
def made(gpu, tmp_path_factory):
    """(tag, restatement lexicon, word model) -> (api.Lexicon, api.TokenLm), each made once; the ARPA text names the words as the
    lexicon does and is read through Lexicon.WriteWords' table."""
    from eesen_amd.api import Lexicon, TokenLm
    d = tmp_path_factory.mktemp("la")
    done = {}

    def get(tag, rl, model):
        if tag not in done:
            trie = Lexicon(rl.write(d, tag), None, K=rl.K, space=None if isinstance(rl, W.WLex) else rl.space)
            table = str(d / (tag + ".words.txt"))
            trie.WriteWords(table)
            by_id = {w: n for n, w in rl.ids.items()}
            arpa, _ = L.Model(model.K, model.order, model.grams, [None] + [by_id[w] for w in range(1, rl.V + 1)]).write(d, tag)
            done[tag] = (trie, TokenLm(arpa, table, K=rl.V + 1))
        return done[tag]
    return get


def _of_case(made, key):
    cfg = kc.CASES[key]
    rl, model = kc.lex_of(key), kc.model_of(cfg["model"])
    return made(("w." if cfg["unspaced"] else "x.") + cfg["lex"] + "." + cfg["model"], rl, model)


def _decode(ctc, lens, m, B, C, N, trie, lm, alpha, beta, eos, la):
    """The tuples of tests/test_gpu_ctc_decode_lex.py: _decode (spaced) / tests/test_gpu_ctc_decode_words.py: _decode (unspaced: the
    word ends behind them)."""
    from eesen_amd.api import CuMatrix
    if isinstance(m, np.ndarray):
        m = CuMatrix.from_numpy(m)
    hyps, scores = ctc.DecodeParallel(lens, m, beam=B, max_classes=C, nbest=N, lm=lm, lm_weight=alpha, lm_eos=eos, lexicon=trie, word_bonus=beta,
                                      lm_lookahead=la)
    out = (hyps, scores, ctc.hyp.copy(), ctc.hyp_len.copy(), ctc.lm_score.copy(), ctc.words.copy(), ctc.words_len.copy())
    return out + (ctc.word_ends.copy(),) if trie.unspaced else out


def _bit_identical(a, b):
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("key", list(kc.CASES))
def test_cases(ctc, made, key):
    lens, probs, T, S, lex, model, cfg, la, ref = A.case(key)
    trie, lm = _of_case(made, key)
    B, Cc = cfg["B"], cfg["C"]
    N = min(B, 4)
    got = _decode(ctc, lens, probs, B, Cc, N, trie, lm, cfg["alpha"], cfg["beta"], cfg["eos"], True)
    hold = TW._hold if cfg["unspaced"] else TX._hold
    hold(f"{key} ({B}, {Cc}) V {lex.V} look-ahead", lens, probs, S, ref, got, N, lex, model, lm, cfg["alpha"], cfg["beta"], cfg["eos"])
    assert ctc.LmLookahead() == 0          # the call restored the object's mode


@pytest.mark.parametrize("key", ["zipf_k7_c3", "zipf_64x32", "zipf_w_k7_c3", "zipf_w_limit"])
def test_zero_weights_are_the_search_without_it(ctc, made, key):
    """alpha = beta = 0: eta is 0 on every node, so every array is the one the kernels without the look-ahead return."""
    lens, probs, T, S = kc.build(key)
    cfg = kc.CASES[key]
    trie, lm = _of_case(made, key)
    off = _decode(ctc, lens, probs, cfg["B"], cfg["C"], 4, trie, lm, 0.0, 0.0, False, False)
    on = _decode(ctc, lens, probs, cfg["B"], cfg["C"], 4, trie, lm, 0.0, 0.0, False, True)
    _bit_identical(on, off)
    assert any(len(h) for h in on[0])


def test_exhaustive_is_unchanged_where_nothing_is_pruned(ctc, made):
    """Beam 64 on the exhaustive cases: every candidate survives every frame, so the rank decides nothing but the order inside the
    beam, and the final ranking is by the real total: labels, scores, LM sums and words are those of the search without it."""
    for unspaced, cases, restate in ((False, xc, X), (True, wc, W)):
        cfg = cases.EXHAUSTIVE
        rl, model = restate.lex_of(cfg["lex"]), restate.model_of(cfg["model"])
        trie, lm = made(("w." if unspaced else "x.") + "exhaustive", rl, model)
        lens, probs, T, S = cases.build_exhaustive()
        off = _decode(ctc, lens, probs, cfg["B"], cfg["C"], 64, trie, lm, cfg["alpha"], cfg["beta"], True, False)
        on = _decode(ctc, lens, probs, cfg["B"], cfg["C"], 64, trie, lm, cfg["alpha"], cfg["beta"], True, True)
        _bit_identical(on, off)
        assert max(len(h) for h in on[0]) > 8


def test_efficacy_on_the_device(ctc, made):
    """The condition of tests/test_ctc_lookahead_cases.py: test_efficacy_condition on the device's own scores."""
    key = "zipf_k30"
    lens, probs, T, S, lex, model, cfg, la, ref = A.case(key)
    trie, lm = _of_case(made, key)
    best = {}
    for mode in (True, False):
        got = _decode(ctc, lens, probs, cfg["B"], cfg["C"], 1, trie, lm, cfg["alpha"], cfg["beta"], cfg["eos"], mode)
        best[mode] = [float(got[1][s, 0]) if got[0][s] else None for s in range(S)]
    better, worse, sum_on, sum_off = A.efficacy(best[True], best[False], [r["bar"] for r in ref])
    print(f"{key} beam {cfg['B']} on the device: higher with the look-ahead on {better} utterances, lower on {worse} of {S}; "
          f"summed 1-best score {sum_on:.3f} with, {sum_off:.3f} without")
    assert better >= 2 * worse and better > 0 and sum_on > sum_off


def test_the_mode_persists_and_the_argument_restores_it(ctc, made):
    key = "zipf_k7_c3"
    lens, probs, T, S = kc.build(key)
    cfg = kc.CASES[key]
    trie, lm = _of_case(made, key)
    args = (ctc, lens, probs, 4, cfg["C"], 2, trie, lm, cfg["alpha"], cfg["beta"], True)      # beam 4: the look-ahead changes the result
    off, on = _decode(*args, False), _decode(*args, True)
    assert any(not np.array_equal(x, y) for x, y in zip(on[1:], off[1:]))
    assert ctc.LmLookahead() == 0
    ctc.SetLmLookahead(1)
    try:
        assert ctc.LmLookahead() == 1
        for _ in range(2):                          # it stays set from call to call
            _bit_identical(_decode(*args, None), on)
        _bit_identical(_decode(*args, False), off)
        assert ctc.LmLookahead() == 1               # ... and the argument put it back
        _bit_identical(_decode(*args, None), on)
    finally:
        ctc.SetLmLookahead(0)
    _bit_identical(_decode(*args, None), off)


def test_plain_and_token_lm_calls_ignore_the_mode(ctc, tmp_path):
    from eesen_amd.api import CuMatrix, TokenLm
    lens, probs, T, S = kc.build("zipf_k7_c3")
    dev = CuMatrix.from_numpy(probs)
    m = L.random_model(seed=7501, K=probs.shape[1], order=2)
    arpa, units = m.write(tmp_path, "tok")
    tok = TokenLm(arpa, units, K=probs.shape[1])

    def both():
        h0, s0 = ctc.DecodeParallel(lens, dev, beam=8, max_classes=4, nbest=2)
        h1, s1 = ctc.DecodeParallel(lens, dev, beam=8, max_classes=4, nbest=2, lm=tok, lm_weight=0.7, insertion_bonus=0.2)
        return h0, s0.tobytes(), h1, s1.tobytes(), ctc.lm_score.tobytes()
    before = both()
    ctc.SetLmLookahead(1)
    try:
        assert both() == before
    finally:
        ctc.SetLmLookahead(0)


def test_the_table_follows_the_lm_and_the_lexicon(gpu, made):
    """Two LMs over one lexicon decoded alternately, then another lexicon: every call is the call of a fresh Ctc."""
    from eesen_amd.api import Ctc
    key = "zipf_k7_c3"
    lens, probs, T, S = kc.build(key)
    cfg = kc.CASES[key]
    rl = kc.lex_of(key)
    trie, lm_a = _of_case(made, key)
    other = kc.zipf_model(seed=7601, V=rl.V, bigrams=30)
    _, lm_b = made("x.k7_sp3.other", rl, other)
    assert not np.array_equal(trie.Lookahead(lm_a), trie.Lookahead(lm_b))
    key2 = "zipf_T1500"
    trie2, lm2 = _of_case(made, key2)
    lens2, probs2, _, _ = kc.build(key2)
    short = (np.minimum(lens2, 40).astype(np.int32), np.ascontiguousarray(probs2[:40 * len(lens2)]))
    calls = [(lens, probs, trie, lm_a), (lens, probs, trie, lm_b), (lens, probs, trie, lm_a), short + (trie2, lm2), (lens, probs, trie, lm_b)]
    one = Ctc()
    for i, (ln, pr, tr, lm) in enumerate(calls):
        args = (ln, pr, 4, 3, 2, tr, lm, cfg["alpha"], cfg["beta"], True, True)
        _bit_identical(_decode(one, *args), _decode(Ctc(), *args))
    a = _decode(one, lens, probs, 4, 3, 2, trie, lm_a, cfg["alpha"], cfg["beta"], True, True)
    b = _decode(one, lens, probs, 4, 3, 2, trie, lm_b, cfg["alpha"], cfg["beta"], True, True)
    assert any(not np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))          # the two models do decode differently


def test_guard_word_set_returns_nan_and_minus_one(gpu, made):
    from eesen_amd import synth
    from eesen_amd.api import Net, Ctc
    for key in ("zipf_k7_c3", "zipf_w_k7_c3"):
        lens, probs, T, S = kc.build(key)
        trie, lm = _of_case(made, key)
        net = Net.from_layers(synth.make_model(**synth.config("tiny_bi")))
        ctc = Ctc()
        ctc.SetGuard(net)
        ok = _decode(ctc, lens, probs, 4, 3, 2, trie, lm, 0.5, 0.1, True, True)
        assert np.all(np.isfinite(ok[1])) and np.all(ok[3][:, 0] >= 0)
        net._raise_error_word(2)
        bad = _decode(ctc, lens, probs, 4, 3, 2, trie, lm, 0.5, 0.1, True, True)
        assert np.all(np.isnan(bad[1])) and np.all(np.isnan(bad[4])) and np.all(bad[3] == -1) and np.all(bad[2] == -1) and all(h == [] for h in bad[0])
        assert all(np.all(x == -1) for x in bad[5:])
        net._raise_error_word(0)
        _bit_identical(_decode(ctc, lens, probs, 4, 3, 2, trie, lm, 0.5, 0.1, True, True), ok)
        ctc.SetGuard(None)


def test_stamps_after_a_lookahead_decode(ctc, made):
    """DecodeStamps aligns what the look-ahead decode returned, as tests/test_gpu_ctc_stamps.py holds it for the other modes."""
    for key in ("zipf_k7_c3", "zipf_w_k7_c3"):
        lens, probs, T, S = kc.build(key)
        cfg = kc.CASES[key]
        trie, lm = _of_case(made, key)
        dev = TS._dev(probs)
        _, scores = ctc.DecodeParallel(lens, dev, beam=8, max_classes=cfg["C"], nbest=3, lm=lm, lm_weight=cfg["alpha"], lm_eos=True, lexicon=trie,
                                       word_bonus=cfg["beta"], lm_lookahead=True)
        st = ctc.DecodeStamps(lens, dev)
        aligned = TS._hold(key, ctc, lens, np.asarray(probs), dev, st, scores, False, space=None if cfg["unspaced"] else kc.lex_of(key).space)
        assert aligned >= S


def test_refusals(ctc, made):
    from eesen_amd.api import CuMatrix, EesenError
    for key in ("zipf_k7_c3", "zipf_w_k7_c3"):
        lens, probs, T, S = kc.build(key)
        trie, lm = _of_case(made, key)
        dev = CuMatrix.from_numpy(probs)
        with pytest.raises(EesenError, match="look-ahead.*needs the word LM"):
            ctc.DecodeParallel(lens, dev, beam=4, max_classes=3, lexicon=trie, lm_lookahead=True)
        assert ctc.LmLookahead() == 0
        hyps, _ = ctc.DecodeParallel(lens, dev, beam=4, max_classes=3, lexicon=trie)          # the Ctc is none the worse for it
        assert any(hyps)
    with pytest.raises(EesenError, match="look-ahead.*lexicon"):
        ctc.DecodeParallel(lens, dev, beam=4, max_classes=3, lm_lookahead=True)
    for mode in (2, -1):
        assert ctc.lib.eesen_ctc_set_lm_lookahead(ctc.h, mode) == -1 and b"0 (off) or 1 (unigram)" in ctc.lib.eesen_last_error()
    assert ctc.LmLookahead() == 0
    m = C.c_int(7)
    assert ctc.lib.eesen_ctc_get_lm_lookahead(None, C.byref(m)) != 0 and ctc.lib.eesen_ctc_set_lm_lookahead(None, 1) != 0
