"""-m gpu: minimum Bayes risk over the N-best lists of a real DecodeParallel in each of the four modes (eesen_ctc_decode_mbr over
csrc/edit_distance.hip, through api.Ctc.MbrNbest).

Distances: every integer equals the host routine eesen_edit_distance on what the decode call returned (ctc.hyp / ctc.words).
Posterior, risk and order: the fp64 expression of INTEGRATION.md "Minimum Bayes risk" (tests/mbr_restatement.py) on the RETURNED
distances and scores -- the order exactly, the doubles to 1e-12 relative (the same expression in the same order; the slack is exp's).
"""
import ctypes as C

import numpy as np
import pytest

from tests import ctc_decode_cases as dc
from tests import ctc_lex_cases as xc
from tests import ctc_lex_restatement as X
from tests import ctc_lm_cases as lc
from tests import ctc_lm_restatement as L
from tests import ctc_words_cases as wc
from tests import ctc_words_restatement as W
from tests import mbr_cases as M
from tests import mbr_restatement as Q
from tests.test_gpu_ctc_stamps import small_batch

pytestmark = pytest.mark.gpu

REL = 1e-12
FIELDS = ("dist", "posterior", "risk", "order")


@pytest.fixture(scope="module")
def ctc(gpu):
    from eesen_amd.api import Ctc
    return Ctc()


def _dev(m):
    from eesen_amd.api import CuMatrix
    return CuMatrix.from_numpy(m)


def host(a, b):
    from eesen_amd import _lib
    lib = _lib.load()
    a, b = np.ascontiguousarray(a, np.int32), np.ascontiguousarray(b, np.int32)
    err = C.c_int(-1)
    _lib.check(lib.eesen_edit_distance(a.ctypes.data_as(C.c_void_p), a.size, b.ctypes.data_as(C.c_void_p), b.size, C.byref(err)))
    return err.value


def _tokens(ctc, s, i, level):
    """The tokens of returned entry i of utterance s at `level`; None beyond the returned count."""
    if ctc.hyp_len[s, i] < 0:
        return None
    if level == 1 or ctc.words is None:
        return ctc.hyp[s, i, :int(ctc.hyp_len[s, i])].tolist()
    return ctc.words[s, i, :int(ctc.words_len[s, i])].tolist()


def _close(got, want):
    return abs(got - want) <= REL * abs(want)


def _hold_mbr(name, ctc, res, z, level=0, scale=1.0, refs=None):
    """Every field of `res` against the host routine and the restatement; returns the number of counting entries."""
    S, N = ctc.hyp_len.shape
    assert res.dist.shape == (S, N, N) and res.dist.dtype == np.int32 and res.order.shape == (S, N) and res.order.dtype == np.int32
    assert res.posterior.shape == res.risk.shape == (S, N) and res.posterior.dtype == res.risk.dtype == np.float64
    assert (res.ref_dist is None) == (refs is None)
    counting = 0
    for s in range(S):
        tok = [_tokens(ctc, s, i, level) for i in range(N)]
        cnt = Q.counts(z[s], [len(t) if t is not None else -1 for t in tok])
        counting += sum(cnt)
        for i in range(N):
            for k in range(N):
                want = host(tok[i], tok[k]) if cnt[i] and cnt[k] else -1
                assert res.dist[s, i, k] == want, (name, s, i, k, res.dist[s, i, k], want)
            if refs is not None:
                want = host(tok[i], refs[s]) if cnt[i] else -1
                assert res.ref_dist[s, i] == want, (name, s, i, res.ref_dist[s, i], want)
        P = Q.posterior(z[s], cnt, scale)
        R = Q.risk(P, res.dist[s], cnt)
        for i in range(N):
            if cnt[i]:
                assert _close(res.posterior[s, i], P[i]) and _close(res.risk[s, i], R[i]), (name, s, i, res.posterior[s, i], P[i], res.risk[s, i], R[i])
            else:
                assert res.posterior[s, i] == res.risk[s, i] == Q.NOT_COUNTING, (name, s, i)
        assert res.order[s].tolist() == Q.order(R, z[s], cnt), (name, s, res.order[s], R)
        assert sorted(res.order[s].tolist()) == list(range(N))
        if any(cnt):
            assert abs(sum(p for p, c in zip(P, cnt) if c) - 1.0) < 1e-12
    return counting


def _same(a, b, fields):
    return all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True) for f in fields)


STAMPS = ("label_start", "label_end", "word_start", "word_end", "word_conf", "path_score")
RESCORED = ("am_score", "lm_score", "total", "order")


def _word_lm(d, tag, rl, trie, model):
    from eesen_amd.api import TokenLm
    table = str(d / (tag + ".words.txt"))
    trie.WriteWords(table)
    by_id = {w: n for n, w in rl.ids.items()}
    arpa, _ = L.Model(model.K, model.order, model.grams, [None] + [by_id[w] for w in range(1, rl.V + 1)]).write(d, tag)
    return TokenLm(arpa, table, K=rl.V + 1)


# ------------------------------------------------------------------------------------------------ the four modes
def test_plain_mode_with_references_and_what_the_decode_call_left(ctc):
    lens, probs, T, S = dc.build("dense_3x12x7")
    dev = _dev(probs)
    hyps, scores = ctc.DecodeParallel(lens, dev, beam=8, max_classes=6, nbest=8)
    scores = scores.copy()
    stamps, rescored = ctc.DecodeStamps(lens, dev), ctc.RescoreNbest(lens, dev)
    refs = [hyps[0][2], [], hyps[2][0][::-1] + [3]]
    res = ctc.MbrNbest(refs=refs)
    assert _hold_mbr("plain", ctc, res, scores, refs=refs) == sum(len(h) for h in hyps) > S
    assert res.ref_dist[0, 2] == 0 and res.ref_dist[1, 0] == len(hyps[1][0])
    for scale in (0.0, 0.3, 7.0):
        _hold_mbr(f"plain scale {scale}", ctc, ctc.MbrNbest(scale=scale), scores, scale=scale)
    flat = ctc.MbrNbest(scale=0.0)
    n0 = len(hyps[0])
    assert np.all(flat.posterior[0, :n0] == 1.0 / n0)          # scale 0: the list's medoid wins
    # level 1 is level 0 without a lexicon
    assert _same(ctc.MbrNbest(level=1), ctc.MbrNbest(level=0), FIELDS)
    # nothing the decode call left has moved
    assert _same(stamps, ctc.DecodeStamps(lens, dev), STAMPS) and _same(rescored, ctc.RescoreNbest(lens, dev), RESCORED)
    assert _same(res, ctc.MbrNbest(refs=refs), FIELDS + ("ref_dist",))
    # totals from the second pass, and the same with an entry the second pass found infeasible
    _hold_mbr("plain, second pass totals", ctc, ctc.MbrNbest(totals=rescored.total, scale=0.5), rescored.total, scale=0.5)
    totals = rescored.total.copy()
    totals[0, 1] = -1e30
    totals[2, 0] = -1e30
    res = ctc.MbrNbest(totals=totals, refs=refs)
    _hold_mbr("plain, an infeasible entry", ctc, res, totals, refs=refs)
    assert res.order[0, -1] == 1 and res.order[2, 0] != 0 and res.ref_dist[0, 1] == -1 and np.all(res.dist[0, 1] == -1) and np.all(res.dist[0, :, 1] == -1)


def test_token_lm_mode(ctc, tmp_path):
    from eesen_amd.api import TokenLm
    cfg = lc.CASES["dense_3x12x7_16x6"]
    lens, probs, T, S = dc.build(cfg["case"])
    model = L.model_of(cfg["model"])
    arpa, units = model.write(tmp_path, "first")
    lm = TokenLm(arpa, units, K=model.K)
    dev = _dev(probs)
    hyps, scores = ctc.DecodeParallel(lens, dev, beam=8, max_classes=cfg["C"], nbest=8, lm=lm, lm_weight=cfg["alpha"], insertion_bonus=cfg["beta"],
                                      lm_eos=cfg["eos"])
    scores = scores.copy()
    assert _hold_mbr("token LM", ctc, ctc.MbrNbest(scale=0.8), scores, scale=0.8) > S


@pytest.mark.parametrize("level", [0, 1])
def test_spaced_lexicon_mode(ctc, tmp_path, level):
    from eesen_amd.api import Lexicon
    cfg = xc.CASES["k7_nolm"]
    lens, probs, T, S = xc.build("k7_nolm")
    rl = X.lex_of(cfg["lex"])
    trie = Lexicon(rl.write(tmp_path, "lex"), None, K=rl.K, space=rl.space)
    dev = _dev(probs)
    hyps, scores = ctc.DecodeParallel(lens, dev, beam=8, max_classes=cfg["C"], nbest=8, lexicon=trie, word_bonus=cfg["beta"])
    scores = scores.copy()
    assert any(rl.space in h for hs in hyps for h in hs) and np.any(ctc.words_len > 1)
    del trie                                                  # the call speaks of the decode call's words, not of the lexicon
    stamps = ctc.DecodeStamps(lens, dev)
    refs = [_tokens(ctc, s, 0, level) + [1] for s in range(S)]
    res = ctc.MbrNbest(level=level, refs=refs)
    assert _hold_mbr(f"spaced level {level}", ctc, res, scores, level=level, refs=refs) > S
    other = ctc.MbrNbest(level=1 - level)
    assert not np.array_equal(other.dist, res.dist)           # words and labels are different tokens: the space is a label
    assert _same(stamps, ctc.DecodeStamps(lens, dev), STAMPS)


@pytest.mark.parametrize("level", [0, 1])
def test_unspaced_lexicon_mode(ctc, tmp_path, level):
    from eesen_amd.api import Lexicon
    cfg = wc.CASES["k7_c3"]
    lens, probs, T, S = wc.build("k7_c3")
    rl = W.lex_of(cfg["lex"])
    trie = Lexicon(rl.write(tmp_path, "wlex"), None, K=rl.K, space=None)
    lm = _word_lm(tmp_path, "wwords", rl, trie, W.model_of(cfg["model"]))
    dev = _dev(probs)
    hyps, scores = ctc.DecodeParallel(lens, dev, beam=8, max_classes=cfg["C"], nbest=8, lexicon=trie, lm=lm, lm_weight=cfg["alpha"],
                                      word_bonus=cfg["beta"], lm_eos=cfg["eos"])
    scores = scores.copy()
    assert ctc.word_ends is not None and np.any(ctc.words_len > 1)
    refs = [_tokens(ctc, s, 0, level)[1:] for s in range(S)]
    rescored = ctc.RescoreNbest(lens, dev, lm=lm, lm_weight=1.5, bonus=-0.25)
    res = ctc.MbrNbest(level=level, refs=refs)
    assert _hold_mbr(f"unspaced level {level}", ctc, res, scores, level=level, refs=refs) > S
    _hold_mbr(f"unspaced level {level}, second pass totals", ctc, ctc.MbrNbest(level=level, totals=rescored.total), rescored.total, level=level)
    assert _same(rescored, ctc.RescoreNbest(lens, dev, lm=lm, lm_weight=1.5, bonus=-0.25), RESCORED)


# ------------------------------------------------------------------------------------------------ constructed lists
def test_the_winner_is_not_the_most_probable_entry_and_the_count_is_below_nbest(ctc):
    """tests/mbr_cases.py: all ten labellings of a two-frame utterance in a list of sixteen ranks."""
    lens, probs = M.winner_batch()
    cfg = M.WINNER
    hyps, scores = ctc.DecodeParallel(lens, _dev(probs), beam=cfg["beam"], max_classes=3, nbest=cfg["nbest"])
    scores = scores.copy()
    assert len(hyps[0]) == cfg["count"] < cfg["nbest"] and hyps[0][0] == cfg["map"]
    assert sorted(hyps[0]) == sorted(l for l, _ in M.all_labellings(probs.astype(np.float64)))
    res = ctc.MbrNbest(refs=[cfg["mbr"]])
    assert _hold_mbr("winner", ctc, res, scores, refs=[cfg["mbr"]]) == cfg["count"]
    w = int(res.order[0, 0])
    assert w != 0 and hyps[0][w] == cfg["mbr"] and res.risk[0, w] < res.risk[0, 0] - 0.05 and res.ref_dist[0, w] == 0
    # the ranks beyond the count: last, in rank order, -1 and -1e30
    assert res.order[0, cfg["count"]:].tolist() == list(range(cfg["count"], cfg["nbest"]))
    assert np.all(res.dist[0, cfg["count"]:] == -1) and np.all(res.posterior[0, cfg["count"]:] == Q.NOT_COUNTING)
    # a sharp posterior hands the list back to the most probable entry
    assert ctc.MbrNbest(scale=50.0).order[0, 0] == 0


def test_small_batch_with_an_empty_list_entry_and_an_utterance_without_frames(ctc):
    lens, probs, lab = small_batch()
    dev = _dev(probs)
    hyps, scores = ctc.DecodeParallel(lens, dev, beam=8, max_classes=5, nbest=4)
    scores = scores.copy()
    assert hyps[1][0] == [] and hyps[2] == [[]]
    res = ctc.MbrNbest(refs=[lab, [], [1, 2]])
    assert _hold_mbr("small", ctc, res, scores, refs=[lab, [], [1, 2]]) == 9
    assert res.ref_dist[0, 0] == 0 and res.ref_dist[1, 0] == 0 and res.ref_dist[2].tolist() == [2, -1, -1, -1]
    assert res.posterior[2].tolist() == [1.0] + [Q.NOT_COUNTING] * 3 and res.risk[2, 0] == 0.0
    only = ctc.MbrNbest(refs=[lab, [], [1, 2]], ref_only=True)
    assert only.dist is None and np.array_equal(only.ref_dist, res.ref_dist)


# ------------------------------------------------------------------------------------------------ refusals, guard, times
def test_errors(gpu):
    from eesen_amd.api import Ctc, EesenError
    lens, probs, T, S = dc.build("ties")
    dev = _dev(probs)
    ctc = Ctc()

    def refused(code, fn, *a, **kw):
        with pytest.raises(EesenError) as e:
            fn(*a, **kw)
        assert e.value.code == code, (e.value.code, code)

    refused(-3, ctc.MbrNbest)                                 # no decode call yet
    assert ctc.MbrTimes() == {"build": 0.0, "kernel": 0.0, "host": 0.0}
    ctc.DecodeParallel(lens, dev, beam=4, max_classes=3, nbest=2)
    ok = ctc.MbrNbest()
    for v in (float("nan"), float("inf"), -0.5):
        refused(-1, ctc.MbrNbest, scale=v)
    for v in (-1, 2):
        refused(-1, ctc.MbrNbest, level=v)
    refused(-1, ctc.MbrNbest, refs=[[1] * 8193] + [[]] * (S - 1))
    ctc.hyp_len = ctc.hyp_len[:S - 1]                         # (what the binding sizes S by)
    refused(-3, ctc.MbrNbest)                                 # another S
    ctc.DecodeParallel(lens, dev, beam=4, max_classes=3, nbest=2)
    assert _same(ok, ctc.MbrNbest(), FIELDS)                  # a refused call leaves the state alone


def test_guard_word_set_returns_nan_and_minus_one(gpu):
    from eesen_amd import synth
    from eesen_amd.api import Net, Ctc
    lens, probs, _ = small_batch()
    dev = _dev(probs)
    net = Net.from_layers(synth.make_model(**synth.config("tiny_bi")))
    ctc = Ctc()
    ctc.SetGuard(net)
    ctc.DecodeParallel(lens, dev, beam=4, max_classes=3, nbest=2)
    refs = [[1], [2], []]
    ok = ctc.MbrNbest(refs=refs)
    assert np.all(ok.posterior[:, 0] > 0)
    net._raise_error_word(2)
    bad = ctc.MbrNbest(refs=refs)                             # raised now
    assert np.all(bad.dist == -1) and np.all(bad.ref_dist == -1) and np.all(bad.order == -1)
    assert np.all(np.isnan(bad.posterior)) and np.all(np.isnan(bad.risk))
    ctc.DecodeParallel(lens, dev, beam=4, max_classes=3, nbest=2)          # raised in the decode call
    net._raise_error_word(0)
    bad = ctc.MbrNbest(refs=refs)
    assert np.all(bad.dist == -1) and np.all(bad.order == -1) and np.all(np.isnan(bad.risk))
    ctc.DecodeParallel(lens, dev, beam=4, max_classes=3, nbest=2)
    assert _same(ok, ctc.MbrNbest(refs=refs), FIELDS + ("ref_dist",))
    ctc.SetGuard(None)


def test_times_are_populated_and_summed_under_profiling(gpu):
    from eesen_amd import _lib
    from eesen_amd.api import Ctc
    ctc = Ctc()
    lens, probs, T, S = dc.build("dense_3x12x7")
    dev = _dev(probs)
    ctc.DecodeParallel(lens, dev, beam=8, max_classes=6, nbest=8)
    ctc.MbrNbest()
    one = ctc.MbrTimes()
    assert set(one) == {"build", "kernel", "host"} and all(0 < v < 1 for v in one.values())
    assert ctc.MbrTimes() == one                              # the last call's, until the next
    _lib.check(ctc.lib.eesen_ctc_set_profiling(ctc.h, 2))
    for _ in range(3):
        ctc.MbrNbest()
    three = ctc.MbrTimes()
    assert all(three[k] > 0 for k in three) and ctc.MbrTimes() == {"build": 0.0, "kernel": 0.0, "host": 0.0}          # read and cleared
    _lib.check(ctc.lib.eesen_ctc_set_profiling(ctc.h, 0))
