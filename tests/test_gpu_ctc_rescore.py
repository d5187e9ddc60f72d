"""-m gpu: exact CTC scores and the second pass over N-best lists (csrc/ctc.hip: ctc_score_kernel, the scoring instantiation of
ctc_sweep; csrc/ctc_decode.hip: ctc_hyp_lattices in its scoring form; through api.Ctc.ScoreParallel and api.Ctc.RescoreNbest).

Accuracy: every scored entry is held to the exact fp64 value of tests/ctc_rescore_restatement.py,
    |a - lnp64| / max(1, |lnp64|) < max(2e-6, 3 * floor),   floor = the fp32 restatement's own figure on that entry
-- the project's bar on ln p (LNP_TOL of tests/test_gpu_ctc_per_utterance.py).  The worst figure of every case is printed.
Everything else is exact: bits against EvalParallel where the two closes are the same expression, totals and orders against the stated
fp64 expression on the returned values.
"""
import numpy as np
import pytest

from tests import ctc_beam_restatement as R
from tests import ctc_cases as cc
from tests import ctc_decode_cases as dc
from tests import ctc_lex_cases as xc
from tests import ctc_lex_restatement as X
from tests import ctc_lm_cases as lc
from tests import ctc_lm_restatement as L
from tests import ctc_rescore_cases as Z
from tests import ctc_rescore_restatement as Q
from tests import ctc_words_cases as wc
from tests import ctc_words_restatement as W
from tests.test_gpu_ctc_per_utterance import LNP_TOL
from tests.test_gpu_ctc_stamps import long_batch, small_batch

pytestmark = pytest.mark.gpu

NEG32 = np.float32(-1e30)


@pytest.fixture(scope="module")
def ctc(gpu):
    from eesen_amd.api import Ctc
    return Ctc()


def _dev(m):
    from eesen_amd.api import CuMatrix
    return CuMatrix.from_numpy(m)


def _logs(rows, is_log):
    """(fp32, fp64) log-scores of an utterance's rows as the library sees them."""
    if is_log:
        l32 = np.maximum(np.asarray(rows, np.float32), NEG32)
        return l32, l32.astype(np.float64)
    return R.log32(rows), R.log64(rows)


class Worst:
    """The worst accuracy figure of a case, printed when the case is done."""

    def __init__(self, name):
        self.name, self.fig, self.floor, self.n = name, 0.0, 0.0, 0

    def hold(self, where, got, rows, labels, is_log=False):
        assert Q.LNP_TOL == LNP_TOL
        l32, l64 = _logs(rows, is_log)
        a64 = Q.lnp(l64, labels)
        bar, floor, _ = Q.bar(l32, labels, ref64=a64)
        fig = Q.figure(got, a64)
        print(f"{self.name} {where}: U {len(labels)} n {len(rows)} a {float(got):.9g} lnp64 {a64:.12g} figure {fig:.3g} floor {floor:.3g} bar {bar:.3g}")
        assert a64 > Q.DEAD and np.isfinite(got), (self.name, where, got, a64)
        assert fig < bar, (self.name, where, float(got), a64, fig, floor, bar)
        self.fig, self.floor, self.n = max(self.fig, fig), max(self.floor, floor), self.n + 1
        return a64, bar * max(1.0, abs(a64))

    def done(self):
        print(f"WORST {self.name}: figure {self.fig:.3g} (fp32 restatement {self.floor:.3g}) over {self.n} entries")
        return self.n


def _tokens(ctc, s, i):
    """The LM tokens of returned entry i of utterance s in the mode of the last DecodeParallel."""
    if ctc.words is None:
        return ctc.hyp[s, i, :int(ctc.hyp_len[s, i])].tolist()
    return ctc.words[s, i, :int(ctc.words_len[s, i])].tolist()


def _hold_rescore(name, ctc, lens, m, res, is_log=False, lm=None, lm_weight=1.0, bonus=0.0, eos=False):
    """Every entry of the last DecodeParallel on `ctc` against the statement of INTEGRATION.md "Rescoring"."""
    S, N = ctc.hyp_len.shape
    worst = Worst(name)
    for a in (res.am_score, res.lm_score, res.total, res.order):
        assert a.shape == (S, N), name
    assert res.order.dtype == np.int32 and res.total.dtype == np.float32
    for s in range(S):
        n = int(lens[s])
        rows = np.ascontiguousarray(m[s::S])[:n]
        count = int(np.sum(ctc.hyp_len[s] >= 0))
        totals64, slack = [], 0.0
        for i in range(N):
            if i >= count:
                assert res.am_score[s, i] == NEG32 and res.lm_score[s, i] == NEG32 and res.total[s, i] == NEG32, (name, s, i)
                continue
            labels = ctc.hyp[s, i, :int(ctc.hyp_len[s, i])].tolist()
            a64, bar_abs = worst.hold(f"utterance {s} entry {i}", res.am_score[s, i], rows, labels, is_log)
            tok = _tokens(ctc, s, i)
            if lm is not None:
                g = lm.Score(tok, eos=eos)
            else:
                g = float(ctc.lm_score[s, i]) if ctc.lm_score is not None else 0.0
            assert res.lm_score[s, i] == np.float32(g), (name, s, i, res.lm_score[s, i], g)
            assert res.total[s, i].tobytes() == Q.total_of(res.am_score[s, i], g, len(tok), lm_weight, bonus).tobytes(), (name, s, i)
            totals64.append(a64 + float(np.float32(lm_weight)) * g + float(np.float32(bonus)) * len(tok))
            slack = max(slack, bar_abs)
        ok = [i < count for i in range(N)]
        assert res.order[s].tolist() == Q.order_of(res.total[s].tolist(), ok), (name, s, res.order[s], res.total[s])
        assert sorted(res.order[s].tolist()) == list(range(N))
        if Q.min_gap(totals64) > 2 * slack:
            assert res.order[s, :count].tolist() == Q.order_of(totals64, [True] * count), (name, s)
    return worst.done()


def _same_stamps(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True)
               for f in ("label_start", "label_end", "word_start", "word_end", "word_conf", "path_score"))


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("is_log", [False, True])
def test_small_batch(ctc, is_log):
    """S = 3, nbest = 4, K = 6, ld = 8, T = 40: L' = 65 and 63 in one launch, a one-frame all-blank utterance, one without frames."""
    lens, probs, lab = small_batch()
    m = R.log32(probs) if is_log else probs
    dev = _dev(m)
    assert dev.stride == 8
    hyps, scores = ctc.DecodeParallel(lens, dev, beam=8, max_classes=5, nbest=4, is_log=is_log)
    scores = scores.copy()
    assert hyps[0][0] == lab and len(hyps[0][1]) == 31 and hyps[1][0] == [] and len(hyps[1]) == 4 and hyps[2] == [[]]
    before = ctc.DecodeStamps(lens, dev, is_log=is_log)
    res = ctc.RescoreNbest(lens, dev, is_log=is_log)
    assert _hold_rescore(f"small is_log {is_log}", ctc, lens, m, res, is_log) == 9
    # no LM anywhere: the total is the exact score
    assert np.array_equal(res.total, res.am_score) and np.all(res.lm_score[res.am_score > -1e29] == 0)
    # the empty labelling: the blank's scores, and 0 over no frames; ranks beyond the count
    l32 = _logs(np.ascontiguousarray(m[1::3])[:1], is_log)[0]
    assert not is_log or res.am_score[1, 0] == l32[0, 0]
    assert res.am_score[2, 0] == 0 and np.all(res.am_score[2, 1:] == NEG32)
    assert res.order[2].tolist() == [0, 1, 2, 3]
    # the exact score is never below the beam's (plain mode: the beam's score is a part of the same sum)
    for s in range(3):
        for i in range(len(hyps[s])):
            assert float(res.am_score[s, i]) >= float(scores[s, i]) - R.bar_of(float(scores[s, i]), int(lens[s])), (s, i)
    # the same entries through the host-label call: the same lattices, the same bits
    alone = ctc.ScoreParallel(lens, dev, hyps, is_log=is_log)
    for s in range(3):
        assert alone[s].tobytes() == res.am_score[s, :len(hyps[s])].tobytes(), s
    # nothing the decode call left has moved
    assert _same_stamps(before, ctc.DecodeStamps(lens, dev, is_log=is_log))
    again = ctc.RescoreNbest(lens, dev, is_log=is_log)
    assert all(np.array_equal(getattr(again, f), getattr(res, f)) for f in ("am_score", "lm_score", "total", "order"))


def test_a_lattice_of_more_than_one_wave(ctc):
    lens, probs, labs = long_batch()
    dev = _dev(probs)
    hyps, scores = ctc.DecodeParallel(lens, dev, beam=4, max_classes=3, nbest=2)
    scores = scores.copy()
    assert hyps[0][0] == labs[0] and len(hyps[0][0]) >= 128 and hyps[1][0] == labs[1]
    res = ctc.RescoreNbest(lens, dev)
    assert _hold_rescore("long", ctc, lens, probs, res) == 4
    for s in range(2):
        for i in range(2):
            assert float(res.am_score[s, i]) >= float(scores[s, i]) - R.bar_of(float(scores[s, i]), int(lens[s])), (s, i)


@pytest.mark.parametrize("T,K,U,positions", [(1300, 30, 600, 2048), (2900, 8, 2047, 4096)])
def test_long_labellings_through_score_parallel(ctc, T, K, U, positions):
    lens, probs, labels = cc.long_case(1, T, K, U, 9600 + U)
    lab = labels[0].tolist()
    assert len(lab) == U and positions // 2 < 2 * U + 1 <= positions and U + cc.num_repeats(lab) < T
    dev = _dev(probs)
    short = lab[:5]
    got = ctc.ScoreParallel(lens, dev, [[lab, short, []]])[0]
    worst = Worst(f"U{U}")
    for i, l in enumerate((lab, short, [])):
        worst.hold(f"entry {i}", got[i], probs, l)
    worst.done()
    # alone, in a narrower row, the short entry has the bits it has beside the long one
    assert ctc.ScoreParallel(lens, dev, [[short]])[0].tobytes() == got[1:2].tobytes()


def test_more_than_2047_labels(ctc):
    from eesen_amd.api import EesenError
    lens, probs, _ = small_batch()
    dev = _dev(probs)
    with pytest.raises(EesenError) as e:
        ctc.ScoreParallel(lens, dev, [[[1, 2] * 1024], [], []])
    assert e.value.code == -1
    got = ctc.ScoreParallel(lens, dev, [[([1, 2] * 1024)[:2047]], [], []])      # 2047: a lattice, and no path on 40 frames
    assert got[0][0] == NEG32 and got[1].size == 0 and got[2].size == 0


def test_decode_resident_entry_of_more_than_2047_labels(ctc):
    """The infeasible convention, as in DecodeStamps, beside an ordinary utterance."""
    from tests.test_gpu_ctc_stamps import _batch, _frames_of
    T, U = 2100, 2050
    lab = [1 + (u & 1) for u in range(U)]
    lens, probs = _batch([T, 30], [_frames_of(lab, T, top=0.99999), _frames_of([3, 3, 4], 30)], T)
    dev = _dev(probs)
    hyps, _ = ctc.DecodeParallel(lens, dev, beam=2, max_classes=2, nbest=1)
    assert hyps[0][0] == lab and hyps[1][0] == [3, 3, 4]
    res = ctc.RescoreNbest(lens, dev)
    assert res.am_score[0, 0] == NEG32 and res.total[0, 0] == NEG32 and res.lm_score[0, 0] == NEG32 and res.order[0, 0] == 0
    Worst("beside too long").hold("utterance 1", res.am_score[1, 0], np.ascontiguousarray(probs[1::2])[:30], [3, 3, 4])


# ------------------------------------------------------------------------------------------------ infeasible and clamped
def test_infeasible_and_clamped_scores(ctc):
    K = 6
    rng = np.random.default_rng(9701)
    probs = cc.softmax32(rng.standard_normal((10 * 2, K)).astype(np.float32))
    lens = np.array([10, 4], np.int32)
    dev = _dev(probs)
    hyps = [[[1, 2, 3], [1, 1, 1, 1, 1, 1]], [[2, 2, 3], [2, 3], [4, 4, 4]]]          # 6 + 5 > 10; 3 + 1 = 4; 3 + 2 > 4
    got = ctc.ScoreParallel(lens, dev, hyps)
    assert got[0][1] == NEG32 and got[1][2] == NEG32
    worst = Worst("feasible beside infeasible")
    worst.hold("0/0", got[0][0], probs[0::2][:10], hyps[0][0])
    worst.hold("1/0", got[1][0], probs[1::2][:4], hyps[1][0])              # n = U + repeats exactly: no final blank
    worst.hold("1/1", got[1][1], probs[1::2][:4], hyps[1][1])
    # log-scores with -1e30 (and below, and -inf) on every path: one frame is closed to every class of the lattice
    logs = R.log32(probs).copy()
    logs[3 * 2 + 0, :] = [-1e30, -1e30, -3e30, -np.inf, -0.5, -0.25]       # classes 0 .. 3 of frame 3 of utterance 0
    dlog = _dev(logs)
    got = ctc.ScoreParallel(lens, dlog, [[[1, 2, 3], [4, 5]], [[2, 3]]], is_log=True)
    assert got[0][0] == NEG32
    worst.hold("classes 4 and 5 stay open", got[0][1], np.maximum(logs[0::2][:10], NEG32), [4, 5], is_log=True)
    worst.hold("the other utterance", got[1][0], logs[1::2][:4], [2, 3], is_log=True)
    # posteriors with exact zeros: the logarithm's -inf is clamped, never NaN
    z = probs.copy()
    z[5 * 2 + 0, :4] = 0
    got = ctc.ScoreParallel(lens, _dev(z), [[[1, 2, 3], [4, 5]], []])
    assert got[0][0] == NEG32 and np.isfinite(got[0][1]) and got[0][1] > -1e29
    worst.hold("zeros", got[0][1], z[0::2][:10], [4, 5])
    worst.done()


# ------------------------------------------------------------------------------------------------ where eval_parallel's close fails
@pytest.mark.parametrize("name", ["no_final_blank", "no_final_blank_h12", "last_frame_spike"])
def test_quirk_cases(ctc, name):
    lens, probs, labels, T, S = Z.quirk_cases()[name]
    lab = labels[0].tolist()
    dev = _dev(probs)
    got = ctc.ScoreParallel(lens, dev, [[lab]])[0][0]
    worst = Worst(name)
    a64, _ = worst.hold("entry", got, probs, lab)
    worst.done()
    ctc.EvalParallel(lens, dev, [lab])
    pzx = float(ctc.pzx[0])
    print(f"{name}: EvalParallel ln p {pzx:.9g}")
    assert pzx < -1e29 or abs(pzx - a64) > 1.0, (name, pzx, a64)


# ------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("name", sorted(Z.BITWISE))
def test_bits_of_the_training_sweep(gpu, name, monkeypatch):
    from eesen_amd.api import Ctc
    lens, probs, labels, T, S = Z.bitwise_case(name)
    labs = [l.tolist() for l in labels]
    dev = _dev(probs)
    ctc = Ctc()
    batch = np.concatenate(ctc.ScoreParallel(lens, dev, [[l] for l in labs]))
    worst = Worst(name)
    for s in range(S):
        n = int(lens[s])
        rows = np.ascontiguousarray(probs[s::S])
        one = _dev(rows)
        ctc.EvalParallel([n], one, [labs[s]])
        assert ctc.pzx[0].tobytes() == batch[s].tobytes(), (name, s, ctc.pzx[0], batch[s])          # the training sweep's bits
        assert ctc.ScoreParallel([n], one, [[labs[s]]])[0].tobytes() == batch[s:s + 1].tobytes(), (name, s)      # alone as in the batch
        worst.hold(f"utterance {s}", batch[s], rows[:n], labs[s])
    worst.done()
    for w in Z.WAVES[Z.BITWISE[name]["positions"]]:
        monkeypatch.setenv("EESEN_CTC_WAVES", str(w))
        other = Ctc()
        monkeypatch.delenv("EESEN_CTC_WAVES")
        got = np.concatenate(other.ScoreParallel(lens, dev, [[l] for l in labs]))
        assert got.tobytes() == batch.tobytes(), (name, w)


# ------------------------------------------------------------------------------------------------ the second pass, four modes
def test_reorder_case_and_stamps(ctc):
    lens, probs, S = Z.reorder_batch()
    dev = _dev(probs)
    cfg = Z.REORDER
    hyps, scores = ctc.DecodeParallel(lens, dev, beam=cfg["B"], max_classes=cfg["C"], nbest=cfg["N"])
    before = ctc.DecodeStamps(lens, dev)
    res = ctc.RescoreNbest(lens, dev)
    _hold_rescore("reorder", ctc, lens, probs, res)
    for s in range(S):
        f = Z.reorder_facts(Z.utt(probs, s, S, int(lens[s])))
        assert hyps[s] == f["labels"], s
        assert res.order[s, 0] != 0 and res.order[s].tolist() == f["order64"], (s, res.order[s], f["order64"])
    assert _same_stamps(before, ctc.DecodeStamps(lens, dev))


def test_plain_mode(ctc, tmp_path):
    from eesen_amd.api import TokenLm
    lens, probs, T, S = dc.build("dense_3x12x7")
    dev = _dev(probs)
    hyps, scores = ctc.DecodeParallel(lens, dev, beam=4, max_classes=6, nbest=4)
    scores = scores.copy()
    res = ctc.RescoreNbest(lens, dev, lm_weight=0.7, bonus=0.4)          # no LM at all: g = 0, the bonus counts labels
    assert _hold_rescore("plain", ctc, lens, probs, res, lm_weight=0.7, bonus=0.4) == 12
    for s in range(S):
        for i in range(4):
            assert float(res.am_score[s, i]) >= float(scores[s, i]) - R.bar_of(float(scores[s, i]), int(lens[s])), (s, i)
    model = L.model_of("k7_o2")
    arpa, units = model.write(tmp_path, "second")
    lm = TokenLm(arpa, units, K=model.K)
    res = ctc.RescoreNbest(lens, dev, lm=lm, lm_weight=0.5, bonus=1.0, lm_eos=True)
    assert _hold_rescore("plain + LM", ctc, lens, probs, res, lm=lm, lm_weight=0.5, bonus=1.0, eos=True) == 12


def test_token_lm_mode(ctc, tmp_path):
    from eesen_amd.api import TokenLm
    cfg = lc.CASES["dense_3x12x7_16x6"]
    lens, probs, T, S = dc.build(cfg["case"])
    model = L.model_of(cfg["model"])
    arpa, units = model.write(tmp_path, "first")
    first = TokenLm(arpa, units, K=model.K)
    dev = _dev(probs)
    ctc.DecodeParallel(lens, dev, beam=4, max_classes=cfg["C"], nbest=4, lm=first, lm_weight=cfg["alpha"], insertion_bonus=cfg["beta"],
                       lm_eos=cfg["eos"])
    before = ctc.DecodeStamps(lens, dev)
    res = ctc.RescoreNbest(lens, dev, lm_weight=cfg["alpha"], bonus=cfg["beta"])          # the first pass's LM sums
    assert _hold_rescore("token LM, first pass's sums", ctc, lens, probs, res, lm_weight=cfg["alpha"], bonus=cfg["beta"]) == 12
    second = L.model_of("k7_o2")
    arpa, units = second.write(tmp_path, "second")
    lm = TokenLm(arpa, units, K=second.K)
    res = ctc.RescoreNbest(lens, dev, lm=lm, lm_weight=1.25, bonus=-0.5, lm_eos=True)
    assert _hold_rescore("token LM + second LM", ctc, lens, probs, res, lm=lm, lm_weight=1.25, bonus=-0.5, eos=True) == 12
    assert _same_stamps(before, ctc.DecodeStamps(lens, dev))


def _word_lm(d, tag, rl, trie, model):
    from eesen_amd.api import TokenLm
    table = str(d / (tag + ".words.txt"))
    trie.WriteWords(table)
    by_id = {w: n for n, w in rl.ids.items()}
    arpa, _ = L.Model(model.K, model.order, model.grams, [None] + [by_id[w] for w in range(1, rl.V + 1)]).write(d, tag)
    return TokenLm(arpa, table, K=rl.V + 1)


def test_spaced_lexicon_mode(ctc, tmp_path):
    from eesen_amd.api import Lexicon
    cfg = xc.CASES["k7_nolm"]
    lens, probs, T, S = xc.build("k7_nolm")
    rl = X.lex_of(cfg["lex"])
    trie = Lexicon(rl.write(tmp_path, "lex"), None, K=rl.K, space=rl.space)
    lm = _word_lm(tmp_path, "words", rl, trie, X.model_of("v12_o3_unk"))
    dev = _dev(probs)
    hyps, _ = ctc.DecodeParallel(lens, dev, beam=4, max_classes=cfg["C"], nbest=4, lexicon=trie, word_bonus=cfg["beta"])
    assert any(rl.space in h for hs in hyps for h in hs)
    before = ctc.DecodeStamps(lens, dev)
    del trie                                                  # the call speaks of the decode call's words, not of the lexicon
    res = ctc.RescoreNbest(lens, dev, bonus=cfg["beta"])      # a lexicon without an LM: the sums are 0, the bonus counts words
    assert _hold_rescore("spaced", ctc, lens, probs, res, bonus=cfg["beta"]) > 0
    res = ctc.RescoreNbest(lens, dev, lm=lm, lm_weight=0.8, bonus=0.2, lm_eos=True)
    assert _hold_rescore("spaced + word LM", ctc, lens, probs, res, lm=lm, lm_weight=0.8, bonus=0.2, eos=True) > 0
    assert _same_stamps(before, ctc.DecodeStamps(lens, dev))


def test_unspaced_lexicon_mode(ctc, tmp_path):
    from eesen_amd.api import Lexicon
    cfg = wc.CASES["k7_c3"]
    lens, probs, T, S = wc.build("k7_c3")
    rl = W.lex_of(cfg["lex"])
    trie = Lexicon(rl.write(tmp_path, "wlex"), None, K=rl.K, space=None)
    lm = _word_lm(tmp_path, "wwords", rl, trie, W.model_of(cfg["model"]))
    dev = _dev(probs)
    ctc.DecodeParallel(lens, dev, beam=4, max_classes=cfg["C"], nbest=4, lexicon=trie, lm=lm, lm_weight=cfg["alpha"], word_bonus=cfg["beta"],
                       lm_eos=cfg["eos"])
    assert ctc.word_ends is not None and np.any(ctc.words_len > 1)
    before = ctc.DecodeStamps(lens, dev)
    res = ctc.RescoreNbest(lens, dev, lm_weight=cfg["alpha"], bonus=cfg["beta"])
    assert _hold_rescore("unspaced, first pass's sums", ctc, lens, probs, res, lm_weight=cfg["alpha"], bonus=cfg["beta"]) > 0
    res = ctc.RescoreNbest(lens, dev, lm=lm, lm_weight=1.5, bonus=-0.25, lm_eos=False)
    assert _hold_rescore("unspaced + word LM", ctc, lens, probs, res, lm=lm, lm_weight=1.5, bonus=-0.25, eos=False) > 0
    assert _same_stamps(before, ctc.DecodeStamps(lens, dev))


# ------------------------------------------------------------------------------------------------ refusals, guard, times
def test_errors(gpu, tmp_path):
    from eesen_amd.api import Ctc, CuMatrix, EesenError, TokenLm
    lens, probs, T, S = dc.build("ties")                      # K = 12
    dev = _dev(probs)
    ctc = Ctc()

    def refused(code, fn, *a, **kw):
        with pytest.raises(EesenError) as e:
            fn(*a, **kw)
        assert e.value.code == code, (e.value.code, code)

    refused(-3, ctc.RescoreNbest, lens, dev)                  # no decode call yet
    ctc.DecodeParallel(lens, dev, beam=4, max_classes=3, nbest=2)
    ok = ctc.RescoreNbest(lens, dev)
    refused(-3, ctc.RescoreNbest, lens[:2], _dev(probs[:T * 2]))                          # another S
    refused(-3, ctc.RescoreNbest, lens, _dev(np.concatenate([probs, probs[:S]])))         # other rows
    other = lens.copy()
    other[0] -= 1
    refused(-3, ctc.RescoreNbest, other, dev)
    for v in (float("nan"), float("inf")):
        refused(-1, ctc.RescoreNbest, lens, dev, lm_weight=v)
        refused(-1, ctc.RescoreNbest, lens, dev, bonus=v)
    narrow = CuMatrix.view(dev.ptr, dev.rows, dev.cols, dev.cols - 1, keepalive=dev)     # ld < K
    refused(-1, ctc.RescoreNbest, lens, narrow)
    refused(-1, ctc.ScoreParallel, lens, narrow, [[[1]]] * S)
    noeos = L.model_of("k12_o3_noeos")
    arpa, units = noeos.write(tmp_path, "noeos")
    lm = TokenLm(arpa, units, K=noeos.K)
    refused(-1, ctc.RescoreNbest, lens, dev, lm=lm, lm_eos=True)                          # no </s> in the model
    assert ctc.RescoreNbest(lens, dev, lm=lm).am_score.tobytes() == ok.am_score.tobytes()
    k7 = L.model_of("k7_o2")
    arpa, units = k7.write(tmp_path, "k7")
    refused(-1, ctc.RescoreNbest, lens, dev, lm=TokenLm(arpa, units, K=k7.K))            # an LM over another class count
    for bad in (0, 12, -1):
        refused(-1, ctc.ScoreParallel, lens, dev, [[[1, bad]]] + [[]] * (S - 1))
    refused(-1, ctc.ScoreParallel, lens, dev, [[[1]]] * (S - 1))                          # one list per utterance
    again = ctc.RescoreNbest(lens, dev)                       # a refused call leaves the state alone
    assert all(np.array_equal(getattr(again, f), getattr(ok, f)) for f in ("am_score", "lm_score", "total", "order"))


def test_score_parallel_leaves_the_training_state_alone(gpu):
    from eesen_amd.api import Ctc
    lens, probs, labels, T, S = cc.build("dense_3x12x7")
    dev = _dev(probs)
    ctc = Ctc()
    ctc.EvalParallel(lens, dev, [l.tolist() for l in labels])
    ctc._rows = T * S                                         # (what the parity accessor sizes its arrays by)
    a0, b0 = ctc.alpha_beta()
    stats = ctc.stats()
    ctc.ScoreParallel(lens, dev, [[[1, 2, 3, 1, 2, 3, 1]], [[2], []], [[3, 3]]])
    a1, b1 = ctc.alpha_beta()
    assert np.array_equal(a0, a1) and np.array_equal(b0, b1) and ctc.stats() == stats


def test_guard_word_set_returns_nan_and_minus_one(gpu):
    from eesen_amd import synth
    from eesen_amd.api import Net, Ctc
    lens, probs, _ = small_batch()
    dev = _dev(probs)
    net = Net.from_layers(synth.make_model(**synth.config("tiny_bi")))
    ctc = Ctc()
    ctc.SetGuard(net)
    hyps, _ = ctc.DecodeParallel(lens, dev, beam=4, max_classes=3, nbest=2)
    ok = ctc.RescoreNbest(lens, dev)
    assert np.all(np.isfinite(ok.am_score[:, 0]))
    net._raise_error_word(2)
    bad = ctc.RescoreNbest(lens, dev)
    assert np.all(np.isnan(bad.am_score)) and np.all(np.isnan(bad.lm_score)) and np.all(np.isnan(bad.total)) and np.all(bad.order == -1)
    assert all(np.all(np.isnan(a)) for a in ctc.ScoreParallel(lens, dev, hyps))
    net._raise_error_word(0)
    again = ctc.RescoreNbest(lens, dev)
    assert np.array_equal(again.total, ok.total) and np.array_equal(again.order, ok.order)
    ctc.SetGuard(None)


def test_times_are_populated(ctc):
    lens, probs, _ = small_batch()
    dev = _dev(probs)
    ctc.DecodeParallel(lens, dev, beam=4, max_classes=3, nbest=2)
    ctc.RescoreNbest(lens, dev)
    t = ctc.RescoreTimes()
    assert set(t) == {"lattices", "sweep", "host"} and all(0 <= v < 1 for v in t.values()) and t["sweep"] > 0
