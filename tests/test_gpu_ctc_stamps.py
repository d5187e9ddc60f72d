"""-m gpu: time stamps and confidences of decoded hypotheses (csrc/ctc_decode.hip: ctc_hyp_lattices_kernel; csrc/ctc.hip:
ctc_best_path_kernel over lattices-per-utterance, ctc_traceback_kernel, ctc_stamp_kernel; through api.Ctc.DecodeStamps).

The yardstick is the existing device path, which tests/test_gpu_ctc_align.py pins to the restatement: every returned entry with at
least one label is aligned by Ctc.AlignParallel on its own, as an S = 1 call on its utterance's rows.  Both run the same kernels with
the same addition order, so there is no tolerance: the label intervals are those of AlignParallel's `pos` (derived by
tests/ctc_stamps_restatement.py) and path_score is AlignParallel's score bit for bit.  The restatement's own fp32 path
(tests/ctc_align_restatement.py) must collapse to the entry's labels, as must the device's.

Word intervals and confidences are held against the restatement over the returned labels, words and totals.  wconf is the fp32
rounding of an fp64 value in [0, 1]: 1e-6 absolute.  path_score <= score holds in the plain mode only (the score is a log-sum over
paths there; with an LM or a bonus it carries terms the path score does not), within tests/ctc_beam_restatement.bar_of -- the
fp32 log-add slack tests/test_gpu_ctc_decode.py allows against the exact ln p.
"""
import numpy as np
import pytest

from tests import ctc_align_restatement as A
from tests import ctc_beam_restatement as R
from tests import ctc_decode_cases as dc
from tests import ctc_lex_cases as xc
from tests import ctc_lex_restatement as X
from tests import ctc_lm_cases as lc
from tests import ctc_lm_restatement as L
from tests import ctc_stamps_restatement as Z
from tests import ctc_words_cases as wc
from tests import ctc_words_restatement as W

pytestmark = pytest.mark.gpu

CONF_ABS = 1e-6
K6 = 6


@pytest.fixture(scope="module")
def ctc(gpu):
    from eesen_amd.api import Ctc
    return Ctc()


def _spiked(plan, K, top=0.9):
    """[n x K] float32 probabilities: frame t gives plan[t] = (class, p) that p and shares the rest evenly."""
    out = np.empty((len(plan), K), np.float32)
    for t, (c, p) in enumerate(plan):
        out[t] = (1.0 - p) / (K - 1)
        out[t, c] = p
    return out


def _frames_of(labels, n, weak=None, top=0.9):
    """A frame plan of n frames that spells `labels`: one frame per label, a blank between adjacent repeats, the rest blanks spread
    at the end and the front (top: the planned class's probability; many blank frames need it high, or a label inserted at any
    one of them outweighs the plan).  weak: index of a label whose frame is 0.5 label / 0.45 blank."""
    plan = []
    for u, c in enumerate(labels):
        if u and labels[u - 1] == c:
            plan.append((0, top))
        plan.append((int(c), 0.5 if u == weak else top))
    assert len(plan) <= n, (len(plan), n)
    pad = n - len(plan)
    plan = [(0, top)] * (pad // 2) + plan + [(0, top)] * (pad - pad // 2)
    probs = _spiked(plan, K6)
    if weak is not None:
        t = [i for i, (c, p) in enumerate(plan) if p == 0.5][0]
        probs[t] = 0.05 / (K6 - 2)
        probs[t, plan[t][0]], probs[t, 0] = 0.5, 0.45
    return probs


def _batch(lens, per_utt, T):
    S = len(lens)
    probs = np.full((T * S, K6), 1.0 / K6, np.float32)
    for s, p in enumerate(per_utt):
        if p is not None:
            probs[s:len(p) * S:S] = p
    return np.asarray(lens, np.int32), probs


def small_batch():
    """S = 3, nbest = 4, K = 6 (ld = 8), T = 40: a 32-label utterance with an adjacent repeat and one weak label (its 31-label
    neighbour is in the list: L' = 65 and 63, Lpad crosses 64), an all-blank utterance of one frame, an utterance without frames."""
    rng = np.random.default_rng(7201)
    lab = [1, 1]
    while len(lab) < 32:
        c = int(rng.integers(1, K6))
        if c != lab[-1] and (len(lab) != 21 or c != lab[19]):     # no other repeat; dropping label 20 must not merge 19 and 21
            lab.append(c)
    blank = _spiked([(0, 0.9)], K6)
    lens, probs = _batch([40, 1, 0], [_frames_of(lab, 40, weak=20), blank, None], 40)
    return lens, probs, lab


def long_batch():
    """S = 2, nbest = 2, T = 300: a 130-label utterance (L' = 261 > 256: the sweep takes more than one wave) beside a short one."""
    rng = np.random.default_rng(7202)
    labs = []
    for U in (130, 20):
        lab = [int(rng.integers(1, K6))]
        while len(lab) < U:
            c = int(rng.integers(1, K6))
            if c != lab[-1] or rng.random() < 0.3:
                lab.append(c)
        labs.append(lab)
    lens, probs = _batch([300, 200], [_frames_of(labs[0], 300, top=0.9999), _frames_of(labs[1], 200, top=0.9999)], 300)
    return lens, probs, labs


def _dev(m):
    from eesen_amd.api import CuMatrix
    return CuMatrix.from_numpy(m)


def _words_of(ctc, s, i, space):
    """[(id, a, b)] of returned entry i of utterance s in the mode of the last DecodeParallel."""
    U = int(ctc.hyp_len[s, i])
    labels = ctc.hyp[s, i, :U].tolist()
    if ctc.words is None:
        return Z.words_plain(labels)
    nw = int(ctc.words_len[s, i])
    ids = ctc.words[s, i, :nw].tolist()
    if ctc.word_ends is None:
        return Z.words_spaced(labels, space, ids)
    return Z.words_unspaced(ids, ctc.word_ends[s, i, :nw].tolist())


def _hold(name, ctc, lens, m, dev, st, scores, is_log, conf_scale=1.0, space=None, plain=False):
    """Every entry of the last DecodeParallel on `ctc` (scores [S, N]) against AlignParallel and the restatement."""
    S, N = scores.shape
    T = m.shape[0] // S
    hyp, hlen = ctc.hyp.copy(), ctc.hyp_len.copy()
    words = [[_words_of(ctc, s, i, space) if hlen[s, i] >= 0 else None for i in range(N)] for s in range(S)]
    for a in (st.label_start, st.label_end, st.word_start, st.word_end, st.word_conf):
        assert a.shape == (S, N, T), name
    assert st.path_score.shape == (S, N)
    aligned = 0
    for s in range(S):
        n = int(lens[s])
        rows = np.ascontiguousarray(m[s::S])
        count = int(np.sum(hlen[s] >= 0))
        entries = []
        for i in range(N):
            where = f"{name} utterance {s} (n {n}) entry {i}"
            ls, le, ws, we, wconf = (a[s, i] for a in (st.label_start, st.label_end, st.word_start, st.word_end, st.word_conf))
            if i >= count:
                assert np.all(ls == -1) and np.all(le == -1) and np.all(ws == -1) and np.all(we == -1), where
                assert st.path_score[s, i] == np.float32(-1e30) and np.all(wconf == np.float32(-1e30)), where
                continue
            U = int(hlen[s, i])
            labels = hyp[s, i, :U].tolist()
            if U == 0:       # the empty hypothesis: no lattice, no words, path score 0
                assert st.path_score[s, i] == 0 and np.all(ls == -1) and np.all(le == -1) and np.all(ws == -1) and np.all(we == -1), where
                assert np.all(wconf == np.float32(-1e30)), where
                entries.append([])
                continue
            _, pos, score = ctc.AlignParallel([n], _dev(rows), [labels], is_log=is_log)
            aligned += 1
            pos = pos[:n, 0]
            assert A.path_is_valid(pos, labels, n), where
            want_ls, want_le = Z.label_intervals(pos, U, T)
            print(f"{where}: U {U} path_score {st.path_score[s, i]:.9g} align {score[0]:.9g} score {scores[s, i]:.9g}")
            assert np.array_equal(ls, want_ls) and np.array_equal(le, want_le), where
            assert st.path_score[s, i].tobytes() == score[0].tobytes(), (where, st.path_score[s, i], score[0])
            assert np.all(ls[:U] >= 0) and np.all(le[:U] > ls[:U]) and np.all(ls[1:U] >= le[:U - 1]) and le[U - 1] <= n, where
            pos32, _, _ = A.viterbi(rows[:n] if is_log else A.log32(rows[:n]), labels, np.float32)
            assert A.path_is_valid(pos32, labels, n), where
            if plain:
                bar = R.bar_of(float(scores[s, i]), n)
                assert float(st.path_score[s, i]) <= float(scores[s, i]) + bar, (where, st.path_score[s, i], scores[s, i], bar)
            iv = Z.word_intervals(words[s][i], ls, le)
            nw = len(iv)
            assert ws[:nw].tolist() == [b for _, b, _ in iv] and we[:nw].tolist() == [e for _, _, e in iv], where
            assert np.all(ws[nw:] == -1) and np.all(we[nw:] == -1) and np.all(wconf[nw:] == np.float32(-1e30)), where
            if space is not None:    # no word owns a frame of a space label
                for u in np.flatnonzero(np.asarray(labels) == space):
                    assert all(e <= ls[u] or b >= le[u] for _, b, e in iv), (where, u)
            entries.append(iv)
        conf = Z.confidence(scores[s, :count].astype(np.float64), entries, conf_scale)
        for i, row in enumerate(conf):
            got = st.word_conf[s, i, :len(row)]
            assert np.all(np.abs(got.astype(np.float64) - np.asarray(row)) <= CONF_ABS), (name, s, i, got, row)
            if count == 1:
                assert np.all(got == 1.0), (name, s, i)
    return aligned


def _same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("label_start", "label_end", "word_start", "word_end", "word_conf", "path_score"))


@pytest.mark.parametrize("is_log", [False, True])
def test_small_batch_meets_the_cases(ctc, is_log):
    lens, probs, lab = small_batch()
    m = A.log32(probs) if is_log else probs
    dev = _dev(m)
    assert dev.stride == 8
    hyps, scores = ctc.DecodeParallel(lens, dev, beam=8, max_classes=5, nbest=4, is_log=is_log)
    scores = scores.copy()
    # the cases the batch was built for
    assert hyps[0][0] == lab and len(hyps[0][1]) == 31, [len(h) for h in hyps[0]]      # L' = 65 and 63 in one call
    assert hyps[1][0] == [] and len(hyps[1]) == 4 and hyps[2] == [[]] and scores[2, 0] == 0
    st = ctc.DecodeStamps(lens, dev, is_log=is_log, conf_scale=0.7)
    assert _hold(f"small is_log {is_log}", ctc, lens, m, dev, st, scores, is_log, conf_scale=0.7, plain=True) >= 7
    # the adjacent repeat: label 1 starts behind label 0's end, with the blank between them in neither
    assert st.label_start[0, 0, 1] > st.label_end[0, 0, 0]
    # the state the call reads survives align calls on the same object, and a second call is the first
    assert _same(st, ctc.DecodeStamps(lens, dev, is_log=is_log, conf_scale=0.7))
    # 12 lattices in groups of 5: 5 divides neither 12 nor nbest
    ctc.SetStampGroup(5)
    try:
        assert _same(st, ctc.DecodeStamps(lens, dev, is_log=is_log, conf_scale=0.7))
    finally:
        ctc.SetStampGroup(0)
    one = ctc.DecodeStamps(lens, dev, is_log=is_log, conf_scale=0.0)      # uniform P: the 1-best's confidences are counts / entries
    assert np.array_equal(one.label_start, st.label_start) and np.array_equal(one.path_score, st.path_score)


def test_a_lattice_of_more_than_one_wave(ctc):
    lens, probs, labs = long_batch()
    dev = _dev(probs)
    hyps, scores = ctc.DecodeParallel(lens, dev, beam=4, max_classes=3, nbest=2)
    scores = scores.copy()
    assert hyps[0][0] == labs[0] and len(hyps[0][0]) >= 128 and hyps[1][0] == labs[1]
    st = ctc.DecodeStamps(lens, dev)
    assert _hold("long", ctc, lens, probs, dev, st, scores, False, plain=True) == 4
    ctc.SetStampGroup(3)
    try:
        assert _same(st, ctc.DecodeStamps(lens, dev))
    finally:
        ctc.SetStampGroup(0)


def test_a_labelling_too_long_for_a_lattice(ctc):
    """More than 2047 labels (L' > 4096): the infeasible convention -- path score -1e30, -1 stamps, words without an interval and
    with confidence 0 -- beside an ordinary utterance that is stamped as ever."""
    T, U = 2100, 2050
    lab = [1 + (u & 1) for u in range(U)]
    lens, probs = _batch([T, 30], [_frames_of(lab, T, top=0.99999), _frames_of([3, 3, 4], 30)], T)
    dev = _dev(probs)
    hyps, scores = ctc.DecodeParallel(lens, dev, beam=2, max_classes=2, nbest=1)
    assert hyps[0][0] == lab and hyps[1][0] == [3, 3, 4]
    st = ctc.DecodeStamps(lens, dev)
    assert st.path_score[0, 0] == np.float32(-1e30)
    for a in (st.label_start, st.label_end, st.word_start, st.word_end):
        assert np.all(a[0, 0] == -1)
    assert np.all(st.word_conf[0, 0, :U] == 0) and np.all(st.word_conf[0, 0, U:] == np.float32(-1e30))
    _, pos, score = ctc.AlignParallel([30], _dev(np.ascontiguousarray(probs[1::2])), [[3, 3, 4]])
    want_ls, want_le = Z.label_intervals(pos[:30, 0], 3, T)
    assert np.array_equal(st.label_start[1, 0], want_ls) and np.array_equal(st.label_end[1, 0], want_le)
    assert st.path_score[1, 0].tobytes() == score[0].tobytes() and np.all(st.word_conf[1, 0, :3] == 1.0)


def test_nbest_1_is_certain(ctc):
    lens, probs, lab = small_batch()
    dev = _dev(probs)
    hyps, scores = ctc.DecodeParallel(lens, dev, beam=8, max_classes=5, nbest=1)
    st = ctc.DecodeStamps(lens, dev, conf_scale=2.0)
    assert np.all(st.word_conf[0, 0, :32] == 1.0) and np.all(st.word_conf[0, 0, 32:] == np.float32(-1e30))
    _hold("nbest 1", ctc, lens, probs, dev, st, scores.copy(), False, conf_scale=2.0, plain=True)


def test_token_lm_mode(ctc, tmp_path):
    from eesen_amd.api import TokenLm
    cfg = lc.CASES["dense_3x12x7_16x6"]
    lens, probs, T, S = dc.build(cfg["case"])
    model = L.model_of(cfg["model"])
    arpa, units = model.write(tmp_path, "lm")
    lm = TokenLm(arpa, units, K=model.K)
    dev = _dev(probs)
    hyps, scores = ctc.DecodeParallel(lens, dev, beam=cfg["B"], max_classes=cfg["C"], nbest=4, lm=lm, lm_weight=cfg["alpha"],
                                      insertion_bonus=cfg["beta"], lm_eos=cfg["eos"])
    st = ctc.DecodeStamps(lens, dev)
    assert _hold("token lm", ctc, lens, probs, dev, st, scores.copy(), False) > 0


def test_spaced_lexicon_mode(ctc, tmp_path):
    from eesen_amd.api import Lexicon
    cfg = xc.CASES["k7_nolm"]
    lens, probs, T, S = xc.build("k7_nolm")
    rl = X.lex_of(cfg["lex"])
    trie = Lexicon(rl.write(tmp_path, "lex"), None, K=rl.K, space=rl.space)
    dev = _dev(probs)
    hyps, scores = ctc.DecodeParallel(lens, dev, beam=cfg["B"], max_classes=cfg["C"], nbest=4, lexicon=trie, word_bonus=cfg["beta"])
    assert any(rl.space in h for hs in hyps for h in hs)      # some entry has more than one word
    del trie                                                  # the call speaks of the decode call's words, not of the lexicon
    st = ctc.DecodeStamps(lens, dev, conf_scale=0.5)
    assert _hold("spaced", ctc, lens, probs, dev, st, scores.copy(), False, conf_scale=0.5, space=rl.space) > 0


def test_unspaced_lexicon_mode(ctc, tmp_path):
    from eesen_amd.api import Lexicon
    cfg = wc.CASES["k7_c3"]
    lens, probs, T, S = wc.build("k7_c3")
    rl = W.lex_of(cfg["lex"])
    trie = Lexicon(rl.write(tmp_path, "wlex"), None, K=rl.K, space=None)
    dev = _dev(probs)
    hyps, scores = ctc.DecodeParallel(lens, dev, beam=cfg["B"], max_classes=cfg["C"], nbest=4, lexicon=trie, word_bonus=cfg["beta"])
    assert ctc.word_ends is not None and np.any(ctc.words_len > 1)
    st = ctc.DecodeStamps(lens, dev)
    assert _hold("unspaced", ctc, lens, probs, dev, st, scores.copy(), False) > 0


def test_errors(gpu):
    from eesen_amd.api import Ctc, CuMatrix, EesenError
    lens, probs, _ = small_batch()
    dev = _dev(probs)
    ctc = Ctc()
    with pytest.raises(EesenError) as e:
        ctc.DecodeStamps(lens, dev)                           # no decode call yet
    assert e.value.code == -3
    ctc.DecodeParallel(lens, dev, beam=4, max_classes=3, nbest=2)
    ok = ctc.DecodeStamps(lens, dev)
    for bad_lens, bad_dev in (([40, 1], _dev(probs[:80])), (lens, _dev(np.concatenate([probs, probs[:3]])))):    # another S, other rows
        with pytest.raises(EesenError) as e:
            ctc.DecodeStamps(bad_lens, bad_dev)
        assert e.value.code == -3
    for c in (-1.0, float("nan"), float("inf")):
        with pytest.raises(EesenError) as e:
            ctc.DecodeStamps(lens, dev, conf_scale=c)
        assert e.value.code == -1
    narrow = CuMatrix.view(dev.ptr, dev.rows, dev.cols, dev.cols - 1, keepalive=dev)     # ld < K
    with pytest.raises(EesenError) as e:
        ctc.DecodeStamps(lens, narrow)
    assert e.value.code == -1
    assert _same(ok, ctc.DecodeStamps(lens, dev))             # a refused call leaves the state alone


def test_guard_word_set_returns_nan_and_minus_one(gpu):
    from eesen_amd import synth
    from eesen_amd.api import Net, Ctc
    lens, probs, _ = small_batch()
    dev = _dev(probs)
    net = Net.from_layers(synth.make_model(**synth.config("tiny_bi")))
    ctc = Ctc()
    ctc.SetGuard(net)
    ctc.DecodeParallel(lens, dev, beam=4, max_classes=3, nbest=2)
    ok = ctc.DecodeStamps(lens, dev)
    assert np.all(np.isfinite(ok.path_score[:, 0]))
    net._raise_error_word(2)
    bad = ctc.DecodeStamps(lens, dev)
    for a in (bad.label_start, bad.label_end, bad.word_start, bad.word_end):
        assert np.all(a == -1)
    assert np.all(np.isnan(bad.path_score)) and np.all(np.isnan(bad.word_conf))
    net._raise_error_word(0)
    assert _same(ok, ctc.DecodeStamps(lens, dev))
    ctc.SetGuard(None)


def test_times_are_populated(ctc):
    lens, probs, _ = small_batch()
    dev = _dev(probs)
    ctc.DecodeParallel(lens, dev, beam=4, max_classes=3, nbest=2)
    ctc.DecodeStamps(lens, dev)
    t = ctc.StampTimes()
    assert set(t) == {"lattices", "sweep", "stamps"} and all(0 <= v < 1 for v in t.values()) and t["sweep"] > 0
