"""CPU: the host half of the time stamps (INTEGRATION.md "Time stamps and CTM") -- eesen_word_confidence through
api.word_confidence against the numpy restatement (tests/ctc_stamps_restatement.py), and the restatement's own interval rules on
hand-made paths.  eesen_word_confidence does no device work, so nothing here needs a GPU.

The bar of confidence comparisons is 1e-12 relative: both sides evaluate the same formula in fp64 over at most 64 terms.
"""
import numpy as np
import pytest

from tests import ctc_stamps_restatement as Z

REL = 1e-12


def _conf(scores, entries, c=1.0, stride=None):
    from eesen_amd.api import word_confidence
    stride = stride or max(1, max(len(e) for e in entries if e is not None))
    wl, ids, b, e = Z.pack(entries, stride)
    return word_confidence(scores, wl, ids, b, e, conf_scale=c), wl


def _hold(scores, entries, c=1.0, stride=None):
    got, wl = _conf(scores, entries, c, stride)
    want = Z.confidence(scores, entries, c)
    for i, row in enumerate(want):
        for j, v in enumerate(row):
            assert abs(got[i, j] - v) <= REL * abs(v), (i, j, got[i, j], v)
        assert np.all(got[i, len(row):] == Z.BEYOND), i
    return got


def test_label_intervals_of_a_path():
    #          t: 0  1  2  3  4  5  6  7  8
    pos = np.array([0, 1, 1, 2, 3, 3, 5, 6, 6])          # labels 0 .. 2 of U = 3; label 1 -> 2 is the skip 3 -> 5
    ls, le = Z.label_intervals(pos, 3, T=12)
    assert ls[:3].tolist() == [1, 4, 6] and le[:3].tolist() == [3, 6, 7]
    assert np.all(ls[3:] == -1) and np.all(le[3:] == -1) and ls.shape == le.shape == (12,)
    ls, le = Z.label_intervals(np.full(9, -1), 3)         # no path
    assert np.all(ls == -1) and np.all(le == -1)


def test_word_intervals_of_the_three_word_notions():
    labels = [4, 4, 9, 5, 9, 6, 6]                        # space = 9: words (4 4) (5) (6 6)
    #                  b  4  b  4  9  5  5  b  9  6  b  6
    pos = np.array([0, 1, 2, 3, 5, 7, 7, 8, 9, 11, 12, 13])
    ls, le = Z.label_intervals(pos, len(labels))
    plain = Z.word_intervals(Z.words_plain(labels), ls, le)
    assert plain == [(4, 1, 2), (4, 3, 4), (9, 4, 5), (5, 5, 7), (9, 8, 9), (6, 9, 10), (6, 11, 12)]
    spaced = Z.word_intervals(Z.words_spaced(labels, 9, [30, 31, 32]), ls, le)
    assert spaced == [(30, 1, 4), (31, 5, 7), (32, 9, 12)]   # the blank inside (4 b 4) and (6 b 6) is inside, the spaces' frames nowhere
    for (_, b, e) in spaced:
        assert not (b <= 4 < e) and not (b <= 8 < e)          # frames 4 and 8 are the spaces'
    unspaced = Z.word_intervals(Z.words_unspaced([70, 71, 72], [2, 5, 7]), ls, le)
    assert unspaced == [(70, 1, 4), (71, 4, 9), (72, 9, 12)]


def test_one_entry_is_certain():
    got = _hold([-3.5], [[(7, 0, 4), (2, 5, 9), (7, 9, 12)]], c=0.3)
    assert np.all(got[0, :3] == 1.0)                       # exactly


def test_same_word_overlapping_and_not():
    z = [-1.0, -2.0]
    apart = _hold(z, [[(5, 0, 4)], [(5, 4, 8)]])           # [0, 4) and [4, 8) do not intersect
    p = np.exp(np.array(z) - z[0]); p /= p.sum()
    assert abs(apart[0, 0] - p[0]) <= REL and abs(apart[1, 0] - p[1]) <= REL
    meet = _hold(z, [[(5, 0, 5)], [(5, 4, 8)]])
    assert abs(meet[0, 0] - 1.0) <= REL and abs(meet[1, 0] - 1.0) <= REL
    other = _hold(z, [[(5, 0, 5)], [(6, 4, 8)]])           # another id at the same place
    assert abs(other[0, 0] - p[0]) <= REL and abs(other[1, 0] - p[1]) <= REL


def test_a_word_twice_in_one_entry_counts_once():
    z = [-1.0, -1.5, -4.0]
    got = _hold(z, [[(5, 2, 6)], [(5, 0, 3), (5, 3, 8)], [(9, 0, 8)]])
    p = np.exp(np.array(z) - z[0]); p /= p.sum()
    assert abs(got[0, 0] - (p[0] + p[1])) <= REL           # entry 1 holds two intersecting 5s and counts once
    assert got[0, 0] <= 1.0


def test_conf_scale_zero_is_uniform():
    got = _hold([-1.0, -50.0, -7000.0, -7001.0], [[(1, 0, 2)], [(1, 1, 3)], [(2, 0, 3)], [(1, 5, 6)]], c=0.0)
    assert abs(got[0, 0] - 0.5) <= REL and abs(got[2, 0] - 0.25) <= REL and abs(got[3, 0] - 0.25) <= REL


def test_scores_1e4_apart_do_not_overflow():
    got = _hold([1e4, 0.0, -1e4], [[(1, 0, 2)], [(1, 1, 3)], [(1, 2, 9)]], c=1.0)
    assert np.all(np.isfinite(got[:, 0])) and got[0, 0] == 1.0 and got[2, 0] == 0.0
    got = _hold([1e4, 0.0, -1e4], [[(1, 0, 2)], [(1, 1, 3)], [(1, 2, 9)]], c=1e-4)   # exponents 0, -1, -2
    assert 0.0 < got[2, 0] < got[0, 0] < 1.0


def test_random_lists_64_entries():
    rng = np.random.default_rng(7101)
    for trial in range(20):
        n = int(rng.integers(1, 65))
        z = np.sort(rng.normal(-30, 5, n))[::-1]
        entries = []
        for _ in range(n):
            cuts = np.sort(rng.choice(np.arange(1, 40), size=int(rng.integers(0, 9)) * 2, replace=False))
            entries.append([(int(rng.integers(1, 6)), int(b), int(e)) for b, e in zip(cuts[0::2], cuts[1::2])])
        _hold(z, entries, c=float(rng.uniform(0, 2)), stride=9)


def test_absent_entries_and_errors():
    from eesen_amd.api import EesenError
    got, _ = _conf([-1.0, -1e30, -1e30], [[(3, 0, 2)], None, None])      # ranks beyond the returned count are no entries
    assert got[0, 0] == 1.0 and np.all(got[1:] == Z.BEYOND)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(EesenError):
            _conf([-1.0], [[(3, 0, 2)]], c=bad)
