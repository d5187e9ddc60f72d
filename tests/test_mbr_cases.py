"""CPU: the restatement of INTEGRATION.md "Minimum Bayes risk" (tests/mbr_restatement.py) against the host C routine and a brute-force
recursion, the order rule, and the promises of tests/mbr_cases.py -- so that the GPU tests, which hold the device to the host routine
and to this restatement, cannot pass on lists that lack what they claim to contain."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import mbr_cases as M
from tests import mbr_restatement as Q


@pytest.fixture(scope="module")
def host():
    from eesen_amd import _lib
    lib = _lib.load()

    def distance(a, b):
        a, b = np.ascontiguousarray(a, np.int32), np.ascontiguousarray(b, np.int32)
        err = C.c_int(-1)
        _lib.check(lib.eesen_edit_distance(a.ctypes.data_as(C.c_void_p), a.size, b.ctypes.data_as(C.c_void_p), b.size, C.byref(err)))
        return err.value

    return distance


def test_restatement_equals_brute_force_on_all_short_pairs():
    seqs = [list(s) for n in range(5) for s in itertools.product(range(3), repeat=n)]
    assert len(seqs) == 1 + 3 + 9 + 27 + 81
    for a in seqs:
        for b in seqs:
            assert Q.levenshtein(a, b) == Q.brute_force(a, b) == Q.levenshtein_np(a, b), (a, b)


@pytest.mark.parametrize("alphabet", M.ALPHABETS)
def test_restatement_equals_the_host_routine_on_the_length_pairs(host, alphabet):
    groups = M.length_pairs(alphabet)
    assert sorted({(len(a), len(b)) for a, b in groups}) == sorted(itertools.product(M.LENGTHS, M.LENGTHS))
    symbols = {t for g in groups for q in g for t in q}
    assert len(symbols) == 2 if alphabet == 2 else (len(symbols) > 500 and min(symbols) < 0 < max(symbols))
    ties = 0
    for a, b in groups:
        d = host(a, b)
        assert d == Q.levenshtein_np(a, b) == host(b, a), (len(a), len(b))
        assert abs(len(a) - len(b)) <= d <= max(len(a), len(b))
        ties += d < max(len(a), len(b))
    if alphabet == 2:
        assert ties > 50          # two symbols: tokens match all the time, and the three moves tie


def test_the_lengths_cover_the_schedule():
    pairs = list(itertools.product(M.LENGTHS, M.LENGTHS))
    assert any(M.swaps(a, b) for a, b in pairs) and any(not M.swaps(a, b) and a > 64 and b > 64 for a, b in pairs)
    strips = {(max(b, 1) + 63) // 64 for b in M.LENGTHS}
    assert {1, 2, 3, 4} <= strips
    assert M.swaps(64, 200) and not M.swaps(200, 64) and not M.swaps(0, 5)          # one strip of 263 steps, not four of 127
    assert M.sweep_cost(8191, 8192) == 128 * 8254 < M.sweep_cost(8192, 8191)          # the long pair: 128 strips either way


def test_structured_pairs_are_what_they_say(host):
    cases = M.structured_pairs()
    assert {"identical", "prefix", "suffix", "reversed", "all_different", "insertion_at_0", "insertion_at_63", "insertion_at_64",
            "insertion_at_150"} == set(cases)
    for name, (a, b, want) in cases.items():
        assert host(a, b) == Q.levenshtein_np(a, b) == want, name
    a, b, _ = cases["prefix"]
    assert a[:len(b)] == b
    a, b, _ = cases["suffix"]
    assert a[-len(b):] == b
    a, b, _ = cases["insertion_at_150"]
    assert len(a) == 150 and b[:150] == a          # "last": behind every token
    a, b, _ = cases["all_different"]
    assert not set(a) & set(b)


def test_groups_and_the_long_pair(host):
    groups = M.groups_of()
    assert [len(g) for g in groups] == [1, 2, 3, 64]
    g = groups[2]
    for i in range(3):
        for j in range(3):
            assert host(g[i], g[j]) == Q.levenshtein(g[i], g[j])
    lens = {len(q) for q in groups[3]}
    assert min(lens) < 64 < 128 < max(lens)
    a, b = M.long_pair()
    assert (len(a), len(b)) == (8192, 8191)
    d = host(a, b)
    assert d == Q.levenshtein_np(a, b) and 1 < d <= 41


@pytest.mark.parametrize("name", sorted(M.ORDER_CASES))
def test_order_rule(name):
    z, tokens, scale, want = M.ORDER_CASES[name]
    dist, P, R, order, cnt = Q.mbr(z, tokens, scale)
    assert order == want, (name, order, R)
    if name == "tie_by_rank":
        assert R[0] == R[2] and z[0] == z[2] and R[1] > R[0]
    if name == "tie_by_z":
        assert R[0] == R[1] == R[2] and P[0] == P[1] == P[2] == 1.0 / 3.0          # scale 0: the uniform posterior
    if name == "non_counting_last":
        assert cnt == [True, False, False, False, True]
        assert P[1] == R[2] == Q.NOT_COUNTING and dist[0][1] == dist[3][3] == -1 and dist[0][4] == 1 and dist[0][0] == 0
        assert abs(P[0] + P[4] - 1.0) < 1e-15 and R[0] == P[4] and R[4] == P[0]


def test_counting_rule():
    assert Q.counts([0.0, -1e29, -0.9e29, float("nan"), 0.0, 0.0], [3, 3, 3, 3, -1, 8193]) == [True, False, True, False, False, False]
    assert Q.counts([0.0], [8192]) == [True] and Q.counts([0.0], [0]) == [True]


def test_the_winner_case_contains_what_it_says():
    """The whole list of a two-frame utterance: its most probable labelling is not the one of least expected errors."""
    lens, probs = M.winner_batch()
    full = M.all_labellings(probs.astype(np.float64))
    assert len(full) == M.WINNER["count"] <= M.WINNER["nbest"] and full[0][0] == M.WINNER["map"]
    z = [np.log(p) for _, p in full]
    dist, P, R, order, cnt = Q.mbr(z, [l for l, _ in full], 1.0)
    assert all(cnt) and abs(sum(P) - 1.0) < 1e-12
    assert full[order[0]][0] == M.WINNER["mbr"] and order[0] == 1
    assert R[0] - R[order[0]] > 0.05 and z[0] - z[1] > 0.2          # neither the ranks nor the winner hang on rounding
