"""-m gpu: batched Levenshtein distances on the device (csrc/edit_distance.hip: edit_distance_kernel, through
api.Ctc.EditDistanceParallel) against the host routine eesen_edit_distance.  Every integer must be equal: there is no tolerance.

The shapes (tests/mbr_cases.py, whose promises tests/test_mbr_cases.py asserts) are the smallest at which the schedule can go wrong:
empty sides, one lane, one full strip, one token into the second strip, the third and fourth strip, both orientations.
"""
import ctypes as C

import numpy as np
import pytest

from tests import mbr_cases as M
from tests import mbr_restatement as Q

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctc(gpu):
    from eesen_amd.api import Ctc
    return Ctc()


def host(a, b):
    from eesen_amd import _lib
    lib = _lib.load()
    a, b = np.ascontiguousarray(a, np.int32), np.ascontiguousarray(b, np.int32)
    err = C.c_int(-1)
    _lib.check(lib.eesen_edit_distance(a.ctypes.data_as(C.c_void_p), a.size, b.ctypes.data_as(C.c_void_p), b.size, C.byref(err)))
    return err.value


def host_matrix(group):
    return np.array([[host(a, b) for b in group] for a in group], np.int32).reshape(len(group), len(group))


@pytest.mark.parametrize("alphabet", M.ALPHABETS)
def test_all_pairs_of_the_lengths(ctc, alphabet):
    """100 groups of two in one call, with each group's second sequence reversed as its reference: a pair job and two reference jobs
    per group."""
    groups = M.length_pairs(alphabet)
    refs = [b[::-1] for _, b in groups]
    pair, ref_dist = ctc.EditDistanceParallel(groups, refs)
    assert len(pair) == len(ref_dist) == len(groups) == 100
    for g, (a, b) in enumerate(groups):
        d = host(a, b)
        assert pair[g].dtype == np.int32 and pair[g].tolist() == [[0, d], [d, 0]], (alphabet, len(a), len(b), pair[g], d)
        assert ref_dist[g].tolist() == [host(a, refs[g]), host(b, refs[g])], (alphabet, len(a), len(b))


def test_structured_pairs(ctc):
    cases = M.structured_pairs()
    names = sorted(cases)
    pair, _ = ctc.EditDistanceParallel([[cases[n][0], cases[n][1]] for n in names])
    for n, p in zip(names, pair):
        a, b, want = cases[n]
        assert p.tolist() == [[0, want], [want, 0]] and host(a, b) == want, (n, p, want)
    # ... and the other way round: the second sequence first
    pair, _ = ctc.EditDistanceParallel([[cases[n][1], cases[n][0]] for n in names])
    assert [int(p[0, 1]) for p in pair] == [cases[n][2] for n in names]


def test_groups_both_triangles_and_the_diagonal(ctc):
    groups = M.groups_of()
    pair, none = ctc.EditDistanceParallel(groups)
    assert none is None and [p.shape for p in pair] == [(1, 1), (2, 2), (3, 3), (64, 64)]
    for g, p in zip(groups, pair):
        want = host_matrix(g)
        assert np.array_equal(p, want), np.argwhere(p != want)[:5]
        assert np.array_equal(p, p.T) and np.all(np.diag(p) == 0)


def test_no_groups_an_empty_group_and_an_empty_reference(ctc):
    pair, ref_dist = ctc.EditDistanceParallel([])
    assert pair == [] and ref_dist is None
    pair, ref_dist = ctc.EditDistanceParallel([], [])
    assert pair == [] and ref_dist == []
    seqs = [[[1, 2, 3], []], [], [[4] * 70]]
    pair, ref_dist = ctc.EditDistanceParallel(seqs, [[], [9, 9], [4] * 69 + [5]])
    assert pair[0].tolist() == [[0, 3], [3, 0]] and pair[1].shape == (0, 0) and pair[2].tolist() == [[0]]
    assert ref_dist[0].tolist() == [3, 0] and ref_dist[1].size == 0 and ref_dist[2].tolist() == [1]
    pair, ref_dist = ctc.EditDistanceParallel([[], []], [[1], [2]])          # groups without a sequence only: nothing to launch
    assert [p.shape for p in pair] == [(0, 0), (0, 0)] and all(r.size == 0 for r in ref_dist)


def test_the_longest_sequences_and_one_too_long(ctc):
    from eesen_amd.api import EesenError
    a, b = M.long_pair()
    want = Q.levenshtein_np(a, b)
    assert want == host(a, b)
    pair, ref_dist = ctc.EditDistanceParallel([[a, b]], [a[:100]])
    assert pair[0].tolist() == [[0, want], [want, 0]] and ref_dist[0].tolist() == [8092, host(b, a[:100])]
    before = ctc.MbrTimes()
    for seqs, refs in (([[a + [1], b]], None), ([[b]], [a + [1]])):
        with pytest.raises(EesenError) as e:
            ctc.EditDistanceParallel(seqs, refs)
        assert e.value.code == -1
    assert ctc.MbrTimes() == before          # refused before anything was launched or timed


def test_times_and_statistics(ctc):
    stats = ctc.stats()
    ctc.EditDistanceParallel(M.groups_of((8,)))
    t = ctc.MbrTimes()
    assert set(t) == {"build", "kernel", "host"} and all(0 <= v < 1 for v in t.values()) and t["kernel"] > 0
    assert ctc.stats() == stats
