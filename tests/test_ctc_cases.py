"""The inputs of tests/test_gpu_ctc_per_utterance.py, held with the oracle alone (no GPU): what the GPU bars rely on is asserted here for
every case, so that a bar can never be loosened by the inputs drifting.  A case that breaks a condition is to be replaced, not waved
through.

Held regime (spike heights <= 86, dense posteriors): both oracle precisions finite, and every utterance's fp32-vs-fp64 gradient floor under a
cap that depends on T alone -- 2e-3 up to T = 1500, 2e-2 above (the exponent of gamma carries ulp(|alpha|), |alpha| grows with T).  Above
T = 1500 the fp64 bar is therefore a few per cent; what is tight there is the element-wise check of alpha and beta against the fp32 oracle.
Extreme regime (heights >= 95, probabilities 1e-42 ... 0): the fp32 reference is no accurate evaluation there; the conditions are the special
cases the GPU test then holds the kernel to.
"""
import numpy as np
import pytest

from tests import ctc_cases as cc


@pytest.fixture(scope="module")
def evaluated():
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()                                   # (one case at a time: the largest holds ~0.5 GB of lattices)
            lens, probs, labels, T, S = cc.build(name)
            cache[name] = (lens, probs, labels, T, S) + cc.oracle_pair(lens, probs, labels, T, S)
        return cache[name]
    return get


def _finite(o, lattice=True):
    """Gradient and ln p; the lattice too where no probability is an exact zero (ln 0 = -inf enters alpha and beta as it is)."""
    return bool(np.isfinite(o["diff"]).all() and np.isfinite(o["pzx"]).all() and
                (not lattice or (np.isfinite(o["alpha"]).all() and np.isfinite(o["beta"]).all())))


def test_generator_shapes():
    S, T, K, U = 6, 120, 25, 20
    lens, probs, labels = cc.peaky_case(S, T, K, U, (4, 30), seed=5)
    assert probs.dtype == np.float32 and probs.shape == (T * S, K)
    assert np.all(np.diff(lens) >= 0) and lens[-1] == T and lens[0] >= 0.7 * T
    assert len(labels[-1]) == U and all(U // 2 <= len(l) <= U for l in labels)
    assert all(l.min() >= 1 and l.max() < K for l in labels)
    np.testing.assert_allclose(probs.astype(np.float64).sum(1), 1.0, atol=1e-5)
    # about 20 % adjacent repeats, and the spikes sit on a monotone alignment: the greedy path of a tall-spike utterance is its label sequence
    big = cc.peaky_case(4, 2000, 30, 400, (30,), seed=6, wrong=0.0)
    reps = sum(cc.num_repeats(l) for l in big[2]) / sum(len(l) - 1 for l in big[2])
    assert 0.15 < reps < 0.25
    for s in range(4):
        path = np.argmax(cc.utt(big[1], s, 4, int(big[0][s])), axis=1)
        hyp = [int(c) for i, c in enumerate(path) if c != 0 and (i == 0 or path[i - 1] != c)]
        assert hyp == big[2][s].tolist()
    # class 0 as a label only when asked for
    assert any((l == 0).any() for l in cc.peaky_case(3, 300, 40, 40, (4,), seed=13, label_low=0)[2])


def test_dispatch_cases_cover_every_step():
    """csrc/ctc.hip: ctc_error_diff picks its instantiation by the longest lattice 2 U + 1 (steps at 128, 256, 384, 512, 768, 1024, 1536, 2048,
    3072), ctc_host.cpp pads the rows to 64 * 2^n."""
    Ls = [2 * u + 1 for u in cc.BOUNDARY_U]
    for step in (64, 128, 256, 384, 512, 768, 1024, 1536, 2048, 3072):
        assert step - 1 in Ls and step + 1 in Ls
    for name, frames in cc.FRAMES_CASES.items():
        lens, probs, labels, T, S = cc.build(name)
        assert max(1, min(8, T * S // 16384)) == frames and T % 2 == 1 and T % frames != 0
        starts = np.arange(0, T, frames)                   # some chunk of `frames` frames straddles the end of an utterance
        assert sum(int(((starts < n) & (starts + frames > n)).any()) for n in lens) >= S // 4
        assert max(len(l) for l in labels) <= 40 and probs.shape[1] == 30


@pytest.mark.parametrize("name", list(cc.CASES))
def test_case_conditions(name, evaluated):
    lens, probs, labels, T, S, o32, o64 = evaluated(name)
    reg = cc.regime(name)
    assert _finite(o32, reg != "extreme") and _finite(o64, reg != "extreme")
    if reg == "held":
        for s in range(S):
            n = int(lens[s])
            floor = cc.grad_figure(cc.utt(o32["diff"], s, S, n), cc.utt(o64["diff"], s, S, n))
            assert floor < cc.floor_cap(T), (s, floor)
            assert cc.lnp_figure(o32["pzx"][s], o64["pzx"][s]) < 1e-5, s
    elif reg == "quirk":
        # one frame short of the ln p formula's reach: the last blank is unreachable, ln p = -1e30 + log(1 + FLT_MAX) rounds to -1e30
        assert np.all(o32["pzx"] < -1e29)
    else:
        assert min(cc.CASES[name][1][4]) >= 95
        infeasible, feasible_outside = 0, 0
        for s in range(S):
            n = int(lens[s])
            p = cc.utt(probs, s, S, n)
            lat = cc.lattice_classes(labels[s])
            d32, d64 = cc.utt(o32["diff"], s, S, n), cc.utt(o64["diff"], s, S, n)
            if o32["pzx"][s] < -1e29:
                assert (p[:, lat] == 0).any()                                    # infeasible because of an exact zero
                assert not d32.any() and not d64.any()                          # and its reference gradient is all zeros
                infeasible += 1
                continue
            assert cc.lnp_figure(o32["pzx"][s], o64["pzx"][s]) < 1e-5
            assert cc.broken_frames(d32, d64).sum() <= 0.05 * n, s
            feasible_outside += int((p == 0).any() and not (p[:, lat] == 0).any())
        assert infeasible >= 1 and feasible_outside >= 1
    if name in cc.DENORMAL_CASES:
        n_den = 0
        for s in range(S):
            p = cc.utt(probs, s, S, int(lens[s]))[:, cc.lattice_classes(labels[s])]
            n_den += int(((p > 0) & (p < cc.FLT_MIN_NORMAL)).sum())
            assert not (p == 0).any()
        assert n_den > 100
    if name in cc.CLASS0_CASES:
        assert sum(int((l == 0).sum()) for l in labels) >= 2


def test_tie_case_has_ties_at_both_ends():
    lens, probs, labels = cc.tie_case(4, 120, 12, 3)
    mx = probs.max(axis=1, keepdims=True)
    ties = (probs == mx).sum(axis=1)
    assert (ties == 2).sum() >= probs.shape[0] // 10
    first = np.argmax(probs, axis=1)
    last = probs.shape[1] - 1 - np.argmax(probs[:, ::-1], axis=1)
    assert ((first == 0) & (ties == 1)).any() and ((last == probs.shape[1] - 1) & (ties == 1)).any()
    assert ((first == 0) & (last == probs.shape[1] - 1) & (ties == 2)).any()


def test_last_frame_spike_is_a_reference_quirk():
    """Why the generator keeps labels off the last frame: the reference's ln p clamps there in fp32 (and not in fp64)."""
    lens, probs, labels = cc.last_frame_spike_case()
    o32, o64 = cc.oracle_pair(lens, probs, labels, len(probs), 1)
    assert abs(o64["pzx"][0]) < 1e-6 and -40 < o32["pzx"][0] < -20
