"""Inputs of the exact-score and second-pass tests (tests/test_ctc_rescore_cases.py on the CPU, tests/test_gpu_ctc_rescore.py and
tests/test_gpu_ctc_rescore_cli.py on the GPU).  The CPU test holds, with the restatements alone, every property of these inputs the
GPU tests rely on.

reorder    dense posteriors (softmax of N(0, 2^2) logits), n = 12 frames, K = 5, beam 4, max_classes 4, nbest 4: utterances whose four
           returned entries rank differently by their exact fp64 scores than the beam ranked them, every pair of exact scores and
           every pair of beam totals more than 1e-3 apart (so neither order hangs on rounding), found by `search_reorder` over the
           seeds from 0 and recorded in REORDER_SEEDS.
quirk      where the reference's closing formula (the final blank as the base) fails: `no_final_blank` has n = U + repeats frames, so
           the final blank is unreachable; `last_frame_spike` is tests/ctc_cases.last_frame_spike_case.
bitwise    peaky posteriors whose last frame is a blank spike: the final blank's alpha is far above the final label's, where the
           symmetric close and eval_parallel's are the same expression.  L' = 201 (256 positions, one wave) and 401 (512 positions,
           four waves by default).
"""
import functools

import numpy as np

from tests import ctc_beam_restatement as R
from tests import ctc_cases as cc
from tests import ctc_rescore_restatement as Q

REORDER = dict(n=12, K=5, B=4, C=4, N=4)
REORDER_SEEDS = (0, 3, 4)          # search_reorder's first three hits (the CPU test runs the search again)
GAP = 1e-3


def reorder_utterance(seed):
    rng = np.random.default_rng(90000 + seed)
    return cc.softmax32((2.0 * rng.standard_normal((REORDER["n"], REORDER["K"]))).astype(np.float32))


def reorder_facts(probs):
    """The first pass in both precisions and the exact scores of its entries: dict(labels, beam, exact, order64, ok)."""
    l32, l64 = R.log32(probs), R.log64(probs)
    b64 = R.beam_search(l64, l32, REORDER["B"], REORDER["C"], np.float64)[:REORDER["N"]]
    b32 = R.beam_search(l32, l32, REORDER["B"], REORDER["C"], np.float32)[:REORDER["N"]]
    labels = [list(p) for p, _ in b32]
    exact = [Q.lnp(l64, lab) for lab in labels]
    order64 = Q.order_of(exact, [True] * len(exact))
    ok = (len(b32) == REORDER["N"] and [p for p, _ in b64] == [p for p, _ in b32] and order64 != list(range(len(exact)))
          and order64[0] != 0 and Q.min_gap(exact) > GAP and Q.min_gap([v for _, v in b64]) > GAP)
    return dict(labels=labels, beam=[v for _, v in b32], exact=exact, order64=order64, ok=ok)


def search_reorder(count=3, limit=400):
    hits = [seed for seed in range(limit) if reorder_facts(reorder_utterance(seed))["ok"]]
    return tuple(hits[:count])


@functools.lru_cache(maxsize=None)
def reorder_batch():
    """lens, probs [n*S x K], S: the utterances of REORDER_SEEDS side by side."""
    utts = [reorder_utterance(seed) for seed in REORDER_SEEDS]
    S, n, K = len(utts), REORDER["n"], REORDER["K"]
    probs = np.empty((n * S, K), np.float32)
    for s, u in enumerate(utts):
        probs[s::S] = u
    probs.setflags(write=False)
    return np.full(S, n, np.int32), probs, S


@functools.lru_cache(maxsize=None)
def quirk_cases():
    """name -> (lens, probs, labels, T, S), S = 1."""
    out = {}
    lens, probs, labels = cc.shortest_case((5,), 8, None, 9301, short_by=1)
    assert int(lens[0]) == len(labels[0]) + cc.num_repeats(labels[0])
    out["no_final_blank"] = (lens, probs, labels, int(lens[0]), 1)
    lens, probs, labels = cc.shortest_case((40,), 12, 12.0, 9302, short_by=1)
    out["no_final_blank_h12"] = (lens, probs, labels, int(lens[0]), 1)
    lens, probs, labels = cc.last_frame_spike_case()
    out["last_frame_spike"] = (lens, probs, labels, int(lens[0]), 1)
    return out


BITWISE = {
    "peaky_L201": dict(args=(3, 300, 40, 100, (12, 30, 12), 9401), positions=256),
    "peaky_L401": dict(args=(2, 460, 20, 200, (12, 30), 9402), positions=512),
}
# EESEN_CTC_WAVES values the existing bit-for-bit tests create a Ctc under, per padded row (tests/test_gpu_parity.py:
# test_ctc_multi_wave_sweep_is_bit_identical; 256 positions: the 2 x 2 arm of csrc/ctc.hip)
WAVES = {256: (1, 2), 512: (1, 2, 4)}


@functools.lru_cache(maxsize=None)
def bitwise_case(name):
    lens, probs, labels = cc.peaky_case(*BITWISE[name]["args"])
    S = len(lens)
    probs = np.ascontiguousarray(probs, np.float32)
    probs.setflags(write=False)
    return np.asarray(lens, np.int32), probs, [np.asarray(l, np.int32) for l in labels], probs.shape[0] // S, S


def utt(probs, s, S, n):
    return np.asarray(probs)[s:n * S:S]
