"""Inputs of the CTC prefix beam search tests (tests/test_ctc_beam_restatement.py on the CPU, tests/test_gpu_ctc_decode.py on the GPU):
the smallest shapes at which each piece of csrc/ctc_decode.hip can go wrong.  Existing minibatches come from tests/ctc_cases.py under
their names there; the new ones are built from its generators with seeds of their own.  A decoder needs no labels: a case is
(lens, probs [T*S x K] float32, T, S).

CONFIGS lists, per case, every (beam, max_classes) the GPU test decodes it at, so that the CPU test can hold the conditions the GPU
checks rely on (the stability cap, fp32 against fp64) with the restatement alone."""
import numpy as np

from tests import ctc_cases as cc


def _exhaustive():
    """K = 3, lens 1, 3, 5, 5: at most 63 prefixes exist, nothing is ever pruned at beam 64."""
    _, probs, _ = cc.dense_case(4, 5, 3, 2, 9101)
    return np.array([1, 3, 5, 5], np.int32), probs


def _wide():
    """K = 4100: ctc_row_topc takes 65 values per lane."""
    lens, probs, _ = cc.dense_case(2, 20, 4100, 4, 9102)
    return lens, probs


def _k2():
    """Blank plus one class: max_classes is clipped to 1."""
    lens, probs, _ = cc.dense_case(3, 9, 2, 2, 9103)
    return lens, probs


def _ties():
    lens, probs, _ = cc.tie_case(4, 20, 12, 9104)
    return lens, probs


def _uniform():
    S, T, K = 3, 10, 5
    return np.array([T, T - 3, T], np.int32), np.full((T * S, K), 1.0 / K, np.float32)


NEW = {"exhaustive": _exhaustive, "wide_K4100": _wide, "k2": _k2, "ties": _ties, "uniform": _uniform}

# case -> the (beam, max_classes) it is decoded at
CONFIGS = {
    "exhaustive": ((64, 2),),
    "dense_3x12x7": ((1, 6), (3, 1), (16, 6)),
    "dense_8x60x46": ((16, 20), (64, 32)),
    "dense_33x40x100": ((4, 8), (32, 64)),
    "wide_K4100": ((8, 64),),
    "k2": ((8, 1),),
    "peaky_h4_60": ((16, 20),),
    "peaky_denormal": ((16, 20),),
    "peaky_T1500": ((4, 4),),
}
TIE_CASES = ("ties", "uniform")        # exact ties: determinism and the invariants only, no equality with the restatement


def build(name):
    if name in NEW:
        lens, probs = NEW[name]()
    else:
        lens, probs, _, _, _ = cc.build(name)
    S = len(lens)
    return np.asarray(lens, np.int32), np.ascontiguousarray(probs, np.float32), probs.shape[0] // S, S
