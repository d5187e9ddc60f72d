"""The cases of the edit-distance kernel and of N-best MBR (tests/test_mbr_cases.py on the CPU, tests/test_gpu_edit_distance.py and
tests/test_gpu_ctc_mbr.py on the GPU).  What each list promises is asserted in tests/test_mbr_cases.py, so the GPU tests cannot pass
on lists that do not contain what they say.

The lengths are the smallest at which the kernel's schedule can go wrong: an empty side, one lane, one full strip of 64 columns, one
token into the second strip, the third strip, and pairs whose cheaper orientation puts the second sequence on the rows.
"""
import itertools

import numpy as np

LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 200]
ALPHABETS = [2, 1000]
LANES = 64


def sweep_cost(rows, cols):
    """Steps of the kernel with `rows` on the rows: strips * (rows + 63) (csrc/edit_distance.hip)."""
    return ((cols + LANES - 1) // LANES) * (rows + LANES - 1)


def swaps(la, lb):
    """Does the kernel put b on the rows?"""
    return la > 0 and lb > 0 and sweep_cost(lb, la) < sweep_cost(la, lb)


def length_pairs(alphabet, seed=9800):
    """One group per ordered pair of LENGTHS: [a, b] random over `alphabet` symbols.  The symbols of the large alphabet are spread over
    the whole int32 range, negative values included: tokens may be any int32."""
    rng = np.random.default_rng(seed + alphabet)
    table = np.arange(alphabet, dtype=np.int64) if alphabet <= 2 else rng.integers(-2**31, 2**31, alphabet)
    groups = []
    for la, lb in itertools.product(LENGTHS, LENGTHS):
        groups.append([table[rng.integers(0, alphabet, la)].astype(np.int32).tolist(), table[rng.integers(0, alphabet, lb)].astype(np.int32).tolist()])
    return groups


def structured_pairs(seed=9810):
    """name -> (a, b, the distance the structure implies)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(1, 50, 150).astype(np.int32).tolist()
    distinct = list(range(1000, 1130))
    out = {
        "identical": (base, list(base), 0),
        "prefix": (base, base[:70], 80),
        "suffix": (base, base[80:], 80),
        "reversed": (distinct, distinct[::-1], 130),          # distinct symbols, even length: no token stays in place
        "all_different": (list(range(100)), list(range(500, 629)), 129),
    }
    for pos in (0, 63, 64, 150):
        out[f"insertion_at_{pos}"] = (base, base[:pos] + [777] + base[pos:], 1)
    return out


def groups_of(ns=(1, 2, 3, 64), seed=9820):
    """Groups of n sequences of mixed lengths (0 .. 140) over 3 symbols: both triangles and the diagonal of n x n."""
    rng = np.random.default_rng(seed)
    return [[rng.integers(0, 3, int(rng.integers(0, 141))).astype(np.int32).tolist() for _ in range(n)] for n in ns]


def long_pair(seed=9830):
    """8192 tokens against 8191 over 4 symbols: the limit, two waves' worth of boundary column."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, 8192).astype(np.int32)
    b = a[:8191].copy()
    flip = rng.integers(0, 8191, 40)
    b[flip] = 5 + (b[flip] & 1)
    return a.tolist(), b.tolist()


# ------------------------------------------------------------------------------------------------ MBR
# Two frames, K = 4 (blank, 1, 2, 3): the list of ALL labellings (10 of them; beam 16 holds every prefix, so the search is exact) whose
# most probable entry [2, 3] is not the one of least expected errors -- that is [3], which is one edit from most of the mass.
WINNER_POST = np.array([[0.30, 0.30, 0.50, 0.05], [0.20, 0.05, 0.05, 0.50]], np.float64)
WINNER = {"T": 2, "K": 4, "beam": 16, "nbest": 16, "count": 10, "map": [2, 3], "mbr": [3]}


def winner_batch():
    """lens, posteriors [T * S, K] float32 of the one-utterance batch."""
    p = WINNER_POST / WINNER_POST.sum(1, keepdims=True)
    return np.array([2], np.int32), np.ascontiguousarray(p, np.float32)


def all_labellings(post):
    """Every labelling of a short utterance with its exact probability, most probable first (by enumeration of all paths)."""
    T, K = post.shape
    mass = {}
    for path in itertools.product(range(K), repeat=T):
        p = float(np.prod([post[t, c] for t, c in enumerate(path)]))
        lab, prev = [], -1
        for c in path:
            if c != prev and c != 0:
                lab.append(c)
            prev = c
        mass[tuple(lab)] = mass.get(tuple(lab), 0.0) + p
    return sorted(((list(k), v) for k, v in mass.items()), key=lambda kv: -kv[1])


# the order rule on hand-made lists: (z, tokens, scale, the order it must give, what the list shows)
ORDER_CASES = {
    # entries 0 and 2 are the same tokens with the same z: same risk, same z -> the smaller rank first
    "tie_by_rank": ([-1.0, -1.5, -1.0], [[1, 2], [1, 3], [1, 2]], 1.0, [0, 2, 1]),
    # scale 0: the uniform posterior; every entry is 1 from both others, so all three risks are equal; the larger z first
    "tie_by_z": ([-3.0, -2.0, -1.0], [[1, 2], [1, 3], [1]], 0.0, [2, 1, 0]),
    # rank 1 beyond the count (None), rank 2 dead (z = -1e30), rank 3 NaN: last, in rank order
    "non_counting_last": ([-2.0, -1e30, -1e30, float("nan"), -1.0], [[1, 2, 3], None, [1], [1], [1, 2]], 1.0, [4, 0, 1, 2, 3]),
}
