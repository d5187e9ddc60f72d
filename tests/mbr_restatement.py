"""A restatement in plain Python of INTEGRATION.md "Minimum Bayes risk": the Levenshtein distance (unit costs, the total only) and the
posterior / risk / order of eesen_ctc_decode_mbr.  No GPU, no library: tests/test_mbr_cases.py holds it to the host C routine
(eesen_edit_distance) and to a brute-force recursion, the GPU tests hold the library to it.

Every sum runs over the counting entries in ascending rank, in fp64, in the order the header states; the library's doubles are held to
1e-12 relative of these (the slack is for exp alone).
"""
import math
from functools import lru_cache

import numpy as np

MAX_LEN = 8192
DEAD = -1e29
NOT_COUNTING = -1e30


def levenshtein(a, b):
    """d(a, b): the fewest insertions, deletions and substitutions that turn a into b."""
    a, b = list(a), list(b)
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j - 1] + (a[i - 1] != b[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(b)]


def levenshtein_np(a, b):
    """The same by rows in numpy, for the long sequences: cur[j] = min(sub[j], prev[j] + 1, cur[j - 1] + 1); the last term is a running
    minimum of (candidate[j] - j) + j."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    j = np.arange(b.size + 1)
    prev = j.copy()
    for i in range(1, a.size + 1):
        cand = np.empty(b.size + 1, np.int64)
        cand[0] = i
        cand[1:] = np.minimum(prev[:-1] + (b != a[i - 1]), prev[1:] + 1)
        prev = np.minimum.accumulate(cand - j) + j
    return int(prev[b.size])


def brute_force(a, b):
    """The definition itself, by recursion on the last tokens (for the shortest sequences only)."""
    a, b = tuple(a), tuple(b)

    @lru_cache(maxsize=None)
    def d(i, j):
        if i == 0 or j == 0:
            return i + j
        return min(d(i - 1, j) + 1, d(i, j - 1) + 1, d(i - 1, j - 1) + (a[i - 1] != b[j - 1]))

    return d(len(a), len(b))


def counts(z, n_tokens):
    """Which entries count: within the returned count (n_tokens >= 0), z > -1e29 and not NaN, no more than 8192 tokens."""
    return [bool(n >= 0 and n <= MAX_LEN and float(zi) > DEAD and not math.isnan(float(zi))) for zi, n in zip(z, n_tokens)]


def posterior(z, cnt, scale):
    """P_i = exp(c (z_i - z_max)) / sum_k exp(c (z_k - z_max)) over the counting entries; -1e30 elsewhere."""
    n = len(z)
    zmax = -math.inf
    for i in range(n):
        if cnt[i]:
            zmax = max(zmax, float(z[i]))
    e = [math.exp(scale * (float(z[i]) - zmax)) if cnt[i] else 0.0 for i in range(n)]
    total = 0.0
    for i in range(n):
        if cnt[i]:
            total += e[i]
    return [e[i] / total if cnt[i] else NOT_COUNTING for i in range(n)]


def risk(P, dist, cnt):
    """risk_i = sum_k P_k d(i, k), k over the counting entries in ascending rank; -1e30 elsewhere."""
    n = len(P)
    out = []
    for i in range(n):
        r = 0.0
        for k in range(n):
            if cnt[i] and cnt[k]:
                r += P[k] * float(dist[i][k])
        out.append(r if cnt[i] else NOT_COUNTING)
    return out


def order(R, z, cnt):
    """The counting ranks by risk ascending, ties to the larger z, then to the smaller rank; then the others in rank order."""
    n = len(R)
    first = sorted((i for i in range(n) if cnt[i]), key=lambda i: (R[i], -float(z[i]), i))
    return first + [i for i in range(n) if not cnt[i]]


def mbr(z, tokens, scale=1.0):
    """Everything for one list: tokens[i] a list, or None beyond the returned count.  Returns dist, posterior, risk, order, counts."""
    n = len(z)
    cnt = counts(z, [len(t) if t is not None else -1 for t in tokens])
    dist = [[levenshtein(tokens[i], tokens[k]) if cnt[i] and cnt[k] else -1 for k in range(n)] for i in range(n)]
    P = posterior(z, cnt, scale)
    R = risk(P, dist, cnt)
    return dist, P, R, order(R, z, cnt), cnt
