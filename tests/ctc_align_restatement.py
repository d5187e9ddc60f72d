"""The yardstick of the best-path (Viterbi) CTC alignment (eesen_ctc_align_parallel): the recurrence stated directly in numpy.

The reference has no alignment code (it aligns through a per-utterance TLG graph and its WFST decoder, align_ctc_single_utt.sh:67-85),
so there is nothing to compile; the recurrence is, with l' the labels interleaved with blanks (L' = 2U+1 positions, blank = 0) and
s_t(k) the log-score of class k at frame t:

  delta_0(0) = s_0(l'_0),  delta_0(1) = s_0(l'_1),  delta_0(j >= 2) = -1e30
  delta_t(j) = s_t(l'_j) + max(delta_{t-1}(j), delta_{t-1}(j-1), [delta_{t-1}(j-2) iff j odd and l'_j != l'_{j-2}])
  j_end = argmax(delta_{n-1}(L'-1), delta_{n-1}(L'-2));  score = delta_{n-1}(j_end);  trace back to t = 0

A cell none of whose predecessors is reachable (maximum not above -1e30) stays at exactly -1e30.  Tie rule: among equal predecessors
the smallest move wins (stay, then j-1, then j-2); at the end the final blank L'-1 wins over L'-2.  Every path's score is the sum of
its frames' log-scores added in frame order, so two paths that emit the same classes have bit-identical scores in either precision.
Infeasible (best final delta <= -1e29): score -1e30, every position -1.

The bar of every comparison with the fp64 recurrence is bar_s = 64 * 2^-24 * |score64_s| (tests/test_ctc_align_restatement.py says why).
"""
import functools

import numpy as np

NEG = -1e30
BAR_REL = 64.0 * 2.0 ** -24


def expand(labels):
    lab = np.asarray(labels, np.int64)
    out = np.zeros(2 * lab.size + 1, np.int64)
    out[1::2] = lab
    return out


def _skip(lab):
    """skip[j]: the move j-2 -> j exists (j odd, j > 1, another class than two positions back)."""
    sk = np.zeros(lab.size, bool)
    sk[3::2] = lab[3::2] != lab[1:-2:2]
    return sk


def _forward(e, sk, dtype):
    n, L = e.shape
    neg = dtype(NEG)
    d = np.full((n, L), neg, dtype)
    d[0, :2] = e[0, :2]
    for t in range(1, n):
        p = d[t - 1]
        a1 = np.concatenate([[neg], p[:-1]]).astype(dtype)
        a2 = np.where(sk, np.concatenate([[neg, neg], p[:-2]]).astype(dtype), neg)
        m = np.maximum(np.maximum(p, a1), a2)
        d[t] = np.where(m > neg, e[t] + m, neg)
    return d


def viterbi(logp, labels, dtype=np.float64):
    """logp [n x K] log-scores of ONE utterance's frames.  Returns (pos [n] int32, cls [n] int32, score) with the tie rule; all -1
    and -1e30 without a feasible path."""
    dtype = np.dtype(dtype).type
    lab = expand(labels)
    L = lab.size
    lp = np.asarray(logp).astype(dtype)
    n = lp.shape[0]
    none = np.full(n, -1, np.int32), np.full(n, -1, np.int32), dtype(NEG)
    if n == 0:
        return none
    sk = _skip(lab)
    with np.errstate(invalid="ignore"):
        d = _forward(lp[:, lab], sk, dtype)
    a, b = d[n - 1, L - 1], d[n - 1, L - 2]
    j = L - 1 if a >= b else L - 2
    score = a if a >= b else b
    if not score > -1e29:
        return none
    neg = dtype(NEG)
    pos = np.empty(n, np.int32)
    pos[n - 1] = j
    for t in range(n - 1, 0, -1):
        p = d[t - 1]
        a0 = p[j]
        a1 = p[j - 1] if j >= 1 else neg
        a2 = p[j - 2] if sk[j] else neg
        j -= 0 if (a0 >= a1 and a0 >= a2) else (1 if a1 >= a2 else 2)
        pos[t - 1] = j
    return pos, lab[pos].astype(np.int32), score


def path_is_valid(pos, labels, n):
    """The path starts in {0, 1}, ends in {L'-2, L'-1}, every move is one of the three legal ones, and its classes collapse
    (repeats merged, blanks dropped) to the label sequence."""
    lab = expand(labels)
    L = lab.size
    pos = np.asarray(pos)
    if pos.shape != (n,) or n == 0 or pos.min() < 0 or pos.max() >= L:
        return False
    if pos[0] not in (0, 1) or pos[-1] not in (L - 2, L - 1):
        return False
    sk = _skip(lab)
    for a, b in zip(pos[:-1], pos[1:]):
        if not (b == a or b == a + 1 or (b == a + 2 and sk[b])):
            return False
    cls = lab[pos]
    col = cls[np.concatenate([[True], cls[1:] != cls[:-1]])]
    # (a label that names class 0 itself collapses away like a blank: the classes are compared without it, the label positions with it)
    if [int(c) for c in col if c != 0] != [int(x) for x in labels if x != 0]:
        return False
    return [int(lab[j]) for j in sorted(set(int(p) for p in pos)) if j & 1] == [int(x) for x in labels]


def path_score(logp, labels, pos, dtype=np.float64):
    """The sum, in frame order, of the log-scores along `pos`."""
    lab = expand(labels)
    lp = np.asarray(logp).astype(dtype)
    acc = np.dtype(dtype).type(0)
    for t, j in enumerate(pos):
        acc = lp[t, lab[j]] if t == 0 else acc + lp[t, lab[j]]
    return acc


def runner_up_gap(logp64, labels):
    """Best score minus the best score of any path that leaves the optimal one: with delta the forward and epsilon the backward
    max-plus lattice, delta + epsilon - s at a cell is the best score of a path through it; the runner-up is the maximum over the
    cells off the best path.  +inf when no other path exists, 0 for an exact tie (up to the rounding of the two-lattice sum)."""
    lab = expand(labels)
    L = lab.size
    lp = np.asarray(logp64, np.float64)
    n = lp.shape[0]
    pos, _, score = viterbi(lp, labels, np.float64)
    if n == 0 or pos[0] < 0:
        return float("nan")
    sk = _skip(lab)
    e = lp[:, lab]
    d = _forward(e, sk, np.float64)
    eps = np.full((n, L), NEG)
    eps[n - 1, L - 2:] = e[n - 1, L - 2:]
    for t in range(n - 2, -1, -1):
        q = eps[t + 1]
        b1 = np.concatenate([q[1:], [NEG]])
        b2 = np.where(np.concatenate([sk[2:], [False, False]]), np.concatenate([q[2:], [NEG, NEG]]), NEG)
        m = np.maximum(np.maximum(q, b1), b2)
        eps[t] = np.where(m > NEG, e[t] + m, NEG)
    through = np.where((d > NEG) & (eps > NEG), d + (eps - e), -np.inf)
    through[np.arange(n), pos] = -np.inf
    return float(score - through.max())


def utterance(probs, s, S, n):
    """float32 probabilities of utterance s (its first n frames) of a [T*S x K] matrix."""
    return np.asarray(probs)[s:n * S:S]


def log64(p):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(p, np.float64))


def log32(p):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(p, np.float32), dtype=np.float32)


def reference_of(lens, probs, labels, S, with_gap=True):
    """Per utterance: dict(pos64, score64, bar, gap, pos32, score32) on the same float32 probabilities."""
    out = []
    for s in range(S):
        p = utterance(probs, s, S, int(lens[s]))
        pos64, _, score64 = viterbi(log64(p), labels[s], np.float64)
        pos32, _, score32 = viterbi(log32(p), labels[s], np.float32)
        out.append(dict(pos64=pos64, score64=float(score64), bar=BAR_REL * abs(float(score64)), pos32=pos32, score32=float(score32),
                        gap=runner_up_gap(log64(p), labels[s]) if with_gap else None))
    return out


# every tests/ctc_cases.py input the GPU test (tests/test_gpu_ctc_align.py) uses
DISPATCH_CASES = ("boundary_U31", "boundary_U32", "boundary_U127", "boundary_U128", "boundary_U511", "long_U2047",
                  "dense_3x12x7", "dense_33x40x100", "peaky_h4_60", "peaky_denormal")
FEASIBILITY_CASES = ("shortest_dense", "shortest_h12", "one_short_dense")
TIE_CASES = ("peaky_class0",)
GAP_EXEMPT = ("long_U2047",)         # gaps of 6e-4 and 8e-3 nats on scores of several thousand


@functools.lru_cache(maxsize=None)
def case(name):
    """(lens, probs, labels, T, S, per-utterance references) of a tests/ctc_cases.py case; computed once, shared, not to be changed."""
    from tests import ctc_cases
    lens, probs, labels, T, S = ctc_cases.build(name)
    probs.setflags(write=False)
    return lens, probs, labels, T, S, reference_of(lens, probs, labels, S)


def uniform_case():
    """Every row uniform: every reachable cell ties, and the path is the tie rule's alone."""
    S, T, K = 3, 20, 5
    labels = [np.array(l, np.int32) for l in ([1], [2, 2, 3], [1, 2, 3, 4])]
    return np.full(S, T, np.int32), np.full((T * S, K), 1.0 / K, np.float32), labels, T, S
