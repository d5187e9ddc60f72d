"""The yardstick of the exact CTC scores and of the second pass over N-best lists (eesen_ctc_score_parallel, eesen_ctc_decode_rescore;
INTEGRATION.md "Rescoring"), stated literally in numpy and on Python lists.

Scores.  Log-scores s_t(k) clamped from below at -1e30, blank = class 0.  For labels l_1 .. l_U the lattice is l' = (0, l_1, 0, ...,
l_U, 0) of L' = 2 U + 1 positions and

    alpha_0(j)  = s_0(l'_j) for j < 2, -1e30 beyond
    alpha_t(j)  = s_t(l'_j) + logadd(logadd(alpha_{t-1}(j-1), alpha_{t-1}(j)), alpha_{t-1}(j-2) if j is odd and l'_j != l'_{j-2})
    a           = m + log(1 + exp(n - m)),  m = max, n = min of alpha_{n_s-1}(L'-1) and alpha_{n_s-1}(L'-2)    (U = 0: the one cell)

with the finite sentinel -1e30 standing for "no path" (x + -1e30 = -1e30 and logadd(-1e30, x) = x in both precisions).  The empty
labelling over no frames scores 0; a result <= -1e29 is "no path" and reads -1e30.  `dtype` is the precision of every operation:
float64 is the exact value (tests/ctc_beam_restatement.lnp64 to 1e-12), float32 the arithmetic of the device in the device's order,
whose distance from float64 is the `floor` of the GPU test's bar.

Second pass.  total_i = float32(float64(a_i) + float64(float32(lm_weight)) * g_i + float64(float32(bonus)) * n_i); the order lists
the first-pass ranks by total descending, ties to the smaller rank, then the entries without a score in rank order.
"""
import numpy as np

NEG = -1e30
DEAD = -1e29
LNP_TOL = 2e-6          # tests/test_gpu_ctc_per_utterance.py: LNP_TOL, the project's bar on ln p
FLOOR_FACTOR = 3.0      # ... and the factor on the fp32 restatement's own distance from fp64


def _logadd(a, b, dt):
    m, n = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(under="ignore", over="ignore"):      # (log(1 + e), as the device writes it, not log1p)
        return (m + np.log((dt(1) + np.exp((n - m).astype(dt))).astype(dt)).astype(dt)).astype(dt)


def lattice(labels):
    lab = np.zeros(2 * len(labels) + 1, np.int64)
    lab[1::2] = np.asarray(labels, np.int64)
    return lab


def final_cells(logp, labels, dtype=np.float64):
    """(alpha of the final blank, alpha of the final label or None for the empty labelling) after the last of n >= 1 frames."""
    dt = np.dtype(dtype).type
    lp = np.maximum(np.asarray(logp).astype(dt), dt(NEG))
    n = lp.shape[0]
    lab = lattice(labels)
    L = lab.size
    neg = dt(NEG)
    skip = np.zeros(L, bool)
    skip[3::2] = lab[3::2] != lab[1:-2:2]
    a = np.full(L, neg, dt)
    a[:2] = lp[0, lab[:2]]
    for t in range(1, n):
        a1 = np.concatenate([[neg], a[:-1]]).astype(dt)
        a2 = np.where(skip, np.concatenate([[neg, neg], a[:-2]])[:L], neg).astype(dt)
        acc = _logadd(a1, a, dt)
        acc = _logadd(a2, acc, dt)          # (the sentinel is the identity: even positions and repeats pass through)
        a = (lp[t, lab] + acc).astype(dt)
    return a[-1], (a[-2] if L >= 2 else None)


def lnp(logp, labels, dtype=np.float64):
    """a = ln p(labels | x) on logp [n x K] with the symmetric close, in `dtype`; -1e30 without a path."""
    dt = np.dtype(dtype).type
    n = np.asarray(logp).shape[0]
    if n == 0:
        return 0.0 if len(labels) == 0 else NEG
    b, l = final_cells(logp, labels, dtype)
    v = b if l is None else _logadd(np.array([b], dt), np.array([l], dt), dt)[0]
    v = float(v)
    return NEG if v <= DEAD else v


def figure(got, ref):
    """|got - ref| / max(1, |ref|): the ln p figure of tests/ctc_cases.py."""
    return abs(float(got) - float(ref)) / max(1.0, abs(float(ref)))


def bar(logp, labels, ref64=None):
    """(bar, floor, a64): max(LNP_TOL, 3 * floor) with floor the fp32 restatement's own figure against fp64 on this entry."""
    a64 = lnp(logp, labels, np.float64) if ref64 is None else ref64
    a32 = lnp(np.asarray(logp, np.float32), labels, np.float32)
    floor = figure(a32, a64)
    return max(LNP_TOL, FLOOR_FACTOR * floor), floor, a64


def total_of(a, g, n, lm_weight, bonus):
    """The stated fp64 expression on a (float32) acoustic score, rounded to float32."""
    return np.float32(float(np.float32(a)) + float(np.float32(lm_weight)) * float(g) + float(np.float32(bonus)) * int(n))


def rescore(am, g, n, lm_weight, bonus):
    """Python lists over the ranks of one utterance; am[i] None (or <= -1e29) marks an entry without a score.  Returns (totals, order):
    totals[i] float32 (-1e30 without a score), order the first-pass ranks as the second pass lists them."""
    N = len(am)
    ok = [am[i] is not None and float(am[i]) > DEAD for i in range(N)]
    totals = [total_of(am[i], g[i], n[i], lm_weight, bonus) if ok[i] else np.float32(NEG) for i in range(N)]
    return totals, order_of(totals, ok)


def order_of(totals, ok):
    ranked = sorted((i for i in range(len(totals)) if ok[i]), key=lambda i: (-float(totals[i]), i))
    return ranked + [i for i in range(len(totals)) if not ok[i]]


def min_gap(values):
    v = sorted(float(x) for x in values)
    return min((b - a for a, b in zip(v, v[1:])), default=float("inf"))
