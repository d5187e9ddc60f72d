"""The yardstick of the CTC prefix beam search (eesen_ctc_decode_parallel): the computation of INTEGRATION.md "Decoding" stated
literally in numpy, with dictionaries keyed by label tuples.

Per utterance of n frames, log-scores s_t(k) clamped from below at -1e30, blank = class 0, beam = B, max_classes = C:

  candidates of a frame   the C' = min(C, K-1) non-blank classes with the largest s_t(k), ties to the smaller id (comparisons on the
                          fp32 values: exact)
  entry                   (prefix, lb, lnb); the beam starts as the empty prefix with lb = 0, lnb = -1e30
  frame t                 tot = logadd(lb, lnb), e = the prefix's last label
      stay of p           lb' = s_t(0) + tot, lnb' = s_t(e) + lnb (-1e30 for the empty prefix)
      extension p + c     lb' = -1e30, lnb' = s_t(c) + (c == e ? lb : tot), for every candidate c
      merge               p + c in the beam as q: its lnb' is log-added into q's stay, it is no candidate of its own
  selection               total = logadd(lb', lnb'); <= -1e29 is dead; the B largest survive -- higher total first, then stays before
                          extensions, stays by previous rank, extensions by parent's rank, then by class id

Sums are clamped from below at -1e30 (unobservable: everything at or below -1e29 is dead; it keeps fp32 away from -inf).
`jitter = (seed, bar)`: every selection compares total + u, u uniform in [-bar, bar] -- the stability figure of the GPU test.

bar_s = 64 * 2^-24 * |score64_s| + 4e-7 * sqrt(n_s)  (tests/test_ctc_beam_restatement.py says why).
"""
import functools
import itertools

import numpy as np

NEG = -1e30
DEAD = -1e29
BAR_REL = 64.0 * 2.0 ** -24
BAR_STEP = 4e-7
JITTER_SEEDS = tuple(range(8))


def bar_of(score64, n):
    return BAR_REL * abs(float(score64)) + BAR_STEP * float(np.sqrt(n))


def log32(p):
    with np.errstate(divide="ignore"):
        return np.maximum(np.log(np.asarray(p, np.float32), dtype=np.float32), np.float32(NEG))


def log64(p):
    with np.errstate(divide="ignore"):
        return np.maximum(np.log(np.asarray(p, np.float64)), NEG)


def utterance(a, s, S, n):
    """Rows of utterance s (its first n frames) of a [T*S x K] matrix."""
    return np.asarray(a)[s:n * S:S]


def candidates(row32, C):
    """Class ids (ascending) of the min(C, K-1) largest non-blank fp32 scores of one frame, ties to the smaller id."""
    K = row32.shape[0]
    Cc = min(C, K - 1)
    ids = np.arange(1, K)
    order = np.lexsort((ids, -row32[1:].astype(np.float64)))     # (exact: float32 -> float64)
    return np.sort(ids[order[:Cc]])


def _logadd(a, b, dt):
    m, n = np.maximum(a, b), np.minimum(a, b)
    return (m + np.log1p(np.exp((n - m).astype(dt)))).astype(dt)


def beam_search(logp, sel32, B, C, dtype=np.float64, jitter=None):
    """logp [n x K]: the log-scores the arithmetic runs on (dtype); sel32 [n x K] float32: the values the class selection compares.
    Returns the final beam, best first: list of (labels tuple, total)."""
    dt = np.dtype(dtype).type
    lp = np.maximum(np.asarray(logp).astype(dt), dt(NEG))
    n, K = lp.shape
    neg = dt(NEG)
    rng = np.random.default_rng(jitter[0]) if jitter is not None else None
    add = lambda a, b: np.maximum((a + b).astype(dt), neg)
    beam = [((), dt(0), neg)]
    for t in range(n):
        cand = candidates(np.asarray(sel32[t], np.float32), C)
        Cc = cand.size
        nb = len(beam)
        index = {pre: p for p, (pre, _, _) in enumerate(beam)}
        lb = np.array([e[1] for e in beam], dt)
        lnb = np.array([e[2] for e in beam], dt)
        last = np.array([e[0][-1] if e[0] else -1 for e in beam], np.int64)
        tot = _logadd(lb, lnb, dt)
        stay_lb = add(lp[t, 0], tot)
        stay_lnb = np.where(last >= 0, add(lp[t, np.maximum(last, 0)], lnb), neg).astype(dt)
        ext = add(lp[t, cand][None, :], np.where(cand[None, :] == last[:, None], lb[:, None], tot[:, None]))      # [nb x C']
        merged = np.zeros((nb, Cc), bool)
        for q, (pre, _, _) in enumerate(beam):
            if not pre:
                continue
            p = index.get(pre[:-1])
            ci = int(np.searchsorted(cand, pre[-1]))
            if p is not None and ci < Cc and cand[ci] == pre[-1]:
                stay_lnb[q] = _logadd(stay_lnb[q], ext[p, ci], dt)
                merged[p, ci] = True
        total = np.concatenate([_logadd(stay_lb, stay_lnb, dt), ext.reshape(-1)]).astype(dt)
        tie = np.concatenate([np.arange(nb), 64 + np.arange(nb * Cc)])
        alive = np.concatenate([np.ones(nb, bool), ~merged.reshape(-1)]) & (total > DEAD)
        keyed = total.astype(np.float64) + (rng.uniform(-jitter[1], jitter[1], size=total.size) if rng is not None else 0.0)
        idx = np.flatnonzero(alive)
        idx = idx[np.lexsort((tie[idx], -keyed[idx]))][:B]
        new = []
        for i in idx:
            if i < nb:
                new.append((beam[i][0], stay_lb[i], stay_lnb[i]))
            else:
                p, ci = divmod(int(i) - nb, Cc)
                new.append((beam[p][0] + (int(cand[ci]),), neg, ext[p, ci]))
        beam = new
        if not beam:
            break
    out = [(pre, float(_logadd(np.array([lb_], dt), np.array([lnb_], dt), dt)[0])) for pre, lb_, lnb_ in beam]
    return out


def lnp64(logp, labels):
    """The exact CTC forward log-probability of a labelling (blank = 0) on logp [n x K], fp64."""
    lp = np.maximum(np.asarray(logp, np.float64), NEG)
    n = lp.shape[0]
    lab = np.zeros(2 * len(labels) + 1, np.int64)
    lab[1::2] = np.asarray(labels, np.int64)
    L = lab.size
    if n == 0:
        return 0.0 if L == 1 else NEG
    skip = np.zeros(L, bool)
    skip[3::2] = lab[3::2] != lab[1:-2:2]
    a = np.full(L, -np.inf)
    a[:2] = lp[0, lab[:2]]
    for t in range(1, n):
        a1 = np.concatenate([[-np.inf], a])[:L]
        a2 = np.where(skip, np.concatenate([[-np.inf, -np.inf], a])[:L], -np.inf)
        a = lp[t, lab] + np.logaddexp(np.logaddexp(a, a1), a2)
    v = np.logaddexp(a[-1], a[-2]) if L >= 2 else a[-1]
    return float(max(v, NEG))


def collapse(path):
    out, prev = [], 0
    for c in path:
        if c != 0 and c != prev:
            out.append(int(c))
        prev = c
    return tuple(out)


def enumerate_paths(logp):
    """{labelling: ln sum over its paths} over all K^n paths (tiny cases), fp64."""
    lp = np.asarray(logp, np.float64)
    n, K = lp.shape
    acc = {}
    for path in itertools.product(range(K), repeat=n):
        v = float(sum(lp[t, c] for t, c in enumerate(path)))
        key = collapse(path)
        acc[key] = np.logaddexp(acc[key], v) if key in acc else v
    return acc


def reference_of(lens, probs, S, B, C, is_log=False):
    """Per utterance: dict(beam64 [(labels, score)], score64, bar, beam32, stable, n).  `probs`: float32 posteriors, or log-scores with
    is_log.  stable: in the 8 jittered fp64 runs the 1-best labelling is the unjittered one and its score moves by at most bar."""
    out = []
    for s in range(S):
        n = int(lens[s])
        p = utterance(probs, s, S, n)
        if is_log:
            l32 = np.maximum(np.asarray(p, np.float32), np.float32(NEG))
            l64 = l32.astype(np.float64)
        else:
            l32, l64 = log32(p), log64(p)
        b64 = beam_search(l64, l32, B, C, np.float64)
        b32 = beam_search(l32, l32, B, C, np.float32)
        score64 = b64[0][1] if b64 else NEG
        bar = bar_of(score64, n) if b64 else 0.0
        stable = True
        for seed in JITTER_SEEDS if b64 else ():
            j = beam_search(l64, l32, B, C, np.float64, jitter=(seed, bar))
            if not j or j[0][0] != b64[0][0] or abs(j[0][1] - score64) > bar:
                stable = False
                break
        out.append(dict(beam64=b64, score64=score64, bar=bar, beam32=b32, stable=stable, n=n))
    return out


@functools.lru_cache(maxsize=None)
def case(name, B, C):
    """(lens, probs, T, S, per-utterance references) of a tests/ctc_decode_cases.py case at (B, C); computed once, shared, not to be changed."""
    from tests import ctc_decode_cases as dc
    lens, probs, T, S = dc.build(name)
    probs.setflags(write=False)
    return lens, probs, T, S, reference_of(lens, probs, S, B, C)
