"""The yardstick of the unigram LM look-ahead in the two lexicon searches (eesen_lex_lookahead, eesen_ctc_set_lm_lookahead):
INTEGRATION.md "LM look-ahead" stated literally, on dictionaries keyed by spelling prefixes -- no trie anywhere in this file.

  unigram(m, w)  float32 of the model's cond(w, empty history): the listed unigram, or <unk>'s for a word without one -- what
                 eesen_lm_step(lm, 0, w) returns.
  table(lex, m)  {spelling prefix: max unigram(w) over the words w with a spelling that starts with the prefix}; for a WLex every
                 word of a spelling counts.  The empty prefix holds the vocabulary's maximum.
  beam_search    tests/ctc_lex_restatement.py: beam_search with one more argument, `la` (such a table, or None): a frame's candidates
                 are ranked by max(total + eta, -1e30) + 0 with eta = (alpha * la[node] + beta), node the spelling prefix the candidate
                 stands on after the step (a stay: partial(p); a unit: partial(p) + c; the space: the empty prefix).  Alive is decided
                 on the real total, every carried value and the end of the utterance are the original's.  la=None returns exactly what
                 the original returns (tests/test_ctc_lookahead_cases.py holds that).
  word_search    tests/ctc_words_restatement.py: beam_search in the same way (inside successor: partial(p) + c; closing successor:
                 (c,), the root's child).
  `jitter` moves the rank keys, as it moves the totals in the originals.

reference_of / word_reference_of: the originals' `stable` rule and `bar`, with the table passed through.
"""
import functools

import numpy as np

from tests import ctc_beam_restatement as R
from tests import ctc_lex_restatement as X
from tests import ctc_lm_restatement as L
from tests import ctc_words_restatement as W

NEG, DEAD = R.NEG, R.DEAD
EOS = L.EOS


def unigram(model, w):
    return np.float32(model.cond(int(w), (), np.float32)[0])


def table(lex, model):
    """{prefix: la} in float32, by comparisons only."""
    assert model.K == lex.V + 1
    la = {}
    for sp, ws in lex.spell.items():
        for w in (ws if isinstance(ws, (list, tuple)) else (ws,)):
            u = unigram(model, w)
            for i in range(len(sp) + 1):
                if sp[:i] not in la or u > la[sp[:i]]:
                    la[sp[:i]] = u
    assert set(la) == set(lex.prefixes)
    return la


def _rank(total, node, la, al, be, dt):
    """The rank key of a candidate with the real total `total` that stands on `node`."""
    if la is None:
        return total
    eta = dt(dt(al * dt(la[node])) + be)
    return dt(np.maximum(dt(total + eta), dt(NEG)) + dt(0))


def beam_search(logp, sel32, B, C, lex, model, alpha, beta, eos, dtype=np.float64, jitter=None, with_live=False, la=None):
    """tests/ctc_lex_restatement.py: beam_search, the candidates of a frame ranked with `la`."""
    dt = np.dtype(dtype).type
    lp = np.maximum(np.asarray(logp).astype(dt), dt(NEG))
    n, K = lp.shape
    neg = dt(NEG)
    al, be = dt(alpha), dt(beta)
    rng = np.random.default_rng(jitter[0]) if jitter is not None else None
    add = lambda a, b: np.maximum((a + b).astype(dt), neg)
    beam = [((), dt(0), neg, dt(0))]
    for t in range(n):
        cand = R.candidates(np.asarray(sel32[t], np.float32), C)
        Cc = cand.size
        nb = len(beam)
        index = {pre: p for p, (pre, _, _, _) in enumerate(beam)}
        lb = np.array([e[1] for e in beam], dt)
        lnb = np.array([e[2] for e in beam], dt)
        last = np.array([e[0][-1] if e[0] else -1 for e in beam], np.int64)
        ok = np.array([[lex.allowed(e[0], int(c)) for c in cand] for e in beam], bool).reshape(nb, Cc)
        w = np.zeros((nb, Cc), dt)
        g = np.zeros((nb, Cc), dt)
        for ci in np.flatnonzero(cand == lex.space):
            for p, e in enumerate(beam):
                if ok[p, ci]:
                    w[p, ci] = X._cond(model, lex.spell[lex.partial(e[0])], lex.closed(e[0]), dt)[0]
            g[:, ci] = ((al * w[:, ci]).astype(dt) + be).astype(dt)
        tot = L._logadd(lb, lnb, dt)
        stay_lb = add(lp[t, 0], tot)
        stay_lnb = np.where(last >= 0, add(lp[t, np.maximum(last, 0)], lnb), neg).astype(dt)
        ext = add(add(lp[t, cand][None, :], g), np.where(cand[None, :] == last[:, None], lb[:, None], tot[:, None]))
        ext = np.where(ok, ext, neg).astype(dt)
        merged = np.zeros((nb, Cc), bool)
        for q, (pre, _, _, _) in enumerate(beam):
            if not pre:
                continue
            p = index.get(pre[:-1])
            ci = int(np.searchsorted(cand, pre[-1]))
            if p is not None and ci < Cc and cand[ci] == pre[-1]:
                stay_lnb[q] = L._logadd(stay_lnb[q], ext[p, ci], dt)
                merged[p, ci] = True
        total = np.concatenate([L._logadd(stay_lb, stay_lnb, dt), ext.reshape(-1)]).astype(dt)
        tie = np.concatenate([np.arange(nb), 64 + np.arange(nb * Cc)])
        alive = np.concatenate([np.ones(nb, bool), ~merged.reshape(-1)]) & (total > DEAD)
        rank = total.copy()
        if la is not None:
            for i in np.flatnonzero(alive):
                if i < nb:
                    node = lex.partial(beam[i][0])
                else:
                    p, ci = divmod(int(i) - nb, Cc)
                    node = () if cand[ci] == lex.space else lex.partial(beam[p][0]) + (int(cand[ci]),)
                rank[i] = _rank(total[i], node, la, al, be, dt)
        keyed = rank.astype(np.float64) + (rng.uniform(-jitter[1], jitter[1], size=total.size) if rng is not None else 0.0)
        idx = np.flatnonzero(alive)
        idx = idx[np.lexsort((tie[idx], -keyed[idx]))][:B]
        new = []
        for i in idx:
            if i < nb:
                new.append((beam[i][0], stay_lb[i], stay_lnb[i], beam[i][3]))
            else:
                p, ci = divmod(int(i) - nb, Cc)
                new.append((beam[p][0] + (int(cand[ci]),), neg, ext[p, ci], dt(beam[p][3] + w[p, ci])))
        beam = new
        if not beam:
            break
    out = []
    live = max((float(L._logadd(np.array([lb_], dt), np.array([lnb_], dt), dt)[0]) for _, lb_, lnb_, _ in beam), default=None)
    for pre, lb_, lnb_, ls in beam:
        if not lex.complete(pre):
            continue
        total = L._logadd(np.array([lb_], dt), np.array([lnb_], dt), dt)[0]
        words = lex.closed(pre)
        if pre:
            wt = X._cond(model, lex.spell[lex.partial(pre)], words, dt)[0]
            total = np.maximum(dt(total + dt(dt(al * wt) + be)), neg)
            ls = dt(ls + wt)
            words += (lex.spell[lex.partial(pre)],)
        if eos:
            f = dt(model.cond(EOS, model.history(words))[0])
            total = np.maximum(dt(total + dt(al * f)), neg)
            ls = dt(ls + f)
        out.append((pre, float(total), float(ls)))
    if out:
        keyed = np.array([o[1] for o in out]) + (rng.uniform(-jitter[1], jitter[1], size=len(out)) if rng is not None else 0.0)
        out = [out[i] for i in np.lexsort((np.arange(len(out)), -keyed))]
    return (out, live) if with_live else out


def word_search(logp, sel32, B, C, lex, model, alpha, beta, eos, dtype=np.float64, jitter=None, with_live=False, la=None):
    """tests/ctc_words_restatement.py: beam_search, the candidates of a frame ranked with `la`."""
    dt = np.dtype(dtype).type
    lp = np.maximum(np.asarray(logp).astype(dt), dt(NEG))
    n, K = lp.shape
    neg = dt(NEG)
    al, be = dt(alpha), dt(beta)
    rng = np.random.default_rng(jitter[0]) if jitter is not None else None
    add = lambda a, b: np.maximum(dt(a + b), neg)
    ladd = lambda a, b: L._logadd(np.array([a], dt), np.array([b], dt), dt)[0]
    split, partial, mark, is_mark = W.split, W.partial, W.mark, W.is_mark
    H1 = 1 + lex.H
    beam = [((), dt(0), neg, dt(0))]
    for t in range(n):
        cand = R.candidates(np.asarray(sel32[t], np.float32), C)
        Cc = cand.size
        nb = len(beam)
        index = {hyp: p for p, (hyp, _, _, _) in enumerate(beam)}
        starts = [(int(c),) in lex.prefixes for c in cand]
        succ = {}                                                   # (p, ci, slot) -> (value, word or 0, its LM weight, node behind it)
        stay_lb, stay_lnb = [], []
        for p, (hyp, lb, lnb, _) in enumerate(beam):
            labels, words, _ = split(hyp)
            last = labels[-1] if labels else -1
            part = partial(hyp)
            here = lex.spell.get(part, [])
            wts = [W._cond(model, w, words, dt) for w in here]
            tot = ladd(lb, lnb)
            stay_lb.append(add(lp[t, 0], tot))
            stay_lnb.append(add(lp[t, last], lnb) if last >= 0 else neg)
            for ci, c in enumerate(cand):
                c = int(c)
                base = lb if c == last else tot
                if part + (c,) in lex.prefixes:
                    succ[(p, ci, 0)] = (add(add(lp[t, c], dt(0)), base), 0, dt(0), part + (c,))
                if starts[ci]:
                    for i, w in enumerate(here):
                        g = dt(dt(al * wts[i]) + be)
                        succ[(p, ci, 1 + i)] = (add(add(lp[t, c], g), base), w, wts[i], (c,))
        merged = set()
        for q, (hyp, _, _, _) in enumerate(beam):
            if not hyp:
                continue
            e = hyp[-1]
            closed = len(hyp) >= 2 and is_mark(hyp[-2])
            parent = hyp[:-2] if closed else hyp[:-1]
            p = index.get(parent)
            ci = int(np.searchsorted(cand, e))
            if p is not None and ci < Cc and cand[ci] == e:
                slot = 1 + lex.spell[partial(parent)].index(hyp[-2][1]) if closed else 0
                stay_lnb[q] = ladd(stay_lnb[q], succ[(p, ci, slot)][0])
                merged.add((p, ci, slot))
        items = [(ladd(stay_lb[q], stay_lnb[q]), q, None, partial(beam[q][0])) for q in range(nb)]
        items += [(v[0], 64 + (k[0] * Cc + k[1]) * H1 + k[2], k, v[3]) for k, v in sorted(succ.items()) if k not in merged]
        total = np.array([it[0] for it in items], np.float64)
        alive = total > DEAD
        rank = np.array([float(_rank(dt(it[0]), it[3], la, al, be, dt)) if ok else float(it[0]) for it, ok in zip(items, alive)], np.float64)
        keyed = rank + (rng.uniform(-jitter[1], jitter[1], size=total.size) if rng is not None else 0.0)
        tie = np.array([it[1] for it in items])
        idx = np.flatnonzero(alive)
        idx = idx[np.lexsort((tie[idx], -keyed[idx]))][:B]
        new = []
        for i in idx:
            k = items[i][2]
            if k is None:
                q = items[i][1]
                new.append((beam[q][0], stay_lb[q], stay_lnb[q], beam[q][3]))
            else:
                p, ci, slot = k
                v, w, wt, _ = succ[k]
                step = ((mark(w),) if slot else ()) + (int(cand[ci]),)
                new.append((beam[p][0] + step, neg, v, dt(beam[p][3] + wt) if slot else beam[p][3]))
        beam = new
        if not beam:
            break
    out = []
    live = max((float(ladd(lb_, lnb_)) for _, lb_, lnb_, _ in beam), default=None)
    for hyp, lb_, lnb_, ls0 in beam:
        _, words, _ = split(hyp)
        for w in (lex.spell.get(partial(hyp), []) if hyp else [None]):
            total, ls, closed = ladd(lb_, lnb_), ls0, words
            if w is not None:
                wt = W._cond(model, w, words, dt)
                total = np.maximum(dt(total + dt(dt(al * wt) + be)), neg)
                ls = dt(ls + wt)
                closed = words + (w,)
            if eos:
                f = dt(model.cond(EOS, model.history(closed))[0])
                total = np.maximum(dt(total + dt(al * f)), neg)
                ls = dt(ls + f)
            out.append((hyp + ((mark(w),) if w is not None else ()), float(total), float(ls)))
    if out:
        keyed = np.array([o[1] for o in out]) + (rng.uniform(-jitter[1], jitter[1], size=len(out)) if rng is not None else 0.0)
        out = [out[i] for i in np.lexsort((np.arange(len(out)), -keyed))]
    return (out, live) if with_live else out


def _reference(search, words_of, lens, probs, S, B, C, lex, model, alpha, beta, eos, la):
    out = []
    for s in range(S):
        n = int(lens[s])
        p = R.utterance(probs, s, S, n)
        l32, l64 = R.log32(p), R.log64(p)
        b64, live = search(l64, l32, B, C, lex, model, alpha, beta, eos, np.float64, with_live=True, la=la)
        b32 = search(l32, l32, B, C, lex, model, alpha, beta, eos, np.float32, la=la)
        score64 = b64[0][1] if b64 else NEG
        bar = R.bar_of(score64, n) + X.lm_term(model, alpha, words_of(b64[0][0]), eos)[0] if b64 else 0.0
        stable = True
        for seed in R.JITTER_SEEDS if b64 else ():
            j = search(l64, l32, B, C, lex, model, alpha, beta, eos, np.float64, jitter=(seed, bar), la=la)
            if not j or j[0][0] != b64[0][0] or abs(j[0][1] - score64) > bar:
                stable = False
                break
        if not b64 and live is not None:
            stable = not any(search(l64, l32, B, C, lex, model, alpha, beta, eos, np.float64, jitter=(seed, R.bar_of(live, n)), la=la) for seed in R.JITTER_SEEDS)
        out.append(dict(beam64=b64, score64=score64, bar=bar, beam32=b32, stable=stable, n=n))
    return out


def reference_of(lens, probs, S, B, C, lex, model, alpha, beta, eos, la):
    """tests/ctc_lex_restatement.py: reference_of with the table (posteriors only)."""
    return _reference(beam_search, lex.segment, lens, probs, S, B, C, lex, model, alpha, beta, eos, la)


def word_reference_of(lens, probs, S, B, C, lex, model, alpha, beta, eos, la):
    """tests/ctc_words_restatement.py: reference_of with the table."""
    return _reference(word_search, lambda hyp: W.split(hyp)[1], lens, probs, S, B, C, lex, model, alpha, beta, eos, la)


@functools.lru_cache(maxsize=None)
def case(key):
    """(lens, probs, T, S, lex, model, cfg, la, per-utterance references with the look-ahead) of tests/ctc_lookahead_cases.py:
    CASES[key]; computed once, shared, never written to."""
    from tests import ctc_lookahead_cases as kc
    cfg = kc.CASES[key]
    lex, model = kc.lex_of(key), kc.model_of(cfg["model"])
    lens, probs, T, S = kc.build(key)
    probs.setflags(write=False)
    la = table(lex, model)
    ref_of = word_reference_of if cfg["unspaced"] else reference_of
    return lens, probs, T, S, lex, model, cfg, la, ref_of(lens, probs, S, cfg["B"], cfg["C"], lex, model, cfg["alpha"], cfg["beta"], cfg["eos"], la)


def best_scores(key, B, la_on, dtype=np.float64):
    """The restatement's 1-best score per utterance of CASES[key] at beam B (None where no entry is complete): the efficacy figures."""
    from tests import ctc_lookahead_cases as kc
    cfg = kc.CASES[key]
    lex, model = kc.lex_of(key), kc.model_of(cfg["model"])
    lens, probs, T, S = kc.build(key)
    la = table(lex, model) if la_on else None
    search = word_search if cfg["unspaced"] else beam_search
    out = []
    for s in range(S):
        p = R.utterance(probs, s, S, int(lens[s]))
        b = search(R.log64(p) if dtype == np.float64 else R.log32(p), R.log32(p), B, cfg["C"], lex, model, cfg["alpha"], cfg["beta"], cfg["eos"], dtype, la=la)
        out.append(b[0][1] if b else None)
    return out


def efficacy(on, off, bars):
    """(better, worse, sum on, sum off) of two lists of 1-best scores: better / worse by more than the utterance's bar; the sums over
    the utterances that have an entry both ways."""
    better = sum(1 for a, b, r in zip(on, off, bars) if a is not None and b is not None and a > b + r)
    worse = sum(1 for a, b, r in zip(on, off, bars) if a is not None and b is not None and a < b - r)
    both = [(a, b) for a, b in zip(on, off) if a is not None and b is not None]
    return better, worse, sum(a for a, _ in both), sum(b for _, b in both)
