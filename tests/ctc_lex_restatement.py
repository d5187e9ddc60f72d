"""The yardstick of the lexicon-constrained CTC prefix beam search (eesen_ctc_decode_parallel_lex, eesen_lex_*): INTEGRATION.md
"Lexicon" stated literally, on dictionaries keyed by label tuples -- no trie anywhere in this file, which is what holds the compile
step of csrc/lex.cpp.

  Lex          entries [(word name, spelling tuple)] in file order.  spell {spelling: word id}, ids 1 .. V in order of first
               appearance; prefixes: the set of every prefix of every spelling (the empty one included).
  partial(p)   the labels of p behind its last space; closed(p) the word ids of the spellings before it.  Both are functions of the
               label tuple alone, and so is everything the search knows about an entry.
  allowed      p + c for a unit c: partial(p) + (c,) is a prefix of a spelling; for the space: partial(p) is a spelling.
  complete     p is empty, or partial(p) is a spelling.  segment(p): the word ids of a complete p, None for any other tuple.
  beam_search  tests/ctc_lm_restatement.py's with `allowed`, g = alpha * w + beta on the space alone (w = cond(word, closed words) of
               tests/ctc_lm_restatement.Model over word ids, 0 without a model), g = 0 on a unit, and the end of the utterance:
               the last word closes, fin joins with eos, incomplete entries leave, the rest is re-ranked.  fp64 or fp32.

bar_s = bar_of(score64_s, n_s) + lm_term(model, alpha, words, eos): tests/ctc_lm_restatement.py's LM term with the words as its
labels -- one fp32 addition of an LM weight per word.  Without a model the term is 0.
"""
import functools
import os

import numpy as np

from tests import ctc_beam_restatement as R
from tests import ctc_lm_restatement as L

NEG, DEAD = R.NEG, R.DEAD
EOS = L.EOS


class Lex:
    def __init__(self, K, space, entries):
        self.K, self.space, self.entries = K, space, [(str(w), tuple(int(c) for c in sp)) for w, sp in entries]
        self.ids, self.spell = {}, {}
        for w, sp in self.entries:
            wid = self.ids.setdefault(w, len(self.ids) + 1)
            assert sp and all(1 <= c < K and c != space for c in sp) and self.spell.get(sp, wid) == wid
            self.spell[sp] = wid
        self.V = len(self.ids)
        self.prefixes = {sp[:i] for sp in self.spell for i in range(len(sp) + 1)}

    def partial(self, pre):
        pre = tuple(pre)
        return pre[len(pre) - pre[::-1].index(self.space):] if self.space in pre else pre

    def closed(self, pre):
        """Word ids of the spellings before the last space (the prefix is one the search can hold: they are all spellings)."""
        pre, out, cur = tuple(pre), [], ()
        for c in pre:
            if c == self.space:
                out.append(self.spell[cur])
                cur = ()
            else:
                cur += (c,)
        return tuple(out)

    def allowed(self, pre, c):
        part = self.partial(pre)
        return part in self.spell if c == self.space else part + (c,) in self.prefixes

    def complete(self, pre):
        return len(pre) == 0 or self.partial(pre) in self.spell

    def segment(self, pre):
        """The word ids of a labelling of L = {()} + {w1 Sp w2 ... Sp wn}, None for a tuple outside L."""
        pre = tuple(pre)
        if not pre:
            return ()
        parts, cur = [], ()
        for c in pre:
            if c == self.space:
                parts.append(cur)
                cur = ()
            else:
                cur += (c,)
        parts.append(cur)
        if any(p not in self.spell for p in parts):
            return None
        return tuple(self.spell[p] for p in parts)

    def spelling_of(self, words):
        """A labelling of the word ids (the first listed spelling of each)."""
        first = {}
        for sp, w in self.spell.items():
            first.setdefault(w, sp)
        out = ()
        for i, w in enumerate(words):
            out += (() if i == 0 else (self.space,)) + first[int(w)]
        return out

    def text(self, names=None):
        """The lexicon file: units as decimal ids, or through names [K]."""
        return "".join(w + " " + " ".join(str(c) if names is None else names[c] for c in sp) + "\n" for w, sp in self.entries)

    def write(self, directory, stem="lex", names=None):
        path = os.path.join(str(directory), stem + ".txt")
        with open(path, "w") as f:
            f.write(self.text(names))
        return path


def _cond(model, word, closed, dt):
    """(ln P(word | closed words), sum of |terms|) of the word model; (0, 0) without one."""
    if model is None:
        return dt(0), 0.0
    return model.cond(word, model.history(closed), dt)


def lm64(model, words, eos):
    return model.lm64(list(words), eos) if model is not None else (0.0, 0.0)


def beam_search(logp, sel32, B, C, lex, model, alpha, beta, eos, dtype=np.float64, jitter=None, with_live=False):
    """Returns the final beam, complete entries only, best first: [(labels, total, lmsum)]; with_live: (that, the best total among the
    live entries before the end of the utterance dropped the incomplete ones, or None if the beam died)."""
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
        w = np.zeros((nb, Cc), dt)                                   # lm_step of (entry, its node's word), on the space alone
        g = np.zeros((nb, Cc), dt)
        for ci in np.flatnonzero(cand == lex.space):
            for p, e in enumerate(beam):
                if ok[p, ci]:
                    w[p, ci] = _cond(model, lex.spell[lex.partial(e[0])], lex.closed(e[0]), dt)[0]
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
        keyed = total.astype(np.float64) + (rng.uniform(-jitter[1], jitter[1], size=total.size) if rng is not None else 0.0)
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
            wt = _cond(model, lex.spell[lex.partial(pre)], words, dt)[0]
            total = np.maximum(dt(total + dt(dt(al * wt) + be)), neg)
            ls = dt(ls + wt)
            words += (lex.spell[lex.partial(pre)],)
        if eos:
            f = dt(model.cond(EOS, model.history(words))[0])          # (fp64 sum, rounded once: the stored `final`)
            total = np.maximum(dt(total + dt(al * f)), neg)
            ls = dt(ls + f)
        out.append((pre, float(total), float(ls)))
    if out:
        keyed = np.array([o[1] for o in out]) + (rng.uniform(-jitter[1], jitter[1], size=len(out)) if rng is not None else 0.0)
        out = [out[i] for i in np.lexsort((np.arange(len(out)), -keyed))]
    return (out, live) if with_live else out


def lm_term(model, alpha, words, eos):
    """(|alpha| * x, x): tests/ctc_lm_restatement.py's term with one label per word; (0, 0) without a model."""
    return L.lm_term(model, alpha, list(words), eos) if model is not None else (0.0, 0.0)


def reference_of(lens, probs, S, B, C, lex, model, alpha, beta, eos, is_log=False):
    """Per utterance: dict(beam64 [(labels, score, lmsum)], score64, bar, beam32, stable, n).  stable: in the 8 jittered fp64 runs the
    1-best labelling is the unjittered one and its score moves by at most bar.  beam64 may be empty: no entry was complete.  Such an
    utterance is stable if the 8 runs, jittered by bar_of(the best live entry's total, n), all end without a complete entry too."""
    out = []
    for s in range(S):
        n = int(lens[s])
        p = R.utterance(probs, s, S, n)
        if is_log:
            l32 = np.maximum(np.asarray(p, np.float32), np.float32(NEG))
            l64 = l32.astype(np.float64)
        else:
            l32, l64 = R.log32(p), R.log64(p)
        b64, live = beam_search(l64, l32, B, C, lex, model, alpha, beta, eos, np.float64, with_live=True)
        b32 = beam_search(l32, l32, B, C, lex, model, alpha, beta, eos, np.float32)
        score64 = b64[0][1] if b64 else NEG
        bar = R.bar_of(score64, n) + lm_term(model, alpha, lex.segment(b64[0][0]), eos)[0] if b64 else 0.0
        stable = True
        for seed in R.JITTER_SEEDS if b64 else ():
            j = beam_search(l64, l32, B, C, lex, model, alpha, beta, eos, np.float64, jitter=(seed, bar))
            if not j or j[0][0] != b64[0][0] or abs(j[0][1] - score64) > bar:
                stable = False
                break
        if not b64 and live is not None:
            stable = not any(beam_search(l64, l32, B, C, lex, model, alpha, beta, eos, np.float64, jitter=(seed, R.bar_of(live, n))) for seed in R.JITTER_SEEDS)
        out.append(dict(beam64=b64, score64=score64, bar=bar, beam32=b32, stable=stable, n=n))
    return out


def exact_of(lex, model, alpha, beta, eos, lp64, labels):
    """The exact score of a labelling of L on fp64 log-scores: ln p + alpha * ln P_lm(words [, </s>]) + beta * |words|."""
    words = lex.segment(labels)
    return R.lnp64(lp64, labels) + alpha * lm64(model, words, eos)[0] + beta * len(words)


def enumerate_language(lex, lp64):
    """{labelling of L: ln sum over its paths} over all K^n paths (tiny cases), fp64."""
    return {h: v for h, v in R.enumerate_paths(lp64).items() if lex.segment(h) is not None}


def valid_prefixes(lex, n):
    """Every label tuple of at most n labels that the search can hold: each step allowed."""
    level, out = [()], [()]
    for _ in range(n):
        level = [p + (c,) for p in level for c in range(1, lex.K) if lex.allowed(p, c)]
        out += level
    return out


@functools.lru_cache(maxsize=None)
def lex_of(name):
    from tests import ctc_lex_cases as xc
    return xc.lexicon(name)


@functools.lru_cache(maxsize=None)
def model_of(name):
    from tests import ctc_lex_cases as xc
    return None if name is None else L.random_model(**xc.MODELS[name])


@functools.lru_cache(maxsize=None)
def case(key):
    """(lens, probs, T, S, lex, model, cfg, per-utterance references) of tests/ctc_lex_cases.py: CASES[key]; computed once, shared."""
    from tests import ctc_lex_cases as xc
    cfg = xc.CASES[key]
    lex = lex_of(cfg["lex"])
    lens, probs, T, S = xc.build(key)
    probs.setflags(write=False)
    m = model_of(cfg["model"])
    assert lex.K == probs.shape[1] and (m is None or m.K == lex.V + 1)
    return lens, probs, T, S, lex, m, cfg, reference_of(lens, probs, S, cfg["B"], cfg["C"], lex, m, cfg["alpha"], cfg["beta"], cfg["eos"])
