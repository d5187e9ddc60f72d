"""The yardstick of the CTC word beam search along a lexicon without a boundary unit (eesen_ctc_decode_parallel_words,
eesen_lex_create_unspaced): INTEGRATION.md "Words without a boundary unit" stated literally, on dictionaries keyed by tuples of
augmented symbols -- no trie and no fingerprint anywhere in this file, which is what holds csrc/lex.cpp's compile step and the
kernel's merge.

  WLex         entries [(word name, spelling tuple)] in file order.  spell {spelling: ascending word ids}, ids 1 .. V in order of
               first appearance; prefixes: the set of every prefix of every spelling; H: the largest word list.
  hypothesis   a tuple of units (ints) and closing marks ("#", w).  split(hyp) -> (labels, words, ends): ends[j] is the number of
               labels up to and including word j's last.  partial(hyp): the units behind the last mark.
  successors   of entry p and candidate class c, in slot order: slot 0 p + c if partial(p) + c is a prefix of a spelling; slot 1 + i
               p + #w + c for the i-th word w of spell[partial(p)], if c starts a spelling; g = alpha * w_lm + beta on a close alone.
  beam_search  tests/ctc_lex_restatement.py's shape with these successors; the end of the utterance fans a complete entry out into one
               final hypothesis per word of its spelling.  fp64 or fp32, the same `jitter`.

bar_s = bar_of(score64_s, n_s) + lm_term(model, alpha, words, eos), as in tests/ctc_lex_restatement.py.
"""
import functools
import os

import numpy as np

from tests import ctc_beam_restatement as R
from tests import ctc_lex_restatement as X
from tests import ctc_lm_restatement as L

NEG, DEAD = R.NEG, R.DEAD
EOS = L.EOS
lm_term, lm64 = X.lm_term, X.lm64


def mark(w):
    return ("#", int(w))


def is_mark(x):
    return isinstance(x, tuple)


def split(hyp):
    """(labels, words, ends) of an augmented sequence; a trailing run without a mark belongs to no word."""
    labels, words, ends = [], [], []
    for x in hyp:
        if is_mark(x):
            words.append(x[1])
            ends.append(len(labels))
        else:
            labels.append(x)
    return tuple(labels), tuple(words), tuple(ends)


def partial(hyp):
    i = len(hyp)
    while i > 0 and not is_mark(hyp[i - 1]):
        i -= 1
    return tuple(hyp[i:])


class WLex:
    def __init__(self, K, entries):
        self.K, self.entries = K, [(str(w), tuple(int(c) for c in sp)) for w, sp in entries]
        self.ids, spell = {}, {}
        for w, sp in self.entries:
            wid = self.ids.setdefault(w, len(self.ids) + 1)
            assert sp and all(1 <= c < K for c in sp)
            spell.setdefault(sp, set()).add(wid)
        self.spell = {sp: sorted(ws) for sp, ws in spell.items()}
        self.V = len(self.ids)
        self.H = max(len(ws) for ws in self.spell.values())
        self.prefixes = {sp[:i] for sp in self.spell for i in range(len(sp) + 1)}

    def spellings_of(self, word):
        return [sp for sp, ws in self.spell.items() if word in ws]

    def text(self, names=None):
        return "".join(w + " " + " ".join(str(c) if names is None else names[c] for c in sp) + "\n" for w, sp in self.entries)

    def write(self, directory, stem="wlex", names=None):
        path = os.path.join(str(directory), stem + ".txt")
        with open(path, "w") as f:
            f.write(self.text(names))
        return path

    def consistent(self, labels, words, ends):
        """The labels are the concatenation of spellings of the words, cut at the ends."""
        if len(words) != len(ends) or (len(ends) and ends[-1] != len(labels)) or (not len(ends) and len(labels)):
            return False
        at = 0
        for w, e in zip(words, ends):
            if e <= at or int(w) not in self.spell.get(tuple(labels[at:e]), ()):
                return False
            at = e
        return True


def _cond(model, word, closed, dt):
    if model is None:
        return dt(0)
    return model.cond(word, model.history(closed), dt)[0]


def beam_search(logp, sel32, B, C, lex, model, alpha, beta, eos, dtype=np.float64, jitter=None, with_live=False, live_count=None, walk_count=None):
    """Returns the final hypotheses, best first: [(hypothesis ending in a mark, or (), total, lmsum)]; with_live: (that, the best
    total among the live entries before the end of the utterance, or None if the beam died).  live_count: a list that takes the
    number of live candidates of every frame before the cut to B; walk_count: one that takes the frame's number of (entry, word of
    its node) pairs, the LM walks of step 0."""
    dt = np.dtype(dtype).type
    lp = np.maximum(np.asarray(logp).astype(dt), dt(NEG))
    n, K = lp.shape
    neg = dt(NEG)
    al, be = dt(alpha), dt(beta)
    rng = np.random.default_rng(jitter[0]) if jitter is not None else None
    add = lambda a, b: np.maximum(dt(a + b), neg)
    ladd = lambda a, b: L._logadd(np.array([a], dt), np.array([b], dt), dt)[0]
    H1 = 1 + lex.H
    beam = [((), dt(0), neg, dt(0))]
    for t in range(n):
        cand = R.candidates(np.asarray(sel32[t], np.float32), C)
        Cc = cand.size
        nb = len(beam)
        index = {hyp: p for p, (hyp, _, _, _) in enumerate(beam)}
        starts = [(int(c),) in lex.prefixes for c in cand]          # the root's child
        succ = {}                                                   # (p, ci, slot) -> (value, word or 0, its LM weight)
        stay_lb, stay_lnb = [], []
        if walk_count is not None:
            walk_count.append(sum(len(lex.spell.get(partial(hyp), ())) for hyp, _, _, _ in beam))
        for p, (hyp, lb, lnb, _) in enumerate(beam):
            labels, words, _ = split(hyp)
            last = labels[-1] if labels else -1
            part = partial(hyp)
            here = lex.spell.get(part, [])
            wts = [_cond(model, w, words, dt) for w in here]        # lm_step of (entry, word of its node)
            tot = ladd(lb, lnb)
            stay_lb.append(add(lp[t, 0], tot))
            stay_lnb.append(add(lp[t, last], lnb) if last >= 0 else neg)
            for ci, c in enumerate(cand):
                c = int(c)
                base = lb if c == last else tot
                if part + (c,) in lex.prefixes:
                    succ[(p, ci, 0)] = (add(add(lp[t, c], dt(0)), base), 0, dt(0))
                if starts[ci]:
                    for i, w in enumerate(here):
                        g = dt(dt(al * wts[i]) + be)
                        succ[(p, ci, 1 + i)] = (add(add(lp[t, c], g), base), w, wts[i])
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
        items = [(ladd(stay_lb[q], stay_lnb[q]), q, None) for q in range(nb)]
        items += [(v[0], 64 + (k[0] * Cc + k[1]) * H1 + k[2], k) for k, v in sorted(succ.items()) if k not in merged]
        total = np.array([it[0] for it in items], np.float64)
        keyed = total + (rng.uniform(-jitter[1], jitter[1], size=total.size) if rng is not None else 0.0)
        tie = np.array([it[1] for it in items])
        idx = np.flatnonzero(total > DEAD)
        if live_count is not None:
            live_count.append(idx.size)
        idx = idx[np.lexsort((tie[idx], -keyed[idx]))][:B]
        new = []
        for i in idx:
            _, _, k = items[i]
            if k is None:
                q = items[i][1]
                new.append((beam[q][0], stay_lb[q], stay_lnb[q], beam[q][3]))
            else:
                p, ci, slot = k
                v, w, wt = succ[k]
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
                wt = _cond(model, w, words, dt)
                total = np.maximum(dt(total + dt(dt(al * wt) + be)), neg)
                ls = dt(ls + wt)
                closed = words + (w,)
            if eos:
                f = dt(model.cond(EOS, model.history(closed))[0])          # (fp64 sum, rounded once: the stored `final`)
                total = np.maximum(dt(total + dt(al * f)), neg)
                ls = dt(ls + f)
            out.append((hyp + ((mark(w),) if w is not None else ()), float(total), float(ls)))
    if out:
        keyed = np.array([o[1] for o in out]) + (rng.uniform(-jitter[1], jitter[1], size=len(out)) if rng is not None else 0.0)
        out = [out[i] for i in np.lexsort((np.arange(len(out)), -keyed))]
    return (out, live) if with_live else out


def reference_of(lens, probs, S, B, C, lex, model, alpha, beta, eos, is_log=False):
    """Per utterance: dict(beam64 [(hypothesis, score, lmsum)], score64, bar, beam32, stable, n), as tests/ctc_lex_restatement.py's:
    stable: in the 8 jittered fp64 runs the 1-best hypothesis (labels, words and ends) is the unjittered one and its score moves by at
    most bar; an utterance without a complete entry is stable if the jittered runs have none either."""
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
        bar = R.bar_of(score64, n) + lm_term(model, alpha, split(b64[0][0])[1], eos)[0] if b64 else 0.0
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


def exact_of(model, alpha, beta, eos, lp64, labels, words):
    """ln p(labels) + alpha * ln P_lm(words [, </s>]) + beta * |words| on fp64 log-scores."""
    return R.lnp64(lp64, labels) + alpha * lm64(model, words, eos)[0] + beta * len(words)


def segmentations(lex, labels):
    """Every hypothesis (ending in a mark, or empty) whose labels are `labels`."""
    labels = tuple(labels)
    if not labels:
        return [()]
    out = []

    def walk(at, hyp):
        if at == len(labels):
            out.append(hyp)
            return
        for e in range(at + 1, len(labels) + 1):
            for w in lex.spell.get(labels[at:e], ()):
                walk(e, hyp + labels[at:e] + (mark(w),))
    walk(0, ())
    return out


def enumerate_hypotheses(lex, lp64):
    """{complete hypothesis: ln sum over the paths of its labels} over all K^n paths (tiny cases), fp64."""
    return {hyp: v for h, v in R.enumerate_paths(lp64).items() for hyp in segmentations(lex, h)}


@functools.lru_cache(maxsize=None)
def lex_of(name):
    from tests import ctc_words_cases as wc
    return wc.lexicon(name)


@functools.lru_cache(maxsize=None)
def model_of(name):
    from tests import ctc_words_cases as wc
    return None if name is None else L.random_model(**wc.MODELS[name])


@functools.lru_cache(maxsize=None)
def case(key):
    """(lens, probs, T, S, lex, model, cfg, per-utterance references) of tests/ctc_words_cases.py: CASES[key]; computed once, shared."""
    from tests import ctc_words_cases as wc
    cfg = wc.CASES[key]
    lex = lex_of(cfg["lex"])
    lens, probs, T, S = wc.build(key)
    probs.setflags(write=False)
    m = model_of(cfg["model"])
    assert lex.K == probs.shape[1] and (m is None or m.K == lex.V + 1)
    return lens, probs, T, S, lex, m, cfg, reference_of(lens, probs, S, cfg["B"], cfg["C"], lex, m, cfg["alpha"], cfg["beta"], cfg["eos"])
