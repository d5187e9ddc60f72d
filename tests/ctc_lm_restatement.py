"""The yardstick of the LM-fused CTC prefix beam search (eesen_ctc_decode_parallel_lm, eesen_lm_*): INTEGRATION.md "LM fusion" stated
literally, on plain dictionaries of n-gram tuples -- no automaton anywhere in this file, which is what holds the compile step of
csrc/lm.cpp.

  Model        grams {tuple of symbols: (log10 value, log10 backoff or None)}; a symbol is a class id (int, 1 .. K-1) or one of the
               strings "<s>", "</s>", "<unk>".  The arithmetic runs on the stored values float32(v * ln 10), as the library's does.
  cond(w, h)   the textbook ARPA definition: the listed value of h.w if there is one, else bo(h) + cond(w, h[1:]) with bo = 0 for an
               unlisted h; at the empty history an unlisted word falls to <unk>.  Accumulated as acc = 0; acc += bo ...; acc + value.
  lm64         ln P(labels [, </s>]) = sum of cond(label_i, last N-1 symbols of <s> . labels[:i]), and the absolute sum of every
               value and backoff weight that went into it.
  beam_search  tests/ctc_beam_restatement.py's, with g = alpha * w + beta joining every extension, the unweighted LM sum carried per
               entry, and the re-rank on alpha * ln P(</s> | labels) at the end.  fp64 or fp32, the same `jitter`.
  random_model a seeded generator of backoff models (not normalised: only the arithmetic is under test) and their ARPA text.

bar_s = bar_of(score64_s, n_s) + |alpha| * (len + order + 1) * 2^-23 * sum|terms|: each of the len + order fp32 additions of LM
weights rounds to 2^-24 of a partial sum that sum|terms| bounds, and a factor 2 covers the fp32 storage of the weights.  The same
expression without |alpha| bounds an entry's lm_score against eesen_lm_score.
"""
import functools
import os

import numpy as np

from tests import ctc_beam_restatement as R

NEG, DEAD = R.NEG, R.DEAD
LN10 = float(np.log(10.0))
BOS, EOS, UNK = "<s>", "</s>", "<unk>"


class Model:
    def __init__(self, K, order, grams, names=None):
        self.K, self.order, self.grams, self.names = K, order, dict(grams), names
        self.p = {g: float(np.float32(v * LN10)) for g, (v, _) in self.grams.items()}
        self.bo = {g: float(np.float32(b * LN10)) for g, (_, b) in self.grams.items() if b is not None}
        self.has_eos = (EOS,) in self.grams
        self._rows = {}

    # ---- the textbook definition
    def cond(self, w, h, dt=np.float64):
        """(ln P(w | h), sum of |terms|); h is cut to its last order - 1 symbols."""
        h = tuple(h)[-(self.order - 1):] if self.order > 1 else ()
        acc, absum = dt(0), 0.0
        while True:
            g = h + (w,)
            if g in self.p:
                return dt(acc + dt(self.p[g])), absum + abs(self.p[g])
            if not h:
                v = self.p[(UNK,)]              # (KeyError: the model covers neither the word nor <unk>)
                return dt(acc + dt(v)), absum + abs(v)
            b = self.bo.get(h, 0.0)
            acc = dt(acc + dt(b))
            absum += abs(b)
            h = h[1:]

    def history(self, labels):
        return ((BOS,) + tuple(labels))[-(self.order - 1):] if self.order > 1 else ()

    def row(self, h, dt):
        """cond(c, h) for every class c (index c; index 0 unused), cached."""
        key = (h, np.dtype(dt).char)
        r = self._rows.get(key)
        if r is None:
            r = np.zeros(self.K, dt)
            for c in range(1, self.K):
                r[c] = self.cond(c, h, dt)[0]
            self._rows[key] = r
        return r

    def lm64(self, labels, eos=False):
        """(ln P(labels [, </s>]), sum of |terms|), fp64."""
        tot, absum = 0.0, 0.0
        for i, c in enumerate(labels):
            v, a = self.cond(int(c), self.history(labels[:i]))
            tot += float(v)
            absum += a
        if eos:
            v, a = self.cond(EOS, self.history(labels))
            tot += float(v)
            absum += a
        return tot, absum

    # ---- the files
    def word(self, sym):
        if isinstance(sym, str):
            return sym
        return self.names[sym] if self.names is not None else str(sym)

    def arpa_text(self):
        by = [[] for _ in range(self.order + 1)]
        for g in self.grams:
            by[len(g)].append(g)
        out = ["", "\\data\\"] + [f"ngram {n}={len(by[n])}" for n in range(1, self.order + 1)] + [""]
        for n in range(1, self.order + 1):
            out.append(f"\\{n}-grams:")
            for g in sorted(by[n], key=lambda g: tuple(map(str, g))):
                v, b = self.grams[g]
                out.append("\t".join([repr(float(v)), " ".join(self.word(s) for s in g)] + ([repr(float(b))] if b is not None else [])))
            out.append("")
        out.append("\\end\\")
        return "\n".join(out) + "\n"

    def units_text(self):
        return "".join(f"{self.names[c]} {c}\n" for c in range(1, self.K))

    def write(self, directory, stem="lm"):
        """(arpa path, units path or None)"""
        arpa = os.path.join(str(directory), stem + ".arpa")
        with open(arpa, "w") as f:
            f.write(self.arpa_text())
        units = None
        if self.names is not None:
            units = os.path.join(str(directory), stem + ".units.txt")
            with open(units, "w") as f:
                f.write(self.units_text())
        return arpa, units


def random_model(seed, K, order, per_order=None, missing=(), unk=True, bos=True, eos=True, named=False, fill=None):
    """A random backoff model over classes 1 .. K-1.  missing: classes without a unigram (they take <unk>'s, if unk).  per_order: how
    many n-grams to draw for n = 2 .. order.  Every n-gram's (n-1)-word prefix is listed (the format demands it), its suffix need not
    be; about a third of the backoff weights are positive, a fifth are left out of the file; named: a units table renames the tokens
    and spells one of them <UNK>.  fill: the largest share of all (context, successor) pairs an order may list (2/3 by default)."""
    rng = np.random.default_rng(seed)
    val = lambda: round(float(rng.uniform(-3.0, -0.05)), 4)
    bow = lambda: None if rng.random() < 0.2 else round(float(rng.uniform(-1.0, 0.5)), 4)
    grams = {}
    top = order == 1
    for c in range(1, K):
        if c not in missing:
            grams[(c,)] = (val(), None if top else bow())
    if bos:
        grams[(BOS,)] = (-99.0, None if top else round(float(rng.uniform(-1.0, 0.5)), 4))
    if eos:
        grams[(EOS,)] = (val(), None)
    if unk:
        grams[(UNK,)] = (val(), None if top else bow())
    succ = [c for c in range(1, K)] + ([EOS] if eos else [])
    prev = [g for g in grams if g[-1] not in (EOS, UNK)]
    for n in range(2, order + 1):
        want = (per_order or {}).get(n, min(len(prev) * len(succ) // 3 + 1, 4000))
        want = min(want, len(prev) * len(succ) * 2 // 3 if fill is None else int(len(prev) * len(succ) * fill))
        new = {}
        while len(new) < want:
            g = prev[int(rng.integers(len(prev)))] + (succ[int(rng.integers(len(succ)))],)
            if g not in new:
                new[g] = (val(), None if n == order else bow())
        grams.update(new)
        prev = [g for g in new if g[-1] != EOS]
    names = None
    if named:
        perm = rng.permutation(K - 1)
        names = [None] + [f"tok{int(perm[c - 1])}" for c in range(1, K)]
        names[1 + int(rng.integers(K - 1))] = "<UNK>"
    return Model(K, order, grams, names)


def features(m):
    """What of the issue's list a generated model exercises (the CPU test asserts it on the models it uses)."""
    g = m.grams
    return dict(
        positive_backoff=any(b is not None and b > 0 for _, b in g.values()),
        suffix_unlisted=any(len(x) >= 2 and x[1:] not in g for x in g),
        bos_context=any(len(x) >= 2 and x[0] == BOS for x in g),
        eos_successor=any(len(x) >= 2 and x[-1] == EOS for x in g),
        missing_at_every_depth=m.order == 1 or any(
            all((h[i:] + (c,)) not in g for i in range(len(h))) for h in g if len(h) == m.order - 1 and h[-1] not in (EOS, UNK) for c in range(1, m.K)),
    )


def _logadd(a, b, dt):
    return R._logadd(a, b, dt)


def beam_search(logp, sel32, B, C, model, alpha, beta, eos, dtype=np.float64, jitter=None):
    """tests/ctc_beam_restatement.py: beam_search with the LM.  Returns the final beam, best first: [(labels, total, lmsum)]."""
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
        w = np.stack([model.row(model.history(e[0]), dt)[cand] for e in beam]).astype(dt)          # [nb x C']: lm_step of (entry, class)
        g = ((al * w).astype(dt) + be).astype(dt)
        tot = _logadd(lb, lnb, dt)
        stay_lb = add(lp[t, 0], tot)
        stay_lnb = np.where(last >= 0, add(lp[t, np.maximum(last, 0)], lnb), neg).astype(dt)
        ext = add(add(lp[t, cand][None, :], g), np.where(cand[None, :] == last[:, None], lb[:, None], tot[:, None]))
        merged = np.zeros((nb, Cc), bool)
        for q, (pre, _, _, _) in enumerate(beam):
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
                new.append((beam[i][0], stay_lb[i], stay_lnb[i], beam[i][3]))
            else:
                p, ci = divmod(int(i) - nb, Cc)
                new.append((beam[p][0] + (int(cand[ci]),), neg, ext[p, ci], dt(beam[p][3] + w[p, ci])))
        beam = new
        if not beam:
            break
    out = []
    for pre, lb_, lnb_, ls in beam:
        total = _logadd(np.array([lb_], dt), np.array([lnb_], dt), dt)[0]
        if eos:
            f = dt(model.cond(EOS, model.history(pre))[0])          # (fp64 sum, rounded once: the stored `final`)
            total = np.maximum(dt(total + dt(al * f)), neg)
            ls = dt(ls + f)
        out.append((pre, float(total), float(ls)))
    if eos and out:
        keyed = np.array([o[1] for o in out]) + (rng.uniform(-jitter[1], jitter[1], size=len(out)) if rng is not None else 0.0)
        out = [out[i] for i in np.lexsort((np.arange(len(out)), -keyed))]
    return out


def lm_term(model, alpha, labels, eos):
    """(|alpha| * x, x), x = (len + order + 1) * 2^-23 * sum|terms| of the labelling's LM walk."""
    _, absum = model.lm64(labels, eos)
    x = (len(labels) + model.order + 1) * 2.0 ** -23 * absum
    return abs(alpha) * x, x


def reference_of(lens, probs, S, B, C, model, alpha, beta, eos, is_log=False):
    """Per utterance: dict(beam64 [(labels, score, lmsum)], score64, bar, beam32, stable, n).  stable: in the 8 jittered fp64 runs the
    1-best labelling is the unjittered one and its score moves by at most bar."""
    out = []
    for s in range(S):
        n = int(lens[s])
        p = R.utterance(probs, s, S, n)
        if is_log:
            l32 = np.maximum(np.asarray(p, np.float32), np.float32(NEG))
            l64 = l32.astype(np.float64)
        else:
            l32, l64 = R.log32(p), R.log64(p)
        b64 = beam_search(l64, l32, B, C, model, alpha, beta, eos, np.float64)
        b32 = beam_search(l32, l32, B, C, model, alpha, beta, eos, np.float32)
        score64 = b64[0][1] if b64 else NEG
        bar = R.bar_of(score64, n) + lm_term(model, alpha, b64[0][0], eos)[0] if b64 else 0.0
        stable = True
        for seed in R.JITTER_SEEDS if b64 else ():
            j = beam_search(l64, l32, B, C, model, alpha, beta, eos, np.float64, jitter=(seed, bar))
            if not j or j[0][0] != b64[0][0] or abs(j[0][1] - score64) > bar:
                stable = False
                break
        out.append(dict(beam64=b64, score64=score64, bar=bar, beam32=b32, stable=stable, n=n))
    return out


def entry_bar(model, alpha, beta, eos, lp64, labels, n):
    """(the exact fused score of a labelling on fp64 log-scores, its bar)."""
    lm, _ = model.lm64(labels, eos)
    exact = R.lnp64(lp64, labels) + alpha * lm + beta * len(labels)
    return exact, R.bar_of(exact, n) + lm_term(model, alpha, labels, eos)[0]


@functools.lru_cache(maxsize=None)
def model_of(name):
    from tests import ctc_lm_cases as lc
    return random_model(**lc.MODELS[name])


@functools.lru_cache(maxsize=None)
def case(key):
    """(lens, probs, T, S, model, cfg, per-utterance references) of tests/ctc_lm_cases.py: CASES[key]; computed once, shared."""
    from tests import ctc_decode_cases as dc
    from tests import ctc_lm_cases as lc
    cfg = lc.CASES[key]
    lens, probs, T, S = dc.build(cfg["case"])
    probs.setflags(write=False)
    m = model_of(cfg["model"])
    assert m.K == probs.shape[1]
    return lens, probs, T, S, m, cfg, reference_of(lens, probs, S, cfg["B"], cfg["C"], m, cfg["alpha"], cfg["beta"], cfg["eos"])
