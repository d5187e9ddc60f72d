"""Word models, minibatches and configurations of the LM look-ahead tests (tests/test_ctc_lookahead_cases.py on the CPU,
tests/test_gpu_ctc_decode_lookahead.py on the GPU), on the lexicons of tests/ctc_lex_cases.py and tests/ctc_words_cases.py.

The look-ahead helps where the unigram says something about the words that are spoken, which tests/ctc_lm_restatement.random_model's
uniform weights do not.  zipf_model is a bigram whose unigrams follow Zipf's law: P(w) proportional to 1 / rank over a random
permutation of the words, normalised to 0.9; `bigrams` pairs (h, w), both drawn from the unigram, with P(w | h) = min(0.8, P(w) *
exp(N(1.5, 1))); every backoff weight -0.25 (log10); </s> 0.1.  zipf_batch draws an utterance's words by the unigram and spikes along
their first listed spellings, as tests/ctc_lex_cases.lex_case does along uniformly drawn ones.

A seed is part of the case: the CPU test holds the stability cap (at most S // 8 unstable utterances) and the efficacy condition on
exactly these, and a seed that misses either is replaced here, never the condition."""
import functools

import numpy as np

from tests import ctc_cases as cc
from tests import ctc_lm_restatement as L

# name -> arguments of zipf_model
MODELS = {
    "zipf_v1000": dict(seed=7201, V=1000, bigrams=6000),
    "zipf_v1000_unk": dict(seed=7202, V=1000, bigrams=6000, missing=(5, 17, 400, 999)),
    "zipf_v12_unk": dict(seed=7203, V=12, bigrams=40, missing=(2, 7)),
    "zipf_v20": dict(seed=7204, V=20, bigrams=80),
}

# key -> the lexicon (of tests/ctc_lex_cases.py, or with unspaced of tests/ctc_words_cases.py), the minibatch (arguments of
# zipf_batch), (beam, max_classes), the word model and the parameters
CASES = {
    "zipf_k30": dict(lex="k30_sp1", unspaced=False, batch=dict(S=32, T=40, height=3.0, seed=7314), B=8, C=8, model="zipf_v1000", alpha=1.0, beta=0.5, eos=True),
    # C' = 3 < K - 1 = 6: the space is rarely a candidate
    "zipf_k7_c3": dict(lex="k7_sp3", unspaced=False, batch=dict(S=3, T=24, height=3.0, seed=7302), B=16, C=3, model="zipf_v12_unk", alpha=0.8, beta=0.2, eos=True),
    "zipf_64x32": dict(lex="k40_sp39", unspaced=False, batch=dict(S=2, T=24, height=4.0, seed=7303), B=64, C=32, model="zipf_v1000_unk", alpha=0.6, beta=0.4, eos=True),
    "zipf_T1500": dict(lex="k8_sp7", unspaced=False, batch=dict(S=2, T=1500, height=10.0, seed=7304, fill=0.5, wrong=0.02), B=4, C=4, model="zipf_v20", alpha=0.75, beta=0.1, eos=True),
    # the unspaced twins: homophones with different unigrams at one node (every homophone set of k30: Zipf unigrams are distinct) ...
    "zipf_w_k30": dict(lex="k30", unspaced=True, batch=dict(S=32, T=40, height=3.0, seed=7322), B=8, C=8, model="zipf_v1000", alpha=1.0, beta=0.5, eos=True),
    "zipf_w_k7_c3": dict(lex="k7", unspaced=True, batch=dict(S=3, T=24, height=3.0, seed=7306), B=16, C=3, model="zipf_v12_unk", alpha=0.8, beta=0.2, eos=True),
    # ... and the key limit: 16 * (1 + 28 * (1 + 8)) = 4048 of 4096 keys (C = 29 would be 4192)
    "zipf_w_limit": dict(lex="k40", unspaced=True, batch=dict(S=2, T=24, height=4.0, seed=7307), B=16, C=28, model="zipf_v1000_unk", alpha=0.6, beta=0.4, eos=True),
}
# the cases the efficacy condition is held on, and the narrower and wider beams the measurements add
EFFICACY = ("zipf_k30", "zipf_w_k30")


def zipf_probs(seed, V):
    """P [V + 1] (index 0 unused) of the unigram: 0.9 / (rank * H_V) over a random permutation."""
    rng = np.random.default_rng(seed)
    rank = np.empty(V, np.int64)
    rank[rng.permutation(V)] = np.arange(1, V + 1)
    p = 1.0 / rank
    return np.concatenate([[0.0], 0.9 * p / p.sum()])


def zipf_model(seed, V, bigrams, missing=(), backoff=-0.25):
    """A ctc_lm_restatement.Model over word ids 1 .. V (K = V + 1), order 2.  missing: words without a unigram (they take <unk>'s,
    which is listed then); no bigram holds them."""
    P = zipf_probs(seed, V)
    rng = np.random.default_rng(seed + 1)
    l10 = lambda v: round(float(np.log10(v)), 5)
    grams = {(w,): (l10(P[w]), backoff) for w in range(1, V + 1) if w not in missing}
    grams[(L.BOS,)] = (-99.0, backoff)
    grams[(L.EOS,)] = (l10(0.1), None)
    if missing:
        grams[(L.UNK,)] = (l10(0.5 / V), backoff)
    listed = np.array([w for w in range(1, V + 1) if w not in missing])
    pl = P[listed] / P[listed].sum()
    n = 0
    while n < bigrams:
        h, w = (int(x) for x in rng.choice(listed, size=2, p=pl))
        if (h, w) in grams:
            continue
        grams[(h, w)] = (l10(min(0.8, P[w] * float(np.exp(rng.normal(1.5, 1.0))))), None)
        n += 1
    return L.Model(V + 1, 2, grams)


@functools.lru_cache(maxsize=None)
def model_of(name):
    return zipf_model(**MODELS[name])


@functools.lru_cache(maxsize=None)
def lex_of(key):
    cfg = CASES[key]
    if cfg["unspaced"]:
        from tests import ctc_words_cases as wc
        return wc.lexicon(cfg["lex"])
    from tests import ctc_lex_cases as xc
    return xc.lexicon(cfg["lex"])


def first_spellings(lex):
    """{word id: its first listed spelling}, for either kind of lexicon."""
    first = {}
    for name, sp in lex.entries:
        first.setdefault(lex.ids[name], sp)
    return first


def zipf_batch(lex, P, unspaced, S, T, height, seed, fill=0.4, wrong=0.05):
    """lens, probs (float32 [T*S x K], row t*S + s), the word ids behind each utterance: tests/ctc_lex_cases.lex_case with the words
    drawn by P [V + 1]."""
    rng = np.random.default_rng(seed)
    lens = np.sort(rng.integers(int(np.ceil(0.7 * T)), T + 1, size=S)).astype(np.int32)
    lens[-1] = T
    logits = rng.standard_normal((T * S, lex.K)).astype(np.float32)
    first = first_spellings(lex)
    pw = P[1:] / P[1:].sum()
    words = []
    for s in range(S):
        lab, ws = (), []
        while True:
            w = 1 + int(rng.choice(lex.V, p=pw))
            more = lab + ((lex.space,) if lab and not unspaced else ()) + first[w]
            if len(more) > fill * lens[s] and ws:
                break
            if len(more) + cc.num_repeats(more) < lens[s]:
                lab, ws = more, ws + [w]
            if len(more) > fill * lens[s]:
                break
        assert ws and len(lab) + cc.num_repeats(lab) < lens[s]
        words.append(ws)
        cc._spike(rng, logits, S, s, cc._alignment(rng, int(lens[s]), np.asarray(lab, np.int64)), height, wrong, lex.K)
    return lens, cc.softmax32(logits), words


@functools.lru_cache(maxsize=None)
def build(key):
    """(lens, probs, T, S) of CASES[key]."""
    cfg = CASES[key]
    m = MODELS[cfg["model"]]
    lens, probs, _ = zipf_batch(lex_of(key), zipf_probs(m["seed"], m["V"]), cfg["unspaced"], **cfg["batch"])
    S = len(lens)
    probs = np.ascontiguousarray(probs, np.float32)
    probs.setflags(write=False)
    return np.asarray(lens, np.int32), probs, probs.shape[0] // S, S
