"""Lexicons, word models, minibatches and configurations of the word beam search tests (tests/test_ctc_words_restatement.py on the
CPU, tests/test_gpu_ctc_decode_words.py on the GPU): the smallest shapes at which each piece of ctc_word_beam_kernel
(csrc/ctc_decode.hip) can go wrong.

As in tests/ctc_lex_cases.py a minibatch is drawn from its lexicon: every utterance spikes along the concatenated spellings -- nothing
but CTC's blank between them -- of a random word sequence over N(0, 1) logits.

A seed is part of the case: the CPU test holds the stability cap (at most S // 8 unstable utterances) on exactly these, and a seed
that misses it is replaced here, never the cap.  Homophones stand in these cases only beside a word model: without one their totals
tie exactly, which is the tie test's ground."""
import numpy as np

from tests import ctc_cases as cc

# name -> dict(K, and either `entries` [(word, spelling)] or the arguments of random_entries)
LEXICONS = {
    # blank and three units: a word that is a prefix of another and one with a repeated unit (a, aa), a homophone pair (to, two)
    "exhaustive": dict(K=4, entries=[("a", (1,)), ("aa", (1, 1)), ("to", (2, 3)), ("two", (2, 3))]),
    "k3": dict(K=3, entries=[("x", (1,)), ("xy", (1, 2)), ("yy", (2, 2)), ("yxy", (2, 1, 2))]),
    "k7": dict(K=7, V=12, max_len=4, seed=6101, groups=(2,)),
    "k8": dict(K=8, V=20, max_len=5, seed=6102, groups=(3, 2, 2)),
    "k30": dict(K=30, V=1000, max_len=8, seed=6103, groups=(4, 3, 2, 2, 2, 2)),
    "k40": dict(K=40, V=1000, max_len=7, seed=6104, groups=(8, 5, 3, 3, 2, 2, 2, 2)),
}

# name -> arguments of tests/ctc_lm_restatement.random_model over the word ids: K = V + 1
MODELS = {
    "v4_o2": dict(seed=6201, K=5, order=2),
    "v12_o3_unk": dict(seed=6203, K=13, order=3, missing=(2, 7), unk=True),
    "v20_o4": dict(seed=6204, K=21, order=4),
    "v1000_o3_unk": dict(seed=6205, K=1001, order=3, missing=(5, 17, 400, 999), unk=True),
    "v1000_o2_noeos": dict(seed=6206, K=1001, order=2, eos=False),
}

# key -> the lexicon, the minibatch (arguments of words_case), (beam, max_classes), the word model and the parameters
CASES = {
    "k3_1x1": dict(lex="k3", batch=dict(S=3, T=20, height=6.0, seed=6301), B=1, C=1, model=None, alpha=1.0, beta=0.4, eos=False),
    # C' = 3 < K - 1 = 6: the class that starts the next word is no candidate on most frames
    "k7_c3": dict(lex="k7", batch=dict(S=3, T=24, height=3.0, seed=6303), B=16, C=3, model="v12_o3_unk", alpha=0.8, beta=0.2, eos=True),
    "k8_h3": dict(lex="k8", batch=dict(S=3, T=24, height=3.0, seed=6304), B=16, C=7, model="v20_o4", alpha=0.7, beta=-0.3, eos=True),
    # the admitted limit shape: 16 * (1 + 20 * 9) = 2896 keys of 4096
    "k40_16x20_h8": dict(lex="k40", batch=dict(S=2, T=24, height=4.0, seed=6305), B=16, C=20, model="v1000_o3_unk", alpha=0.6, beta=0.4, eos=True),
    "k30_33x40": dict(lex="k30", batch=dict(S=33, T=40, height=4.0, seed=6306, empty=5), B=8, C=8, model="v1000_o2_noeos", alpha=0.5, beta=0.6, eos=False),
    "k8_T1500": dict(lex="k8", batch=dict(S=2, T=1500, height=10.0, seed=6307, fill=0.3, wrong=0.02), B=4, C=4, model="v20_o4", alpha=0.3, beta=0.1, eos=True),
}
# T = 5: the CPU test holds that at most 64 hypotheses are live at any frame and at most 64 are final, so that nothing is ever pruned
EXHAUSTIVE = dict(lex="exhaustive", lens=(1, 3, 5, 5), seed=6401, B=64, C=3, model="v4_o2", alpha=0.8, beta=0.5, eos=True)
# the lexicons the tie cases of tests/ctc_decode_cases.py (TIE_CASES: K = 12 and K = 5) are decoded along, without a model: homophones tie
TIE_LEXICONS = {"ties": dict(K=12, V=30, max_len=2, seed=6501, groups=(3, 2, 2)), "uniform": dict(K=5, V=6, max_len=2, seed=6502, groups=(2,))}


def random_entries(seed, K, V, max_len, groups=()):
    """V words w1 .. wV with random spellings of 1 .. max_len units.  groups: sizes of homophone sets -- the words of a set stand one
    behind the other from w3 on, two other words between sets, and share the spelling the first of them drew.  Every tenth word is
    given a second spelling and every seventh is an extension of an earlier word's spelling (that word is a prefix of it)."""
    rng = np.random.default_rng(seed)
    seen, entries, copy_of = set(), [], {}
    w = 3
    for size in groups:
        for i in range(1, size):
            copy_of[w + i] = w
        w += size + 2
    assert w <= V + 3

    def draw(base=()):
        while True:
            sp = tuple(base) + tuple(int(c) for c in rng.integers(1, K, size=int(rng.integers(1, max_len + 1 - len(base)))))
            if sp not in seen:
                seen.add(sp)
                return sp
    first = {}
    for w in range(1, V + 1):
        if w in copy_of:
            entries.append((f"w{w}", first[copy_of[w]]))
            continue
        base = ()
        if w % 7 == 0:
            shorter = [sp for _, sp in entries if len(sp) < max_len]
            base = shorter[int(rng.integers(len(shorter)))]
        first[w] = draw(base)
        entries.append((f"w{w}", first[w]))
        if w % 10 == 0:
            entries.append((f"w{w}", draw()))
    return entries


def lexicon(name, table=None):
    from tests.ctc_words_restatement import WLex
    cfg = dict((table or LEXICONS)[name])
    K = cfg.pop("K")
    return WLex(K, cfg["entries"] if "entries" in cfg else random_entries(K=K, **cfg))


def words_case(lex, S, T, height, seed, fill=0.4, wrong=0.05, empty=None):
    """lens, probs (float32 [T*S x K], row t*S + s), the word ids behind each utterance.  Lengths sorted in [0.7 T, T], the last is T;
    an utterance's words are drawn until their spellings would pass fill * length labels.  empty: an utterance whose length is set
    to 0 afterwards."""
    rng = np.random.default_rng(seed)
    lens = np.sort(rng.integers(int(np.ceil(0.7 * T)), T + 1, size=S)).astype(np.int32)
    lens[-1] = T
    logits = rng.standard_normal((T * S, lex.K)).astype(np.float32)
    spellings = sorted(lex.spell)
    words = []
    for s in range(S):
        lab, ws = (), []
        while True:
            sp = spellings[int(rng.integers(len(spellings)))]
            more = lab + sp
            if len(more) > fill * lens[s] and ws:
                break
            if len(more) + cc.num_repeats(more) < lens[s]:
                lab, ws = more, ws + [lex.spell[sp][int(rng.integers(len(lex.spell[sp])))]]
            if len(more) > fill * lens[s]:
                break
        assert ws and len(lab) + cc.num_repeats(lab) < lens[s]
        words.append(ws)
        cc._spike(rng, logits, S, s, cc._alignment(rng, int(lens[s]), np.asarray(lab, np.int64)), height, wrong, lex.K)
    if empty is not None:
        lens[empty] = 0
    return lens, cc.softmax32(logits), words


def build(key):
    """(lens, probs, T, S) of CASES[key]."""
    cfg = CASES[key]
    lens, probs, _ = words_case(lexicon(cfg["lex"]), **cfg["batch"])
    S = len(lens)
    return np.asarray(lens, np.int32), np.ascontiguousarray(probs, np.float32), probs.shape[0] // S, S


def build_exhaustive():
    """Dense posteriors (softmax of N(0, 2^2) logits): every hypothesis has a path worth finding."""
    cfg = EXHAUSTIVE
    lens = np.asarray(cfg["lens"], np.int32)
    S, T, K = lens.size, int(lens.max()), LEXICONS[cfg["lex"]]["K"]
    rng = np.random.default_rng(cfg["seed"])
    probs = cc.softmax32((2.0 * rng.standard_normal((T * S, K))).astype(np.float32))
    return lens, probs, T, S
