"""Lexicons, word models, minibatches and configurations of the lexicon-constrained prefix beam search tests
(tests/test_ctc_lex_restatement.py on the CPU, tests/test_gpu_ctc_decode_lex.py on the GPU): the smallest shapes at which each piece
of the lexicon mode of csrc/ctc_decode.hip can go wrong.

A decoder held to a lexicon finds nothing on random posteriors, so a minibatch here is drawn from its lexicon: every utterance spikes
(tests/ctc_cases.py: _alignment, _spike; a share of the frames on a wrong class) along the spelling of a random word sequence over
N(0, 1) logits.  The heights are low enough that the beam holds competing words.

A seed is part of the case: the CPU test holds the stability cap (at most S // 8 unstable utterances) on exactly these, and a seed
that misses it is replaced here, never the cap."""
import numpy as np

from tests import ctc_cases as cc

# name -> dict(K, space, and either `entries` [(word, spelling)] or the arguments of random_entries)
LEXICONS = {
    # blank, space and two units (a = 2, b = 3): a word that is a prefix of another, one with a repeated unit
    "exhaustive": dict(K=4, space=1, entries=[("a", (2,)), ("ab", (2, 3)), ("ba", (3, 2)), ("aa", (2, 2))]),
    "k3_sp1": dict(K=3, space=1, entries=[("x", (2,)), ("xx", (2, 2)), ("xxxx", (2, 2, 2, 2))]),
    "k3_sp2": dict(K=3, space=2, entries=[("x", (1,)), ("xxx", (1, 1, 1))]),
    "k7_sp3": dict(K=7, space=3, V=12, max_len=4, seed=5101),
    "k8_sp7": dict(K=8, space=7, V=20, max_len=5, seed=5102),
    "k30_sp1": dict(K=30, space=1, V=1000, max_len=8, seed=5103),
    "k40_sp39": dict(K=40, space=39, V=1000, max_len=7, seed=5104),
}

# name -> arguments of tests/ctc_lm_restatement.random_model over the word ids: K = V + 1
MODELS = {
    "v4_o2": dict(seed=5201, K=5, order=2),
    "v3_o3": dict(seed=5202, K=4, order=3),
    "v12_o3_unk": dict(seed=5203, K=13, order=3, missing=(2, 7), unk=True),
    "v20_o4": dict(seed=5204, K=21, order=4),
    "v1000_o3_unk": dict(seed=5205, K=1001, order=3, missing=(5, 17, 400, 999), unk=True),
    "v1000_o2_noeos": dict(seed=5206, K=1001, order=2, eos=False),
}

# key -> the lexicon, the minibatch (arguments of lex_case), (beam, max_classes), the word model and the parameters
CASES = {
    "k3_sp1": dict(lex="k3_sp1", batch=dict(S=3, T=12, height=3.0, seed=5301), B=8, C=2, model="v3_o3", alpha=0.7, beta=0.3, eos=True),
    "k3_sp2_1x1": dict(lex="k3_sp2", batch=dict(S=3, T=20, height=6.0, seed=5302), B=1, C=1, model=None, alpha=1.0, beta=0.4, eos=False),
    # C' = 3 < K - 1 = 6: the space is no candidate on most frames
    "k7_c3": dict(lex="k7_sp3", batch=dict(S=3, T=24, height=3.0, seed=5303), B=16, C=3, model="v12_o3_unk", alpha=0.8, beta=0.2, eos=True),
    "k7_nolm": dict(lex="k7_sp3", batch=dict(S=3, T=16, height=3.0, seed=5304), B=16, C=6, model=None, alpha=1.0, beta=-0.6, eos=False),
    "k40_64x32": dict(lex="k40_sp39", batch=dict(S=2, T=24, height=4.0, seed=5305), B=64, C=32, model="v1000_o3_unk", alpha=0.6, beta=0.4, eos=True),
    "k30_33x40": dict(lex="k30_sp1", batch=dict(S=33, T=40, height=4.0, seed=5306), B=8, C=8, model="v1000_o2_noeos", alpha=0.5, beta=0.6, eos=False),
    "k8_T1500": dict(lex="k8_sp7", batch=dict(S=2, T=1500, height=10.0, seed=5307, fill=0.5, wrong=0.02), B=4, C=4, model="v20_o4", alpha=0.75, beta=0.1, eos=True),
}
# T = 6: the CPU test holds that at most 64 prefixes the search can hold exist, so that nothing is ever pruned at beam 64
EXHAUSTIVE = dict(lex="exhaustive", lens=(1, 3, 6, 6), seed=5401, B=64, C=3, model="v4_o2", alpha=0.8, beta=0.5, eos=True)
# the lexicons the tie cases of tests/ctc_decode_cases.py (TIE_CASES: K = 12 and K = 5) are decoded along
TIE_LEXICONS = {"ties": dict(K=12, space=4, V=30, max_len=3, seed=5501), "uniform": dict(K=5, space=2, V=6, max_len=2, seed=5502)}


def random_entries(seed, K, space, V, max_len):
    """V words w1 .. wV with pairwise distinct random spellings of 1 .. max_len units; every tenth word is given a second spelling and
    every seventh is an extension of an earlier word's spelling (that word is a prefix of it)."""
    rng = np.random.default_rng(seed)
    units = [c for c in range(1, K) if c != space]
    seen, entries = set(), []

    def draw(base=()):
        while True:
            sp = tuple(base) + tuple(int(units[i]) for i in rng.integers(len(units), size=int(rng.integers(1, max_len + 1 - len(base)))))
            if sp not in seen:
                seen.add(sp)
                return sp
    for w in range(1, V + 1):
        base = ()
        if w % 7 == 0:
            shorter = [sp for _, sp in entries if len(sp) < max_len]
            base = shorter[int(rng.integers(len(shorter)))]
        entries.append((f"w{w}", draw(base)))
        if w % 10 == 0:
            entries.append((f"w{w}", draw()))
    return entries


def lexicon(name, table=None):
    from tests.ctc_lex_restatement import Lex
    cfg = dict((table or LEXICONS)[name])
    K, space = cfg.pop("K"), cfg.pop("space")
    return Lex(K, space, cfg["entries"] if "entries" in cfg else random_entries(K=K, space=space, **cfg))


def lex_case(lex, S, T, height, seed, fill=0.4, wrong=0.05):
    """lens, probs (float32 [T*S x K], row t*S + s), the word ids behind each utterance.  Lengths sorted in [0.7 T, T], the last is T;
    an utterance's words are drawn until their spelling (spaces included) would pass fill * length labels."""
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
            more = lab + ((lex.space,) if lab else ()) + sp
            if len(more) > fill * lens[s] and ws:
                break
            if len(more) + cc.num_repeats(more) < lens[s]:
                lab, ws = more, ws + [lex.spell[sp]]
            if len(more) > fill * lens[s]:
                break
        assert ws and len(lab) + cc.num_repeats(lab) < lens[s]
        words.append(ws)
        cc._spike(rng, logits, S, s, cc._alignment(rng, int(lens[s]), np.asarray(lab, np.int64)), height, wrong, lex.K)
    return lens, cc.softmax32(logits), words


def build(key):
    """(lens, probs, T, S) of CASES[key]."""
    cfg = CASES[key]
    lens, probs, _ = lex_case(lexicon(cfg["lex"]), **cfg["batch"])
    S = len(lens)
    return np.asarray(lens, np.int32), np.ascontiguousarray(probs, np.float32), probs.shape[0] // S, S


def build_exhaustive():
    """Dense posteriors (softmax of N(0, 2^2) logits): every labelling of the language has a path worth finding."""
    cfg = EXHAUSTIVE
    lens = np.asarray(cfg["lens"], np.int32)
    S, T, K = lens.size, int(lens.max()), LEXICONS[cfg["lex"]]["K"]
    rng = np.random.default_rng(cfg["seed"])
    probs = cc.softmax32((2.0 * rng.standard_normal((T * S, K))).astype(np.float32))
    return lens, probs, T, S
