"""CPU: the LM look-ahead's table (eesen_lex_lookahead, host code only) against the dictionary restatement, and what
tests/test_gpu_ctc_decode_lookahead.py relies on, held with the restatement alone (tests/ctc_lookahead_restatement.py).

  the table: exactly the restatement's, node by node along every spelling, for both lexicon kinds; a word without a unigram takes
      <unk>'s; an LM built with skip_oov; homophones with different unigrams at one node; the errors of the call
  the restatement with the rank term removed returns exactly what tests/ctc_lex_restatement.py and tests/ctc_words_restatement.py return
  the stability cap: at most S // 8 utterances per case whose 1-best moves under the eight jitter seeds -- a condition on the cases
  the efficacy condition (INTEGRATION.md "LM look-ahead"), on the fp64 restatement: on zipf_k30 and its unspaced twin the utterances
      whose 1-best score is higher with the look-ahead by more than `bar` are at least twice those where it is lower, and the summed
      1-best score is higher
"""
import ctypes as C

import numpy as np
import pytest

from tests import ctc_beam_restatement as R
from tests import ctc_lex_cases as xc
from tests import ctc_lex_restatement as X
from tests import ctc_lm_restatement as L
from tests import ctc_lookahead_cases as kc
from tests import ctc_lookahead_restatement as A
from tests import ctc_words_cases as wc
from tests import ctc_words_restatement as W


def _made(d, rl, model, tag, skip_oov=False, arpa_model=None):
    """(api.Lexicon, api.TokenLm) of a restatement lexicon and word model: the ARPA text names the words as the lexicon does."""
    from eesen_amd.api import Lexicon, TokenLm
    trie = Lexicon(rl.write(d, tag), None, K=rl.K, space=None if isinstance(rl, W.WLex) else rl.space)
    table = str(d / (tag + ".words.txt"))
    trie.WriteWords(table)
    m = arpa_model or model
    by_id = {w: n for n, w in rl.ids.items()}
    names = [None] + [by_id[w] if w <= rl.V else f"oov{w}" for w in range(1, m.K)]
    arpa, _ = L.Model(m.K, m.order, m.grams, names).write(d, tag + ".lm")
    return trie, TokenLm(arpa, table, K=rl.V + 1, skip_oov=skip_oov)


def _table_is(trie, lm, rl, la):
    """Walks every spelling through the trie: the node of each prefix holds the restatement's value, bit for bit, and every node is met."""
    got = trie.Lookahead(lm)
    assert got.dtype == np.float32 and got.shape == (trie.Info()["nodes"],) == (len(rl.prefixes),)
    seen = {0}
    assert got[0] == la[()] == max(la.values())
    for sp in rl.spell:
        v = 0
        for i, c in enumerate(sp):
            v = trie.Child(v, c)
            assert v > 0 and got[v] == la[sp[:i + 1]], (sp, i, float(got[v]), float(la[sp[:i + 1]]))
            seen.add(v)
    assert len(seen) == got.size
    return got


@pytest.mark.parametrize("key", ["zipf_k30", "zipf_k7_c3", "zipf_64x32", "zipf_w_k30", "zipf_w_k7_c3", "zipf_w_limit"])
def test_table_is_the_restatements(key, tmp_path):
    cfg = kc.CASES[key]
    rl, model = kc.lex_of(key), kc.model_of(cfg["model"])
    trie, lm = _made(tmp_path, rl, model, key)
    la = A.table(rl, model)
    got = _table_is(trie, lm, rl, la)
    # what eesen_lm_step returns at state 0, word by word
    for w in (1, 2, 5, 7, rl.V):
        wt, nxt = C.c_float(), C.c_int()
        assert trie.lib.eesen_lm_step(lm.h, 0, w, C.byref(wt), C.byref(nxt)) == 0
        assert np.float32(wt.value) == A.unigram(model, w)
    assert len(set(got.tolist())) > 3          # a table worth having: the values differ along the trie


def test_a_word_without_a_unigram_takes_unk():
    model = kc.model_of("zipf_v12_unk")
    assert (2,) not in model.grams and (7,) not in model.grams and (L.UNK,) in model.grams
    assert float(A.unigram(model, 2)) == float(np.float32(model.p[(L.UNK,)])) != float(A.unigram(model, 1))
    rl = kc.lex_of("zipf_k7_c3")
    la = A.table(rl, model)
    first = kc.first_spellings(rl)
    # a node that only words without a unigram pass holds <unk>'s weight, if the lexicon has one; the leaf of word 2 is at least that
    assert la[first[2]] >= A.unigram(model, 2)
    only = [p for p in rl.prefixes if p and all(w in (2, 7) for sp, w in rl.spell.items() if sp[:len(p)] == p)]
    assert all(la[p] == A.unigram(model, 2) for p in only)


def test_homophones_with_different_unigrams_share_a_node():
    rl, model = kc.lex_of("zipf_w_k30"), kc.model_of("zipf_v1000")
    la = A.table(rl, model)
    sets = [(sp, ws) for sp, ws in rl.spell.items() if len(ws) > 1]
    assert sets and rl.H >= 4
    for sp, ws in sets:
        us = [float(A.unigram(model, w)) for w in ws]
        assert len(set(us)) == len(us) and la[sp] >= max(us), sp
    assert any(la[sp] == max(A.unigram(model, w) for w in ws) for sp, ws in sets)
    cfg = kc.CASES["zipf_w_limit"]
    H = kc.lex_of("zipf_w_limit").H
    assert cfg["B"] * (1 + cfg["C"] * (1 + H)) <= 4096 < cfg["B"] * (1 + (cfg["C"] + 1) * (1 + H))


def test_table_of_an_lm_built_with_skip_oov(tmp_path):
    """The ARPA file holds two words the lexicon has not, in unigrams and bigrams: skip_oov drops those n-grams, and the table is the
    one of the model without them."""
    rl = xc.lexicon("k7_sp3")
    big = kc.zipf_model(seed=7401, V=rl.V + 2, bigrams=60)
    kept = {g: v for g, v in big.grams.items() if all(isinstance(x, str) or x <= rl.V for x in g)}
    assert len(kept) < len(big.grams) and any(len(g) == 2 for g in set(big.grams) - set(kept))
    model = L.Model(rl.V + 1, 2, kept)
    trie, lm = _made(tmp_path, rl, model, "oov", skip_oov=True, arpa_model=big)
    assert lm.OovDropped() == len(big.grams) - len(kept)
    _table_is(trie, lm, rl, A.table(rl, model))


def test_table_errors(tmp_path):
    from eesen_amd.api import EesenError
    rl, model = xc.lexicon("k7_sp3"), kc.model_of("zipf_v12_unk")
    trie, lm = _made(tmp_path, rl, model, "a")
    other = xc.lexicon("k8_sp7")
    trie20, _ = _made(tmp_path, other, kc.model_of("zipf_v20"), "b")
    with pytest.raises(EesenError, match="word count \\+ 1"):
        trie20.Lookahead(lm)                                  # K = 13 against V + 1 = 21
    nodes = trie.Info()["nodes"]
    out = np.full(nodes + 1, 7.0, np.float32)
    ptr = out.ctypes.data_as(C.c_void_p)
    assert trie.lib.eesen_lex_lookahead(trie.h, lm.h, ptr, nodes - 1) != 0 and np.all(out == 7.0)
    assert b"node" in trie.lib.eesen_last_error()
    assert trie.lib.eesen_lex_lookahead(trie.h, lm.h, ptr, nodes) == 0 and out[nodes] == 7.0 and np.all(out[:nodes] < 0)
    assert trie.lib.eesen_lex_lookahead(trie.h, None, ptr, nodes) != 0 and trie.lib.eesen_lex_lookahead(None, lm.h, ptr, nodes) != 0


@pytest.mark.parametrize("key", ["k3_sp1", "k7_c3", "k7_nolm", "k40_64x32"])
def test_without_the_rank_term_it_is_the_lexicon_restatement(key):
    lens, probs, T, S, lex, model, cfg, ref = X.case(key)
    for s in range(S):
        p = R.utterance(probs, s, S, int(lens[s]))
        for dt, l in ((np.float64, R.log64(p)), (np.float32, R.log32(p))):
            args = (l, R.log32(p), cfg["B"], cfg["C"], lex, model, cfg["alpha"], cfg["beta"], cfg["eos"], dt)
            assert A.beam_search(*args, with_live=True) == X.beam_search(*args, with_live=True), (key, s, dt)
            assert A.beam_search(*args, jitter=(R.JITTER_SEEDS[0], 1e-3)) == X.beam_search(*args, jitter=(R.JITTER_SEEDS[0], 1e-3)), (key, s, dt)


@pytest.mark.parametrize("key", ["k3_1x1", "k7_c3", "k8_h3", "k40_16x20_h8"])
def test_without_the_rank_term_it_is_the_word_restatement(key):
    lens, probs, T, S, lex, model, cfg, ref = W.case(key)
    for s in range(S):
        p = R.utterance(probs, s, S, int(lens[s]))
        for dt, l in ((np.float64, R.log64(p)), (np.float32, R.log32(p))):
            args = (l, R.log32(p), cfg["B"], cfg["C"], lex, model, cfg["alpha"], cfg["beta"], cfg["eos"], dt)
            assert A.word_search(*args, with_live=True) == W.beam_search(*args, with_live=True), (key, s, dt)
            assert A.word_search(*args, jitter=(R.JITTER_SEEDS[0], 1e-3)) == W.beam_search(*args, jitter=(R.JITTER_SEEDS[0], 1e-3)), (key, s, dt)


def test_zero_weights_rank_as_without_the_table():
    """alpha = beta = 0: eta is 0 on every node, and the search with the table is the search without it."""
    key = "zipf_k7_c3"
    cfg = kc.CASES[key]
    lex, model = kc.lex_of(key), kc.model_of(cfg["model"])
    lens, probs, T, S = kc.build(key)
    la = A.table(lex, model)
    for s in range(S):
        p = R.utterance(probs, s, S, int(lens[s]))
        args = (R.log32(p), R.log32(p), cfg["B"], cfg["C"], lex, model, 0.0, 0.0, False, np.float32)
        assert A.beam_search(*args, la=la) == A.beam_search(*args)


@pytest.mark.parametrize("key", list(kc.CASES))
def test_cases_hold_their_conditions(key):
    lens, probs, T, S, lex, model, cfg, la, ref = A.case(key)
    alpha, beta, eos = cfg["alpha"], cfg["beta"], cfg["eos"]
    unstable = [s for s in range(S) if not ref[s]["stable"]]
    assert len(unstable) <= S // 8, (key, unstable)
    assert sum(1 for r in ref if r["beam64"]) >= S - S // 8, key
    worst, nwords = 0.0, 0
    for s in range(S):
        r = ref[s]
        n = int(lens[s])
        lp = R.log64(R.utterance(probs, s, S, n))
        for h, score, lmsum in r["beam64"]:
            labels, words = (W.split(h)[0], W.split(h)[1]) if cfg["unspaced"] else (h, lex.segment(h))
            assert words is not None, (key, s, h)
            lm, absum = X.lm64(model, words, eos)
            exact = R.lnp64(lp, labels) + alpha * lm + beta * len(words)          # the score keeps its meaning under the look-ahead
            assert score <= exact + r["bar"], (key, s, h, score, exact)
            assert abs(lmsum - lm) <= 1e-12 * max(1.0, absum), (key, s, h)
        if not r["beam64"] or not r["stable"]:
            continue
        words = W.split(r["beam64"][0][0])[1] if cfg["unspaced"] else lex.segment(r["beam64"][0][0])
        nwords += len(words)
        assert r["beam32"] and r["beam32"][0][0] == r["beam64"][0][0], (key, s)
        err = abs(r["beam32"][0][1] - r["score64"])
        assert err <= r["bar"], (key, s, err, r["bar"])
        worst = max(worst, err / r["bar"])
    assert nwords >= S, key
    print(f"{key}: unstable {unstable} (cap {S // 8}); fp32 |score - score64| / bar <= {worst:.3g}; {nwords} words in the stable 1-bests")


def test_the_space_is_rarely_a_candidate():
    lens, probs, T, S, lex, model, cfg, la, ref = A.case("zipf_k7_c3")
    assert cfg["C"] < lex.K - 1
    with_space = [lex.space in R.candidates(R.log32(probs[r]), cfg["C"]) for r in range(T * S) if r // S < lens[r % S]]
    assert 0 < sum(with_space) < len(with_space) / 2


@pytest.mark.parametrize("key", kc.EFFICACY)
def test_efficacy_condition(key):
    lens, probs, T, S, lex, model, cfg, la, ref = A.case(key)
    on = [r["score64"] if r["beam64"] else None for r in ref]
    off = A.best_scores(key, cfg["B"], False)
    better, worse, sum_on, sum_off = A.efficacy(on, off, [r["bar"] for r in ref])
    print(f"{key} beam {cfg['B']}: 1-best score higher with the look-ahead on {better} utterances, lower on {worse} of {S}; "
          f"summed 1-best score {sum_on:.3f} with, {sum_off:.3f} without")
    assert better >= 2 * worse and better > 0, (key, better, worse)
    assert sum_on > sum_off, (key, sum_on, sum_off)
