"""CPU: csrc/lex.cpp -- lexicon text -> trie -- against the set definition (tests/ctc_lex_restatement.py: Lex, which has no trie), and
the one addition to csrc/lm.cpp (skip_oov).  eesen_lex_* and eesen_lm_* do no device work, so nothing here needs a GPU.

  the trie: walking eesen_lex_child from the root along a tuple succeeds exactly for the prefixes of the spellings, eesen_lex_word is
      the spelling's word id there and 0 elsewhere, a node's children come in ascending class order, the node count is the prefix count
  a word that is a prefix of another, a word with two spellings, ids in order of first appearance, a units table and decimal ids
  Words() on members and non-members of L
  every malformed file of INTEGRATION.md "Lexicon", with its message, the file and the line
  WriteWords -> TokenLm: the word LM over the lexicon's table is the textbook model over the word ids
  skip_oov: equal to the model with the out-of-vocabulary n-grams removed by hand; without it the file is refused as before
  the same malformed files through lex.cpp and lm.cpp directly, in a stand-alone program built with -fsanitize=address,undefined
"""
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import ctc_lex_cases as xc
from tests import ctc_lex_restatement as X
from tests import ctc_lm_restatement as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(lex, directory, names=None, stem="lex"):
    from eesen_amd.api import Lexicon
    units = None
    if names is not None:
        units = os.path.join(str(directory), stem + ".units.txt")
        with open(units, "w") as f:
            f.write("".join(f"{names[c]} {c}\n" for c in range(1, lex.K)))
    return Lexicon(lex.write(directory, stem, names), units, K=lex.K, space=lex.space)


def _walk(trie, labels):
    v = 0
    for c in labels:
        v = trie.Child(v, int(c))
        if v < 0:
            return -1
    return v


@pytest.mark.parametrize("name", ["exhaustive", "k3_sp1", "k3_sp2", "k7_sp3", "k8_sp7", "k30_sp1"])
def test_trie_is_the_set_definition(name, tmp_path):
    lex = X.lex_of(name)
    names = [None] + [f"u{c}" for c in range(1, lex.K)] if name in ("k7_sp3", "exhaustive") else None
    trie = _compile(lex, tmp_path, names)
    info = trie.Info()
    assert info == dict(words=lex.V, nodes=len(lex.prefixes), max_word_len=max(map(len, lex.spell)))
    nodes = {}
    for pre in lex.prefixes:
        v = _walk(trie, pre)
        assert v >= 0 and nodes.setdefault(v, pre) == pre, pre                     # one node per prefix
        assert trie.Word(v) == lex.spell.get(pre, 0), pre
        kids = [trie.Child(v, c) for c in range(1, lex.K)]
        assert [k >= 0 for k in kids] == [pre + (c,) in lex.prefixes for c in range(1, lex.K)], pre
    assert nodes[0] == () and sorted(nodes) == list(range(len(lex.prefixes)))
    assert trie.Word(0) == 0 and trie.Child(0, lex.space) == -1
    # what is not a prefix: one label more than a leaf, and random tuples
    rng = np.random.default_rng(3)
    for _ in range(300):
        t = tuple(int(c) for c in rng.integers(1, lex.K, size=int(rng.integers(1, 7))))
        assert (_walk(trie, t) >= 0) == (t in lex.prefixes), t


def test_children_are_sorted_and_ids_follow_first_appearance(tmp_path):
    from eesen_amd.api import Lexicon
    path = tmp_path / "l.txt"
    path.write_text("zed 5 2\nab 2 3\na 2\nzed 6\nab 2 3\nb 3 2 2\n")          # a prefix word, two spellings, a repeated line
    trie = Lexicon(str(path), None, K=7, space=1)
    assert trie.Info() == dict(words=4, nodes=9, max_word_len=3)
    assert [trie.Child(0, c) >= 0 for c in range(1, 7)] == [False, True, True, False, True, True]
    a = trie.Child(0, 2)
    assert trie.Word(a) == 3 and trie.Word(trie.Child(a, 3)) == 2                    # a = 3 is a prefix of ab = 2
    assert trie.Word(_walk(trie, (5, 2))) == 1 and trie.Word(_walk(trie, (6,))) == 1 and trie.Word(_walk(trie, (5,))) == 0
    assert trie.Word(_walk(trie, (3, 2, 2))) == 4
    words = tmp_path / "words.txt"
    trie.WriteWords(str(words))
    assert words.read_text() == "zed 1\nab 2\na 3\nb 4\n"
    from eesen_amd.api import EesenError
    for node, c in ((-1, 2), (9, 2)):
        with pytest.raises(EesenError):
            trie.Child(node, c)
    with pytest.raises(EesenError):
        trie.Word(9)


@pytest.mark.parametrize("name", ["exhaustive", "k7_sp3", "k30_sp1"])
def test_words_segments_the_language_and_nothing_else(name, tmp_path):
    from eesen_amd.api import EesenError
    lex = X.lex_of(name)
    trie = _compile(lex, tmp_path)
    assert trie.Words([]) == []
    rng = np.random.default_rng(11)
    spellings = sorted(lex.spell)
    for _ in range(200):
        ws = [spellings[int(i)] for i in rng.integers(len(spellings), size=int(rng.integers(1, 6)))]
        lab = ()
        for i, sp in enumerate(ws):
            lab += (() if i == 0 else (lex.space,)) + sp
        assert trie.Words(lab) == [lex.spell[sp] for sp in ws] == list(lex.segment(lab))
        # one edit away: mostly outside the language
        bad = list(lab)
        at = int(rng.integers(len(bad)))
        bad[at] = int(rng.integers(1, lex.K))
        for cand in (tuple(bad), lab + (lex.space,), (lex.space,) + lab, lab + (lex.space, lex.space) + lab, lab[:-1]):
            want = lex.segment(cand)
            if want is None:
                with pytest.raises(EesenError) as e:
                    trie.Words(cand)
                assert e.value.code == -1
            else:
                assert trie.Words(cand) == list(want)
    if name == "exhaustive":          # every tuple of up to 6 labels
        for n in range(1, 7):
            for t in itertools.product(range(0, lex.K + 1), repeat=n) if n <= 4 else itertools.product(range(1, lex.K), repeat=n):
                want = lex.segment(t) if all(1 <= c < lex.K for c in t) else None
                try:
                    got = tuple(trie.Words(t))
                except EesenError:
                    got = None
                assert got == want, t


MALFORMED = [
    ("a 2\nc 2 9\n", None, "l.txt:2", "unit 9 outside [1, K)"),
    ("a 2\nb 0\n", None, "l.txt:2", "unit 0 outside [1, K)"),
    ("a 2 1 2\n", None, "l.txt:1", "space class"),
    ("a 2\nb x\n", None, "l.txt:2", "no decimal class id"),
    ("a a\nc a q\n", "units", "l.txt:2", "unit q is not in the units table"),
    ("a a <SPACE>\n", "units", "l.txt:1", "space class"),
    ("a a\n\nb\n", "units", "l.txt:3", "word b has an empty spelling"),
    ("a a b\nc b\nb a b\n", "units", "l.txt:3", "words a and b have the same spelling"),
    ("", None, "l.txt", "holds no word"),
    ("\n \n", None, "l.txt", "holds no word"),
]


@pytest.mark.parametrize("text,units,where,words", MALFORMED)
def test_malformed_lexicons_are_errors_with_file_and_line(text, units, where, words, tmp_path):
    from eesen_amd.api import EesenError, Lexicon
    (tmp_path / "l.txt").write_text(text)
    (tmp_path / "units").write_text("<SPACE> 1\na 2\nb 3\n")
    with pytest.raises(EesenError) as e:
        Lexicon(str(tmp_path / "l.txt"), str(tmp_path / units) if units else None, K=4, space=1)
    assert e.value.code == -1 and where in str(e.value) and words in str(e.value), str(e.value)


def test_other_refusals(tmp_path):
    from eesen_amd.api import EesenError, Lexicon
    (tmp_path / "l.txt").write_text("a 2\n")
    for kw, words in ((dict(K=4, space=0), "space class"), (dict(K=4, space=4), "space class"), (dict(K=2, space=1), "K >= 3")):
        with pytest.raises(EesenError) as e:
            Lexicon(str(tmp_path / "l.txt"), None, **kw)
        assert words in str(e.value)
    with pytest.raises(EesenError) as e:
        Lexicon(str(tmp_path / "none.txt"), None, K=4, space=1)
    assert "cannot open" in str(e.value)
    assert Lexicon(str(tmp_path / "l.txt"), None, K=4, space=1).Info()["words"] == 1


def _word_model(lex, name):
    """The restatement model over the word ids, spelled with the lexicon's word names."""
    m = X.model_of(name)
    by_id = {w: n for n, w in lex.ids.items()}
    return L.Model(m.K, m.order, m.grams, [None] + [by_id[w] for w in range(1, lex.V + 1)])


@pytest.mark.parametrize("lex_name,model_name", [("k7_sp3", "v12_o3_unk"), ("k8_sp7", "v20_o4")])
def test_write_words_round_trip_into_a_word_lm(lex_name, model_name, tmp_path):
    from eesen_amd.api import TokenLm
    lex = X.lex_of(lex_name)
    trie = _compile(lex, tmp_path)
    table = str(tmp_path / "words.txt")
    trie.WriteWords(table)
    assert open(table).read() == "".join(f"{n} {w}\n" for n, w in sorted(lex.ids.items(), key=lambda kv: kv[1]))
    model = _word_model(lex, model_name)
    arpa, _ = model.write(tmp_path, "wlm")
    lm = TokenLm(arpa, table, K=lex.V + 1)
    assert lm.OovDropped() == 0 and lm.Info()["order"] == model.order
    rng = np.random.default_rng(17)
    for _ in range(300):
        ws = [int(w) for w in rng.integers(1, lex.V + 1, size=int(rng.integers(0, 6)))]
        want, absum = model.lm64(ws, model.has_eos)
        got = lm.Score(ws, eos=model.has_eos)
        assert abs(got - want) <= 1e-6 * max(absum, 1.0), ws
        assert lm.Score(trie.Words(lex.spelling_of(ws)), eos=model.has_eos) == got


def test_skip_oov_is_the_model_with_the_oov_ngrams_removed(tmp_path):
    from eesen_amd.api import EesenError, TokenLm
    lex = X.lex_of("k7_sp3")
    trie = _compile(lex, tmp_path)
    table = str(tmp_path / "words.txt")
    trie.WriteWords(table)
    clean = _word_model(lex, "v12_o3_unk")
    grams = dict(clean.grams)
    extra = {("zebra",): (-1.5, -0.25), ("yak",): (-2.5, None), (1, "zebra"): (-0.7, -0.1), ("zebra", 3): (-0.4, 0.2), (L.BOS, "zebra"): (-0.3, None),
             (1, "zebra", 3): (-0.2, None), ("zebra", 3, L.EOS): (-0.6, None), ("zebra", "zebra"): (-0.9, None)}
    assert all(g[:-1] in grams or g[:-1] in extra or len(g) == 1 for g in extra)
    grams.update(extra)
    dirty = L.Model(clean.K, clean.order, grams, clean.names)
    a, _ = clean.write(tmp_path, "clean")
    b, _ = dirty.write(tmp_path, "dirty")
    want = TokenLm(a, table, K=lex.V + 1)
    with pytest.raises(EesenError) as e:          # the old entry point keeps refusing the file, naming the word
        TokenLm(b, table, K=lex.V + 1)
    assert e.value.code == -1 and ("zebra" in str(e.value) or "yak" in str(e.value))
    got = TokenLm(b, table, K=lex.V + 1, skip_oov=True)
    assert got.OovDropped() == len(extra) and want.OovDropped() == 0
    assert got.Info() == want.Info() and got.Start() == want.Start()
    for st in range(want.Info()["states"]):
        assert got.Final(st) == want.Final(st)
        for c in range(1, lex.V + 1):
            assert got.Step(st, c) == want.Step(st, c), (st, c)
    # the section counts are the file's own: one line less than the header says is an error, dropped lines or not
    text = open(b).read().splitlines()
    cut = next(i for i, l in enumerate(text) if l.split()[1:] == ["zebra", "zebra"])
    short = tmp_path / "short.arpa"
    short.write_text("\n".join(text[:cut] + text[cut + 1:]) + "\n")
    with pytest.raises(EesenError) as e:
        TokenLm(str(short), table, K=lex.V + 1, skip_oov=True)
    assert "the header says" in str(e.value)


def test_a_lexicon_word_without_a_unigram_is_named(tmp_path):
    """No <unk> in the file: creation fails and names the word, by the name the words table gives it."""
    from eesen_amd.api import EesenError, Lexicon, TokenLm
    (tmp_path / "l.txt").write_text("alpha 2\nbeta 3\ngamma 2 3\n")
    trie = Lexicon(str(tmp_path / "l.txt"), None, K=4, space=1)
    trie.WriteWords(str(tmp_path / "w.txt"))
    (tmp_path / "w.arpa").write_text("\\data\\\nngram 1=3\n\n\\1-grams:\n-1 alpha\n-1 gamma\n-1 </s>\n\n\\end\\\n")
    with pytest.raises(EesenError) as e:
        TokenLm(str(tmp_path / "w.arpa"), str(tmp_path / "w.txt"), K=4)
    assert e.value.code == -1 and "class 2 (beta) has no unigram" in str(e.value), str(e.value)


def test_malformed_files_under_the_sanitizers(tmp_path):
    """tests/native/lex_lm_malformed.cc with lex.cpp and lm.cpp, address and undefined-behaviour sanitizers, as a program of its own
    (the runtimes linked statically: the program needs nothing from its environment)."""
    from eesen_amd import build as hb
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hb.hipcc()))), "include")
    exe = str(tmp_path / "lex_lm_malformed")
    csrc = os.path.join(ROOT, "eesen_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                        "-D__HIP_PLATFORM_AMD__",
                        "-I" + rocm_include, os.path.join(ROOT, "tests", "native", "lex_lm_malformed.cc"), os.path.join(csrc, "lex.cpp"),
                        os.path.join(csrc, "lm.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    scratch = tmp_path / "files"
    scratch.mkdir()
    r = subprocess.run([exe, str(scratch)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("0 failures") and "runtime error" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
