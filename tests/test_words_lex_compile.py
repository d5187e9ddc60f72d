"""CPU: the unspaced kind of csrc/lex.cpp -- no boundary unit, several words per spelling -- against the set definition
(tests/ctc_words_restatement.py: WLex, a dict from spelling to word list, no trie).  eesen_lex_* do no device work.

  the trie: walking eesen_lex_child from the root along a tuple succeeds exactly for the prefixes of the spellings; eesen_lex_node_words
      there is the spelling's ascending word list (empty elsewhere), eesen_lex_word its smallest id or 0; eesen_lex_max_homophones is
      the largest list
  every malformed file of INTEGRATION.md "Words without a boundary unit", with its message, the file and the line; the 16th word on
      one spelling, both lines named; eesen_lex_words refuses an unspaced lexicon
  a lexicon with a space class built through the old call answers Child / Word for every (node, class) as the set definition of
      tests/ctc_lex_restatement.py says -- the fixture is generated here, from the restatement -- and has no homophone tables
  the same files through lex.cpp directly, in a stand-alone program built with -fsanitize=address,undefined
"""
import os
import subprocess

import numpy as np
import pytest

from tests import ctc_lex_restatement as X
from tests import ctc_words_cases as wc
from tests import ctc_words_restatement as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(lex, directory, names=None, stem="wlex"):
    from eesen_amd.api import Lexicon
    units = None
    if names is not None:
        units = os.path.join(str(directory), stem + ".units.txt")
        with open(units, "w") as f:
            f.write("".join(f"{names[c]} {c}\n" for c in range(1, lex.K)))
    return Lexicon(lex.write(directory, stem, names), units, K=lex.K, space=None)


def _walk(trie, labels):
    v = 0
    for c in labels:
        v = trie.Child(v, int(c))
        if v < 0:
            return -1
    return v


@pytest.mark.parametrize("name", ["exhaustive", "k3", "k7", "k8", "k30", "k40", "ties", "uniform"])
def test_trie_is_the_set_definition(name, tmp_path):
    lex = wc.lexicon(name, wc.TIE_LEXICONS) if name in wc.TIE_LEXICONS else W.lex_of(name)
    names = [None] + [f"u{c}" for c in range(1, lex.K)] if name in ("k7", "exhaustive") else None
    trie = _compile(lex, tmp_path, names)
    assert trie.unspaced and trie.space is None
    assert trie.Info() == dict(words=lex.V, nodes=len(lex.prefixes), max_word_len=max(map(len, lex.spell)))
    assert trie.MaxHomophones() == lex.H == max(len(ws) for ws in lex.spell.values())
    nodes = {}
    for pre in lex.prefixes:
        v = _walk(trie, pre)
        assert v >= 0 and nodes.setdefault(v, pre) == pre, pre                     # one node per prefix
        ws = lex.spell.get(pre, [])
        assert trie.NodeWords(v) == ws == sorted(ws) and trie.Word(v) == (ws[0] if ws else 0), pre
        kids = [trie.Child(v, c) for c in range(1, lex.K)]
        assert [k >= 0 for k in kids] == [pre + (c,) in lex.prefixes for c in range(1, lex.K)], pre
    assert nodes[0] == () and sorted(nodes) == list(range(len(lex.prefixes)))
    assert trie.NodeWords(0) == [] and trie.Child(0, 0) == -1
    rng = np.random.default_rng(3)
    for _ in range(300):
        t = tuple(int(c) for c in rng.integers(1, lex.K, size=int(rng.integers(1, 7))))
        assert (_walk(trie, t) >= 0) == (t in lex.prefixes), t
    table = tmp_path / "words.txt"
    trie.WriteWords(str(table))
    assert table.read_text() == "".join(f"{n} {w}\n" for n, w in sorted(lex.ids.items(), key=lambda kv: kv[1]))


def test_homophones_prefix_words_second_spellings_and_repeated_lines(tmp_path):
    from eesen_amd.api import EesenError, Lexicon
    path = tmp_path / "l.txt"
    path.write_text("two 5 2\nab 2 3\na 2\nto 5 2\ntwo 6\nab 2 3\ntoo 5 2\nto 5 2\n")
    trie = Lexicon(str(path), None, K=7, space=None)
    assert trie.Info() == dict(words=5, nodes=6, max_word_len=2) and trie.MaxHomophones() == 3
    assert trie.NodeWords(_walk(trie, (5, 2))) == [1, 4, 5] and trie.Word(_walk(trie, (5, 2))) == 1          # two = 1, to = 4, too = 5
    assert trie.NodeWords(_walk(trie, (6,))) == [1] and trie.NodeWords(_walk(trie, (5,))) == []
    a = trie.Child(0, 2)
    assert trie.NodeWords(a) == [3] and trie.NodeWords(trie.Child(a, 3)) == [2]                               # a = 3 is a prefix of ab = 2
    for node in (-1, 6):
        with pytest.raises(EesenError):
            trie.NodeWords(node)
    with pytest.raises(EesenError) as e:          # the segmentation of a labelling is ambiguous
        trie.Words([5, 2])
    assert e.value.code == -1 and "eesen_ctc_decode_parallel_words" in str(e.value)
    # K = 2 is enough: the blank and one unit
    (tmp_path / "one.txt").write_text("x 1\nxx 1 1\n")
    assert Lexicon(str(tmp_path / "one.txt"), None, K=2, space=None).Info()["words"] == 2


MALFORMED = [
    ("a 2\nc 2 9\n", None, "l.txt:2", "unit 9 outside [1, K)"),
    ("a 2\nb 0\n", None, "l.txt:2", "unit 0 outside [1, K)"),
    ("a 2\nb x\n", None, "l.txt:2", "no decimal class id"),
    ("a a\nc a q\n", "units", "l.txt:2", "unit q is not in the units table"),
    ("a a\n\nb\n", "units", "l.txt:3", "word b has an empty spelling"),
    ("", None, "l.txt", "holds no word"),
    ("\n \n", None, "l.txt", "holds no word"),
]


@pytest.mark.parametrize("text,units,where,words", MALFORMED)
def test_malformed_lexicons_are_errors_with_file_and_line(text, units, where, words, tmp_path):
    from eesen_amd.api import EesenError, Lexicon
    (tmp_path / "l.txt").write_text(text)
    (tmp_path / "units").write_text("a 1\nb 2\nc 3\n")
    with pytest.raises(EesenError) as e:
        Lexicon(str(tmp_path / "l.txt"), str(tmp_path / units) if units else None, K=4, space=None)
    assert e.value.code == -1 and where in str(e.value) and words in str(e.value), str(e.value)


def test_the_sixteenth_homophone_is_refused_and_both_lines_are_named(tmp_path):
    from eesen_amd.api import EesenError, Lexicon
    lines = ["other 3\n"] + [f"h{i} 1 2\n" for i in range(15)]
    (tmp_path / "ok.txt").write_text("".join(lines) + "h3 1 2\n")          # fifteen, and one of them again
    trie = Lexicon(str(tmp_path / "ok.txt"), None, K=4, space=None)
    assert trie.MaxHomophones() == 15 and trie.NodeWords(_walk(trie, (1, 2))) == list(range(2, 17))
    (tmp_path / "l.txt").write_text("".join(lines) + "late 3 3\nh15 1 2\n")
    with pytest.raises(EesenError) as e:
        Lexicon(str(tmp_path / "l.txt"), None, K=4, space=None)
    msg = str(e.value)
    assert e.value.code == -1 and "l.txt:18" in msg and "h15" in msg and "15 words with the same spelling" in msg and "h0, line 2" in msg, msg
    for kw, words in ((dict(K=1), "K >= 2"), (dict(K=0), "K >= 2")):
        with pytest.raises(EesenError) as e:
            Lexicon(str(tmp_path / "ok.txt"), None, space=None, **kw)
        assert words in str(e.value)
    with pytest.raises(EesenError) as e:
        Lexicon(str(tmp_path / "none.txt"), None, K=4, space=None)
    assert "cannot open" in str(e.value)


@pytest.mark.parametrize("name", ["exhaustive", "k7_sp3", "k30_sp1"])
def test_a_spaced_lexicon_is_what_it_was(name, tmp_path):
    """Every (node, class) and every node's word of a lexicon built through eesen_lex_create, against the answers the set definition
    gives; homophones are still refused there, and the unspaced kind's accessors say that it has none."""
    from eesen_amd.api import EesenError, Lexicon
    lex = X.lex_of(name)
    trie = Lexicon(lex.write(tmp_path, "spaced"), None, K=lex.K, space=lex.space)
    assert not trie.unspaced and trie.MaxHomophones() == 0
    order = sorted(lex.prefixes, key=lambda p: (len(p), p))
    node = {pre: _walk(trie, pre) for pre in order}
    fixture = {(node[pre], c): node.get(pre + (c,), -1) for pre in order for c in range(1, lex.K)}          # Child, from the restatement
    assert sorted(node.values()) == list(range(len(order)))
    for (v, c), want in fixture.items():
        assert trie.Child(v, c) == want, (v, c)
    for pre in order:
        w = lex.spell.get(pre, 0)
        assert trie.Word(node[pre]) == w and trie.NodeWords(node[pre]) == ([w] if w else []), pre
    sp = lex.spelling_of([1, 2, 1])
    assert trie.Words(sp) == [1, 2, 1]
    (tmp_path / "hom.txt").write_text("a 2 3\nc 3\nb 2 3\n")
    with pytest.raises(EesenError) as e:
        Lexicon(str(tmp_path / "hom.txt"), None, K=4, space=1)
    assert "hom.txt:3" in str(e.value) and "words a and b have the same spelling" in str(e.value)


def test_malformed_files_under_the_sanitizers(tmp_path):
    """tests/native/words_lex_malformed.cc with lex.cpp, address and undefined-behaviour sanitizers, as a program of its own (the
    runtimes linked statically: the program needs nothing from its environment)."""
    from eesen_amd import build as hb
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hb.hipcc()))), "include")
    exe = str(tmp_path / "words_lex_malformed")
    csrc = os.path.join(ROOT, "eesen_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                        "-D__HIP_PLATFORM_AMD__",
                        "-I" + rocm_include, os.path.join(ROOT, "tests", "native", "words_lex_malformed.cc"), os.path.join(csrc, "lex.cpp"),
                        os.path.join(csrc, "lm.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    scratch = tmp_path / "files"
    scratch.mkdir()
    r = subprocess.run([exe, str(scratch)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("0 failures") and "runtime error" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
