"""-m gpu: --ctm-out of the ctc-decode tools (eesen_amd/bin/ctc-decode and python -m eesen_amd.ctc_decode): a tiny model, the unspaced
K = 7 lexicon with a word LM, and the plain search with a units table.  The two tools write byte-identical CTM files with and without
--ctm-conf; a file has one line per word of every 1-best hypothesis, `key 1 start dur word [conf]`, whose numbers are the api's
(Ctc.DecodeStamps) times --frame-shift, printed in fixed notation; a word ends no later than the next one starts; the final log line
counts the words.  Without --ctm-out every other output file is byte for byte what it is with it, and the log is the same but for
that count."""
import os
import re
import subprocess
import sys
from decimal import Decimal

import numpy as np
import pytest

from eesen_amd import kaldi_io, nnet_io, synth
from tests import ctc_lm_restatement as L
from tests import ctc_words_restatement as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "eesen_amd", "bin", "ctc-decode")
NATIVE, PYTHON = [EXE], [sys.executable, "-m", "eesen_amd.ctc_decode"]
SHIFT = 0.03
CTM_WORDS = r"LOG \(ctc-decode:main\(\)\) Done (\d+) utterances, [^\n]*; (\d+) CTM words\n"


def _run(host, args):
    r = subprocess.run(host + args, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


@pytest.fixture(scope="module")
def data(gpu, tmp_path_factory):
    """2 BiLSTM layers of 32 cells, D = 8, K = 7; five utterances of 20-45 frames; the 12-word unspaced lexicon of the K = 7 cases,
    its units named u1 .. u6; an order-3 word model named as the lexicon names its words."""
    assert os.path.exists(EXE), "run python -m eesen_amd.build"
    tmp = tmp_path_factory.mktemp("ctc_ctm")
    cfg = dict(synth.config("tiny_bi"), H=32)
    assert cfg["K"] == 7
    rng = np.random.default_rng(29)
    feats = [(f"utt{i}", rng.standard_normal((int(rng.integers(20, 46)), cfg["D"])).astype(np.float32) * np.float32(3)) for i in range(5)]
    feats.sort(key=lambda kv: kv[1].shape[0])
    ark, model = str(tmp / "feats.ark"), str(tmp / "final.nnet")
    kaldi_io.write_mat_ark(ark, feats)
    nnet_io.write_nnet(model, synth.make_model(**cfg), binary=True)
    lex = W.lex_of("k7")
    names = [None] + [f"u{c}" for c in range(1, lex.K)]
    units = str(tmp / "units.txt")
    open(units, "w").write("".join(f"{names[c]} {c}\n" for c in range(1, lex.K)))
    lexicon = lex.write(tmp, "lexicon", names)
    m = W.model_of("v12_o3_unk")
    by_id = {w: n for n, w in lex.ids.items()}
    arpa, _ = L.Model(m.K, m.order, m.grams, [None] + [by_id[w] for w in range(1, lex.V + 1)]).write(tmp, "words")
    return dict(tmp=tmp, feats=feats, ark=ark, model=model, lex=lex, by_id=by_id, lexicon=lexicon, units=units, arpa=arpa)


def _lex_args(data, tag, extra):
    out = lambda what: str(data["tmp"] / f"lex_{what}_{tag}")
    return extra + ["--word-boundary=none", "--lexicon=" + data["lexicon"], "--lexicon-units=" + data["units"], "--word-lm=" + data["arpa"], "--lm-weight=0.7",
                    "--word-bonus=0.4", "--lm-eos=true", "--num-sequence=3", "--nbest=3", "--beam=16", "--max-classes=6", "--scores-out=" + out("scores"),
                    "--words-wspecifier=ark:" + out("words"), "--word-ends-wspecifier=ark:" + out("ends"), data["model"], "ark:" + data["ark"], "ark:" + out("hyp")]


@pytest.fixture(scope="module")
def lex_runs(data):
    """tag -> the finished run: both tools, with the CTM and with the CTM and its confidences."""
    ctm = lambda tag: ["--ctm-out=" + str(data["tmp"] / f"lex_ctm_{tag}"), f"--frame-shift={SHIFT}"]
    return {tag: _run(host, _lex_args(data, tag, ctm(tag) + more)) for tag, host, more in
            (("cc", NATIVE, []), ("py", PYTHON, []), ("cc_conf", NATIVE, ["--ctm-conf=true", "--conf-scale=0.5"]),
             ("py_conf", PYTHON, ["--ctm-conf=true", "--conf-scale=0.5"]))}


def _ctm(path, columns):
    """key -> [(start, dur, word[, conf])] as Decimals and the word, in file order; every line has `columns` fields and channel 1."""
    out = {}
    for line in open(path):
        f = line.split()
        assert len(f) == columns and f[1] == "1" and line == " ".join(f) + "\n", line
        out.setdefault(f[0], []).append((Decimal(f[2]), Decimal(f[3]), f[4]) + ((Decimal(f[5]),) if columns == 6 else ()))
    return out


def _ordered(ctm):
    for key, rows in ctm.items():
        for a, b in zip(rows[:-1], rows[1:]):
            assert a[0] + a[1] <= b[0], (key, a, b)
        assert all(r[1] > 0 for r in rows), key


def test_lexicon_ctm_of_both_tools_and_the_api(data, lex_runs):
    from eesen_amd.api import Net, Ctc, Lexicon, TokenLm
    tmp, lex = data["tmp"], data["lex"]
    f = lambda what, tag: str(tmp / f"lex_{what}_{tag}")
    assert open(f("ctm", "cc"), "rb").read() == open(f("ctm", "py"), "rb").read()
    assert open(f("ctm", "cc_conf"), "rb").read() == open(f("ctm", "py_conf"), "rb").read()
    plain, conf = _ctm(f("ctm", "cc"), 5), _ctm(f("ctm", "cc_conf"), 6)
    assert {k: [r[:3] for r in v] for k, v in conf.items()} == plain           # the sixth column is the only difference
    _ordered(plain)
    words = kaldi_io.read_vec_int_table("ark:" + f("words", "cc"))
    best = {k[:-2]: v for k, v in words.items() if k.endswith("-1")}
    total = sum(len(v) for v in best.values())
    assert total > 0 and sum(len(v) for v in plain.values()) == total
    for key, ids in best.items():
        assert [r[2] for r in plain.get(key, [])] == [data["by_id"][int(w)] for w in ids], key       # the lexicon's word symbols
    for tag, r in lex_runs.items():
        m = re.search(CTM_WORDS, r.stderr)
        assert m and m.group(1) == "5" and int(m.group(2)) == total, (tag, r.stderr[-1000:])
    # the numbers are the api's
    table = str(tmp / "words_table.txt")
    trie = Lexicon(data["lexicon"], data["units"], K=lex.K, space=None)
    trie.WriteWords(table)
    lm = TokenLm(data["arpa"], table, K=lex.V + 1)
    net = Net().Read(data["model"])
    net.SetTestMode()
    ctc = Ctc()
    for key, m in data["feats"]:
        n = m.shape[0]
        net.SetSeqLengths([n])
        out = net.Propagate(m)
        hyps, score = ctc.DecodeParallel([n], out, beam=16, max_classes=6, nbest=3, lexicon=trie, lm=lm, lm_weight=0.7, word_bonus=0.4, lm_eos=True)
        st = ctc.DecodeStamps([n], out, conf_scale=0.5)
        nw = int(ctc.words_len[0, 0])
        want = [(f"{SHIFT * int(b):.2f}", f"{SHIFT * int(e - b):.2f}", data["by_id"][int(w)], f"{float(c):.2f}")
                for w, b, e, c in zip(ctc.words[0, 0, :nw], st.word_start[0, 0, :nw], st.word_end[0, 0, :nw], st.word_conf[0, 0, :nw])]
        assert [tuple(str(x) for x in r) for r in conf.get(key, [])] == want, key
        assert all(0 <= r[3] <= 1 for r in conf.get(key, [])), key


def test_without_ctm_out_nothing_changes(data, lex_runs):
    tmp = data["tmp"]
    f = lambda what, tag: str(tmp / f"lex_{what}_{tag}")
    strip = lambda text: [l for l in text.splitlines() if l.startswith(("LOG", "WARNING"))]
    for tag, host in (("cc_none", NATIVE), ("py_none", PYTHON)):
        r = _run(host, _lex_args(data, tag, []))
        with_ctm = tag[:2]
        for what in ("hyp", "words", "ends", "scores"):
            assert open(f(what, tag), "rb").read() == open(f(what, with_ctm), "rb").read() == open(f(what, with_ctm + "_conf"), "rb").read(), (what, tag)
        assert not os.path.exists(f("ctm", tag)) and "CTM" not in r.stderr
        assert strip(r.stderr) == [re.sub(r"; \d+ CTM words$", "", l) for l in strip(lex_runs[with_ctm].stderr)], tag


def test_plain_ctm_names_units_or_class_ids(data):
    tmp = data["tmp"]
    f = lambda what, tag: str(tmp / f"plain_{what}_{tag}")
    args = lambda tag, extra: extra + ["--ctm-out=" + f("ctm", tag), f"--frame-shift={SHIFT}", "--ctm-precision=3", "--ctm-conf=true", "--nbest=2", "--beam=8",
                                       "--num-sequence=2", data["model"], "ark:" + data["ark"], "ark,t:" + f("hyp", tag)]
    named = ["--ctm-units=" + data["units"]]
    _run(NATIVE, args("cc", named)), _run(PYTHON, args("py", named)), _run(NATIVE, args("cc_ids", []))
    assert open(f("ctm", "cc"), "rb").read() == open(f("ctm", "py"), "rb").read()
    ctm, ids = _ctm(f("ctm", "cc"), 6), _ctm(f("ctm", "cc_ids"), 6)
    _ordered(ctm)
    hyp = {l.split()[0]: l.split()[1:] for l in open(f("hyp", "cc"))}
    best = {k[:-2]: v for k, v in hyp.items() if k.endswith("-1")}
    assert sum(len(v) for v in best.values()) == sum(len(v) for v in ctm.values()) > 0
    for key, labels in best.items():
        assert [r[2] for r in ctm.get(key, [])] == ["u" + c for c in labels] and [r[2] for r in ids.get(key, [])] == labels, key
        assert [r[:2] + r[3:] for r in ctm.get(key, [])] == [r[:2] + r[3:] for r in ids.get(key, [])], key
        assert all(len(str(r[0]).split(".")[1]) == 3 for r in ctm.get(key, [])), key


def test_ctm_misuse_is_refused(data):
    tail = [data["model"], "ark:" + data["ark"], "ark,t:" + str(data["tmp"] / "hyp_err.ark")]
    ctm = "--ctm-out=" + str(data["tmp"] / "err.ctm")
    for host in (NATIVE, PYTHON):
        run = lambda args: subprocess.run(host + args + tail, capture_output=True, text=True, cwd=ROOT, timeout=600)
        r = run(["--ctm-conf=true"])
        assert r.returncode == 255 and "need --ctm-out" in r.stderr, r.stderr[-1000:]
        r = run([ctm, "--conf-scale=-1"])
        assert r.returncode == 255 and "conf_scale" in r.stderr, r.stderr[-1000:]
