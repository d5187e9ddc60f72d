"""-m gpu: --rescore of the ctc-decode tools (eesen_amd/bin/ctc-decode and python -m eesen_amd.ctc_decode): a tiny model, the unspaced
K = 7 lexicon with a word LM in the first pass and another in the second, and the plain search rescored with a token LM.  With
--rescore=true the two tools write byte-identical hypotheses, words, word ends, scores (`key total am lm`) and CTM files (with
--ctm-conf); the hypotheses are the first pass's in the order of Ctc.RescoreNbest, the numbers are the api's, and the final log line
counts the re-ranked utterances.  Without the flag -- no option, or --rescore=false -- every output byte is the same in both tools,
and the log does not speak of a second pass."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from eesen_amd import kaldi_io, nnet_io, synth
from tests import ctc_lex_restatement as X
from tests import ctc_lm_restatement as L
from tests import ctc_words_restatement as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "eesen_amd", "bin", "ctc-decode")
NATIVE, PYTHON = [EXE], [sys.executable, "-m", "eesen_amd.ctc_decode"]
RERANKED = r"LOG \(ctc-decode:main\(\)\) Done (\d+) utterances, [^\n]*; (\d+) utterances re-ranked\n"
FILES = ("hyp", "words", "ends", "scores", "ctm")


def _run(host, args):
    r = subprocess.run(host + args, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


@pytest.fixture(scope="module")
def data(gpu, tmp_path_factory):
    """The model, features, lexicon and first word model of tests/test_gpu_ctc_stamps_cli.py; a second word model over the same words
    (the spaced cases' model of the same shape) and a token model over the units u1 .. u6."""
    assert os.path.exists(EXE), "run python -m eesen_amd.build"
    tmp = tmp_path_factory.mktemp("ctc_rescore")
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
    by_id = {w: n for n, w in lex.ids.items()}
    word_names = [None] + [by_id[w] for w in range(1, lex.V + 1)]
    m1, m2 = W.model_of("v12_o3_unk"), X.model_of("v12_o3_unk")
    assert m1.K == m2.K == lex.V + 1
    first, _ = L.Model(m1.K, m1.order, m1.grams, word_names).write(tmp, "words_first")
    second, _ = L.Model(m2.K, m2.order, m2.grams, word_names).write(tmp, "words_second")
    t = L.model_of("k7_o2")
    tok, _ = L.Model(t.K, t.order, t.grams, names).write(tmp, "tokens")
    return dict(tmp=tmp, feats=feats, ark=ark, model=model, lex=lex, lexicon=lexicon, units=units, first=first, second=second, tok=tok)


def _lex_args(data, tag, extra):
    out = lambda what: str(data["tmp"] / f"lex_{what}_{tag}")
    return extra + ["--word-boundary=none", "--lexicon=" + data["lexicon"], "--lexicon-units=" + data["units"], "--word-lm=" + data["first"], "--lm-weight=0.7",
                    "--word-bonus=0.4", "--lm-eos=true", "--num-sequence=3", "--nbest=3", "--beam=4", "--max-classes=6", "--scores-out=" + out("scores"),
                    "--words-wspecifier=ark,t:" + out("words"), "--word-ends-wspecifier=ark,t:" + out("ends"), "--ctm-out=" + out("ctm"), "--ctm-conf=true",
                    "--conf-scale=0.5", "--frame-shift=0.03", data["model"], "ark:" + data["ark"], "ark,t:" + out("hyp")]


def _plain_args(data, tag, extra):
    out = lambda what: str(data["tmp"] / f"plain_{what}_{tag}")
    return extra + ["--num-sequence=2", "--nbest=4", "--beam=4", "--max-classes=6", "--scores-out=" + out("scores"), "--ctm-out=" + out("ctm"), "--ctm-conf=true",
                    "--ctm-units=" + data["units"], "--ctm-precision=3", data["model"], "ark:" + data["ark"], "ark,t:" + out("hyp")]


def _table(path):
    """key -> the rest of its line, in file order."""
    return {l.split()[0]: l.split()[1:] for l in open(path)}


def _lists(table):
    """utterance -> its entries in written order."""
    out = {}
    for k, v in table.items():
        out.setdefault(k.rsplit("-", 1)[0], []).append(v)
    return out


def test_lexicon_mode_both_tools(data):
    tmp = data["tmp"]
    f = lambda what, tag: str(tmp / f"lex_{what}_{tag}")
    second = ["--rescore=true", "--rescore-lm=" + data["second"], "--rescore-lm-weight=1.3", "--rescore-bonus=0.1", "--rescore-lm-eos=true"]
    runs = {tag: _run(host, _lex_args(data, tag, more)) for tag, host, more in
            (("cc", NATIVE, second), ("py", PYTHON, second), ("cc_first", NATIVE, []), ("py_first", PYTHON, []), ("cc_off", NATIVE, ["--rescore=false"]),
             ("py_off", PYTHON, ["--rescore=false"]))}
    for what in FILES:
        assert open(f(what, "cc"), "rb").read() == open(f(what, "py"), "rb").read(), what
        assert len({open(f(what, t), "rb").read() for t in ("cc_first", "py_first", "cc_off", "py_off")}) == 1, what      # without the flag
    counts = set()
    for tag in ("cc", "py"):
        m = re.search(RERANKED, runs[tag].stderr)
        assert m and m.group(1) == "5", runs[tag].stderr[-1000:]
        counts.add(m.group(2))
    assert len(counts) == 1
    for tag in ("cc_first", "py_first", "cc_off", "py_off"):
        assert "re-ranked" not in runs[tag].stderr
    strip = lambda text: [l for l in text.splitlines() if l.startswith(("LOG", "WARNING"))]
    assert strip(runs["cc_first"].stderr) == strip(runs["cc_off"].stderr) and strip(runs["py_first"].stderr) == strip(runs["py_off"].stderr)
    # the second pass permutes the first pass's entries: labels, words and word ends travel together
    for what in ("hyp", "words", "ends"):
        a, b = _lists(_table(f(what, "cc"))), _lists(_table(f(what, "cc_first")))
        assert a.keys() == b.keys() and all(sorted(a[k]) == sorted(b[k]) for k in a), what
    scores = _table(f("scores", "cc"))
    assert scores and all(len(v) == 3 for v in scores.values())                      # key total am lm
    for utt, rows in _lists(scores).items():
        totals = [float(r[0]) for r in rows]
        assert totals == sorted(totals, reverse=True), utt
    assert all(len(l.split()) == 6 and 0 <= float(l.split()[5]) <= 1 for l in open(f("ctm", "cc")))
    # the CTM speaks of the new best hypothesis
    words = _lists(_table(f("words", "cc")))
    ctm = {}
    for l in open(f("ctm", "cc")):
        ctm.setdefault(l.split()[0], []).append(l.split()[4])
    by_id = {w: n for n, w in data["lex"].ids.items()}
    for utt, rows in words.items():
        assert ctm.get(utt, []) == [by_id[int(w)] for w in rows[0]], utt


def test_plain_mode_both_tools_and_the_api(data):
    from eesen_amd.api import Net, Ctc, TokenLm
    tmp = data["tmp"]
    f = lambda what, tag: str(tmp / f"plain_{what}_{tag}")
    second = ["--rescore=true", "--rescore-lm=" + data["tok"], "--lm-units=" + data["units"], "--rescore-lm-weight=0.6", "--rescore-bonus=0.8"]
    runs = {tag: _run(host, _plain_args(data, tag, more)) for tag, host, more in
            (("cc", NATIVE, second), ("py", PYTHON, second), ("cc_first", NATIVE, []), ("py_first", PYTHON, []), ("cc_off", NATIVE, ["--rescore=false"]))}
    for what in ("hyp", "scores", "ctm"):
        assert open(f(what, "cc"), "rb").read() == open(f(what, "py"), "rb").read(), what
        assert len({open(f(what, t), "rb").read() for t in ("cc_first", "py_first", "cc_off")}) == 1, what
    hyp, first = _lists(_table(f("hyp", "cc"))), _lists(_table(f("hyp", "cc_first")))
    scores = _lists(_table(f("scores", "cc")))
    assert all(len(r) == 1 for rows in _lists(_table(f("scores", "cc_first"))).values() for r in rows)      # as ever: key log-probability
    # the numbers and the order are the api's
    lm = TokenLm(data["tok"], data["units"], K=7)
    net = Net().Read(data["model"])
    net.SetTestMode()
    ctc = Ctc()
    reranked = 0
    for key, m in data["feats"]:
        n = m.shape[0]
        net.SetSeqLengths([n])
        out = net.Propagate(m)
        hyps, _ = ctc.DecodeParallel([n], out, beam=4, max_classes=6, nbest=4)
        res = ctc.RescoreNbest([n], out, lm=lm, lm_weight=0.6, bonus=0.8)
        order = [int(r) for r in res.order[0] if r < len(hyps[0])]
        assert first[key] == [[str(c) for c in h] for h in hyps[0]], key
        assert hyp[key] == [[str(c) for c in hyps[0][r]] for r in order], key
        assert scores[key] == [[f"{float(a[0, r]):.9g}" for a in (res.total, res.am_score, res.lm_score)] for r in order], key
        reranked += order != sorted(order)
    for tag in ("cc", "py"):
        m = re.search(RERANKED, runs[tag].stderr)
        assert m and m.group(1) == "5" and int(m.group(2)) == reranked, (tag, runs[tag].stderr[-1000:])
    assert reranked > 0
    ctm = {}
    for l in open(f("ctm", "cc")):
        ctm.setdefault(l.split()[0], []).append(l.split()[4])
    for key, rows in hyp.items():
        assert ctm.get(key, []) == ["u" + c for c in rows[0]], key


def test_misuse_is_refused(data):
    tail = [data["model"], "ark:" + data["ark"], "ark,t:" + str(data["tmp"] / "hyp_err.ark")]
    for host in (NATIVE, PYTHON):
        run = lambda args: subprocess.run(host + args + tail, capture_output=True, text=True, cwd=ROOT, timeout=600)
        r = run(["--rescore-bonus=1"])
        assert r.returncode == 255 and "need --rescore=true" in r.stderr, r.stderr[-1000:]
        r = run(["--rescore=true", "--rescore-lm-weight=nan"])
        assert r.returncode == 255 and "must be finite" in r.stderr, r.stderr[-1000:]
        r = run(["--rescore=true", "--rescore-lm=" + data["second"]])          # a word LM (13 classes) over the net's 7
        assert r.returncode == 255, r.stderr[-1000:]
