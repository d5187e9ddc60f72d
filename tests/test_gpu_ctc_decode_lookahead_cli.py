"""-m gpu: the ctc-decode tools with --lm-lookahead (eesen_amd/bin/ctc-decode and python -m eesen_amd.ctc_decode): a tiny model, the
12-word lexicons of the K = 7 cases (spaced and unspaced) and a Zipf word model.  With the flag the two tools write byte-identical
hypothesis, word and scores files, which are what the api returns with lm_lookahead=True, and say so in the start-up log; without it
they write what they wrote before; without --word-lm the library's refusal reaches the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

from eesen_amd import kaldi_io, nnet_io, synth
from tests import ctc_lex_cases as xc
from tests import ctc_lm_restatement as L
from tests import ctc_lookahead_cases as kc
from tests import ctc_words_cases as wc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "eesen_amd", "bin", "ctc-decode")
SPACE = 3
DECODE = dict(beam=4, max_classes=6, nbest=2)          # a beam narrow enough for the look-ahead to change what comes back


@pytest.fixture(scope="module")
def data(gpu, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ctc_decode_la")
    cfg = dict(synth.config("tiny_bi"), H=32)
    assert cfg["K"] == 7
    rng = np.random.default_rng(41)
    feats = [(f"utt{i}", rng.standard_normal((int(rng.integers(20, 46)), cfg["D"])).astype(np.float32) * np.float32(3)) for i in range(4)]
    feats.sort(key=lambda kv: kv[1].shape[0])
    ark, model = str(tmp / "feats.ark"), str(tmp / "final.nnet")
    kaldi_io.write_mat_ark(ark, feats)
    nnet_io.write_nnet(model, synth.make_model(**cfg), binary=True)
    m = kc.model_of("zipf_v12_unk")
    out = dict(tmp=tmp, feats=feats, ark=ark, model=model)
    for kind, lex in (("unit", xc.lexicon("k7_sp3")), ("none", wc.lexicon("k7"))):
        assert lex.V + 1 == m.K
        by_id = {w: n for n, w in lex.ids.items()}
        arpa, _ = L.Model(m.K, m.order, m.grams, [None] + [by_id[w] for w in range(1, lex.V + 1)]).write(tmp, "words_" + kind)
        out[kind] = dict(lex=lex, lexicon=lex.write(tmp, "lexicon_" + kind), arpa=arpa)
    return out


def _both(args):
    assert os.path.exists(EXE), "run python -m eesen_amd.build"
    r_cc = subprocess.run([EXE] + args("cc"), capture_output=True, text=True, timeout=600)
    r_py = subprocess.run([sys.executable, "-m", "eesen_amd.ctc_decode"] + args("py"), capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r_cc.returncode == 0 and r_py.returncode == 0, (r_cc.stderr[-2000:], r_py.stderr[-2000:])
    return r_cc, r_py


def _args(data, kind, flag, out):
    d = data[kind]
    a = ["--lexicon=" + d["lexicon"], "--word-boundary=" + kind, "--word-lm=" + d["arpa"], "--lm-weight=0.9", "--word-bonus=0.3", "--lm-eos=true",
         "--num-sequence=2", "--beam=%d" % DECODE["beam"], "--max-classes=%d" % DECODE["max_classes"], "--nbest=%d" % DECODE["nbest"]]
    if kind == "unit":
        a.append(f"--space-unit={SPACE}")
    if flag is not None:
        a.append("--lm-lookahead=" + flag)
    return lambda tag: a + ["--scores-out=" + out(tag, "scores"), "--words-wspecifier=ark:" + out(tag, "words"), "--words-table-out=" + out(tag, "table"),
                            data["model"], "ark:" + data["ark"], "ark:" + out(tag, "hyp")]


def _api(data, kind, table, la):
    """{key-i: (labels, words, score)} of the api on every utterance by itself."""
    from eesen_amd.api import Net, Ctc, Lexicon, TokenLm
    d = data[kind]
    trie = Lexicon(d["lexicon"], None, K=d["lex"].K, space=SPACE if kind == "unit" else None)
    lm = TokenLm(d["arpa"], table, K=d["lex"].V + 1)
    net = Net().Read(data["model"])
    net.SetTestMode()
    ctc = Ctc()
    want = {}
    for key, m in data["feats"]:
        net.SetSeqLengths([m.shape[0]])
        hyps, score = ctc.DecodeParallel([m.shape[0]], net.Propagate(m), lexicon=trie, lm=lm, lm_weight=0.9, word_bonus=0.3, lm_eos=True, lm_lookahead=la, **DECODE)
        for i, h in enumerate(hyps[0]):
            want[f"{key}-{i + 1}"] = (list(h), ctc.words[0, i, :ctc.words_len[0, i]].tolist(), score[0, i])
    return want, trie.Lookahead(lm)


def _is_the_api(out, want):
    got = kaldi_io.read_vec_int_table("ark:" + out("cc", "hyp"))
    words = kaldi_io.read_vec_int_table("ark:" + out("cc", "words"))
    lines = {l.split()[0]: np.float32(float(l.split()[1])) for l in open(out("cc", "scores"))}
    assert list(got) == list(words) == list(want)
    for k, (h, w, s) in want.items():
        assert got[k].tolist() == h and words[k].tolist() == w and lines[k] == s, k


@pytest.mark.parametrize("kind", ["unit", "none"])
def test_tools_with_the_flag_equal_each_other_and_the_api(data, kind):
    out = lambda tag, what: str(data["tmp"] / f"{kind}_on_{what}_{tag}")
    r_cc, r_py = _both(_args(data, kind, "true", out))
    for what in ("hyp", "words", "scores", "table"):
        assert open(out("cc", what), "rb").read() == open(out("py", what), "rb").read(), what
    want, la = _api(data, kind, out("cc", "table"), True)
    _is_the_api(out, want)
    for r in (r_cc, r_py):
        assert f"LOG (ctc-decode:main()) unigram look-ahead over {la.size} lexicon nodes, la in [{float(la.min()):.9g}, {float(la[0]):.9g}]\n" in r.stderr, r.stderr[-1500:]
    off, _ = _api(data, kind, out("cc", "table"), False)
    print(f"{kind}: {sum(1 for k in want if off.get(k) != want[k])} of {len(want)} returned entries differ from the search without the flag")


def test_without_the_flag_nothing_changes(data):
    out = lambda tag, what: str(data["tmp"] / f"unit_off_{what}_{tag}")
    r_cc, r_py = _both(_args(data, "unit", None, out))
    for what in ("hyp", "words", "scores"):
        assert open(out("cc", what), "rb").read() == open(out("py", what), "rb").read(), what
    want, _ = _api(data, "unit", out("cc", "table"), False)
    _is_the_api(out, want)
    for r in (r_cc, r_py):
        assert "look-ahead" not in r.stderr
    out2 = lambda tag, what: str(data["tmp"] / f"unit_false_{what}_{tag}")
    _both(_args(data, "unit", "false", out2))
    for tag in ("cc", "py"):
        for what in ("hyp", "words", "scores"):
            assert open(out2(tag, what), "rb").read() == open(out("cc", what), "rb").read(), (tag, what)


def test_refusals_reach_the_command_line(data):
    tail = [data["model"], "ark:" + data["ark"], "ark,t:" + str(data["tmp"] / "hyp_err.ark")]
    for host in ([EXE], [sys.executable, "-m", "eesen_amd.ctc_decode"]):
        run = lambda args: subprocess.run(host + args + tail, capture_output=True, text=True, cwd=ROOT, timeout=600)
        r = run(["--lexicon=" + data["unit"]["lexicon"], f"--space-unit={SPACE}", "--lm-lookahead=true"])
        assert r.returncode == 255 and "look-ahead" in r.stderr and "needs the word LM" in r.stderr, r.stderr[-1000:]
        r = run(["--lm-lookahead=true"])
        assert r.returncode == 255 and "--lm-lookahead needs --lexicon and --word-lm" in r.stderr, r.stderr[-1000:]
