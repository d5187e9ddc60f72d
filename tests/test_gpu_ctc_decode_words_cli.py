"""-m gpu: the ctc-decode tools with --word-boundary=none (eesen_amd/bin/ctc-decode and python -m eesen_amd.ctc_decode): a tiny model, a
lexicon without a boundary unit that has a homophone pair, with a units table, and a word n-gram LM.  The two tools write
byte-identical hypothesis, word, word-end and scores files and the same words table; words and ends are what the api returns and
cut the labels into spellings; the word-error line is a Python count; --space-unit beside none is refused; without the option, and
with --word-boundary=unit, a lexicon with a space unit decodes as it did."""
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
FINAL = (r"LOG \(ctc-decode:main\(\)\) Done (\d+) utterances, (\d+) empty hypotheses; average log-probability per frame ([-0-9.e]+)"
         r"; average LM log-probability per word ([-0-9.e]+)\n")


@pytest.fixture(scope="module")
def data(gpu, tmp_path_factory):
    """2 BiLSTM layers of 32 cells, D = 8, K = 7; five utterances of 20-45 frames; the 12-word unspaced lexicon of the K = 7 cases (one
    homophone pair), its units named u1 .. u6; an order-3 word model named as the lexicon names its words."""
    tmp = tmp_path_factory.mktemp("ctc_decode_words")
    cfg = dict(synth.config("tiny_bi"), H=32)
    assert cfg["K"] == 7
    rng = np.random.default_rng(29)
    feats = [(f"utt{i}", rng.standard_normal((int(rng.integers(20, 46)), cfg["D"])).astype(np.float32) * np.float32(3)) for i in range(5)]
    feats.sort(key=lambda kv: kv[1].shape[0])
    ark, model = str(tmp / "feats.ark"), str(tmp / "final.nnet")
    kaldi_io.write_mat_ark(ark, feats)
    nnet_io.write_nnet(model, synth.make_model(**cfg), binary=True)
    lex = W.lex_of("k7")
    assert lex.H == 2
    names = [None] + [f"u{c}" for c in range(1, lex.K)]
    units = str(tmp / "units.txt")
    open(units, "w").write("".join(f"{names[c]} {c}\n" for c in range(1, lex.K)))
    lexicon = lex.write(tmp, "lexicon", names)
    m = W.model_of("v12_o3_unk")
    by_id = {w: n for n, w in lex.ids.items()}
    arpa, _ = L.Model(m.K, m.order, m.grams, [None] + [by_id[w] for w in range(1, lex.V + 1)]).write(tmp, "words")
    return dict(tmp=tmp, cfg=cfg, feats=feats, ark=ark, model=model, lex=lex, lexicon=lexicon, units=units, arpa=arpa, wmodel=m)


def _run(host, args):
    r = subprocess.run(host + args, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


NATIVE, PYTHON = [EXE], [sys.executable, "-m", "eesen_amd.ctc_decode"]


def _edit_distance(ref, hyp):
    d = list(range(len(hyp) + 1))
    for i in range(1, len(ref) + 1):
        prev, d[0] = d[0], i
        for j in range(1, len(hyp) + 1):
            prev, d[j] = d[j], min(prev + (ref[i - 1] != hyp[j - 1]), d[j] + 1, d[j - 1] + 1)
    return d[len(hyp)]


def test_words_tools_equal_each_other_and_the_api(data):
    from eesen_amd.api import Net, Ctc, Lexicon, TokenLm
    assert os.path.exists(EXE), "run python -m eesen_amd.build"
    tmp, feats, lex = data["tmp"], data["feats"], data["lex"]
    out = lambda tag, what: str(tmp / f"w_{what}_{tag}")
    rng = np.random.default_rng(31)
    refs = {key: rng.integers(1, lex.V + 1, size=int(rng.integers(1, 4))).astype(np.int32) for key, _ in feats[:4]}          # one utterance has none
    kaldi_io.write_vec_int_ark(str(tmp / "word_refs.ark"), refs.items())
    args = lambda tag: ["--word-boundary=none", "--lexicon=" + data["lexicon"], "--lexicon-units=" + data["units"], "--word-lm=" + data["arpa"], "--lm-weight=0.7",
                        "--word-bonus=0.4", "--lm-eos=true", "--word-ref-rspecifier=ark:" + str(tmp / "word_refs.ark"), "--num-sequence=3", "--nbest=3",
                        "--beam=16", "--max-classes=6", "--scores-out=" + out(tag, "scores"), "--words-wspecifier=ark:" + out(tag, "words"),
                        "--word-ends-wspecifier=ark:" + out(tag, "ends"), "--words-table-out=" + out(tag, "table"), data["model"], "ark:" + data["ark"],
                        "ark:" + out(tag, "hyp")]
    r_cc, r_py = _run(NATIVE, args("cc")), _run(PYTHON, args("py"))
    for what in ("hyp", "words", "ends", "scores", "table"):
        assert open(out("cc", what), "rb").read() == open(out("py", what), "rb").read(), what
    assert open(out("cc", "table")).read() == "".join(f"{n} {w}\n" for n, w in sorted(lex.ids.items(), key=lambda kv: kv[1]))
    got = kaldi_io.read_vec_int_table("ark:" + out("cc", "hyp"))
    words = kaldi_io.read_vec_int_table("ark:" + out("cc", "words"))
    ends = kaldi_io.read_vec_int_table("ark:" + out("cc", "ends"))
    lines = [l.split() for l in open(out("cc", "scores"))]
    assert all(len(l) == 3 for l in lines) and [l[0] for l in lines] == list(got) == list(words) == list(ends)
    trie = Lexicon(data["lexicon"], data["units"], K=lex.K, space=None)
    lm = TokenLm(data["arpa"], out("cc", "table"), K=lex.V + 1)
    net = Net().Read(data["model"])
    net.SetTestMode()
    ctc = Ctc()
    by_key = {l[0]: (float(l[1]), float(l[2])) for l in lines}
    keys, tot_lm, tot_words, tot_score, tot_frames, err, nref, scored = [], 0.0, 0, 0.0, 0, 0, 0, 0
    for key, m in feats:
        net.SetSeqLengths([m.shape[0]])
        hyps, score = ctc.DecodeParallel([m.shape[0]], net.Propagate(m), beam=16, max_classes=6, nbest=3, lexicon=trie, lm=lm, lm_weight=0.7, word_bonus=0.4,
                                         lm_eos=True)
        assert hyps[0], key
        for i, h in enumerate(hyps[0]):
            k = f"{key}-{i + 1}"
            keys.append(k)
            nw = int(ctc.words_len[0, i])
            assert np.array_equal(got[k], np.asarray(h, np.int32)), k
            assert np.array_equal(words[k], ctc.words[0, i, :nw]) and np.array_equal(ends[k], ctc.word_ends[0, i, :nw]), k
            assert lex.consistent(tuple(h), tuple(words[k].tolist()), tuple(ends[k].tolist())), k
            assert np.float32(by_key[k][0]) == score[0, i] and np.float32(by_key[k][1]) == ctc.lm_score[0, i], k
        best = ctc.words[0, 0, :ctc.words_len[0, 0]].tolist()
        tot_lm += float(ctc.lm_score[0, 0]); tot_words += len(best); tot_score += float(score[0, 0]); tot_frames += m.shape[0]
        if key in refs:
            err += _edit_distance(refs[key].tolist(), best); nref += refs[key].size; scored += 1
    assert list(got) == keys and scored == 4
    for r in (r_cc, r_py):
        assert f"LOG (ctc-decode:main()) the largest homophone set of {data['lexicon']} holds 2 words\n" in r.stderr, r.stderr[-1500:]
        assert f"LOG (ctc-decode:main()) {err} word errors on {nref} reference words of {scored} utterances\n" in r.stderr, r.stderr[-1500:]
        acc = re.search(r"LOG \(ctc-decode:main\(\)\) \nWORD_ACCURACY >> ([-0-9.e]+)% <<\n", r.stderr)
        assert acc and abs(float(acc.group(1)) - 100.0 * (1.0 - err / nref)) < 1e-3, r.stderr[-1500:]
        m = re.search(FINAL, r.stderr)
        assert m and m.group(1) == "5", r.stderr[-1000:]
        assert abs(float(m.group(3)) - tot_score / tot_frames) < 1e-4 * max(1.0, abs(tot_score / tot_frames))
        assert abs(float(m.group(4)) - tot_lm / max(tot_words, 1)) < 1e-4 * max(1.0, abs(tot_lm / max(tot_words, 1)))


def test_space_unit_beside_none_and_other_misuse_is_refused(data):
    tail = [data["model"], "ark:" + data["ark"], "ark,t:" + str(data["tmp"] / "hyp_err.ark")]
    lexicon = ["--lexicon=" + data["lexicon"], "--lexicon-units=" + data["units"]]
    for host in (NATIVE, PYTHON):
        run = lambda args: subprocess.run(host + args + tail, capture_output=True, text=True, cwd=ROOT, timeout=600)
        r = run(["--word-boundary=none", "--space-unit=X"] + lexicon)
        assert r.returncode == 255 and "--space-unit=X together with --word-boundary=none" in r.stderr, r.stderr[-1000:]
        r = run(["--word-boundary=none"])
        assert r.returncode == 255 and "--word-boundary=none needs --lexicon" in r.stderr, r.stderr[-1000:]
        r = run(["--word-boundary=blank"] + lexicon)
        assert r.returncode == 255 and "neither unit nor none" in r.stderr, r.stderr[-1000:]
        r = run(["--word-ends-wspecifier=ark:" + str(data["tmp"] / "ends_err.ark"), "--space-unit=u3"] + lexicon)
        assert r.returncode == 255 and "--word-ends-wspecifier needs --word-boundary=none" in r.stderr, r.stderr[-1000:]


def test_a_spaced_lexicon_decodes_as_before_with_and_without_the_option(data):
    tmp = data["tmp"]
    lex = X.lex_of("k7_sp3")
    numbers = lex.write(tmp, "spaced_numbers")
    out = lambda tag, what: str(tmp / f"sp_{what}_{tag}")
    args = lambda tag, extra: extra + ["--lexicon=" + numbers, f"--space-unit={lex.space}", "--word-bonus=-0.3", "--num-sequence=5", "--nbest=2",
                                       "--scores-out=" + out(tag, "scores"), "--words-wspecifier=ark,t:" + out(tag, "words"), data["model"], "ark:" + data["ark"],
                                       "ark,t:" + out(tag, "hyp")]
    runs = dict(cc=_run(NATIVE, args("cc", [])), cc_unit=_run(NATIVE, args("cc_unit", ["--word-boundary=unit"])), py_unit=_run(PYTHON, args("py_unit", ["--word-boundary=unit"])))
    for what in ("hyp", "words", "scores"):
        for tag in ("cc_unit", "py_unit"):
            assert open(out("cc", what), "rb").read() == open(out(tag, what), "rb").read(), (what, tag)
    hyp = {l.split()[0]: tuple(map(int, l.split()[1:])) for l in open(out("cc", "hyp"))}
    words = {l.split()[0]: tuple(map(int, l.split()[1:])) for l in open(out("cc", "words"))}
    assert hyp and list(hyp) == list(words) and all(lex.segment(hyp[k]) == words[k] for k in hyp)
    strip = lambda text: [l for l in text.splitlines() if l.startswith(("LOG", "WARNING"))]
    assert strip(runs["cc"].stderr) == strip(runs["cc_unit"].stderr) and "homophone" not in runs["cc"].stderr + runs["py_unit"].stderr
