"""-m gpu: the ctc-decode tools with --lexicon (eesen_amd/bin/ctc-decode and python -m eesen_amd.ctc_decode): a tiny model, a lexicon
with a units table and a word n-gram LM with out-of-vocabulary n-grams.  The two tools write byte-identical hypothesis, word and
scores files and the same words table; the words are the segmentation of the labels written and what the api returns; the word-error
line is a Python count; without --lexicon both write what they wrote before."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from eesen_amd import kaldi_io, nnet_io, synth
from tests import ctc_lex_cases as xc
from tests import ctc_lex_restatement as X
from tests import ctc_lm_restatement as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "eesen_amd", "bin", "ctc-decode")
FINAL = (r"LOG \(ctc-decode:main\(\)\) Done (\d+) utterances, (\d+) empty hypotheses; average log-probability per frame ([-0-9.e]+)"
         r"; average LM log-probability per word ([-0-9.e]+)\n")
SPACE = 3


@pytest.fixture(scope="module")
def data(gpu, tmp_path_factory):
    """2 BiLSTM layers of 32 cells, D = 8, K = 7; five utterances of 20-45 frames; the 12-word lexicon of the K = 7 cases, its units
    named u1 .. u6 with <SPACE> = 3; an order-3 word model, named as the lexicon names its words, with three n-grams over a word the
    lexicon does not have."""
    tmp = tmp_path_factory.mktemp("ctc_decode_lex")
    cfg = dict(synth.config("tiny_bi"), H=32)
    assert cfg["K"] == 7
    rng = np.random.default_rng(29)
    feats = [(f"utt{i}", rng.standard_normal((int(rng.integers(20, 46)), cfg["D"])).astype(np.float32) * np.float32(3)) for i in range(5)]
    feats.sort(key=lambda kv: kv[1].shape[0])
    ark, model = str(tmp / "feats.ark"), str(tmp / "final.nnet")
    kaldi_io.write_mat_ark(ark, feats)
    nnet_io.write_nnet(model, synth.make_model(**cfg), binary=True)
    lex = X.lex_of("k7_sp3")
    assert lex.space == SPACE
    names = [None] + [f"u{c}" if c != SPACE else "<SPACE>" for c in range(1, lex.K)]
    units = str(tmp / "units.txt")
    open(units, "w").write("".join(f"{names[c]} {c}\n" for c in range(1, lex.K)))
    lexicon = lex.write(tmp, "lexicon", names)
    m = X.model_of("v12_o3_unk")
    by_id = {w: n for n, w in lex.ids.items()}
    grams = dict(m.grams)
    grams.update({("zebra",): (-1.5, -0.25), (1, "zebra"): (-0.7, None), ("zebra", 3): (-0.4, None)})
    arpa, _ = L.Model(m.K, m.order, grams, [None] + [by_id[w] for w in range(1, lex.V + 1)]).write(tmp, "words")
    return dict(tmp=tmp, cfg=cfg, feats=feats, ark=ark, model=model, lex=lex, lexicon=lexicon, units=units, arpa=arpa, wmodel=m)


def _both(args):
    assert os.path.exists(EXE), "run python -m eesen_amd.build"
    r_cc = subprocess.run([EXE] + args("cc"), capture_output=True, text=True, timeout=600)
    r_py = subprocess.run([sys.executable, "-m", "eesen_amd.ctc_decode"] + args("py"), capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r_cc.returncode == 0 and r_py.returncode == 0, (r_cc.stderr[-2000:], r_py.stderr[-2000:])
    return r_cc, r_py


def _edit_distance(ref, hyp):
    d = list(range(len(hyp) + 1))
    for i in range(1, len(ref) + 1):
        prev, d[0] = d[0], i
        for j in range(1, len(hyp) + 1):
            prev, d[j] = d[j], min(prev + (ref[i - 1] != hyp[j - 1]), d[j] + 1, d[j - 1] + 1)
    return d[len(hyp)]


def test_lexicon_tools_equal_each_other_and_the_api(data):
    from eesen_amd.api import Net, Ctc, Lexicon, TokenLm
    tmp, feats, lex = data["tmp"], data["feats"], data["lex"]
    out = lambda tag, what: str(tmp / f"lex_{what}_{tag}")
    rng = np.random.default_rng(31)
    refs = {key: rng.integers(1, lex.V + 1, size=int(rng.integers(1, 4))).astype(np.int32) for key, _ in feats[:4]}          # one utterance has none
    kaldi_io.write_vec_int_ark(str(tmp / "word_refs.ark"), refs.items())
    lex_args = ["--lexicon=" + data["lexicon"], "--lexicon-units=" + data["units"], "--space-unit=<SPACE>", "--word-lm=" + data["arpa"], "--lm-skip-oov=true",
                "--lm-weight=0.7", "--word-bonus=0.4", "--lm-eos=true", "--word-ref-rspecifier=ark:" + str(tmp / "word_refs.ark")]
    r_cc, r_py = _both(lambda tag: lex_args + ["--num-sequence=3", "--nbest=3", "--beam=16", "--max-classes=6", "--scores-out=" + out(tag, "scores"),
                                              "--words-wspecifier=ark:" + out(tag, "words"), "--words-table-out=" + out(tag, "table"),
                                              data["model"], "ark:" + data["ark"], "ark:" + out(tag, "hyp")])
    for what in ("hyp", "words", "scores", "table"):
        assert open(out("cc", what), "rb").read() == open(out("py", what), "rb").read(), what
    assert open(out("cc", "table")).read() == "".join(f"{n} {w}\n" for n, w in sorted(lex.ids.items(), key=lambda kv: kv[1]))
    # without --words-table-out the word LM reads the table from a temporary file of the tool's own: the same hypotheses
    _both(lambda tag: lex_args + ["--num-sequence=3", "--nbest=3", "--beam=16", "--max-classes=6", data["model"], "ark:" + data["ark"], "ark:" + out(tag, "hyp2")])
    for tag in ("cc", "py"):
        assert open(out(tag, "hyp2"), "rb").read() == open(out("cc", "hyp"), "rb").read(), tag
    got = kaldi_io.read_vec_int_table("ark:" + out("cc", "hyp"))
    words = kaldi_io.read_vec_int_table("ark:" + out("cc", "words"))
    lines = [l.split() for l in open(out("cc", "scores"))]
    assert all(len(l) == 3 for l in lines) and [l[0] for l in lines] == list(got) == list(words)
    trie = Lexicon(data["lexicon"], data["units"], K=lex.K, space=SPACE)
    lm = TokenLm(data["arpa"], out("cc", "table"), K=lex.V + 1, skip_oov=True)
    assert lm.OovDropped() == 3
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
            assert np.array_equal(got[k], np.asarray(h, np.int32)), k
            assert tuple(words[k]) == lex.segment(h) == tuple(ctc.words[0, i, :ctc.words_len[0, i]]), k
            assert np.float32(by_key[k][0]) == score[0, i] and np.float32(by_key[k][1]) == ctc.lm_score[0, i], k
        best = list(lex.segment(hyps[0][0]))
        tot_lm += float(ctc.lm_score[0, 0]); tot_words += len(best); tot_score += float(score[0, 0]); tot_frames += m.shape[0]
        if key in refs:
            err += _edit_distance(refs[key].tolist(), best); nref += refs[key].size; scored += 1
    assert list(got) == keys and scored == 4
    for r in (r_cc, r_py):
        assert f"LOG (ctc-decode:main()) {err} word errors on {nref} reference words of {scored} utterances\n" in r.stderr, r.stderr[-1500:]
        acc = re.search(r"LOG \(ctc-decode:main\(\)\) \nWORD_ACCURACY >> ([-0-9.e]+)% <<\n", r.stderr)
        assert acc and abs(float(acc.group(1)) - 100.0 * (1.0 - err / nref)) < 1e-3, r.stderr[-1500:]
        assert "3 n-grams of " in r.stderr and "were dropped" in r.stderr
        m = re.search(FINAL, r.stderr)
        assert m and m.group(1) == "5", r.stderr[-1000:]
        assert abs(float(m.group(3)) - tot_score / tot_frames) < 1e-4 * max(1.0, abs(tot_score / tot_frames))
        assert abs(float(m.group(4)) - tot_lm / max(tot_words, 1)) < 1e-4 * max(1.0, abs(tot_lm / max(tot_words, 1)))


def test_lexicon_of_decimal_ids_without_a_word_lm(data):
    """lexicon_numbers.txt and --space-unit as an id; no word LM: two columns in the scores file, no LM figure in the log."""
    tmp, lex = data["tmp"], data["lex"]
    numbers = lex.write(tmp, "lexicon_numbers")
    out = lambda tag, what: str(tmp / f"num_{what}_{tag}")
    r_cc, r_py = _both(lambda tag: ["--lexicon=" + numbers, f"--space-unit={SPACE}", "--word-bonus=-0.3", "--num-sequence=5", "--scores-out=" + out(tag, "scores"),
                                    "--words-wspecifier=ark,t:" + out(tag, "words"), data["model"], "ark:" + data["ark"], "ark,t:" + out(tag, "hyp")])
    for what in ("hyp", "words", "scores"):
        assert open(out("cc", what), "rb").read() == open(out("py", what), "rb").read(), what
    hyp = {l.split()[0]: tuple(map(int, l.split()[1:])) for l in open(out("cc", "hyp"))}
    words = {l.split()[0]: tuple(map(int, l.split()[1:])) for l in open(out("cc", "words"))}
    assert list(hyp) == list(words) == [k for k, _ in data["feats"]]
    assert all(lex.segment(hyp[k]) == words[k] for k in hyp)
    assert all(len(l.split()) == 2 for l in open(out("cc", "scores")))
    for r in (r_cc, r_py):
        assert "LM log-probability" not in r.stderr and "WORD_ACCURACY" not in r.stderr


def test_without_lexicon_nothing_changes(data):
    tmp = data["tmp"]
    out = lambda tag, what: str(tmp / f"plain_{what}_{tag}")
    r_cc, r_py = _both(lambda tag: ["--num-sequence=3", "--nbest=2", "--beam=8", "--max-classes=6", "--scores-out=" + out(tag, "scores"), data["model"],
                                    "ark:" + data["ark"], "ark:" + out(tag, "hyp")])
    assert open(out("cc", "hyp"), "rb").read() == open(out("py", "hyp"), "rb").read()
    assert open(out("cc", "scores")).read() == open(out("py", "scores")).read()
    assert all(len(l.split()) == 2 for l in open(out("cc", "scores")))
    for r in (r_cc, r_py):
        assert "LM log-probability" not in r.stderr and "WORD_ACCURACY" not in r.stderr and "lexicon" not in r.stderr and re.search(r"average log-probability per frame [-0-9.e]+\n", r.stderr)
    # the hypotheses are the api's plain call's, as before
    from eesen_amd.api import Net, Ctc
    net = Net().Read(data["model"])
    net.SetTestMode()
    ctc = Ctc()
    got = kaldi_io.read_vec_int_table("ark:" + out("cc", "hyp"))
    for key, m in data["feats"]:
        net.SetSeqLengths([m.shape[0]])
        hyps, _ = ctc.DecodeParallel([m.shape[0]], net.Propagate(m), beam=8, max_classes=6, nbest=2)
        for i, h in enumerate(hyps[0]):
            assert np.array_equal(got[f"{key}-{i + 1}"], np.asarray(h, np.int32))


def test_lexicon_errors_reach_the_command_line(data):
    o_t = str(data["tmp"] / "hyp_err.ark")
    tail = [data["model"], "ark:" + data["ark"], "ark,t:" + o_t]
    for host in ([EXE], [sys.executable, "-m", "eesen_amd.ctc_decode"]):
        run = lambda args: subprocess.run(host + args + tail, capture_output=True, text=True, cwd=ROOT, timeout=600)
        r = run(["--lexicon=" + data["lexicon"], "--lexicon-units=" + data["units"], "--lm=" + data["arpa"]])
        assert r.returncode == 255 and "--lexicon together with --lm" in r.stderr, r.stderr[-1000:]
        r = run(["--word-lm=" + data["arpa"]])
        assert r.returncode == 255 and "need --lexicon" in r.stderr, r.stderr[-1000:]
        r = run(["--lexicon=" + data["lexicon"], "--lexicon-units=" + data["units"], "--word-lm=" + data["arpa"]])          # no --lm-skip-oov
        assert r.returncode == 255 and "zebra" in r.stderr, r.stderr[-1000:]
        r = run(["--lexicon=" + data["lexicon"], "--lexicon-units=" + data["units"], "--space-unit=<SPC>"])
        assert r.returncode == 255 and "--space-unit=<SPC> is not in" in r.stderr, r.stderr[-1000:]
        r = run(["--lexicon=" + data["lexicon"]])          # symbols without their table
        assert r.returncode == 255 and "no decimal class id" in r.stderr, r.stderr[-1000:]
