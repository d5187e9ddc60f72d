"""-m gpu: --mbr of the ctc-decode tools (eesen_amd/bin/ctc-decode and python -m eesen_amd.ctc_decode) on a tiny archive: the plain
search, and the unspaced K = 7 lexicon with --rescore in front.  With --mbr=true the two tools write byte-identical hypotheses, words,
word ends, scores and CTM files; the written order is Ctc.MbrNbest's, so the first entry is the one order[:, 0] names; the error
counts and the N-best oracle line equal the host routine's distances.  Without the flag -- no option, or --mbr=false -- every output
byte is the same as with the option absent, and the MBR code path is not entered: its times stay 0."""
import ctypes as C
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
TOKEN_ERRORS = r"LOG \(ctc-decode:main\(\)\) (\d+) token errors on (\d+) reference tokens of (\d+) utterances\n"
TOKEN_ORACLE = r"LOG \(ctc-decode:main\(\)\) (\d+) token errors of the N-best oracle \(the best of up to (\d+) hypotheses per utterance\)\n"
WORD_ERRORS = r"LOG \(ctc-decode:main\(\)\) (\d+) word errors on (\d+) reference words of (\d+) utterances\n"
WORD_ORACLE = r"LOG \(ctc-decode:main\(\)\) (\d+) word errors of the N-best oracle \(the best of up to (\d+) hypotheses per utterance\)\n"
MOVED = r"; (\d+) utterances whose hypothesis of least expected errors is not the most probable\n"
FILES = ("hyp", "words", "ends", "scores", "ctm")


def _run(host, args):
    r = subprocess.run(host + args, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def host_distance(a, b):
    from eesen_amd import _lib
    lib = _lib.load()
    a, b = np.ascontiguousarray(a, np.int32), np.ascontiguousarray(b, np.int32)
    err = C.c_int(-1)
    _lib.check(lib.eesen_edit_distance(a.ctypes.data_as(C.c_void_p), a.size, b.ctypes.data_as(C.c_void_p), b.size, C.byref(err)))
    return err.value


@pytest.fixture(scope="module")
def data(gpu, tmp_path_factory):
    """The model, features, lexicon and word models of tests/test_gpu_ctc_rescore_cli.py, and references made from what the plain
    search returns: an utterance's LAST entry with a label appended, so that the list's oracle is better than most of its entries."""
    from eesen_amd.api import Net, Ctc
    assert os.path.exists(EXE), "run python -m eesen_amd.build"
    tmp = tmp_path_factory.mktemp("ctc_mbr")
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
    first, _ = L.Model(m1.K, m1.order, m1.grams, word_names).write(tmp, "words_first")
    second, _ = L.Model(m2.K, m2.order, m2.grams, word_names).write(tmp, "words_second")
    net = Net().Read(model)
    net.SetTestMode()
    ctc = Ctc()
    refs = {}
    for key, m in feats[:4]:                                  # (the last utterance has no reference: it is not scored)
        net.SetSeqLengths([m.shape[0]])
        hyps, _ = ctc.DecodeParallel([m.shape[0]], net.Propagate(m), beam=4, max_classes=6, nbest=4)
        refs[key] = hyps[0][-1] + [1]
    ref_ark = str(tmp / "refs.ark")
    kaldi_io.write_vec_int_ark(ref_ark, ((k, np.asarray(v, np.int32)) for k, v in refs.items()), text=True)
    word_refs = {key: [1 + (i % lex.V), 2] for i, (key, _) in enumerate(feats[:4])}
    word_ref_ark = str(tmp / "word_refs.ark")
    kaldi_io.write_vec_int_ark(word_ref_ark, ((k, np.asarray(v, np.int32)) for k, v in word_refs.items()), text=True)
    return dict(tmp=tmp, feats=feats, ark=ark, model=model, lex=lex, lexicon=lexicon, units=units, first=first, second=second, refs=refs,
                ref_ark=ref_ark, word_refs=word_refs, word_ref_ark=word_ref_ark)


def _plain_args(data, tag, extra):
    out = lambda what: str(data["tmp"] / f"plain_{what}_{tag}")
    return extra + ["--num-sequence=2", "--nbest=4", "--beam=4", "--max-classes=6", "--scores-out=" + out("scores"), "--ctm-out=" + out("ctm"), "--ctm-conf=true",
                    "--ctm-units=" + data["units"], "--ctm-precision=3", "--ref-rspecifier=ark:" + data["ref_ark"], data["model"], "ark:" + data["ark"],
                    "ark,t:" + out("hyp")]


def _lex_args(data, tag, extra):
    out = lambda what: str(data["tmp"] / f"lex_{what}_{tag}")
    return extra + ["--word-boundary=none", "--lexicon=" + data["lexicon"], "--lexicon-units=" + data["units"], "--word-lm=" + data["first"], "--lm-weight=0.7",
                    "--word-bonus=0.4", "--lm-eos=true", "--num-sequence=3", "--nbest=3", "--beam=4", "--max-classes=6", "--scores-out=" + out("scores"),
                    "--words-wspecifier=ark,t:" + out("words"), "--word-ends-wspecifier=ark,t:" + out("ends"), "--ctm-out=" + out("ctm"), "--ctm-conf=true",
                    "--conf-scale=0.5", "--frame-shift=0.03", "--ref-rspecifier=ark:" + data["ref_ark"], "--word-ref-rspecifier=ark:" + data["word_ref_ark"],
                    data["model"], "ark:" + data["ark"], "ark,t:" + out("hyp")]


def _table(path):
    return {l.split()[0]: l.split()[1:] for l in open(path)}


def _lists(table):
    out = {}
    for k, v in table.items():
        out.setdefault(k.rsplit("-", 1)[0], []).append(v)
    return out


def _log_lines(text):
    return [l for l in text.splitlines() if l.startswith(("LOG", "WARNING")) and ("errors" in l or "ACCURACY" in l)]


def test_plain_mode_both_tools_and_the_api(data):
    from eesen_amd.api import Net, Ctc
    tmp = data["tmp"]
    f = lambda what, tag: str(tmp / f"plain_{what}_{tag}")
    on = ["--mbr=true", "--mbr-scale=0.3"]
    runs = {tag: _run(host, _plain_args(data, tag, more)) for tag, host, more in
            (("cc", NATIVE, on), ("py", PYTHON, on), ("cc_first", NATIVE, []), ("py_first", PYTHON, []), ("cc_off", NATIVE, ["--mbr=false"]),
             ("py_off", PYTHON, ["--mbr=false", "--mbr-units=false"]))}
    for what in ("hyp", "scores", "ctm"):
        assert open(f(what, "cc"), "rb").read() == open(f(what, "py"), "rb").read(), what
        assert len({open(f(what, t), "rb").read() for t in ("cc_first", "py_first", "cc_off", "py_off")}) == 1, what      # without the flag
    for t in ("cc", "py"):
        assert _log_lines(runs["cc"].stderr) == _log_lines(runs[t].stderr)
    for t in ("cc_first", "py_first", "cc_off", "py_off"):
        assert "oracle" not in runs[t].stderr and "least expected" not in runs[t].stderr
        assert _log_lines(runs[t].stderr) == _log_lines(runs["cc_first"].stderr)
    hyp, first = _lists(_table(f("hyp", "cc"))), _lists(_table(f("hyp", "cc_first")))
    # the order, the error counts and the oracle are the api's and the host routine's
    net = Net().Read(data["model"])
    net.SetTestMode()
    ctc = Ctc()
    errors = oracle = ref_tokens = moved = first_errors = 0
    for key, m in data["feats"]:
        n = m.shape[0]
        net.SetSeqLengths([n])
        hyps, _ = ctc.DecodeParallel([n], net.Propagate(m), beam=4, max_classes=6, nbest=4)
        ref = data["refs"].get(key)
        res = ctc.MbrNbest(scale=0.3, refs=[ref if ref is not None else []])
        order = [int(r) for r in res.order[0] if r < len(hyps[0])]
        assert first[key] == [[str(c) for c in h] for h in hyps[0]], key
        assert hyp[key] == [[str(c) for c in hyps[0][r]] for r in order], key
        assert hyp[key][0] == [str(c) for c in hyps[0][int(res.order[0, 0])]], key          # the written 1-best is the entry order[:, 0] names
        moved += order[0] != 0
        if ref is not None:
            d = [host_distance(ref, h) for h in hyps[0]]
            assert res.ref_dist[0, :len(d)].tolist() == d
            errors += d[order[0]]; oracle += min(d); ref_tokens += len(ref); first_errors += d[0]
    assert oracle < errors                                    # (the references were made so)
    for tag in ("cc", "py"):
        err = runs[tag].stderr
        m, o, v = re.search(TOKEN_ERRORS, err), re.search(TOKEN_ORACLE, err), re.search(MOVED, err)
        assert m and o and v, err[-1500:]
        assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (errors, ref_tokens, 4), (tag, m.groups(), errors)
        assert (int(o.group(1)), int(o.group(2))) == (oracle, 4), (tag, o.groups(), oracle)
        assert int(v.group(1)) == moved
    m = re.search(TOKEN_ERRORS, runs["cc_first"].stderr)
    assert m and int(m.group(1)) == first_errors
    # the CTM speaks of the written best
    ctm = {}
    for l in open(f("ctm", "cc")):
        ctm.setdefault(l.split()[0], []).append(l.split()[4])
    for key, rows in hyp.items():
        assert ctm.get(key, []) == ["u" + c for c in rows[0]], key


@pytest.mark.parametrize("units", [False, True])
def test_lexicon_mode_behind_the_second_pass(data, units):
    """--rescore first, its totals feed the posterior; word errors and token errors both come back with the list."""
    tmp = data["tmp"]
    tag = lambda t: f"{t}_{int(units)}"
    f = lambda what, t: str(tmp / f"lex_{what}_{tag(t)}")
    second = ["--rescore=true", "--rescore-lm=" + data["second"], "--rescore-lm-weight=1.3", "--rescore-bonus=0.1", "--rescore-lm-eos=true"]
    on = second + ["--mbr=true", "--mbr-scale=0.2"] + (["--mbr-units=true"] if units else [])
    runs = {t: _run(host, _lex_args(data, tag(t), more)) for t, host, more in
            (("cc", NATIVE, on), ("py", PYTHON, on), ("cc_second", NATIVE, second), ("py_second", PYTHON, second + ["--mbr=false"]))}
    for what in FILES:
        assert open(f(what, "cc"), "rb").read() == open(f(what, "py"), "rb").read(), what
        assert open(f(what, "cc_second"), "rb").read() == open(f(what, "py_second"), "rb").read(), what
    assert _log_lines(runs["cc"].stderr) == _log_lines(runs["py"].stderr)
    assert _log_lines(runs["cc_second"].stderr) == _log_lines(runs["py_second"].stderr) and "oracle" not in runs["cc_second"].stderr
    # the lists are the second pass's, permuted: labels, words and word ends travel together
    for what in ("hyp", "words", "ends", "scores"):
        a, b = _lists(_table(f(what, "cc"))), _lists(_table(f(what, "cc_second")))
        assert a.keys() == b.keys() and all(sorted(a[k]) == sorted(b[k]) for k in a), what
    # both kinds of errors of the written best, and both oracles, against the host routine on the written tables
    hyp, words = _lists(_table(f("hyp", "cc"))), _lists(_table(f("words", "cc")))
    for table, refs, errors_re, oracle_re in ((hyp, data["refs"], TOKEN_ERRORS, TOKEN_ORACLE), (words, data["word_refs"], WORD_ERRORS, WORD_ORACLE)):
        errors = oracle = 0
        for key, ref in refs.items():
            d = [host_distance(ref, [int(c) for c in row]) for row in table[key]]
            errors += d[0]; oracle += min(d)
        err = runs["cc"].stderr
        m, o = re.search(errors_re, err), re.search(oracle_re, err)
        assert m and o, err[-1500:]
        assert int(m.group(1)) == errors and int(o.group(1)) == oracle and int(o.group(2)) == 3, (m.groups(), errors, o.groups(), oracle)
    # the CTM speaks of the written best
    ctm = {}
    for l in open(f("ctm", "cc")):
        ctm.setdefault(l.split()[0], []).append(l.split()[4])
    by_id = {w: n for n, w in data["lex"].ids.items()}
    for utt, rows in words.items():
        assert ctm.get(utt, []) == [by_id[int(w)] for w in rows[0]], utt


def test_without_the_flag_the_code_path_is_not_entered(data, monkeypatch):
    """The Python tool in this process, with its Ctc recorded: no MBR call leaves the three times at 0; --mbr=true does not."""
    from eesen_amd import api, ctc_decode
    made = []

    class Recorded(api.Ctc):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(api, "Ctc", Recorded)
    assert ctc_decode.main(_plain_args(data, "in_off", [])) == 0
    assert ctc_decode.main(_plain_args(data, "in_false", ["--mbr=false"])) == 0
    assert ctc_decode.main(_plain_args(data, "in_on", ["--mbr=true"])) == 0
    assert len(made) == 3
    assert made[0].MbrTimes() == made[1].MbrTimes() == {"build": 0.0, "kernel": 0.0, "host": 0.0}
    assert made[2].MbrTimes()["kernel"] > 0
    f = lambda what, tag: open(str(data["tmp"] / f"plain_{what}_{tag}"), "rb").read()
    for what in ("hyp", "scores", "ctm"):
        assert f(what, "in_off") == f(what, "in_false")
