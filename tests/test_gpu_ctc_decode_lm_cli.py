"""-m gpu: the ctc-decode tools with --lm (eesen_amd/bin/ctc-decode and python -m eesen_amd.ctc_decode): a token n-gram LM, ARPA text and a
units table, fused into the search.  The two tools write byte-identical tables and scores files; the lm-logprob column is
TokenLm.Score of the labels written; without --lm both write what they wrote before."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from eesen_amd import kaldi_io, nnet_io, synth
from tests import ctc_lm_restatement as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "eesen_amd", "bin", "ctc-decode")
FINAL = (r"LOG \(ctc-decode:main\(\)\) Done (\d+) utterances, (\d+) empty hypotheses; average log-probability per frame ([-0-9.e]+)"
         r"; average LM log-probability per label ([-0-9.e]+)\n")


@pytest.fixture(scope="module")
def data(gpu, tmp_path_factory):
    """2 BiLSTM layers of 32 cells, D = 8, K = 7; five utterances of 20-45 frames; an order-3 model with a units table."""
    tmp = tmp_path_factory.mktemp("ctc_decode_lm")
    cfg = dict(synth.config("tiny_bi"), H=32)
    rng = np.random.default_rng(23)
    feats = [(f"utt{i}", rng.standard_normal((int(rng.integers(20, 46)), cfg["D"])).astype(np.float32) * np.float32(3)) for i in range(5)]
    feats.sort(key=lambda kv: kv[1].shape[0])
    ark, model = str(tmp / "feats.ark"), str(tmp / "final.nnet")
    kaldi_io.write_mat_ark(ark, feats)
    nnet_io.write_nnet(model, synth.make_model(**cfg), binary=True)
    lm = L.random_model(seed=4120, K=cfg["K"], order=3, named=True)
    arpa, units = lm.write(tmp)
    return dict(tmp=tmp, cfg=cfg, feats=feats, ark=ark, model=model, arpa=arpa, units=units)


def _both(args):
    assert os.path.exists(EXE), "run python -m eesen_amd.build"
    r_cc = subprocess.run([EXE] + args("cc"), capture_output=True, text=True, timeout=600)
    r_py = subprocess.run([sys.executable, "-m", "eesen_amd.ctc_decode"] + args("py"), capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r_cc.returncode == 0 and r_py.returncode == 0, (r_cc.stderr[-2000:], r_py.stderr[-2000:])
    return r_cc, r_py


def test_lm_tools_equal_each_other_and_the_api(data):
    from eesen_amd.api import Net, Ctc, TokenLm
    tmp, feats = data["tmp"], data["feats"]
    out = lambda tag, what: str(tmp / f"lm_{what}_{tag}")
    lm_args = ["--lm=" + data["arpa"], "--lm-units=" + data["units"], "--lm-weight=0.7", "--insertion-bonus=0.4", "--lm-eos=true"]
    r_cc, r_py = _both(lambda tag: lm_args + ["--num-sequence=3", "--nbest=3", "--beam=8", "--max-classes=6", "--scores-out=" + out(tag, "scores"),
                                             data["model"], "ark:" + data["ark"], "ark:" + out(tag, "hyp")])
    assert open(out("cc", "hyp"), "rb").read() == open(out("py", "hyp"), "rb").read()
    assert open(out("cc", "scores")).read() == open(out("py", "scores")).read()
    got = kaldi_io.read_vec_int_table("ark:" + out("cc", "hyp"))
    lines = [l.split() for l in open(out("cc", "scores"))]
    assert all(len(l) == 3 for l in lines) and [l[0] for l in lines] == list(got)
    lm = TokenLm(data["arpa"], data["units"], K=data["cfg"]["K"])
    net = Net().Read(data["model"])
    net.SetTestMode()
    ctc = Ctc()
    by_key = {l[0]: (float(l[1]), float(l[2])) for l in lines}
    keys, tot_lm, tot_len, tot_score, tot_frames = [], 0.0, 0, 0.0, 0
    for key, m in feats:
        net.SetSeqLengths([m.shape[0]])
        hyps, score = ctc.DecodeParallel([m.shape[0]], net.Propagate(m), beam=8, max_classes=6, nbest=3, lm=lm, lm_weight=0.7, insertion_bonus=0.4,
                                         lm_eos=True)
        for i, h in enumerate(hyps[0]):
            k = f"{key}-{i + 1}"
            keys.append(k)
            assert np.array_equal(got[k], np.asarray(h, np.int32)), k
            assert np.float32(by_key[k][0]) == score[0, i] and np.float32(by_key[k][1]) == ctc.lm_score[0, i], k
            want, absum = lm.Score(h, eos=True, with_abs=True)
            assert abs(by_key[k][1] - want) <= (len(h) + 4) * 2.0 ** -23 * absum + 1e-9 * abs(want), k          # (9 digits in the file)
        tot_lm += float(ctc.lm_score[0, 0]); tot_len += len(hyps[0][0]); tot_score += float(score[0, 0]); tot_frames += m.shape[0]
    assert list(got) == keys
    for r in (r_cc, r_py):
        m = re.search(FINAL, r.stderr)
        assert m and m.group(1) == "5", r.stderr[-1000:]
        assert abs(float(m.group(3)) - tot_score / tot_frames) < 1e-4 * max(1.0, abs(tot_score / tot_frames))
        assert abs(float(m.group(4)) - tot_lm / max(tot_len, 1)) < 1e-4 * max(1.0, abs(tot_lm / max(tot_len, 1)))


def test_without_lm_nothing_changes(data):
    tmp = data["tmp"]
    out = lambda tag, what: str(tmp / f"plain_{what}_{tag}")
    r_cc, r_py = _both(lambda tag: ["--num-sequence=3", "--nbest=2", "--beam=8", "--max-classes=6", "--scores-out=" + out(tag, "scores"), data["model"],
                                    "ark:" + data["ark"], "ark:" + out(tag, "hyp")])
    assert open(out("cc", "hyp"), "rb").read() == open(out("py", "hyp"), "rb").read()
    assert open(out("cc", "scores")).read() == open(out("py", "scores")).read()
    assert all(len(l.split()) == 2 for l in open(out("cc", "scores")))
    for r in (r_cc, r_py):
        assert "LM log-probability" not in r.stderr and re.search(r"average log-probability per frame [-0-9.e]+\n", r.stderr)


def test_lm_errors_reach_the_command_line(data):
    o_t = str(data["tmp"] / "hyp_err.ark")
    r = subprocess.run([EXE, "--lm=" + data["arpa"], data["model"], "ark:" + data["ark"], "ark,t:" + o_t], capture_output=True, text=True, timeout=600)
    assert r.returncode == 255 and "is neither a decimal class id" in r.stderr, r.stderr[-1000:]          # the units table is missing
    r = subprocess.run([EXE, "--lm-units=" + data["units"], data["model"], "ark:" + data["ark"], "ark,t:" + o_t], capture_output=True, text=True, timeout=600)
    assert r.returncode == 255 and "--lm-units without --lm" in r.stderr
