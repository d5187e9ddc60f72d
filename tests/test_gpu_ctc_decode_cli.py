"""-m gpu: the ctc-decode tools end to end (eesen_amd/bin/ctc-decode, host C++ over the C-ABI, and its mirror python -m eesen_amd.ctc_decode):
Kaldi tables in, one int32 vector of labels per hypothesis out."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from eesen_amd import kaldi_io, nnet_io, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "eesen_amd", "bin", "ctc-decode")
FINAL = r"LOG \(ctc-decode:main\(\)\) Done (\d+) utterances, (\d+) empty hypotheses; average log-probability per frame ([-0-9.e]+)"


@pytest.fixture(scope="module")
def data(gpu, tmp_path_factory):
    """2 BiLSTM layers of 32 cells, D = 8, K = 7; six utterances of 20-45 frames, sorted by length; references of 2-6 labels."""
    tmp = tmp_path_factory.mktemp("ctc_decode")
    cfg = dict(synth.config("tiny_bi"), H=32)
    rng = np.random.default_rng(19)
    feats = [(f"spk{i % 2}_utt{i}", rng.standard_normal((int(rng.integers(20, 46)), cfg["D"])).astype(np.float32) * np.float32(3)) for i in range(6)]
    feats.sort(key=lambda kv: kv[1].shape[0])
    refs = {k: rng.integers(1, cfg["K"], size=int(rng.integers(2, 7))).astype(np.int32) for k, _ in feats}
    ark, scp, ref, model = (str(tmp / n) for n in ("feats.ark", "feats.scp", "refs.ark", "final.nnet"))
    kaldi_io.write_mat_ark(ark, feats, scp_path=scp)
    kaldi_io.write_vec_int_ark(ref, refs.items())
    nnet_io.write_nnet(model, synth.make_model(**cfg), binary=True)
    return dict(tmp=tmp, cfg=cfg, feats=feats, refs=refs, ark=ark, scp=scp, ref=ref, model=model)


def _both(args):
    assert os.path.exists(EXE), "run python -m eesen_amd.build"
    r_cc = subprocess.run([EXE] + args("cc"), capture_output=True, text=True, timeout=600)
    r_py = subprocess.run([sys.executable, "-m", "eesen_amd.ctc_decode"] + args("py"), capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r_cc.returncode == 0 and r_py.returncode == 0, (r_cc.stderr[-2000:], r_py.stderr[-2000:])
    return r_cc, r_py


def _levenshtein(ref, hyp):
    d = list(range(len(hyp) + 1))
    for i in range(1, len(ref) + 1):
        prev, d[0] = d[0], i
        for j in range(1, len(hyp) + 1):
            prev, d[j] = d[j], min(prev + (ref[i - 1] != hyp[j - 1]), d[j] + 1, d[j - 1] + 1)
    return d[len(hyp)]


def test_tools_equal_each_other_and_the_api_and_count_token_errors(data):
    from eesen_amd.api import Net, Ctc
    tmp, feats, refs = data["tmp"], data["feats"], data["refs"]
    net = Net().Read(data["model"])
    net.SetTestMode()
    ctc = Ctc()
    want, logp = {}, 0.0
    for key, m in feats:
        net.SetSeqLengths([m.shape[0]])
        hyps, score = ctc.DecodeParallel([m.shape[0]], net.Propagate(m), beam=8, max_classes=6)
        want[key] = np.asarray(hyps[0][0], np.int32)
        logp += float(score[0, 0])
    err = sum(_levenshtein(refs[k].tolist(), want[k].tolist()) for k, _ in feats)
    nref = sum(len(refs[k]) for k, _ in feats)
    out = lambda tag: str(tmp / f"hyp_{tag}.ark")
    r_cc, r_py = _both(lambda tag: ["--num-sequence=4", "--beam=8", "--max-classes=6", "--ref-rspecifier=ark:" + data["ref"], data["model"],
                                    "scp:" + data["scp"], "ark:" + out(tag)])
    assert open(out("cc"), "rb").read() == open(out("py"), "rb").read()
    got = kaldi_io.read_vec_int_table("ark:" + out("cc"))
    assert list(got) == [k for k, _ in feats]
    for key, _ in feats:
        assert np.array_equal(got[key], want[key]), key
    for r in (r_cc, r_py):
        m = re.search(FINAL, r.stderr)
        assert m and m.group(1, 2) == ("6", str(sum(len(v) == 0 for v in want.values())))
        assert abs(float(m.group(3)) - logp / sum(m_.shape[0] for _, m_ in feats)) < 1e-4
        assert f"LOG (ctc-decode:main()) {err} token errors on {nref} reference tokens of 6 utterances" in r.stderr
        acc = re.search(r"\nTOKEN_ACCURACY >> ([-0-9.e+]+)% <<", r.stderr)
        assert acc and abs(float(acc.group(1)) - 100.0 * (1.0 - err / nref)) < 1e-3


def test_nbest_keys_scores_and_prior_subtraction(data):
    from eesen_amd import _lib
    from eesen_amd.api import Net, Ctc
    tmp, feats = data["tmp"], data["feats"]
    counts = str(tmp / "label.counts")
    open(counts, "w").write("[ 1200 30 25 45.5 8 19 77 ]\n")
    prior = ["--class-frame-counts=" + counts, "--prior-scale=0.8", "--blank-scale=0.5"]
    out = lambda tag, what: str(tmp / f"nbest_{what}_{tag}")
    _both(lambda tag: prior + ["--num-sequence=3", "--nbest=3", "--beam=8", "--max-classes=6", "--scores-out=" + out(tag, "scores"), data["model"],
                               "ark:" + data["ark"], "ark:" + out(tag, "hyp")])
    assert open(out("cc", "hyp"), "rb").read() == open(out("py", "hyp"), "rb").read()
    assert open(out("cc", "scores")).read() == open(out("py", "scores")).read()
    got = kaldi_io.read_vec_int_table("ark:" + out("cc", "hyp"))
    scores = dict((l.split()[0], float(l.split()[1])) for l in open(out("cc", "scores")))
    assert list(scores) == list(got)
    from eesen_amd.net_output_extract import class_log_priors
    log_pri = class_log_priors(counts, 1e-10, 0.5)
    net = Net().Read(data["model"])
    net.SetTestMode()
    ctc = Ctc()
    keys = []
    for key, m in feats:
        net.SetSeqLengths([m.shape[0]])
        o = net.Propagate(m)
        _lib.check(_lib.load().eesen_op_log_sub_prior(0, None, C.c_void_p(o.ptr), o.rows, o.cols, o.stride, 1, log_pri.ctypes.data_as(C.c_void_p), 0.8))
        hyps, score = ctc.DecodeParallel([m.shape[0]], o, beam=8, max_classes=6, nbest=3, is_log=True)
        assert 1 <= len(hyps[0]) <= 3
        for i, h in enumerate(hyps[0]):        # utt-1, utt-2, ...: best first
            k = f"{key}-{i + 1}"
            keys.append(k)
            assert np.array_equal(got[k], np.asarray(h, np.int32)), k
            assert np.float32(scores[k]) == score[0, i], k
    assert list(got) == keys


def test_text_output_and_usage(data):
    o_t = str(data["tmp"] / "hyp_t.ark")
    r = subprocess.run([EXE, "--beam=4", "--max-classes=3", data["model"], "ark:" + data["ark"], "ark,t:" + o_t], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and re.search(FINAL, r.stderr), r.stderr[-2000:]
    got = kaldi_io.read_vec_int_table("ark,t:" + o_t)
    assert list(got) == [k for k, _ in data["feats"]]
    assert subprocess.run([EXE, data["model"]], capture_output=True).returncode == 1
    r = subprocess.run([EXE, "--beam=65", data["model"], "ark:" + data["ark"], "ark,t:" + o_t], capture_output=True, text=True, timeout=600)
    assert r.returncode == 255 and "beam outside [1, 64]" in r.stderr
