"""-m gpu: the ctc-align tools end to end (eesen_amd/bin/ctc-align, host C++ over the C-ABI, and its mirror python -m eesen_amd.ctc_align):
Kaldi tables in, one int32 vector of class ids per utterance out -- the targets table train-ce-parallel reads."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from eesen_amd import kaldi_io, nnet_io, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "eesen_amd", "bin", "ctc-align")
FINAL = r"LOG \(ctc-align:main\(\)\) Done (\d+) utterances, (\d+) without labels, (\d+) infeasible; average best-path log-score per frame ([-0-9.e]+)"


@pytest.fixture(scope="module")
def data(gpu, tmp_path_factory):
    """2 BiLSTM layers of 32 cells, D = 8, K = 7; six utterances of 20-45 frames with 2-6 labels, sorted by length."""
    tmp = tmp_path_factory.mktemp("ctc_align")
    cfg = dict(synth.config("tiny_bi"), H=32)
    rng = np.random.default_rng(9)
    feats = [(f"spk{i % 2}_utt{i}", rng.standard_normal((int(rng.integers(20, 46)), cfg["D"])).astype(np.float32)) for i in range(6)]
    feats.sort(key=lambda kv: kv[1].shape[0])
    labs = {k: rng.integers(1, cfg["K"], size=int(rng.integers(2, 7))).astype(np.int32) for k, _ in feats}
    ark, scp, lab, model = (str(tmp / n) for n in ("feats.ark", "feats.scp", "labels.ark", "final.nnet"))
    kaldi_io.write_mat_ark(ark, feats, scp_path=scp)
    kaldi_io.write_vec_int_ark(lab, labs.items())
    nnet_io.write_nnet(model, synth.make_model(**cfg), binary=True)
    return dict(tmp=tmp, cfg=cfg, feats=feats, labs=labs, ark=ark, scp=scp, lab=lab, model=model)


def _both(args):
    assert os.path.exists(EXE), "run python -m eesen_amd.build"
    r_cc = subprocess.run([EXE] + args("cc"), capture_output=True, text=True, timeout=600)
    r_py = subprocess.run([sys.executable, "-m", "eesen_amd.ctc_align"] + args("py"), capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r_cc.returncode == 0 and r_py.returncode == 0, (r_cc.stderr[-2000:], r_py.stderr[-2000:])
    return r_cc, r_py


def test_tools_equal_each_other_and_the_api(data):
    from eesen_amd.api import Net, Ctc
    tmp, feats, labs = data["tmp"], data["feats"], data["labs"]
    net = Net().Read(data["model"])
    net.SetTestMode()
    ctc = Ctc()
    want_ali, want_pos = {}, {}
    for key, m in feats:
        net.SetSeqLengths([m.shape[0]])
        ali, pos, score = ctc.AlignParallel([m.shape[0]], net.Propagate(m), [labs[key]])
        assert score[0] > -1e29
        want_ali[key], want_pos[key] = ali[:, 0].copy(), pos[:, 0].copy()
    for ns in (1, 4):
        out = lambda tag, what: str(tmp / f"{what}_{tag}_{ns}.ark")
        r_cc, r_py = _both(lambda tag: [f"--num-sequence={ns}", "--positions-wspecifier=ark:" + out(tag, "pos"), data["model"], "scp:" + data["scp"],
                                        "ark:" + data["lab"], "ark:" + out(tag, "ali")])
        for what, want in (("ali", want_ali), ("pos", want_pos)):
            assert open(out("cc", what), "rb").read() == open(out("py", what), "rb").read()
            got = kaldi_io.read_vec_int_table("ark:" + out("cc", what))
            assert list(got) == [k for k, _ in feats]
            for key, _ in feats:
                assert np.array_equal(got[key], want[key]), (ns, what, key)
        for r in (r_cc, r_py):
            m = re.search(FINAL, r.stderr)
            assert m and m.group(1, 2, 3) == ("6", "0", "0") and float(m.group(4)) < 0
    # text output parses back to the same table
    o_t = str(tmp / "ali_t.ark")
    assert subprocess.run([EXE, data["model"], "ark:" + data["ark"], "ark:" + data["lab"], "ark,t:" + o_t], capture_output=True).returncode == 0
    got = kaldi_io.read_vec_int_table("ark,t:" + o_t)
    assert all(np.array_equal(got[k], want_ali[k]) for k, _ in feats)
    assert subprocess.run([EXE, data["model"]], capture_output=True).returncode == 1


def test_prior_scaled_alignment_equals_the_api_on_net_output_extract_output(data):
    from eesen_amd.api import Ctc, CuMatrix
    tmp, feats, labs = data["tmp"], data["feats"], data["labs"]
    counts = str(tmp / "label.counts")
    open(counts, "w").write("[ 1200 30 25 45.5 8 19 77 ]\n")
    prior = ["--class-frame-counts=" + counts, "--prior-scale=0.8", "--blank-scale=0.5"]
    llk = str(tmp / "llk.ark")
    r = subprocess.run([os.path.join(ROOT, "eesen_amd", "bin", "net-output-extract")] + prior + ["--apply-log=true", data["model"], "scp:" + data["scp"], "ark:" + llk],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    llk = dict(kaldi_io.read_mat_table("ark:" + llk))
    out = lambda tag: str(tmp / f"ali_prior_{tag}.ark")
    _both(lambda tag: prior + ["--num-sequence=4", data["model"], "scp:" + data["scp"], "ark:" + data["lab"], "ark:" + out(tag)])
    assert open(out("cc"), "rb").read() == open(out("py"), "rb").read()
    got = kaldi_io.read_vec_int_table("ark:" + out("cc"))
    ctc = Ctc()
    for key, m in feats:
        ali, _, score = ctc.AlignParallel([m.shape[0]], CuMatrix.from_numpy(llk[key]), [labs[key]], is_log=True)
        assert score[0] > -1e29 and np.array_equal(got[key], ali[:, 0]), key


def test_warnings_counts_and_the_round_trip_into_train_ce_parallel(data):
    tmp, feats, labs, D, K = data["tmp"], data["feats"], data["labs"], data["cfg"]["D"], data["cfg"]["K"]
    rng = np.random.default_rng(10)
    extra = [("spk0_nolabels", rng.standard_normal((12, D)).astype(np.float32)), ("spk1_tooshort", rng.standard_normal((4, D)).astype(np.float32))]
    ark2, lab2 = str(tmp / "feats2.ark"), str(tmp / "labels2.ark")
    kaldi_io.write_mat_ark(ark2, extra + feats)
    kaldi_io.write_vec_int_ark(lab2, list(labs.items()) + [("spk1_tooshort", np.array([3, 3, 2, 5], np.int32))])     # needs 5 frames, has 4
    out = lambda tag: str(tmp / f"ali2_{tag}.ark")
    for r in _both(lambda tag: ["--num-sequence=3", data["model"], "ark:" + ark2, "ark:" + lab2, "ark:" + out(tag)]):
        assert "WARNING (ctc-align:main()) spk0_nolabels, missing labels" in r.stderr
        assert "WARNING (ctc-align:main()) spk1_tooshort, no feasible alignment of 4 labels on 4 frames" in r.stderr
        assert re.search(FINAL, r.stderr).group(1, 2, 3) == ("6", "1", "1")
    assert open(out("cc"), "rb").read() == open(out("py"), "rb").read()
    table = kaldi_io.read_vec_int_table("ark:" + out("cc"))
    assert sorted(table) == sorted(k for k, _ in feats)
    for key, m in feats:
        assert table[key].shape == (m.shape[0],) and table[key].min() >= 0 and table[key].max() < K
        col = [int(c) for i, c in enumerate(table[key]) if c != 0 and (i == 0 or table[key][i - 1] != c)]
        if not np.any(labs[key][1:] == labs[key][:-1]):
            assert col == [int(x) for x in labs[key]]
    # the written table is the targets table of the CE trainer: every utterance accepted, frame for frame
    ce = os.path.join(ROOT, "eesen_amd", "bin", "train-ce-parallel")
    r = subprocess.run([ce, "--cross-validate=true", "--num-sequence=1", "--report-step=0", "ark:" + data["ark"], "ark:" + out("cc"), data["model"]],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Done 6 files, 0 with no targets, 0 with other errors." in r.stderr, r.stderr[-2000:]
    frames = sum(int(x) for x in re.findall(r"frames_progress_=\s+(\d+)", r.stderr))
    assert frames == sum(len(v) for v in table.values()) == sum(m.shape[0] for _, m in feats)
