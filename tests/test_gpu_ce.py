"""-m gpu: frame-level cross-entropy (include/eesen_hip.h `eesen_ce_*`, eesen_amd/csrc/ce.hip) against tests/ce_restatement.py
(the numpy transcription of the reference's ce-loss.cc, pinned to it on the CPU by tests/test_ce_restatement_vs_reference.py):
the fused kernel, the refusal of bad targets, one training step against the oracle Net at senone-sized output layers, the
timed-out-forward guard, and the train-ce-parallel tools end to end."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from eesen_amd import kaldi_io, nnet_io, synth
from tests.ce_restatement import CERestatement, ce_call
from tests.util import rel_err, valid_mask

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _softmax_rows(rng, rows, K):
    x = rng.standard_normal((rows, K)) * 4.0
    e = np.exp(x - x.max(axis=1, keepdims=True))
    y = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    if K > 1:   # no argmax ties: make every row's maximum unique
        top = np.argmax(y, axis=1)
        assert np.all(np.sum(y == y[np.arange(rows), top][:, None], axis=1) == 1)
    return y


def _upload(y, extra_cols=0, misalign=False):
    """y [rows x K] on the device with a row stride beyond pad4(K) (extra_cols), or with an odd stride at a 4-byte offset (misalign:
    the kernel's scalar path); returns (view, keepalive)."""
    from eesen_amd.api import CuMatrix
    rows, K = y.shape
    if misalign:
        ld = K + 1 if (K + 1) % 4 else K + 2
        buf = np.zeros(rows * ld + 1, np.float32)
        buf[1:].reshape(rows, ld)[:, :K] = y
        own = CuMatrix.from_numpy(buf[None, :])
        return CuMatrix.view(own.ptr + 4, rows, K, ld, keepalive=own), own
    own = CuMatrix(rows, K + extra_cols, zero=False)
    buf = np.zeros((rows, own.stride), np.float32)
    buf[:, :K] = y
    from eesen_amd import _lib
    from eesen_amd.api import _np_ptr
    _lib.check(_lib.load().eesen_dev_copy(0, C.c_void_p(own.ptr), _np_ptr(buf), buf.nbytes, 1))
    return CuMatrix.view(own.ptr, rows, K, own.stride, keepalive=own), own


def _diff_matrix(rows, K, like):
    """An output matrix with the same layout as `like` (stride, alignment), pre-filled with NaN so that nothing unwritten passes."""
    from eesen_amd.api import CuMatrix
    from eesen_amd import _lib
    from eesen_amd.api import _np_ptr
    n = rows * like.stride + 1
    own = CuMatrix(1, n, zero=False)
    nan = np.full(own.stride, np.nan, np.float32)
    _lib.check(_lib.load().eesen_dev_copy(0, C.c_void_p(own.ptr), _np_ptr(nan), nan.nbytes, 1))
    off = like.ptr % 16
    return CuMatrix.view(own.ptr + off, rows, K, like.stride, keepalive=own)


def _read(m):
    from eesen_amd import _lib
    from eesen_amd.api import _np_ptr
    buf = np.empty(m.rows * m.stride, np.float32)
    _lib.check(_lib.load().eesen_dev_copy(0, _np_ptr(buf), C.c_void_p(m.ptr), buf.nbytes, 2))
    return buf.reshape(m.rows, m.stride)[:, : m.cols]


def _batch(rng, S, T, K):
    lens = rng.integers(1, T + 1, size=S).astype(np.int32)
    lens[0] = T
    lens[1] = 1
    rows = T * S
    y = _softmax_rows(rng, rows, K)
    mask = valid_mask(lens, T, S).astype(np.float32)
    tg = rng.integers(0, K, size=rows).astype(np.int32)
    right = (mask == 1) & (rng.random(rows) < 0.3)
    tg[right] = np.argmax(y[right], axis=1)
    tg[mask == 0] = 0
    return y, tg, lens, mask


# (S, T) = (7, 23): 161 rows, 41 workgroup partials.  (7, 150): 1050 rows, 263 partials -- ce_reduce_kernel folds 256 at a time, so its
# loop iterates twice.  (5, 1700): 8500 rows, more than the 2048 x 4 wavefronts of ce_eval_kernel's grid: the row stride's second pass.
@pytest.mark.parametrize("K,layout,S,T", [pytest.param(K, lay, 7, 23, id=f"{K}-{lay}") for K in (1, 51, 4000, 9001) for lay in ("pad4", "wide")] +
                         [pytest.param(K, "misaligned", 7, 23, id=f"{K}-misaligned") for K in (1, 51)] +     # misaligned: the scalar path, at the small class counts
                         [pytest.param(5, lay, 7, 150, id=f"7x150-5-{lay}") for lay in ("pad4", "misaligned")] +
                         [pytest.param(6, lay, 5, 1700, id=f"5x1700-6-{lay}") for lay in ("pad4", "wide")])
def test_kernel_equals_restatement(gpu, K, layout, S, T):
    from eesen_amd.api import CE
    rng = np.random.default_rng(K)
    y, tg, lens, mask = _batch(rng, S, T, K)
    assert (S, T) == (7, 23) or (mask[256 * 4 if T == 150 else 8192:] == 1).sum() >= 3               # valid rows in the second pass too
    want_diff, want_obj, want_correct = ce_call(y, tg, mask)
    ref64 = -float(np.sum(np.log(y[np.arange(len(tg)), tg].astype(np.float64)) * mask))
    stats = []
    for _ in range(2):
        ce = CE()
        net_out, keep = _upload(y, extra_cols=8 if layout == "wide" else 0, misalign=layout == "misaligned")
        diff = _diff_matrix(len(tg), K, net_out)
        ce.EvalParallel(net_out, tg, diff, lens)
        got = _read(diff)
        assert np.array_equal(got.view(np.uint32), want_diff.view(np.uint32)), np.nanmax(np.abs(got - want_diff))
        assert np.all(got[mask == 0].view(np.uint32) == 0)            # padded rows: exactly +0
        st = ce.stats()
        assert abs(ce.obj - ref64) <= 1e-6 * abs(ref64) and abs(st["obj"] - want_obj) <= 1e-6 * abs(want_obj)
        assert st["correct"] == want_correct and st["frames"] == T * S and st["sequences"] == S
        stats.append((np.float64(st["obj"]).tobytes(), st["correct"]))
    assert stats[0] == stats[1]                                       # fixed-order reduction: the same bits on every run


@pytest.mark.parametrize("layout", ["pad4", "misaligned"])
def test_correct_follows_the_first_maximum_on_ties(gpu, layout):
    """K = 130, two equal maxima per row: classes 3 and 67 (one lane's stride on the scalar path) and classes 5 and 70 (different lanes
    on either path).  FindRowMaxId takes the FIRST: a target on the first maximum counts as correct, one on the second does not."""
    from eesen_amd.api import CE
    rng = np.random.default_rng(130)
    S, T, K = 2, 4, 130
    lens = np.array([T, T], np.int32)
    mask = np.ones(S * T, np.float32)
    y = rng.uniform(1e-4, 2e-3, (S * T, K)).astype(np.float32)
    first = np.array([3, 3, 3, 3, 5, 5, 5, 5]); second = np.array([67, 67, 67, 67, 70, 70, 70, 70])
    y[np.arange(8), first] = y[np.arange(8), second] = np.float32(0.4)
    for tg, want in ((first, 8), (second, 0)):
        tg = tg.astype(np.int32)
        want_diff, want_obj, want_correct = ce_call(y, tg, mask)
        assert want_correct == want
        ce = CE()
        net_out, keep = _upload(y, misalign=layout == "misaligned")
        diff = _diff_matrix(len(tg), K, net_out)
        ce.EvalParallel(net_out, tg, diff, lens)
        assert np.array_equal(_read(diff).view(np.uint32), want_diff.view(np.uint32))
        assert ce.stats()["correct"] == want


def test_bad_targets_refused_on_valid_rows_only(gpu):
    from eesen_amd.api import CE, EesenError
    rng = np.random.default_rng(3)
    S, T, K = 7, 9, 51
    y, tg, lens, mask = _batch(rng, S, T, K)
    net_out, keep = _upload(y)
    valid, padded = int(np.flatnonzero(mask == 1)[3]), int(np.flatnonzero(mask == 0)[0])
    for bad in (K, K + 100, -1):
        t2 = tg.copy(); t2[valid] = bad
        ce = CE()
        with pytest.raises(EesenError) as e:
            ce.EvalParallel(net_out, t2, None, lens)
        assert e.value.code == -1
        assert f"Class id out of network output dimension. Net outputs: {K}, class ID : {bad}" in str(e.value)
        assert ce.stats()["sequences"] == 0
        t3 = tg.copy(); t3[padded] = bad                              # ignored: the row is padding
        ce.EvalParallel(net_out, t3, None, lens)
        assert ce.stats()["sequences"] == S


STEP_CFGS = {
    "small_bi": synth.config("small_bi"),
    "proj": dict(kind="BiLstmParallel", layers=3, H=64, D=40, K=46, S=8, T=60, proj=32),
    "bi2_k4000": dict(kind="BiLstmParallel", layers=2, H=64, D=40, K=4000, S=8, T=40),
    "bi2_k9001": dict(kind="BiLstmParallel", layers=2, H=64, D=40, K=9001, S=8, T=40),
}


@pytest.mark.parametrize("name", list(STEP_CFGS))
def test_training_step_against_oracle_net(gpu, name):
    """HIP: Propagate -> CE -> Backpropagate + update; oracle: propagate -> restated CE -> backpropagate (the reference's Net in
    numpy, oracle/net.py).  The <Softmax> backward is the identity, so the CE diff is the whole top gradient."""
    from eesen_amd.api import Net, CE
    from oracle import net as onet
    cfg = STEP_CFGS[name]
    layers = synth.make_model(**cfg)
    batch = synth.make_batch(**cfg)
    S, T, K = cfg["S"], cfg["T"], cfg["K"]
    rng = np.random.default_rng(9)
    mask = valid_mask(batch.lens, T, S).astype(np.float32)
    tg = np.where(mask == 1, rng.integers(0, K, size=T * S), 0).astype(np.int32)
    net = Net.from_layers(layers)
    net.SetTrainOptions(0.5, 0.9)
    ce = CE()
    net.SetSeqLengths(batch.lens)
    out = net.Propagate(batch.feats)
    diff = ce.EvalParallel(out, tg, None, batch.lens)
    net.BackpropagateNoUpdate(diff)
    grads = net.GetGrads()
    net.Update()
    ora = onet.OracleNet(layers, "f32")
    ora.set_train_options(0.5, 0.9)
    ora.set_seq_lengths(batch.lens)
    o_out = ora.propagate(batch.feats)
    o_diff, o_obj, o_correct = ce_call(o_out, tg, mask)
    ora.backpropagate(o_diff)
    assert rel_err(diff.numpy(), o_diff) < 1e-4
    assert abs(ce.obj - o_obj) <= 1e-4 * abs(o_obj)
    assert rel_err(grads, ora.fresh_grads_flat()) < 1e-4
    assert rel_err(net.GetParams(), ora.get_params()) < 1e-4


def test_guard_drops_a_minibatch_from_a_timed_out_forward_pass(gpu):
    from eesen_amd.api import Net, CE
    cfg = synth.config("small_bi")
    layers = synth.make_model(**cfg)
    batch = synth.make_batch(**cfg)
    S, T, K = cfg["S"], cfg["T"], cfg["K"]
    mask = valid_mask(batch.lens, T, S).astype(np.float32)
    tg = np.where(mask == 1, np.arange(T * S) % K, 0).astype(np.int32)
    net = Net.from_layers(layers)
    net.SetTrainOptions(0.0, 0.0)
    ce = CE(); ce.SetGuard(net)

    def step():
        net.SetSeqLengths(batch.lens)
        out = net.Propagate(batch.feats)
        ce.EvalParallel(out, tg, None, batch.lens, want_obj=False)

    step()
    one = ce.stats()
    net._raise_error_word(2)      # what the forward milestone waiter stores when it gives up (lstm_persistent.hip)
    step()
    net.Synchronize()
    assert ce.Dropped() == 1
    assert ce.stats() == one      # the dropped minibatch is in no total
    step()
    two = ce.stats()
    assert ce.Dropped() == 1 and two["sequences"] == 2 * S and two["frames"] == 2 * T * S


# ------------------------------------------------------------------------------------------------------------------ the tools
def _dataset(tmp_path, K, D, n=14, seed=5):
    rng = np.random.default_rng(seed)
    feats = [(f"spk{i % 3}_utt{i:02d}", rng.standard_normal((int(rng.integers(8, 30)), D)).astype(np.float32)) for i in range(n)]
    feats.sort(key=lambda kv: kv[1].shape[0])
    tgts = {k: rng.integers(0, K, size=m.shape[0]).astype(np.int32) for k, m in feats}
    ark, scp, lab = str(tmp_path / "feats.ark"), str(tmp_path / "feats.scp"), str(tmp_path / "ali.ark")
    kaldi_io.write_mat_ark(ark, feats, scp_path=scp)
    kaldi_io.write_vec_int_ark(lab, tgts.items())
    return feats, tgts, ark, scp, lab


def _py(args):
    return subprocess.run([sys.executable, "-m", "eesen_amd.train_ce_parallel"] + args, capture_output=True, text=True, cwd=ROOT, timeout=600)


def _native(args):
    exe = os.path.join(ROOT, "eesen_amd", "bin", "train-ce-parallel")
    assert os.path.exists(exe), "run python -m eesen_amd.build"
    return subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)


def _replay(layers, feats, tgts, num_sequence, frame_limit, D, lr, mom, report_step, train=True):
    """The oracle Net and the restated CE driven through the reference trainer's grouping (train-ce-parallel.cc:114-166)."""
    from oracle import net as onet
    from eesen_amd.train_ce_parallel import ce_groups, interleave_targets, Counts
    ora = onet.OracleNet(layers, "f32"); ora.set_train_options(lr, mom)
    res, lines = CERestatement(report_step), []
    for g in ce_groups(iter(feats), tgts, num_sequence, frame_limit, D, Counts()):
        tg, lens, T = interleave_targets(g)
        S = len(g)
        x = np.zeros((T, S, D), np.float32)
        for s, (_, m, _) in enumerate(g):
            x[: m.shape[0], s] = m
        ora.set_seq_lengths(lens)
        out = ora.propagate(x.reshape(T * S, D))
        diff, line = res.eval_parallel(out, tg, valid_mask(lens, T, S).astype(np.float32), S)
        if line:
            lines.append(line)
        if train:
            ora.backpropagate(diff)
    return ora, res, lines


def _nums(line):
    return [float(x) for x in re.findall(r"[-+]?\d+\.?\d*(?:e[-+]?\d+)?", line)]


def test_train_ce_parallel_tools(gpu, tmp_path):
    cfg = synth.config("tiny_bi")
    K, D = 40, cfg["D"]
    cfg.update(K=K)
    layers = synth.make_model(max_grad=50.0, **cfg)
    feats, tgts, ark, scp, lab = _dataset(tmp_path, K, D)
    m_in = str(tmp_path / "nnet.init")
    nnet_io.write_nnet(m_in, layers, binary=True)
    opts = ["--learn-rate=0.01", "--momentum=0.9", "--num-sequence=4", "--frame-limit=90", "--report-step=4"]
    ora, res, lines = _replay(layers, feats, tgts, 4, 90, D, 0.01, 0.9, 4)
    assert lines
    for fspec, lspec in (("scp:" + scp, "ark:" + lab), (f"ark:cat {ark} |", f"ark:cat {lab} |")):
        o_py, o_cc = str(tmp_path / "py.nnet"), str(tmp_path / "cc.nnet")
        r1, r2 = _py(opts + [fspec, lspec, m_in, o_py]), _native(opts + [fspec, lspec, m_in, o_cc])
        assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr[-2000:], r2.stderr[-2000:])
        assert open(o_py, "rb").read() == open(o_cc, "rb").read()
        assert rel_err(nnet_io.flatten_params(nnet_io.read_nnet(o_cc)), ora.get_params()) < 1e-4
        for r in (r1, r2):
            assert "TRAINING STARTED" in r.stderr and "Done 14 files, 0 with no targets, 0 with other errors. [TRAINING" in r.stderr
            acc = float(re.search(r"FRAME_ACCURACY >> ([-0-9.e]+)% <<", r.stderr).group(1))
            assert abs(acc - 100.0 * res.correct / res.frames) < 1e-3
            got = re.findall(r"(After \d+ sequences .*)$", r.stderr, flags=re.M)
            assert len(got) == len(lines)
            for a, b in zip(got, lines):
                assert re.sub(r"[-+]?\d+\.?\d*(?:e[-+]?\d+)?", "#", a) == re.sub(r"[-+]?\d+\.?\d*(?:e[-+]?\d+)?", "#", b), (a, b)
                assert np.allclose(_nums(a), _nums(b), rtol=1e-4, atol=0), (a, b)
        assert re.findall(r"(After \d+ sequences .*)$", r1.stderr, flags=re.M) == re.findall(r"(After \d+ sequences .*)$", r2.stderr, flags=re.M)

    # an utterance without targets, one whose targets are one frame short
    bad = dict(tgts)
    keys = [k for k, _ in feats]
    del bad[keys[2]]
    bad[keys[5]] = bad[keys[5]][:-1]
    lab2 = str(tmp_path / "ali2.ark"); kaldi_io.write_vec_int_ark(lab2, bad.items())
    o_cc = str(tmp_path / "cc2.nnet")
    for r in (_native(opts + ["scp:" + scp, "ark:" + lab2, m_in, o_cc]), _py(opts + ["scp:" + scp, "ark:" + lab2, m_in, o_cc])):
        assert r.returncode == 0, r.stderr[-2000:]
        assert "Done 12 files, 1 with no targets, 1 with other errors." in r.stderr
        assert f"{keys[2]}, missing targets" in r.stderr and f"{keys[5]}, length mismatch" in r.stderr

    # cross-validation: three positional arguments, no backward pass, no model written, the parameters of the model read unchanged
    before, files = open(o_cc, "rb").read(), sorted(os.listdir(tmp_path))
    cv = ["--cross-validate=true", "--num-sequence=4", "--frame-limit=90", "scp:" + scp, "ark:" + lab, o_cc]
    _, res_cv, _ = _replay(nnet_io.read_nnet(o_cc), feats, tgts, 4, 90, D, 0.0, 0.0, 100, train=False)
    for r in (_native(cv), _py(cv)):
        assert r.returncode == 0 and "CROSS-VALIDATION STARTED" in r.stderr, r.stderr[-2000:]
        acc = float(re.search(r"FRAME_ACCURACY >> ([-0-9.e]+)% <<", r.stderr).group(1))
        assert abs(acc - 100.0 * res_cv.correct / res_cv.frames) < 1e-3
    assert open(o_cc, "rb").read() == before and sorted(os.listdir(tmp_path)) == files
    # usage -> 1 (train-ce-parallel.cc:64-67)
    assert _native(["scp:" + scp]).returncode == 1 and _py(["scp:" + scp]).returncode == 1
