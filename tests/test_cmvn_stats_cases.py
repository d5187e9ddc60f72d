"""CPU: the CMVN statistics fixture (tests/golden/cmvn_stats.npz, what the reference's compute-cmvn-stats wrote) against the numpy
restatement of tests/cmvn_stats_cases.py; the double-matrix writer and the float-vector and token-list readers of eesen_amd/kaldi_io.py
and eesen_amd/csrc/tools/kaldi_tables.h against bytes the reference wrote or read; the option errors of the tool, which need no device."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import cmvn_stats_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    return cc.load()


def test_generator_has_not_drifted(g):
    want = json.loads(str(g["hashes"]))
    got = {n: cc.input_hash(x, w) for n, (x, w) in cc.all_inputs().items()}
    assert got == want


@pytest.mark.parametrize("tag", ["u", "w"])
def test_exact_cases_equal_the_restatement_bit_for_bit(g, tag):
    items = [(cc.name_of(T, D),) + cc.utt(T, D) for T, D in cc.SHAPES] + ([("inf7x3",) + cc.inf_utt()] if tag == "w" else [])
    for n, x, w in items:
        want = cc.restate(x, w if tag == "w" else None)
        got = g[f"shapes/{tag}/{n}"]
        assert got.dtype == np.float64 and got.shape == (2, x.shape[1] + 1)
        assert np.array_equal(got, want), n
        assert np.all(np.isfinite(got)) and got[1, -1] == 0
    # fp64 squares are NOT what the reference adds: the check would notice
    x, _ = cc.utt(3000, 40)
    sq = (x.astype(np.float64) ** 2).sum(axis=0)
    rel = np.abs(sq - g["shapes/u/u3000x40"][1, :-1]) / sq
    assert rel.max() > 1e-10


@pytest.mark.parametrize("tag", ["u", "w"])
def test_speaker_and_global_matrices_are_sums_of_the_utterances(g, tag):
    by_name = {cc.name_of(T, D): cc.utt(T, D) for T, D in cc.D40}
    st = {n: cc.restate(x, w if tag == "w" else None) for n, (x, w) in by_name.items()}
    for spk, ulist in cc.SPK2UTT[:2]:
        want = np.zeros((2, 41))
        for u in ulist:
            if u in st:
                want += st[u]
        assert np.array_equal(g[f"d40/{tag}/{spk}"], want)
    assert f"d40/{tag}/spkC" not in g.files
    assert list(g[f"d40/{tag}/spk_counts"]) == [3, 3, 0]
    warns = json.loads(str(g[f"d40/{tag}/spk_warnings"]))
    assert warns == ["Did not find features for utterance gone1", "Did not find features for utterance gone2",
                     "Did not find features for utterance gone3", "No stats accumulated for speaker spkC"]
    total = np.zeros((2, 41))
    for T, D in cc.D40:
        total += st[cc.name_of(T, D)]
    glob = g[f"d40/{tag}/global"]
    assert glob.dtype == np.float32 and np.array_equal(glob, total.astype(np.float32))
    assert list(g[f"d40/{tag}/global_counts"]) == [3, 0, 0]
    assert list(g["none/counts"]) == [0, 2, 1]


@pytest.mark.parametrize("tag", ["u", "w"])
def test_wide_case_within_the_summation_order_bound(g, tag):
    x, w = cc.wide_utt()
    w = w if tag == "w" else None
    got, exact, bound = g[f"wide/{tag}"], cc.restate(x, w), cc.order_bound(x, w)
    assert np.all(np.abs(got - exact) <= bound)
    assert np.any(got != exact)          # sums do round here: the case is not an exact one


@pytest.mark.parametrize("T,D", cc.LONG)
def test_batches_of_33_hash_to_the_restatement(g, T, D):
    items = cc.b33(T, D)
    assert len(items) == 33 and items[cc.B33_AT][0] == cc.name_of(T, D) and len({x.shape[0] for _, x, _ in items}) > 20
    for tag in ("u", "w"):
        mats = [g[f"shapes/{tag}/{n}"] if i == cc.B33_AT else cc.restate(x, w if tag == "w" else None) for i, (n, x, w) in enumerate(items)]
        assert cc.matrices_hash(mats) == str(g[f"b33_{T}x{D}/{tag}/hash"])


# ---------------------------------------------------------------------------------------------- tables
def _small(g):
    return [(cc.name_of(T, D), g[f"shapes/u/{cc.name_of(T, D)}"]) for T, D in cc.SHAPES[:2]]


def test_double_matrix_writer_reproduces_the_reference_bytes(g, tmp_path):
    from eesen_amd import kaldi_io
    for mode, text in (("bin", False), ("txt", True)):
        ref = g["bytes/dm_" + mode].tobytes()
        ark, scp = str(tmp_path / f"{mode}.ark"), str(tmp_path / f"{mode}.scp")
        kaldi_io.write_mat64_ark(ark, _small(g), text=text, scp_path=scp)
        assert open(ark, "rb").read() == ref
        back = list(kaldi_io.read_mat64_table("scp:" + scp))          # the offsets point at the objects
        assert [k for k, _ in back] == [k for k, _ in _small(g)]
        for (_, a), (_, b) in zip(back, _small(g)):
            assert np.array_equal(a, b) if not text else np.allclose(a, b, rtol=1e-6, atol=0)
    # the global matrix is a float matrix; in text mode with the reference's 7 digits
    glob = g["shapes/u/u2x3"].astype(np.float32)
    assert kaldi_io._matrix_bytes(glob, False) == g["bytes/global_bin"].tobytes()
    assert kaldi_io._matrix64_bytes(glob.astype(np.float64), True) == g["bytes/global_txt"].tobytes()


def test_float_vector_and_token_list_readers(g, tmp_path):
    from eesen_amd import kaldi_io
    wark = str(tmp_path / "w.ark")
    open(wark, "wb").write(g["bytes/weights"].tobytes())               # what the reference read when the fixture was made
    got = kaldi_io.read_vec_float_table("ark:" + wark)
    for T, D in cc.SHAPES[:2]:
        w = cc.utt(T, D)[1]
        assert got[cc.name_of(T, D)].dtype == np.float32 and np.array_equal(got[cc.name_of(T, D)], w)
    txt = str(tmp_path / "w.txt")
    open(txt, "w").write("a  [ 0.5 -1 2.25 ]\nb  [ ]\n")
    t = kaldi_io.read_vec_float_table("ark,t:" + txt)
    assert list(t["a"]) == [0.5, -1.0, 2.25] and t["b"].size == 0
    spk = str(tmp_path / "spk2utt")
    open(spk, "w").write(cc.spk2utt_text())
    assert kaldi_io.read_token_lists("ark:" + spk) == cc.SPK2UTT


def test_native_tables_and_rspecifier_forms(g, tmp_path):
    """eesen_amd/csrc/tools/kaldi_tables.h reads and writes what kaldi_io does, byte for byte, and feat_pipeline.h recognises the
    feature rspecifiers compute-cmvn-stats runs as a feeder pipeline (the tap goes on the last boundary)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "cmvn_tables")
    subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "native", "cmvn_tables.cc"), "-o", exe,
                    "-L" + os.path.join(ROOT, "eesen_amd", "lib"), "-leesen_hip", "-Wl,-rpath," + os.path.join(ROOT, "eesen_amd", "lib"),
                    "-Wl,--allow-shlib-undefined"], check=True)
    run = lambda *a: subprocess.run([exe] + list(a), capture_output=True, text=True)
    src = str(tmp_path / "ref.ark")
    open(src, "wb").write(g["bytes/dm_bin"].tobytes())
    for mode, spec in (("bin", "ark:"), ("txt", "ark,t:")):
        out = str(tmp_path / f"out_{mode}.ark")
        r = run("dm", "ark:" + src, spec + out)
        assert r.returncode == 0, r.stderr
        assert open(out, "rb").read() == g["bytes/dm_" + mode].tobytes()
    out, scp = str(tmp_path / "o.ark"), str(tmp_path / "o.scp")
    assert run("dm", "ark:" + src, f"ark,scp:{out},{scp}").returncode == 0
    assert run("dm", "scp:" + scp, "ark:" + str(tmp_path / "again.ark")).returncode == 0
    assert open(str(tmp_path / "again.ark"), "rb").read() == g["bytes/dm_bin"].tobytes()
    wark = str(tmp_path / "w.ark")
    open(wark, "wb").write(g["bytes/weights"].tobytes())
    r = run("weights", "ark:" + wark)
    lines = [l.split() for l in r.stdout.splitlines()]
    assert r.returncode == 0 and sorted(l[0] for l in lines) == ["u1x1", "u2x3"], r.stderr
    for l in lines:
        w = cc.exact_utt(l[0], *map(int, l[0][1:].split("x")))[1]
        assert int(l[1]) == len(w) and np.float32(l[2]) == w[0] and np.float32(l[3]) == w[-1]
    spk = str(tmp_path / "spk2utt")
    open(spk, "w").write(cc.spk2utt_text())
    r = run("spk2utt", "ark:" + spk)
    assert r.returncode == 0 and r.stdout == cc.spk2utt_text()
    forms = ["ark:compute-fbank-feats --num-mel-bins=40 --dither=0 scp:wav.scp ark:- |",
             "ark:compute-fbank-feats --num-mel-bins=40 scp:wav.scp ark:- | add-deltas ark:- ark:- |",
             'ark:paste-feats --length-tolerance=2 "ark:compute-fbank-feats scp:wav.scp ark:- |" '
             '"ark,s,cs:compute-kaldi-pitch-feats scp:wav.scp ark:- | process-kaldi-pitch-feats ark:- ark:- |" ark:- |',
             "ark:copy-feats scp:feats.scp ark:- | splice-feats --left-context=1 --right-context=1 ark:- ark:- |",
             "ark:some-other-tool scp:feats.scp ark:- |", "scp:feats.scp"]
    r = run("pipe", *forms)
    assert r.stdout.splitlines() == ["scp:wav.scp|1|fbank", "scp:wav.scp|2|fbank", "scp:wav.scp|1|fbank+pitch", "scp:feats.scp|1|table", "NONE", "NONE"], r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------- option errors (no device is touched)
def _tools():
    from eesen_amd import build
    build.build()
    return [[os.path.join(build.BINDIR, "compute-cmvn-stats")], [sys.executable, "-m", "eesen_amd.compute_cmvn_stats"]]


@pytest.mark.parametrize("which", [0, 1], ids=["native", "python"])
def test_option_errors(which, tmp_path):
    cmd = _tools()[which]
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda *a: subprocess.run(cmd + list(a), capture_output=True, text=True, env=env, timeout=120)
    r = run("ark:feats.ark")
    assert r.returncode == 1 and "Usage: compute-cmvn-stats  [options] feats-rspecifier (stats-wspecifier|stats-wxfilename)" in r.stderr
    r = run("a", "b", "c")
    assert r.returncode == 1 and "Usage: compute-cmvn-stats" in r.stderr
    r = run("--spk2utt=ark:spk2utt", "ark:feats.ark", str(tmp_path / "global.mat"))
    assert r.returncode == 255 and "--spk2utt option not compatible with wxfilename as output (did you forget ark:?)" in r.stderr
    assert not os.path.exists(str(tmp_path / "global.mat"))
    r = run("--weights=ark:w.ark", "ark:compute-fbank-feats --num-mel-bins=40 scp:wav.scp ark:- |", "ark:" + str(tmp_path / "o.ark"))
    assert r.returncode == 255 and "--weights is not supported with a feature pipeline" in r.stderr
