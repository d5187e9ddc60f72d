"""GPU: the tool compute-cmvn-stats, native (bin/compute-cmvn-stats -> eesen_amd/bin/compute-cmvn-stats) and the Python mirror
(python -m eesen_amd.compute_cmvn_stats), in its three modes against tests/golden/cmvn_stats.npz (what the reference's tool wrote for
the same tables); and from a wav.scp, where the features never leave the device, against the same tool on the archive
bin/compute-fbank-feats wrote."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cmvn_stats_cases as cc
from tests import fbank_cases as fc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PATH="/usr/bin:/bin", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))   # no featbin tool on PATH
LOG = "Done accumulating CMVN stats for {} utterances; {} had errors."


def _tool(kind, name="compute-cmvn-stats"):
    if kind == "native":
        return [os.path.join(ROOT, "bin", name)]
    return [sys.executable, "-m", "eesen_amd." + name.replace("-", "_")]


def _run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300, env=ENV)


def _warnings(stderr):
    return [l.split(") ", 1)[1].strip() for l in stderr.splitlines() if l.startswith("WARNING")]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """The d40 table of the fixture (three utterances of 40 columns) as a binary archive, its weights and the spk2utt file."""
    from eesen_amd import kaldi_io
    d = tmp_path_factory.mktemp("cmvn_cli")
    items = [(cc.name_of(T, D),) + cc.utt(T, D) for T, D in cc.D40]
    kaldi_io.write_mat_ark(str(d / "feats.ark"), [(n, x) for n, x, _ in items], scp_path=str(d / "feats.scp"))
    with open(d / "w.ark", "wb") as f:
        for n, _, w in items:
            f.write(cc.fv_entry(n, w))
    open(d / "none.ark", "wb").close()
    open(d / "spk2utt", "w").write(cc.spk2utt_text())
    return d


@pytest.mark.parametrize("kind", ["native", "python"])
@pytest.mark.parametrize("tag", ["u", "w"])
def test_three_modes_against_the_reference(gpu, table, tmp_path, kind, tag):
    import json
    from eesen_amd import kaldi_io
    g = cc.load()
    wflag = [f"--weights=ark:{table}/w.ark"] if tag == "w" else []
    # per utterance (read through the script file), written as ark,scp
    r = _run(_tool(kind) + wflag + [f"scp:{table}/feats.scp", f"ark,scp:{tmp_path}/utt.ark,{tmp_path}/utt.scp"])
    assert r.returncode == 0 and LOG.format(3, 0) in r.stderr, r.stderr[-2000:]
    got = list(kaldi_io.read_mat64_table(f"scp:{tmp_path}/utt.scp"))
    assert [k for k, _ in got] == [cc.name_of(T, D) for T, D in cc.D40]
    for k, m in got:      # (u33x40 is the one utterance of spkB that exists: its matrix is that speaker's)
        assert _same(m, g[f"shapes/{tag}/{k}"] if k != "u33x40" else g[f"d40/{tag}/spkB"]), k
    # per speaker
    r = _run(_tool(kind) + wflag + [f"--spk2utt=ark:{table}/spk2utt", f"ark:{table}/feats.ark", f"ark:{tmp_path}/spk.ark"])
    done, err, status = g[f"d40/{tag}/spk_counts"]
    assert r.returncode == status and LOG.format(done, err) in r.stderr, r.stderr[-2000:]
    assert _warnings(r.stderr) == json.loads(str(g[f"d40/{tag}/spk_warnings"]))
    got = list(kaldi_io.read_mat64_table(f"ark:{tmp_path}/spk.ark"))
    assert [k for k, _ in got] == ["spkA", "spkB"]
    for k, m in got:
        assert _same(m, g[f"d40/{tag}/{k}"]), k
    # global: a float matrix, binary and text
    r = _run(_tool(kind) + wflag + [f"ark:{table}/feats.ark", f"{tmp_path}/global.mat"])
    done, err, status = g[f"d40/{tag}/global_counts"]
    assert r.returncode == status and LOG.format(done, err) in r.stderr and "Wrote global CMVN stats to" in r.stderr, r.stderr[-2000:]
    raw = open(tmp_path / "global.mat", "rb").read()
    assert raw[:5] == b"\x00BFM " and _same(kaldi_io.read_mat_file(f"{tmp_path}/global.mat"), g[f"d40/{tag}/global"])
    r = _run(_tool(kind) + wflag + ["--binary=false", f"ark:{table}/feats.ark", f"{tmp_path}/global.txt"])
    assert r.returncode == 0
    txt = kaldi_io.read_mat_file(f"{tmp_path}/global.txt")
    assert open(tmp_path / "global.txt", "rb").read().startswith(b" [\n  ") and np.allclose(txt, g[f"d40/{tag}/global"], rtol=1e-6, atol=0)


@pytest.mark.parametrize("kind", ["native", "python"])
def test_weights_missing_or_of_wrong_length(gpu, table, tmp_path, kind):
    g = cc.load()
    r = _run(_tool(kind) + [f"--weights=ark:{table}/none.ark", f"ark:{table}/feats.ark", f"ark:{tmp_path}/none.ark"])
    assert list(g["none/counts"]) == [0, 2, 1]          # the reference on its own two-utterance table: nothing done, exit status 1
    assert r.returncode == 1 and LOG.format(0, 3) in r.stderr, r.stderr[-2000:]
    assert _warnings(r.stderr) == [f"No weights available for utterance {cc.name_of(T, D)}" for T, D in cc.D40]
    assert os.path.getsize(tmp_path / "none.ark") == 0
    with open(tmp_path / "short.ark", "wb") as f:
        for i, (T, D) in enumerate(cc.D40):
            w = cc.utt(T, D)[1]
            f.write(cc.fv_entry(cc.name_of(T, D), w[:-1] if i == 1 else w))
    r = _run(_tool(kind) + [f"--weights=ark:{tmp_path}/short.ark", f"ark:{table}/feats.ark", f"ark:{tmp_path}/short_out.ark"])
    assert r.returncode == 0 and LOG.format(2, 1) in r.stderr, r.stderr[-2000:]
    assert _warnings(r.stderr) == ["Weights for utterance u3000x40 have wrong dimension 2999 vs. 3000"]
    from eesen_amd import kaldi_io
    got = dict(kaldi_io.read_mat64_table(f"ark:{tmp_path}/short_out.ark"))
    assert sorted(got) == ["u257x40", "u33x40"] and _same(got["u257x40"], g["shapes/w/u257x40"])


def test_from_audio_equals_the_archive_path_and_feeds_net_output_extract(gpu, tmp_path):
    """Six waveforms of two speakers (at most 0.4 s, dither 0): compute-cmvn-stats handed `compute-fbank-feats ... scp:wav.scp ark:- |`
    -- run by nobody: PATH holds no featbin tool -- writes byte for byte what it writes for the archive bin/compute-fbank-feats wrote;
    net-output-extract then runs from the same wav.scp with the resulting cmvn.scp."""
    from eesen_amd import kaldi_io, nnet_io, synth
    rng = np.random.default_rng(11)
    sf = 16000
    lens = [6400, 3200, 4801, 5000, 2000, 6000]
    with open(tmp_path / "wav.scp", "w") as scp, open(tmp_path / "utt2spk", "w") as u2s:
        for i, n in enumerate(lens):
            w = fc.tone(n, sf, 180.0 + 70 * i, 3000.0) + fc.noise(rng, n, 200.0)
            fc.write_wav(str(tmp_path / f"w{i}.wav"), np.clip(np.round(w), -32768, 32767).astype(np.int16), sf)
            scp.write(f"utt{i} {tmp_path}/w{i}.wav\n")
            u2s.write(f"utt{i} spk{i % 2}\n")
    open(tmp_path / "spk2utt", "w").write("spk0 utt0 utt2 utt4\nspk1 utt1 utt3 utt5\n")
    flags = "--num-mel-bins=40 --dither=0"
    r = _run(_tool("native", "compute-fbank-feats") + flags.split() + [f"scp:{tmp_path}/wav.scp", f"ark:{tmp_path}/fbank.ark"])
    assert r.returncode == 0, r.stderr[-2000:]
    pipe = f"ark:compute-fbank-feats {flags} scp:{tmp_path}/wav.scp ark:- |"
    outs = {}
    for kind in ("native", "python"):
        for src, spec in (("pipe", pipe), ("ark", f"ark:{tmp_path}/fbank.ark")):
            d = tmp_path / f"{kind}_{src}"
            d.mkdir()
            r = _run(_tool(kind) + [f"--spk2utt=ark:{tmp_path}/spk2utt", spec, f"ark,scp:{d}/cmvn.ark,{d}/cmvn.scp"])
            assert r.returncode == 0 and LOG.format(6, 0) in r.stderr, r.stderr[-2000:]
            outs[(kind, src)] = open(d / "cmvn.ark", "rb").read()
    assert len(outs[("native", "pipe")]) == 2 * (len("spk0 ") + 15 + 2 * 41 * 8)
    assert outs[("native", "pipe")] == outs[("native", "ark")] == outs[("python", "pipe")] == outs[("python", "ark")]
    # the statistics are those of the features: counts are the frame counts
    feats = dict(kaldi_io.read_mat_table(f"ark:{tmp_path}/fbank.ark"))
    st = dict(kaldi_io.read_mat64_table(f"scp:{tmp_path}/native_pipe/cmvn.scp"))
    assert st["spk0"][0, 40] == sum(feats[f"utt{i}"].shape[0] for i in (0, 2, 4))
    want = sum(cc.restate(np.asarray(feats[f"utt{i}"], np.float32)) for i in (1, 3, 5))
    assert np.all(np.abs(st["spk1"] - want) <= 1e-12 * np.abs(want))
    K = 7
    cfg = synth.config("tiny_bi")
    cfg.update(D=40, K=K)
    net = str(tmp_path / "net.nnet")
    nnet_io.write_nnet(net, synth.make_model(**cfg), binary=True)
    spec = (f"ark:compute-fbank-feats {flags} scp:{tmp_path}/wav.scp ark:- | apply-cmvn --norm-vars=true --utt2spk=ark:{tmp_path}/utt2spk "
            f"scp:{tmp_path}/native_pipe/cmvn.scp ark:- ark:- |")
    r = _run(_tool("native", "net-output-extract") + [net, spec, f"ark:{tmp_path}/post.ark"])
    assert r.returncode == 0, r.stderr[-2000:]
    post = dict(kaldi_io.read_mat_table(f"ark:{tmp_path}/post.ark"))
    assert sorted(post) == [f"utt{i}" for i in range(6)] and all(post[f"utt{i}"].shape == (feats[f"utt{i}"].shape[0], K) for i in range(6))
    assert all(np.all(np.isfinite(m)) for m in post.values())
