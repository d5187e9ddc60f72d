"""CPU: the host side of the filterbank + pitch pipeline against tests/golden/paste.npz (tests/paste_cases.py).

* the fixture's own conditions: it is the case list's, every case keeps an utterance, tol0 / s33_8k / snip_mixed drop one;
* eesen_feat_paste_frames and frontend.paste_frames, fed by eesen_fbank_shape and eesen_pitch_shape (host only), give the reference's
  kept / dropped decision and row count on every utterance of every case, and FeaturePipeline.out_frames / out_dim / cmvn_dim follow;
* the parser: the recipe's own command line in both wav.scp spellings, with and without trailing stages, --config files, every listed
  refusal, and every rspecifier tests/test_frontend.py accepts unchanged; the native parser (csrc/tools/feat_pipeline.h) agrees on all
  of it, options included;
* paste-feats on its host path (native and Python), on tables written from the fixture: bit-equal output, the reference's warnings,
  counts and exit status; a missing key; the rxfilename form.
"""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from eesen_amd import frontend as fe
from tests import paste_cases as pc
from tests import test_frontend as tf

GOLD = pc.load_golden()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_is_the_case_list_and_meets_its_conditions():
    assert list(GOLD) == pc.CASE_NAMES
    for c in pc.CASES:
        g = GOLD[c["name"]]
        assert g["fbank"] == c["fbank"] and g["pitch"] == c["pitch"] and g["tolerance"] == c["tolerance"]
        assert len(g["waves"]) == len(c["waves"]) and all(np.array_equal(a, b) for a, b in zip(g["waves"], c["waves"]))
        kept = sum(r is not None for r in g["refs"])
        assert kept == g["done"] >= 1 and g["status"] == 0
        assert c["name"] not in pc.MUST_DROP or kept < len(g["waves"])
        assert max(len(w) for w in g["waves"]) <= 0.6 * c["fbank"].get("samp_freq", 16000.0)
    lens = [len(w) for w in GOLD["tol2_16k"]["waves"]]
    assert 559 in lens and GOLD["tol0"]["refs"][lens.index(559)] is None and GOLD["tol2_16k"]["refs"][lens.index(559)].shape == (1, 43)
    assert len(GOLD["s33_8k"]["waves"]) == 33
    assert GOLD["delay2_raw"]["refs"][0].shape[1] == 44
    assert os.path.getsize(pc.GOLDEN) < 512 * 1024


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_row_rule_on_the_fixture(name):
    """Both statements of the rule on the counts of the library's two host-only shape calls."""
    from eesen_amd import _lib
    from eesen_amd.api import Fbank, Pitch
    lib = _lib.load()
    c = GOLD[name]
    fb, pt = Fbank(**c["fbank"]), Pitch(**c["pitch"])
    pipe = fe.FeaturePipeline(source="scp:wav.scp", fbank=c["fbank"], pitch=c["pitch"], tolerance=c["tolerance"], stages=[(fe.FBANK_PITCH, c["tolerance"], 0)])
    for w, ref, (f_r, p_r, _) in zip(c["waves"], c["refs"], pc.rows_of(c)):
        f = fb.shape(len(w))[0]
        p = pt.shape(len(w))[0]
        p = p + c["pitch"].get("delay", 0) if p else 0
        assert (f, p) == (f_r, p_r), "the restatements' frame counts are the library's"
        counts = (C.c_int * 2)(f, p)
        out = C.c_int(-1)
        assert lib.eesen_feat_paste_frames(counts, 2, c["tolerance"], C.byref(out)) == 0
        want = 0 if ref is None else ref.shape[0]
        assert out.value == want == fe.paste_frames([f, p], c["tolerance"]) == pipe.out_frames(len(w))
        if ref is not None:
            assert ref.shape[1] == pipe.out_dim(1) == pipe.cmvn_dim(1) == fb.shape(0)[1] + pt.shape(0)[2]


def test_row_rule_edges():
    from eesen_amd import _lib
    lib = _lib.load()
    out = C.c_int(-1)
    for frames, tol, want in (([5], 0, 5), ([0], 3, 0), ([5, 5, 5, 5], 0, 5), ([5, 6, 7], 2, 5), ([5, 6, 8], 2, 0), ([0, 1], 2, 0), ([3, 1, 2, 4], 3, 1)):
        arr = (C.c_int * len(frames))(*frames)
        assert lib.eesen_feat_paste_frames(arr, len(frames), tol, C.byref(out)) == 0 and out.value == want == fe.paste_frames(frames, tol), (frames, tol)
    arr = (C.c_int * 2)(1, -1)
    assert lib.eesen_feat_paste_frames(arr, 2, 0, C.byref(out)) == -1
    assert lib.eesen_feat_paste_frames(arr, 0, 0, C.byref(out)) == -1
    arr = (C.c_int * 2)(1, 1)
    assert lib.eesen_feat_paste_frames(arr, 2, -1, C.byref(out)) == -1
    with pytest.raises(ValueError):
        fe.paste_frames([1, 1], -1)


# ------------------------------------------------------------------------------------------------ the parser
FBANK_PIPE = "ark:compute-fbank-feats --verbose=2 --num-mel-bins=40 --dither=0 {wav} ark:- |"
PITCH_PIPE = "ark,s,cs:compute-kaldi-pitch-feats --verbose=2 --sample-frequency=16000 {wav} ark:- | process-kaldi-pitch-feats --add-raw-log-pitch=true --delay=1 ark:- ark:- |"
TAIL = " apply-cmvn --norm-vars=true --utt2spk=ark:data/utt2spk scp:data/cmvn.scp ark:- ark:- | add-deltas ark:- ark:- |"


def paste_line(wav_a="scp,p:data/wav.scp", wav_b=None, tol="--length-tolerance=2 ", tail="", head="ark,s,cs:", fbank=FBANK_PIPE, pitch=PITCH_PIPE, more=""):
    return f'{head}paste-feats {tol}"{fbank.format(wav=wav_a)}" "{pitch.format(wav=wav_b or wav_a)}" {more}ark:- |{tail}'


def test_parser_on_the_recipes_command_line(tmp_path):
    """asr_egs/wsj/steps/make_fbank_pitch.sh:117-121 as an rspecifier, in front of the stages that may follow the filterbank head."""
    p = fe.parse_feature_pipeline(paste_line())
    assert p is not None and p.source == "scp,p:data/wav.scp" and p.stages == [(fe.FBANK_PITCH, 2, 0)] and p.tolerance == 2
    assert p.fbank == dict(num_bins=40, dither=0.0) and p.pitch == dict(samp_freq=16000.0, add_raw_log_pitch=True, delay=1)
    assert p.cmvn is None and p.out_dim(1) == p.cmvn_dim(1) == 44
    # the two spellings of the wav table are one table; the filterbank's spelling is kept
    for a, b in (("scp:data/wav.scp", "scp,p:data/wav.scp"), ("scp,p:data/wav.scp", "scp:data/wav.scp"), ("scp:data/wav.scp", "scp:data/wav.scp")):
        q = fe.parse_feature_pipeline(paste_line(a, b))
        assert q is not None and q.source == a and q.stages == p.stages and q.pitch == p.pitch
    # no tolerance option: 0; single quotes; a path in front of the tools
    q = fe.parse_feature_pipeline(paste_line(tol=""))
    assert q.stages == [(fe.FBANK_PITCH, 0, 0)] and q.tolerance == 0
    q = fe.parse_feature_pipeline(paste_line().replace('"', "'").replace("paste-feats", "/opt/bin/paste-feats").replace("ark:compute-fbank", "ark:/opt/bin/compute-fbank"))
    assert q == p
    # trailing stages
    q = fe.parse_feature_pipeline(paste_line(tail=TAIL))
    assert q.stages == [(fe.FBANK_PITCH, 2, 0), (fe.CMVN, 1, 0), (fe.DELTAS, 2, 2)] and q.cmvn == "scp:data/cmvn.scp" and q.utt2spk == "ark:data/utt2spk"
    assert q.cmvn_dim(1) == 44 and q.out_dim(1) == 132
    q = fe.parse_feature_pipeline(paste_line(tail=" splice-feats --left-context=1 --right-context=1 ark:- ark:- | subsample-feats --n=3 ark:- ark:- |"))
    assert q.stages == [(fe.FBANK_PITCH, 2, 0), (fe.SPLICE, 1, 1), (fe.SUBSAMPLE, 3, 0)] and q.out_dim(1) == 132
    assert q.out_frames(16000) == len(range(0, 98, 3))
    # --config files, read first: the command line overrides them
    (tmp_path / "fbank.conf").write_text("--num-mel-bins=23 # the recipe's\n\n--use-energy=false\n--sample-frequency=8000\n")
    (tmp_path / "pitch.conf").write_text("--sample-frequency=8000\n--min-f0=60\n")
    (tmp_path / "post.conf").write_text("--delay=2\n")
    line = paste_line(fbank=f"ark:compute-fbank-feats --config={tmp_path}/fbank.conf --num-mel-bins=30 {{wav}} ark:- |",
                      pitch=f"ark,s,cs:compute-kaldi-pitch-feats --config={tmp_path}/pitch.conf {{wav}} ark:- | process-kaldi-pitch-feats --config={tmp_path}/post.conf ark:- ark:- |")
    q = fe.parse_feature_pipeline(line)
    assert q.fbank == dict(num_bins=30, use_energy=False, samp_freq=8000.0) and q.pitch == dict(samp_freq=8000.0, min_f0=60.0, delay=2)
    # differing rates parse (the rspecifier is this project's to run) and are an error when set on a feeder: tests/test_gpu_paste.py
    q = fe.parse_feature_pipeline(paste_line(pitch=PITCH_PIPE.replace("16000", "8000")))
    assert q is not None and q.pitch["samp_freq"] == 8000.0


def refused_lines(tmp_path):
    bad_conf = tmp_path / "bad.conf"
    bad_conf.write_text("num-mel-bins=23\n")
    return [
        paste_line(fbank=PITCH_PIPE, pitch=FBANK_PIPE),                                       # the inputs in the other order
        paste_line(more="ark:more.ark "),                                                     # a third input
        paste_line(tol="--length-tolerance=2 --binary=false "),                               # --binary
        paste_line(fbank="ark:extract-segments scp,p:data/wav.scp segments ark:- | compute-fbank-feats ark:- ark:- |"),   # extract-segments
        paste_line("scp:a/wav.scp", "scp:b/wav.scp"),                                         # two wav tables
        paste_line(fbank=FBANK_PIPE.replace("--dither=0", "--vtln-map=ark:warps")),           # an option the extractor does not have
        paste_line(pitch=PITCH_PIPE.replace("--delay=1", "--frames-per-chunk=10")),           # not an option of that tool
        paste_line(pitch=PITCH_PIPE.replace("--verbose=2", "--simulate-first-pass-online=true")),   # refused by the device extractor
        paste_line(pitch=PITCH_PIPE.replace("--verbose=2", "--frames-per-chunk=10")),
        paste_line(pitch="ark,s,cs:compute-kaldi-pitch-feats {wav} ark:- |"),                 # no post-processing
        paste_line(fbank="scp:fbank.scp"),                                                    # a table on disk: the host join's
        paste_line(fbank=f"ark:compute-fbank-feats --config={tmp_path}/none.conf {{wav}} ark:- |"),   # a config file that is not there
        paste_line(fbank=f"ark:compute-fbank-feats --config={bad_conf} {{wav}} ark:- |"),     # or is no option file
        paste_line(tol="--length-tolerance=-1 "),
        paste_line().replace('" ark:- |', '" ark:out.ark |'),                                 # does not write to the pipe
        "ark:apply-cmvn scp:c.scp scp:f.scp ark:- | " + paste_line(head=""),                  # not first
        paste_line().replace('ark:- |" "ark,s,cs', 'ark:- |" "ark,s,cs,p'),                   # an rspecifier option other than s, cs
    ]


def test_parser_leaves_the_rest_to_the_shell(tmp_path):
    for line in refused_lines(tmp_path):
        assert fe.parse_feature_pipeline(line) is None, line


def test_rspecifiers_recognised_before_parse_as_before():
    for line, (src, stages, cmvn, u2s) in tf.RECIPE_LINES.items():
        want = fe.FeaturePipeline(source=src, stages=stages, cmvn=cmvn, utt2spk=u2s, norm_vars=bool(stages and stages[0][:2] == (fe.CMVN, 1)))
        assert fe.parse_feature_pipeline(line) == want, line
        assert want.pitch is None and want.tolerance == 0 and want.fbank is None
    for line in tf.REFUSED:
        assert fe.parse_feature_pipeline(line) is None, line
    p = fe.parse_feature_pipeline("ark,s,cs:compute-fbank-feats --dither=0 --num-mel-bins=40 scp:wav.scp ark:- | apply-cmvn scp:c.scp ark:- ark:- | add-deltas ark:- ark:- |")
    assert p == fe.FeaturePipeline(source="scp:wav.scp", stages=[(fe.FBANK, 0, 0), (fe.CMVN, 0, 0), (fe.DELTAS, 2, 2)], cmvn="scp:c.scp",
                                   fbank=dict(dither=0.0, num_bins=40))


def _struct_fields(o):
    return ",".join(f"{getattr(o, n):.9g}" if t is C.c_float else str(int(getattr(o, n))) for n, t in o._fields_)


def test_native_parser_agrees_with_the_python_one(tmp_path):
    """csrc/tools/feat_pipeline.h against eesen_amd/frontend.py on everything above, the extractors' options included."""
    from eesen_amd.api import fbank_opts, pitch_opts
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "parse_paste_pipeline")
    subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "native", "parse_paste_pipeline.cc"), "-o", exe,
                    "-L" + os.path.join(ROOT, "eesen_amd", "lib"), "-leesen_hip", "-Wl,-rpath," + os.path.join(ROOT, "eesen_amd", "lib"),
                    "-Wl,--allow-shlib-undefined"], check=True)
    (tmp_path / "fbank.conf").write_text("--num-mel-bins=23 # the recipe's\n\n--use-energy=true\n--sample-frequency=8000\n")
    (tmp_path / "pitch.conf").write_text("--sample-frequency=8000\n--min-f0=60\n--snip-edges=false\n")
    conf = paste_line(fbank=f"ark:compute-fbank-feats --config={tmp_path}/fbank.conf --num-mel-bins=30 --channel=1 --min-duration=0.25 {{wav}} ark:- |",
                      pitch=f"ark,s,cs:compute-kaldi-pitch-feats --config={tmp_path}/pitch.conf {{wav}} ark:- | process-kaldi-pitch-feats --srand=3 --noise-seed=7 --pov-offset=0.5 ark:- ark:- |")
    lines = [paste_line(), paste_line("scp:data/wav.scp", "scp,p:data/wav.scp"), paste_line(tol=""), paste_line(tail=TAIL), conf,
             paste_line().replace('"', "'"), paste_line(pitch=PITCH_PIPE.replace("16000", "8000"))] + refused_lines(tmp_path) + sorted(tf.RECIPE_LINES) + tf.REFUSED + [
        "ark,s,cs:compute-fbank-feats --dither=0 --num-mel-bins=40 --use-energy=true --channel=1 scp:wav.scp ark:- | apply-cmvn scp:c.scp ark:- ark:- | add-deltas ark:- ark:- |"]
    out = subprocess.run([exe] + lines, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines)
    for line, got in zip(lines, out):
        p = fe.parse_feature_pipeline(line)
        if p is None:
            want = "NONE"
        else:
            want = "|".join([p.source, p.cmvn or "", p.utt2spk or "", str(int(p.norm_vars)), ",".join(f"{k}:{a}:{b}" for k, a, b in p.stages),
                             str(p.channel), f"{float(np.float32(p.min_duration)):.9g}", str(p.tolerance),
                             "F:" + (_struct_fields(fbank_opts(**p.fbank)) if p.fbank is not None else ""),
                             "P:" + (_struct_fields(pitch_opts(**p.pitch)) if p.pitch is not None else "")])
        assert got == want, (line, got, want)


# ------------------------------------------------------------------------------------------------ paste-feats, the host path
def _tool(kind):
    if kind == "native":
        return [os.path.join(ROOT, "eesen_amd", "bin", "paste-feats")]
    return [sys.executable, "-m", "eesen_amd.paste_feats"]


def _run(cmd, **kw):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env, **kw)


def _tables(c, tmp, rng):
    """The two tables the reference's paste-feats read for this case, rebuilt from the fixture: the kept rows are the pasted matrix's
    columns, the rows past them (which the join trims) and the matrices of dropped utterances are noise of the right shape; an
    utterance without a filterbank matrix is not in the first table, one without a pitch matrix not in the second."""
    from eesen_amd import kaldi_io
    nfb = next(r for r in c["refs"] if r is not None).shape[1] - _pitch_dim(c)
    fb, pt = [], []
    for i, (ref, (f, p, _)) in enumerate(zip(c["refs"], pc.rows_of(c))):
        a, b = rng.normal(0.0, 1.0, (f, nfb)).astype(np.float32), rng.normal(0.0, 1.0, (p, _pitch_dim(c))).astype(np.float32)
        if ref is not None:
            a[:ref.shape[0]], b[:ref.shape[0]] = ref[:, :nfb], ref[:, nfb:]
        if f:
            fb.append((f"utt{i:03d}", a))
        if p:
            pt.append((f"utt{i:03d}", b))
    kaldi_io.write_mat_ark(os.path.join(tmp, "fbank.ark"), fb)
    kaldi_io.write_mat_ark(os.path.join(tmp, "pitch.ark"), pt, scp_path=os.path.join(tmp, "pitch.scp"))
    return fb, pt


def _pitch_dim(c):
    from tests import pitch_restatement as pr
    return pr.process_dim(c["pitch"])


@pytest.mark.parametrize("kind", ["native", "python"])
@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_paste_feats_host_path_against_the_fixture(tmp_path, name, kind):
    from eesen_amd import kaldi_io
    c = GOLD[name]
    _tables(c, str(tmp_path), np.random.default_rng(7))
    for second in (f"ark,s,cs:{tmp_path}/pitch.ark", f"scp:{tmp_path}/pitch.scp"):
        r = _run(_tool(kind) + [f"--length-tolerance={c['tolerance']}", f"ark:{tmp_path}/fbank.ark", second, f"ark:{tmp_path}/out.ark"])
        assert r.returncode == c["status"], r.stderr
        got = dict(kaldi_io.read_mat_table(f"ark:{tmp_path}/out.ark"))
        want = {f"utt{i:03d}": ref for i, ref in enumerate(c["refs"]) if ref is not None}
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k].shape == want[k].shape and np.array_equal(np.asarray(got[k], np.float32).view(np.uint32), want[k].view(np.uint32)), k
        warnings = [w.replace(second, "2") for w in pc.warnings_of(r.stderr)]
        assert warnings == c["warnings"], r.stderr
        assert f"Done {c['done']} utts, errors on {c['err']}" in r.stderr


@pytest.mark.parametrize("kind", ["native", "python"])
def test_paste_feats_usage_missing_keys_and_single_matrices(tmp_path, kind):
    from eesen_amd import kaldi_io
    rng = np.random.default_rng(11)
    a = [(f"u{i}", rng.normal(0, 1, (5 + i, 3)).astype(np.float32)) for i in range(4)]
    b = [(k, rng.normal(0, 1, (m.shape[0] + 1, 2)).astype(np.float32)) for k, m in a if k != "u1"]
    cc = [(k, rng.normal(0, 1, (m.shape[0], 1)).astype(np.float32)) for k, m in reversed(a)]          # unsorted: read whole
    for tag, t in (("a", a), ("b", b), ("c", cc)):
        kaldi_io.write_mat_ark(str(tmp_path / f"{tag}.ark"), t)
    r = _run(_tool(kind) + ["--length-tolerance=1", f"ark:{tmp_path}/a.ark", f"ark,s,cs:{tmp_path}/b.ark", f"ark:{tmp_path}/c.ark", f"ark,t:{tmp_path}/out.txt"])
    assert r.returncode == 0, r.stderr
    assert pc.warnings_of(r.stderr) == ["Missing utt u1 from input 2"] and "Done 3 utts, errors on 1" in r.stderr
    got = dict(kaldi_io.read_mat_table(f"ark,t:{tmp_path}/out.txt"))
    for (k, m) in a:
        if k != "u1":
            np.testing.assert_allclose(got[k], np.hstack([m, dict(b)[k][:m.shape[0]], dict(cc)[k]]), rtol=1e-6)
    # nothing done: the reference returns -1
    r = _run(_tool(kind) + [f"ark:{tmp_path}/a.ark", f"ark:{tmp_path}/b.ark", f"ark:{tmp_path}/none.ark"])
    assert r.returncode == 255 and "Done 0 utts, errors on 4" in r.stderr, r.stderr
    assert sum("exceeds tolerance 0" in w for w in pc.warnings_of(r.stderr)) == 3
    # too few arguments: the usage, status 1
    r = _run(_tool(kind) + [f"ark:{tmp_path}/a.ark", f"ark:{tmp_path}/out.ark"])
    assert r.returncode == 1 and "Usage: paste-feats <in-rspecifier1>" in r.stderr
    # the rxfilename form, binary and text
    x, y = a[0][1], b[0][1]
    kaldi_io.write_mat_file(str(tmp_path / "x.mat"), x)
    kaldi_io.write_mat_file(str(tmp_path / "y.mat"), y, binary=False)
    r = _run(_tool(kind) + ["--length-tolerance=1", str(tmp_path / "x.mat"), str(tmp_path / "y.mat"), str(tmp_path / "xy.mat")])
    assert r.returncode == 0 and "Wrote appended features to" in r.stderr, r.stderr
    assert np.array_equal(kaldi_io.read_mat_file(str(tmp_path / "xy.mat")), np.hstack([x, y[:5]]))
    r = _run(_tool(kind) + ["--length-tolerance=1", "--binary=false", str(tmp_path / "x.mat"), str(tmp_path / "y.mat"), str(tmp_path / "xy.txt")])
    assert r.returncode == 0 and open(tmp_path / "xy.txt").read().lstrip().startswith("[")
    np.testing.assert_allclose(kaldi_io.read_mat_file(str(tmp_path / "xy.txt")), np.hstack([x, y[:5]]), rtol=1e-6)
    r = _run(_tool(kind) + [str(tmp_path / "x.mat"), str(tmp_path / "y.mat"), str(tmp_path / "no.mat")])
    assert r.returncode == 1 and pc.warnings_of(r.stderr) == ["Length mismatch 6 vs. 5 exceeds tolerance 0"] and not os.path.exists(tmp_path / "no.mat")
