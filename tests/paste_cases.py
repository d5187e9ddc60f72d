"""Case list of the filterbank + pitch tests (tests/test_paste_cases.py on the CPU, tests/test_gpu_paste.py on the GPU).

A case is the option set of compute-fbank-feats (keys of `eesen_fbank_opts_t`, dither 0), the option set of compute-kaldi-pitch-feats
and process-kaldi-pitch-feats together (keys of `eesen_pitch_opts_t`, delta-pitch noise 0), paste-feats' --length-tolerance, and the
waveforms of one launch.  tests/golden/paste.npz holds, per case, the int16 waveforms, what the reference's own

    paste-feats --length-tolerance=N "ark:compute-fbank-feats ... scp:wav.scp ark:- |" \
                "ark,s,cs:compute-kaldi-pitch-feats ... scp:wav.scp ark:- | process-kaldi-pitch-feats ... ark:- ark:- |" ark:out

wrote for every waveform (its pasted matrix; nothing for an utterance it left out), and the two counts of its log line
"Done N utts, errors on M".

`write_golden(bindir)` is how the file was made.  The four tools were built out of tree, in a scratch directory that is not kept, the
way tests/pitch_cases.py describes (plus feat/feature-fbank.cc and the two more featbin sources).  The reference's
compute-fbank-feats crashes on a waveform without a frame, its compute-kaldi-pitch-feats writes an EMPTY matrix for one and its
process-kaldi-pitch-feats cannot read that, so write_golden runs the inner pipes one tool at a time through tables on disk, keeps such
waveforms from the filterbank tool and drops the empty matrices in between.  paste-feats then never sees an utterance without a
filterbank matrix (it walks the first table) and reports one without a pitch matrix as "Missing utt" -- it writes nothing for either.
Its warnings (texts only) and exit status are stored with the counts.

Conditions on the fixture, checked by write_golden and again by tests/test_paste_cases.py: every case keeps at least one utterance;
tol0, s33_8k and snip_mixed drop at least one.

Waveforms are at most 0.6 s.  The cases:
  tol2_16k      16 kHz, 40 bins + 3 pitch columns, tolerance 2: three gliding harmonic complexes and one waveform of 559 samples (one
                filterbank frame, two pitch frames)
  tol0          the same at tolerance 0: the 559-sample waveform goes
  s33_8k        8 kHz, 23 bins, S = 33 ragged, voiced and noise alternating; one waveform without a frame in either extractor and one
                with pitch frames but no filterbank frame
  snip_mixed    filterbank --snip-edges=false against pitch --snip-edges=true --frame-length=35 at tolerance 2: lengths searched for on
                both sides of it (counts differ by 2 or 3), and one waveform with filterbank frames but no pitch frame ("Missing utt")
  delay2_raw    process-kaldi-pitch-feats --delay=2 --add-raw-log-pitch=true: four pitch columns, two more rows, tolerance 3
"""
import json
import os
import re
import subprocess
import tempfile

import numpy as np

from tests import fbank_cases as fc
from tests import fbank_restatement as fr
from tests import pitch_cases as pc
from tests import pitch_restatement as pr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "paste.npz")
MUST_DROP = ("tol0", "s33_8k", "snip_mixed")


def fbank_frames(n, case):
    return fr.num_frames(n, case["fbank"])


def pitch_rows(n, case):
    """Rows of the processed pitch matrix: frames + delay, none without a frame."""
    f = pr.num_frames(n, case["pitch"])[1]
    return f + pr.full_process(case["pitch"])["delay"] if f else 0


def paste_rule(counts, tolerance):
    """AppendFeats (paste-feats.cc:35-56) on row counts: the kept rows, 0 = no output."""
    lo, hi = min(counts), max(counts)
    return 0 if hi - lo > tolerance or lo == 0 else lo


def rows_of(case):
    """Per waveform: (filterbank frames, processed pitch rows, pasted rows) from the two restatements' frame counts."""
    return [(fbank_frames(len(w), case), pitch_rows(len(w), case), paste_rule([fbank_frames(len(w), case), pitch_rows(len(w), case)], case["tolerance"]))
            for w in case["waves"]]


def _cases():
    rng = np.random.default_rng(20240915)
    cases = []

    def add(name, fbank, pitch, tolerance, waves):
        fb, pt = dict(fbank, dither=0.0), dict(pitch, delta_pitch_noise_stddev=0.0)
        cases.append(dict(name=name, fbank=fb, pitch=pt, tolerance=tolerance, waves=waves))

    def search(case, want, lo, hi):
        """The first sample count in [lo, hi) whose (filterbank frames, pitch rows) satisfy `want`."""
        for n in range(lo, hi):
            if want(fbank_frames(n, case), pitch_rows(n, case)):
                return n
        raise AssertionError("no such length")

    w16 = [pc.voiced(rng, 9600, 16000.0), pc.voiced(rng, 5600, 16000.0, 120.0, 260.0), pc.voiced(rng, 3437, 16000.0, 280.0, 110.0),
           pc.voiced(rng, 559, 16000.0, 150.0, 170.0)]
    add("tol2_16k", dict(num_bins=40), {}, 2, w16)
    add("tol0", dict(num_bins=40), {}, 0, w16)
    # S = 33 ragged at 8 kHz
    fb, pt = dict(samp_freq=8000.0), dict(samp_freq=8000.0)
    probe = dict(fbank=fb, pitch=pt, tolerance=2)
    w = []
    for i in range(33):
        n = int(rng.integers(400, 1700))
        w.append(pc.voiced(rng, n, 8000.0, 100.0 + 5 * i, 300.0 - 4 * i) if i % 2 == 0 else pc.white(rng, n, 2500.0))
    w[5] = pc.white(rng, search(probe, lambda f, p: f == 0 and p == 0, 60, 400), 2500.0)
    w[11] = pc.voiced(rng, search(probe, lambda f, p: (f == 0) != (p == 0), 100, 400), 8000.0, 150.0, 160.0)
    add("s33_8k", fb, pt, 2, w)
    # centred filterbank frames against snipped pitch frames: about n / shift + 0.5 against (n - window) / shift + 1.  With both
    # windows at 25 ms the difference is 1 or 2 at every length, never past the tolerance; a 35 ms pitch window makes it 2 or 3
    fb, pt = dict(num_bins=40, snip_edges=False), dict(snip_edges=True, frame_length_ms=35.0)
    probe = dict(fbank=fb, pitch=pt, tolerance=2)
    far = search(probe, lambda f, p: p > 0 and f - p > 2, 2000, 4000)
    near = search(probe, lambda f, p: p > 0 and f - p == 2, 4000, 6000)
    add("snip_mixed", fb, pt, 2, [pc.voiced(rng, far, 16000.0), pc.voiced(rng, near, 16000.0, 130.0, 240.0), pc.white(rng, near + 160, 2500.0),
                                  pc.voiced(rng, far + 320, 16000.0, 200.0, 90.0),
                                  pc.white(rng, search(probe, lambda f, p: f > 0 and p == 0, 300, 700), 2500.0)])
    add("delay2_raw", dict(num_bins=40), dict(delay=2, add_raw_log_pitch=True), 3,
        [pc.voiced(rng, 6400, 16000.0, 110.0, 290.0), pc.white(rng, 2000, 2500.0), pc.voiced(rng, 1200, 16000.0, 240.0, 180.0)])
    return cases


CASES = _cases()
CASE_NAMES = [c["name"] for c in CASES]


def load_golden():
    """{case: dict(fbank, pitch, tolerance, waves [int16], refs [pasted float32 matrix or None per waveform], done, err)}"""
    z = np.load(GOLDEN)
    out = {}
    for name in json.loads(str(z["names"])):
        n = int(z[name + "/count"])
        out[name] = dict(name=name, fbank=json.loads(str(z[name + "/fbank"])), pitch=json.loads(str(z[name + "/pitch"])),
                         tolerance=int(z[name + "/tolerance"]), done=int(z[name + "/done"]), err=int(z[name + "/err"]),
                         status=int(z[name + "/status"]), warnings=json.loads(str(z[name + "/warnings"])),
                         waves=[z[f"{name}/wave{i}"] for i in range(n)],
                         refs=[z[f"{name}/ref{i}"] if f"{name}/ref{i}" in z.files else None for i in range(n)])
    return out


def fbank_flags(case):
    return fc.flags(case["fbank"])


def pitch_flags(case):
    """(compute-kaldi-pitch-feats' flags, process-kaldi-pitch-feats' flags)"""
    return pc.flags(case["pitch"]), pc.flags(case["pitch"], pc.PROCESS_FLAGS)


def write_waves(case, tmp, tag="wav", keep=lambda i, w: True):
    """The case's waveforms as files and the wav.scp naming them (keys utt000, utt001, ...; only those `keep` passes)."""
    scp = os.path.join(tmp, tag + ".scp")
    with open(scp, "w") as f:
        for i, w in enumerate(case["waves"]):
            if not keep(i, w):
                continue
            p = os.path.join(tmp, f"{tag}_{i}.wav")
            fc.write_wav(p, w, fr.full(case["fbank"])["samp_freq"])
            f.write(f"utt{i:03d} {p}\n")
    return scp


def warnings_of(stderr):
    """The texts of paste-feats' warnings, the input named in "Missing utt ... from input ..." replaced by its number (2 = the pitch table)."""
    out = []
    for line in stderr.splitlines():
        if line.startswith("WARNING"):
            msg = line.split(") ", 1)[1].strip()
            out.append(re.sub(r"from input .*$", "from input 2", msg))
    return out


# ---------------------------------------------------------------------------------------------- how the fixture was made
def write_golden(bindir, path=GOLDEN):
    """Runs the reference's compute-fbank-feats, compute-kaldi-pitch-feats, process-kaldi-pitch-feats and paste-feats (in `bindir`)
    on every case."""
    from eesen_amd import kaldi_io
    tool = lambda t: os.path.join(bindir, t)
    data = {"names": json.dumps(CASE_NAMES)}
    with tempfile.TemporaryDirectory() as tmp:
        for c in CASES:
            name = c["name"]
            d = os.path.join(tmp, name)
            os.mkdir(d)
            scp = write_waves(c, d)
            fb_scp = write_waves(c, d, "fbwav", lambda i, w: fbank_frames(len(w), c) > 0)    # (the tool crashes on a waveform without a frame)
            cflags, pflags = pitch_flags(c)
            fb_ark, raw_ark, keep_ark, pt_ark, out_ark = (os.path.join(d, t + ".ark") for t in ("fbank", "raw", "keep", "pitch", "out"))
            subprocess.run([tool("compute-fbank-feats")] + fbank_flags(c) + ["scp:" + fb_scp, "ark:" + fb_ark], check=True, capture_output=True)
            subprocess.run([tool("compute-kaldi-pitch-feats")] + cflags + ["scp:" + scp, "ark:" + raw_ark], check=True, capture_output=True)
            raws = [(k, np.asarray(m, np.float32)) for k, m in kaldi_io.read_mat_table("ark:" + raw_ark) if np.asarray(m).size]
            kaldi_io.write_mat_ark(keep_ark, raws)
            subprocess.run([tool("process-kaldi-pitch-feats")] + pflags + ["ark:" + keep_ark, "ark:" + pt_ark], check=True, capture_output=True)
            r = subprocess.run([tool("paste-feats"), f"--length-tolerance={c['tolerance']}", "ark:" + fb_ark, "ark,s,cs:" + pt_ark, "ark:" + out_ark],
                               capture_output=True, text=True)
            m = re.search(r"Done (\d+) utts, errors on (\d+)", r.stderr)
            assert m, r.stderr
            data[name + "/fbank"], data[name + "/pitch"] = json.dumps(c["fbank"]), json.dumps(c["pitch"])
            data[name + "/tolerance"], data[name + "/count"] = c["tolerance"], len(c["waves"])
            data[name + "/done"], data[name + "/err"] = int(m.group(1)), int(m.group(2))
            data[name + "/status"], data[name + "/warnings"] = r.returncode, json.dumps(warnings_of(r.stderr))
            for i, w in enumerate(c["waves"]):
                data[f"{name}/wave{i}"] = w
            kept = 0
            for key, mat in kaldi_io.read_mat_table("ark:" + out_ark):
                data[f"{name}/ref{int(key[3:])}"] = np.asarray(mat, np.float32)
                kept += 1
            # the conditions on the fixture; the float64 pitch restatement must also pick the tool's lag on every frame (as in pitch.npz)
            assert kept == int(m.group(1)) >= 1, (name, kept, r.stderr)
            assert name not in MUST_DROP or kept < len(c["waves"]), name
            lags = pr.lags(c["pitch"])
            for key, raw in raws:
                mine = pr.compute(c["waves"][int(key[3:])].astype(np.float64), c["pitch"])["out"]
                pick = lambda x: np.argmin(np.abs(1.0 / lags.astype(np.float64)[None, :] - np.asarray(x, np.float64)[:, 1:2]), axis=1)
                assert np.array_equal(pick(mine), pick(raw)), (name, key)
    np.savez_compressed(path, **data)
