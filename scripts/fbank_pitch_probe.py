#!/usr/bin/env python3
"""Timings of the filterbank + pitch head stage (EESEN_FEAT_FBANK_PITCH) and of bin/paste-feats on its fused path.

    python scripts/fbank_pitch_probe.py head  [--utts 32 --seconds 10 --batches 20]   # the head stage beside the two extractors
    python scripts/fbank_pitch_probe.py loop  [--utts 32 --seconds 10 --batches 20]   # the head stage alone (to run under a kernel trace)
    python scripts/fbank_pitch_probe.py tools [--utts 512 --seconds 5 --repeats 3]    # bin/paste-feats against tables + host join

`head`: per batch, a host clock from submit_raw to a device synchronise behind acquire (staging into pinned memory, one upload, the
filterbank, the four pitch launches, the join, the interleave), two slots warmed first; beside it eesen_fbank_bench and
eesen_pitch_bench on the same waveforms (device events, kernels only, no copies) and api.Fbank.compute + api.Pitch.compute(process=True)
(host clock, with their uploads and copies back).  `tools`: whole fresh processes by the wall clock, alternating the two ways.
The figures of profiles/fbank_pitch.md were taken with this script.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time
import wave as wavmod

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.pitch_probe import voiced  # noqa: E402

FBANK = dict(num_bins=40, dither=0.0)
PITCH = dict(delta_pitch_noise_stddev=0.0)
FBANK_PITCH = 6


def sync(mat):
    """A device synchronise behind everything the compute stream waits for: a blocking 4-byte copy from the assembled matrix."""
    from eesen_amd import _lib
    word = np.zeros(1, np.float32)
    _lib.check(_lib.load().eesen_dev_copy(mat.device, word.ctypes.data_as(C.c_void_p), C.c_void_p(mat.ptr), 4, 2))


def head_times(feeder, cols, batches):
    out = []
    for i in range(batches + 2):
        t0 = time.perf_counter()
        slot = feeder.submit_raw(cols)
        mat = feeder.acquire(slot)
        sync(mat)
        t1 = time.perf_counter()
        feeder.release(slot)
        if i >= 2:
            out.append((t1 - t0) * 1e3)
    return out


def make_feeder(slots=2):
    from eesen_amd.api import Feeder
    f = Feeder(slots=slots)
    f.set_fbank(**FBANK)
    f.set_pitch(**PITCH)
    f.set_pipeline([(FBANK_PITCH, 2, 0)])
    return f


def head(a, alone=False):
    from eesen_amd import _lib
    from eesen_amd.api import Fbank, Pitch
    rng = np.random.default_rng(1)
    waves = [voiced(rng, int(16000 * a.seconds), 16000.0) for _ in range(a.utts)]
    cols = [w.astype(np.float32).reshape(-1, 1) for w in waves]
    f = make_feeder()
    ms = head_times(f, cols, a.batches)
    r = dict(utts=a.utts, seconds=a.seconds, rows=sum(f.pipeline_shape(1, len(w))[0] for w in waves), cols=f.pipeline_shape(1, len(waves[0]))[1],
             head_ms_median=float(np.median(ms)), head_ms_min=float(np.min(ms)), head_ms_max=float(np.max(ms)), batches=a.batches)
    if not alone:
        fb, pt = Fbank(**FBANK), Pitch(**PITCH)
        S = len(waves)
        w32 = [w.astype(np.float32) for w in waves]
        ptr = (C.c_void_p * S)(*[w.ctypes.data for w in w32])
        ns = np.array([len(w) for w in w32], np.int32)
        one = C.c_float()
        _lib.check(fb.lib.eesen_fbank_bench(fb.h, ptr, ns.ctypes.data_as(C.POINTER(C.c_int)), S, 10, C.byref(one)))
        r["fbank_bench_ms"] = float(one.value)
        pb = [float(v) for v in pt.bench(waves, 5)]
        r["pitch_bench_ms"], r["pitch_viterbi_ms"] = pb[0], pb[3]
        r["sum_bench_ms"] = r["fbank_bench_ms"] + r["pitch_bench_ms"]
        both = []
        for i in range(a.batches // 2 + 1):
            t0 = time.perf_counter()
            fb.compute(waves)
            pt.compute(waves, process=True)
            if i:
                both.append((time.perf_counter() - t0) * 1e3)
        r["two_extractors_with_copies_ms_median"] = float(np.median(both))
    print(json.dumps(r))
    return r


def tools(a):
    rng = np.random.default_rng(2)
    bindir = os.path.join(ROOT, "bin")
    env = dict(os.environ, PATH="/usr/bin:/bin")
    with tempfile.TemporaryDirectory() as tmp:
        scp = os.path.join(tmp, "wav.scp")
        n = int(16000 * a.seconds)
        with open(scp, "w") as f:
            for i in range(a.utts):
                p = os.path.join(tmp, f"u{i:04d}.wav")
                with wavmod.open(p, "wb") as wf:
                    wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000)
                    wf.writeframes(voiced(rng, n - int(rng.integers(0, 8000)), 16000.0).astype("<i2").tobytes())
                f.write(f"u{i:04d} {p}\n")
        fbp = f"ark:compute-fbank-feats --num-mel-bins=40 --dither=0 scp,p:{scp} ark:- |"
        ptp = f"ark,s,cs:compute-kaldi-pitch-feats scp,p:{scp} ark:- | process-kaldi-pitch-feats --delta-pitch-noise-stddev=0 ark:- ark:- |"
        fused_cmd = [[os.path.join(bindir, "paste-feats"), "--length-tolerance=2", fbp, ptp, f"ark:{tmp}/fused.ark"]]
        tables_cmd = [[os.path.join(bindir, "compute-fbank-feats"), "--num-mel-bins=40", "--dither=0", f"scp:{scp}", f"ark:{tmp}/fbank.ark"],
                      [os.path.join(bindir, "compute-kaldi-pitch-feats"), f"scp:{scp}", f"ark:{tmp}/raw.ark"],
                      [os.path.join(bindir, "process-kaldi-pitch-feats"), "--delta-pitch-noise-stddev=0", f"ark:{tmp}/raw.ark", f"ark:{tmp}/pitch.ark"],
                      [os.path.join(bindir, "paste-feats"), "--length-tolerance=2", f"ark:{tmp}/fbank.ark", f"ark,s,cs:{tmp}/pitch.ark", f"ark:{tmp}/host.ark"]]

        def run(cmds):
            t0 = time.perf_counter()
            for c in cmds:
                subprocess.run(c, check=True, capture_output=True, env=env, cwd=ROOT, timeout=600)
            return time.perf_counter() - t0

        run(fused_cmd); run(tables_cmd)         # the page cache holds the wav files for every timed run
        fused, tables = [], []
        for _ in range(a.repeats):
            fused.append(run(fused_cmd))
            tables.append(run(tables_cmd))
        same = open(f"{tmp}/fused.ark", "rb").read() == open(f"{tmp}/host.ark", "rb").read()
    r = dict(utts=a.utts, seconds=a.seconds, fused_s=fused, tables_s=tables, ratio=float(np.median(tables) / np.median(fused)), identical=same)
    print(json.dumps(r))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["head", "loop", "tools"])
    ap.add_argument("--utts", type=int, default=0)
    ap.add_argument("--seconds", type=float, default=0.0)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    a.utts = a.utts or (512 if a.what == "tools" else 32)
    a.seconds = a.seconds or (5.0 if a.what == "tools" else 10.0)
    r = tools(a) if a.what == "tools" else head(a, alone=a.what == "loop")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(r, f)


if __name__ == "__main__":
    main()
