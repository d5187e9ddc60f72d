#!/usr/bin/env python3
"""Device time of the pitch extractor (eesen_pitch_bench): S waveforms of a given length, per launch and per kernel, without the
copies; optionally the same waveforms through a build of the reference's compute-kaldi-pitch-feats on one host thread.

    python scripts/pitch_probe.py --rate 16000 --utts 32 --seconds 10 [--ref-binary PATH] [--json out.json]

The figures of profiles/pitch.md were taken with this script.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
import wave as wavmod

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def voiced(rng, n, sf):
    t = np.arange(n) / sf
    f0 = 120.0 + 60.0 * np.sin(2.0 * np.pi * 0.4 * t + rng.uniform(0, 6.28))
    phase = 2.0 * np.pi * np.cumsum(f0) / sf
    x = sum(np.sin(k * phase) / k for k in range(1, 6)) * (0.5 + 0.5 * np.sin(2.0 * np.pi * 1.3 * t) ** 2)
    return np.clip(np.rint(5000.0 * x + rng.normal(0.0, 30.0, n)), -32768, 32767).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=float, default=16000.0)
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--ref-binary", default="")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    from eesen_amd.api import Pitch
    rng = np.random.default_rng(1)
    waves = [voiced(rng, int(a.rate * a.seconds), a.rate) for _ in range(a.utts)]
    pt = Pitch(samp_freq=a.rate, delta_pitch_noise_stddev=0.0)
    frames = sum(pt.shape(len(w))[0] for w in waves)
    ms = [float(v) for v in pt.bench(waves, a.iters)]
    longest = max(pt.shape(len(w))[0] for w in waves)
    r = dict(rate=a.rate, utts=a.utts, seconds=a.seconds, frames=frames, states=len(pt.lags()), ms_launch=ms[0], ms_downsample=ms[1],
             ms_nccf=ms[2], ms_viterbi=ms[3], ms_process=ms[4], frames_per_second=frames / (ms[0] * 1e-3),
             viterbi_share=ms[3] / ms[0], viterbi_us_per_frame_step=ms[3] * 1e3 / longest)
    t0 = time.perf_counter()
    out = pt.compute(waves, process=True)
    r["ms_compute_with_copies"] = (time.perf_counter() - t0) * 1e3
    assert sum(m.shape[0] for m in out) == frames
    if a.ref_binary:
        with tempfile.TemporaryDirectory() as tmp:
            with open(os.path.join(tmp, "wav.scp"), "w") as f:
                for i, w in enumerate(waves):
                    p = os.path.join(tmp, f"u{i}.wav")
                    with wavmod.open(p, "wb") as wf:
                        wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(int(a.rate)); wf.writeframes(w.astype("<i2").tobytes())
                    f.write(f"u{i:03d} {p}\n")
            env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1")
            t0 = time.perf_counter()
            subprocess.run([a.ref_binary, f"--sample-frequency={int(a.rate)}", f"scp:{tmp}/wav.scp", f"ark:{tmp}/out.ark"], check=True,
                           capture_output=True, env=env)
            r["ref_ms"] = (time.perf_counter() - t0) * 1e3
            r["ref_frames_per_second"] = frames / (r["ref_ms"] * 1e-3)
    print(json.dumps(r))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(r, f)


if __name__ == "__main__":
    main()
