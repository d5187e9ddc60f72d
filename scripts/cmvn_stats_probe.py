#!/usr/bin/env python3
"""Writes profiles/cmvn_stats.md: timings of the CMVN statistics kernel, of the feeder's statistics tap and of compute-cmvn-stats.

  python scripts/cmvn_stats_probe.py [--out profiles/cmvn_stats.md] [--iters 50] [--rounds 7] [--utts 512] [--bench-parent DIR]

* the kernel alone (eesen_cmvn_stats_bench: HIP events around back-to-back launches after a warm-up, no copies) at 32 x 1000 x 43,
  64 x 3000 x 43 and 32 x 1000 x 120, median and minimum over the rounds, next to the time the bytes need at the HBM rate a float4
  copy reaches (the other decomposition, one workgroup per utterance, was timed by an earlier form of this script and is gone: the
  figures are in csrc/cmvn_stats.hip);
* the tap: feeder submit_raw -> acquire -> device synchronise on the filterbank head, 32 waveforms of 10 s, tap on and off alternating;
* the tool end to end on a synthetic wav.scp: from the audio in one process, against bin/compute-fbank-feats writing an archive and
  the tool reading it, and against the reference's host compute-cmvn-stats on that archive where oracle/_ref holds it;
* with --bench-parent DIR (a built tree of the parent commit): `python bench.py --gpus 1 --steps 20 --warmup 5` in DIR
  and in this tree, alternating, three times each: the headline must not move.
Without a GPU nothing is measured.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eesen_amd import _lib, api, frontend as fe              # noqa: E402
from tests import fbank_cases as fc                          # noqa: E402

HBM_COPY_RATE = 6.29e12     # bytes / s, a float4 copy on this device (the vendor's peak is 8.0e12)
HBM_PEAK = 8.0e12
SHAPES = [(32, 1000, 43), (64, 3000, 43), (32, 1000, 120)]


def kernel_times(iters, rounds):
    rng = np.random.default_rng(0)
    out = {}
    for S, T, D in SHAPES:
        mats = [rng.normal(15.0, 3.0, (T, D)).astype(np.float32) for _ in range(S)]
        out[(S, T, D)] = [api.cmvn_stats_bench(mats, iters) for _ in range(rounds)]
    return out


def headline(parent, repeats=3):
    """ms per step of bench.py's headline in the parent's tree and in this one, alternating."""
    res = {"parent": [], "this commit": []}
    for _ in range(repeats):
        for tag, d in (("parent", parent), ("this commit", ROOT)):
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=d, capture_output=True, text=True)
            lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
            assert r.returncode == 0 and lines, r.stderr[-2000:]
            res[tag].append(json.loads(lines[-1])["ms_per_step"])
    return res


def tap_cost(rounds):
    S, n = 32, 160000
    rng = np.random.default_rng(1)
    waves = [np.rint(rng.normal(0.0, 3000.0, n)).astype(np.float32).reshape(-1, 1) for _ in range(S)]
    f = api.Feeder(slots=2)
    f.set_fbank(num_bins=40, dither=1.0)
    f.set_pipeline([(fe.FBANK, 0, 0)])
    lib = _lib.load()

    def once():
        t0 = time.perf_counter()
        slot = f.submit_raw(waves)
        f.acquire(slot)
        _lib.check(lib.eesen_device_synchronize(0))
        dt = time.perf_counter() - t0
        f.release(slot)
        return dt * 1e3

    res = {"off": [], "on": []}
    for _ in range(3):
        once()
    for _ in range(rounds):
        for tag, b in (("off", -1), ("on", 1)):
            f.set_stats_tap(b)
            once()
            res[tag].append(once())
    return res


def tool_times(utts, tmp):
    rng = np.random.default_rng(2)
    sf = 16000
    with open(os.path.join(tmp, "wav.scp"), "w") as scp:
        for i in range(utts):
            n = int(rng.integers(3 * sf, 8 * sf))
            w = np.clip(np.rint(rng.normal(0.0, 3000.0, n)), -32768, 32767).astype(np.int16)
            fc.write_wav(os.path.join(tmp, f"w{i}.wav"), w, sf)
            scp.write(f"utt{i:04d} {tmp}/w{i}.wav\n")
    env = dict(os.environ, PATH="/usr/bin:/bin")
    flags = ["--num-mel-bins=40", "--dither=0"]

    def run(cmd):
        t0 = time.perf_counter()
        r = subprocess.run(cmd, capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        return time.perf_counter() - t0

    tool = os.path.join(ROOT, "bin", "compute-cmvn-stats")
    fbank = os.path.join(ROOT, "bin", "compute-fbank-feats")
    res = {}
    for _ in range(2):      # the second pass reads the files from the page cache
        res["from audio, one process"] = run([tool, f"ark:compute-fbank-feats {' '.join(flags)} scp:{tmp}/wav.scp ark:- |", f"ark:{tmp}/a.ark"])
        res["compute-fbank-feats -> archive"] = run([fbank] + flags + [f"scp:{tmp}/wav.scp", f"ark:{tmp}/fbank.ark"])
        res["this tool on the archive"] = run([tool, f"ark:{tmp}/fbank.ark", f"ark:{tmp}/b.ark"])
    same = open(f"{tmp}/a.ark", "rb").read() == open(f"{tmp}/b.ark", "rb").read()
    ref = os.path.join(ROOT, "oracle", "_ref", "featbin", "compute-cmvn-stats")
    if os.path.exists(ref):
        for _ in range(2):
            res["reference host tool on the archive"] = run([ref, f"ark:{tmp}/fbank.ark", f"ark:{tmp}/c.ark"])
    frames = sum(1 for _ in open(f"{tmp}/wav.scp"))
    return res, same, frames, os.path.getsize(f"{tmp}/fbank.ark")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmvn_stats.md"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--utts", type=int, default=512)
    ap.add_argument("--bench-parent", default=None, help="a built tree of the parent commit: alternate bench.py there and here")
    a = ap.parse_args()
    try:
        on_gpu = _lib.device_count() > 0
    except Exception:
        on_gpu = False
    L = ["# CMVN statistics on the device (`csrc/cmvn_stats.hip`)", "",
         "Written by `scripts/cmvn_stats_probe.py`" + (" on one MI355X." if on_gpu else " WITHOUT a GPU: nothing is measured."), ""]
    if on_gpu:
        med, mn = statistics.median, min
        L += ["## Kernel time", "",
              f"`eesen_cmvn_stats_bench`: HIP events around {a.iters} back-to-back launches (the chunk kernel and the finishing one) after a warm-up,",
              f"no copies; {a.rounds} rounds, median (minimum).  The inputs fit the Infinity Cache, so repeated launches read them from there; the HBM",
              "column is what a cold launch could not beat.", "",
              "| S x frames x D | bytes read | both launches | HBM-bound (6.29 TB/s float4 copy) | bytes read / time, share of the 8 TB/s peak |",
              "|---|---|---|---|---|"]
        for (S, T, D), ms in kernel_times(a.iters, a.rounds).items():
            nbytes = S * T * D * 4
            L.append(f"| {S} x {T} x {D} | {nbytes / 1e6:.1f} MB | {med(ms) * 1e3:.1f} us ({mn(ms) * 1e3:.1f}) | {nbytes / HBM_COPY_RATE * 1e6:.1f} us | "
                     f"{nbytes / (med(ms) * 1e-3) / HBM_PEAK * 100:.1f} % |")
        L += ["", "Not measured: a cold (HBM-resident) input, counters."]
        t = tap_cost(a.rounds)
        L += ["", "## Cost of the tap: filterbank head, 32 waveforms of 10 s (40 bins, dither 1)", "",
              "Host clock around `submit_raw` -> `acquire` -> device synchronise, tap off and on (boundary 1) alternating in one process, the second of",
              f"two batches after each switch, {a.rounds} rounds.", "",
              "| tap | median | minimum | maximum |", "|---|---|---|---|"]
        for tag in ("off", "on"):
            L.append(f"| {tag} | {med(t[tag]):.3f} ms | {min(t[tag]):.3f} ms | {max(t[tag]):.3f} ms |")
        with tempfile.TemporaryDirectory() as tmp:
            res, same, n, ark_bytes = tool_times(a.utts, tmp)
        L += ["", f"## The tool end to end: a synthetic wav.scp of {n} utterances of 3 to 8 s (16 kHz, 40 bins, dither 0)", "",
              "Wall clock of each process, second of two runs (files in the page cache); start-up of the runtime included.", "",
              "| | wall clock |", "|---|---|"]
        for k, v in res.items():
            L.append(f"| {k} | {v:.2f} s |")
        L += ["", f"The feature archive is {ark_bytes / 1e6:.0f} MB.  The two outputs of this tool are " + ("byte-identical." if same else "NOT identical.")]
        L += ["", "## Headline untouched: `python bench.py --gpus 1 --steps 20 --warmup 5`, parent commit and this one alternating", ""]
        if a.bench_parent:
            h = headline(a.bench_parent)
            L += ["| tree | ms per step of the repeats | median | spread (max - min) |", "|---|---|---|---|"]
            for tag, v in h.items():
                L.append(f"| {tag} | {', '.join(f'{x:.3f}' for x in v)} | {med(v):.3f} | {max(v) - min(v):.3f} |")
            diff = abs(med(h["this commit"]) - med(h["parent"]))
            spread = max(h["parent"]) - min(h["parent"])
            L += ["", f"The medians differ by {diff:.3f} ms; the parent's own repeats spread over {spread:.3f} ms: the difference lies " +
                  ("inside" if diff <= spread else "OUTSIDE") + " that spread."]
        else:
            L += ["not measured (no --bench-parent)"]
    else:
        L += ["not measured"]
    with open(a.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
