"""Case list of the pitch tests (tests/test_pitch_cases.py on the CPU, tests/test_gpu_pitch.py on the GPU).

A case is one option set (keys of `eesen_pitch_opts_t`) and the waveforms of one launch.  tests/golden/pitch.npz holds, per case, the
int16 waveforms, what the reference's own compute-kaldi-pitch-feats wrote for every waveform (its (NCCF, pitch) matrix; nothing for
a waveform without a frame), and whether its --verbose=3 log shows the energy re-estimate ("Forward-cost per frame changed from").
PROCESS_CASES are option sets of process-kaldi-pitch-feats (noise 0); the fixture holds that tool's output on the raw matrices of
PROCESS_INPUTS.  SWEEP is a table of sample count -> frame count from the same tool on silent waveforms, per rate and edge mode.

`write_golden(bindir)` is how the file was made.  The two tools are `make -C oracle/ref_build pitchbin`: the reference's base/,
cpucompute/ and util/ sources, feat/{pitch-functions,resample,feature-functions,wave-reader,mel-computations,srfft}.cc and the two
featbin sources, compiled where they lie with that Makefile's flags (g++ -std=c++11 -O2, -DHAVE_CLAPACK -DKALDI_DOUBLEPRECISION=0,
blas_rename.h) and linked against the same SciPy OpenBLAS, into oracle/_ref/pitchbin (the `bindir`; not kept in the repository).

A second fixture, tests/golden/pitch_edges.npz (`write_golden_edges`, `load_golden_edges`; `python -m tests.pitch_cases` remakes it
with the same two tools), holds what the first one's shapes leave out -- the sizes at which the kernels take another path:
* GRID_STATES: lag grids of 63, 64, 65, 448, 449, 1023 and 1024 states (`delta_pitch_for` searches the option).  The search kernel
  runs one thread per state in ceil(states / 64) wavefronts and reads the previous costs four at a time: one wavefront alone, a last
  wavefront that is full (no +inf filler), one with a single state in it, states % 4 of 0, 1 and 3 next to a wavefront edge, and the
  sixteen wavefronts of kPitchMaxStates.  One more state is refused;
* RESAMPLE_OPTS: down-sampling ratios 16:3, 441:40 and 16:5 -- a few filter phases with more than one output sample per unit, where
  the first fixture has 1 (16 and 8 kHz) or 160 (11025 Hz);
* EDGE_LENGTHS: post-processing of the first 255, 256, 257, 512, 513 and 598 rows of the tool's own long_6s output, and of three
  utterances of 598, 1 and 300 rows in one call.  pitch_process_kernel scans the pov-weighted prefix sums 256 frames at a time with a
  carry between the chunks; the first fixture's utterances stay under 59 frames and never reach the carry or a default +-75 window
  with both ends inside the utterance.
The same condition holds: the float64 restatement picks the tool's lag on every frame of every edge case.

A condition on the fixture (tests/test_pitch_cases.py): the float64 restatement picks the tool's lag on EVERY frame of every case.  A
case that does not is a badly chosen input (clipping, exact ties) and is replaced, not tolerated.

Waveforms are at most 0.6 s but for one of 6 s (598 frames, past recompute_frame).  NCCF_FRAMES_PER_BLOCK frames share a workgroup of
the NCCF kernel: the two S = 3 cases total one above a multiple of it, the S = 33 case one below.
"""
import json
import math
import os
import subprocess
import tempfile

import numpy as np

from tests.fbank_cases import write_wav
from tests.pitch_restatement import full, lags, num_frames

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pitch.npz")
GOLDEN_EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pitch_edges.npz")
NCCF_FRAMES_PER_BLOCK = 4


def voiced(rng, n, sf, f0a=100.0, f0b=300.0, amp=6000.0, noise=20.0):
    """A gliding harmonic complex, five harmonics at 1/k, f0 from f0a to f0b, plus a little noise."""
    t = np.arange(n) / sf
    dur = max(n / sf, 1e-9)
    phase = 2.0 * np.pi * (f0a * t + 0.5 * (f0b - f0a) * t * t / dur)
    x = sum(np.sin(k * phase) / k for k in range(1, 6))
    return np.clip(np.rint(amp * x + rng.normal(0.0, noise, n)), -32768, 32767).astype(np.int16)


def white(rng, n, sigma):
    return np.clip(np.rint(rng.normal(0.0, sigma, n)), -32768, 32767).astype(np.int16)


def loud_tail(rng, body, tail):
    """A quiet body, ten loud samples (under int16 clipping), and quiet again up to `tail` samples after the body.  With tail = 10 the
    loud samples end the waveform: the down-sampler's first pass stops short of them, the flushed tail holds them, and the two mean
    squares differ.  With tail = 40 both passes see them and the re-estimate is not taken.  (Forty samples that are ALL loud do take
    the branch in the reference's tool: the flushed tail then still holds a fifth of the loud energy.)"""
    x = rng.normal(0.0, 30.0, body + tail)
    x[body:body + 10] = rng.normal(0.0, 8000.0, 10)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def samples_for(frames, opts, extra=0):
    """A sample count that gives exactly `frames` frames (searched for; the count is not linear in the rate ratio)."""
    n = 1
    while num_frames(n, opts)[1] < frames:
        n += 1
    return n + extra if num_frames(n + extra, opts)[1] == frames else n


def _cases():
    rng = np.random.default_rng(20240703)
    cases = []

    def add(name, kind, opts, waves):
        cases.append(dict(name=name, kind=kind, opts=dict(opts), waves=waves))

    def pad_total(opts, waves, want_mod, make):
        """Appends one waveform so that the launch's frame total is want_mod modulo NCCF_FRAMES_PER_BLOCK."""
        total = sum(num_frames(len(w), opts)[1] for w in waves)
        t = 5
        while (total + t) % NCCF_FRAMES_PER_BLOCK != want_mod:
            t += 1
        waves.append(make(samples_for(t, opts, 3)))

    o = {}
    w = [voiced(rng, 9600, 16000.0), voiced(rng, 5600, 16000.0, 120.0, 260.0)]
    pad_total(o, w, 1, lambda n: voiced(rng, n, 16000.0, 280.0, 110.0))
    add("voiced_16k_s3", "voiced", o, w)
    o = dict(samp_freq=8000.0)
    w = [voiced(rng, 4800, 8000.0), voiced(rng, 2000, 8000.0, 90.0, 200.0)]
    pad_total(o, w, 1, lambda n: voiced(rng, n, 8000.0, 250.0, 100.0))
    add("voiced_8k_s3", "voiced", o, w)
    add("noise", "noise", {}, [white(rng, 8000, 3000.0)])
    qvq = np.concatenate([white(rng, 2400, 15.0), voiced(rng, 4800, 16000.0, 110.0, 220.0), white(rng, 2400, 15.0)])
    add("quiet_voiced_quiet", "voiced", {}, [qvq])
    add("silence", "zero", {}, [np.zeros(4800, np.int16)])
    add("rate_11025", "voiced", dict(samp_freq=11025.0), [voiced(rng, 6000, 11025.0), white(rng, 3000, 2000.0)])
    # S = 33 ragged at 8 kHz: one waveform without a frame, one with exactly one, voiced and noise alternating
    o = dict(samp_freq=8000.0)
    w = []
    for i in range(32):
        n = int(rng.integers(400, 1700))
        w.append(voiced(rng, n, 8000.0, 100.0 + 5 * i, 300.0 - 4 * i) if i % 2 == 0 else white(rng, n, 2500.0))
    w[5] = white(rng, samples_for(1, o) - 4, 2500.0)
    w[11] = voiced(rng, samples_for(1, o), 8000.0, 150.0, 160.0)
    pad_total(o, w, NCCF_FRAMES_PER_BLOCK - 1, lambda n: voiced(rng, n, 8000.0, 130.0, 210.0))
    add("s33_ragged", "mixed", o, w)
    add("snip_false", "voiced", dict(snip_edges=False), [voiced(rng, 4000, 16000.0), white(rng, 1000, 3000.0)])
    o = dict(min_f0=60.0, max_f0=500.0, delta_pitch=0.01, upsample_filter_width=3, lowpass_filter_width=2, penalty_factor=0.3,
             soft_min_f0=20.0, nccf_ballast=1000.0)
    add("grid", "voiced", o, [voiced(rng, 6400, 16000.0, 90.0, 330.0), white(rng, 2400, 1500.0)])
    for body in (1590, 7990):
        for tail in (10, 40):
            add(f"tail_{body}_{tail}", "tail", {}, [loud_tail(rng, body, tail)])
    add("long_6s", "voiced", dict(samp_freq=8000.0), [np.concatenate([voiced(rng, 16000, 8000.0, 100.0, 300.0), white(rng, 8000, 40.0),
                                                                      voiced(rng, 16000, 8000.0, 280.0, 120.0), white(rng, 8000, 1500.0)])])
    return cases


CASES = _cases()
CASE_NAMES = [c["name"] for c in CASES]
TAIL_TAKEN = {"tail_1590_10": True, "tail_7990_10": True, "tail_1590_40": False, "tail_7990_40": False}

PROCESS_CASES = [
    dict(name="defaults", opts={}),
    dict(name="all_delay2", opts=dict(add_raw_log_pitch=True, delay=2)),
    dict(name="ctx_10_3", opts=dict(normalization_left_context=10, normalization_right_context=3)),
    dict(name="delta_window3", opts=dict(delta_window=3)),
    dict(name="raw_only", opts=dict(add_pov_feature=False, add_normalized_log_pitch=False, add_delta_pitch=False, add_raw_log_pitch=True)),
]
for _p in PROCESS_CASES:
    _p["opts"]["delta_pitch_noise_stddev"] = 0.0
PROCESS_INPUTS = ["voiced_16k_s3", "s33_ragged"]      # the raw matrices these option sets run on: long, short and one-frame utterances

SWEEP_LENGTHS = [399, 400, 401, 559, 560, 561, 720, 1000, 200, 275, 276, 300, 641, 1111, 1599, 1600, 1601]
SWEEP_RATES = [8000.0, 11025.0, 16000.0]


# ---------------------------------------------------------------------------------------------- the edge cases (pitch_edges.npz)
GRID_STATES = [63, 64, 65, 448, 449, 1023, 1024]
GRID_NAMES = [f"grid_{ns}" for ns in GRID_STATES]
MAX_STATES = 1024                                       # kPitchMaxStates
RESAMPLE_OPTS = dict(resample_3000=dict(resample_freq=3000.0), rate_44100=dict(samp_freq=44100.0),
                     resample_5000_cut1500=dict(resample_freq=5000.0, lowpass_cutoff=1500.0))
RESAMPLE_OUT_UNITS = dict(resample_3000=3, rate_44100=40, resample_5000_cut1500=5)
EDGE_SECONDS = (0.3, 0.2, 0.15)                         # two voiced glides and one of white noise per case


def delta_pitch_for(states, opts=None):
    """A delta_pitch of six decimals whose lag grid has exactly `states` states (searched for: the grid's values are float32
    roundings, so the count is not a formula of the option).  Starts where the grid's last step would fall half a step short of
    1 / min_f0 and walks in steps of 1e-6."""
    o = dict(opts or {})
    f = full(o)
    d = round(math.expm1(math.log(f["max_f0"] / f["min_f0"]) / (states - 0.5)), 6)
    for _ in range(2000):
        n = len(lags(dict(o, delta_pitch=d)))
        if n == states:
            return d
        d = round(d + (1e-6 if n > states else -1e-6), 6)
    raise ValueError(f"no delta_pitch of six decimals gives {states} states")


def _edge_cases():
    cases = []

    def three(sf):
        # one generator per case, so that a case whose input has to be replaced (a float32 tie between two lag paths, say: see the
        # condition in the docstring) gets another seed and leaves the others as they are
        rng = np.random.default_rng([20240917, len(cases)])
        n = [int(round(s * sf)) for s in EDGE_SECONDS]
        up = voiced(rng, n[0], sf, float(rng.uniform(80.0, 160.0)), float(rng.uniform(220.0, 340.0)))
        down = voiced(rng, n[1], sf, float(rng.uniform(220.0, 340.0)), float(rng.uniform(80.0, 160.0)))
        return [up, down, white(rng, n[2], float(rng.uniform(1000.0, 3000.0)))]

    for ns in GRID_STATES:
        cases.append(dict(name=f"grid_{ns}", kind="mixed", opts=dict(delta_pitch=delta_pitch_for(ns)), waves=three(16000.0)))
    for name, o in RESAMPLE_OPTS.items():
        cases.append(dict(name=name, kind="mixed", opts=dict(o), waves=three(full(o)["samp_freq"])))
    return cases


EDGE_CASES = _edge_cases()
EDGE_NAMES = [c["name"] for c in EDGE_CASES]

EDGE_SOURCE = "long_6s"                                 # whose tool output (598 rows) the post-processing inputs are cut from
EDGE_LENGTHS = [255, 256, 257, 512, 513, 598]
EDGE_THREE = "three_598_1_300"
SCAN_CHUNK = 256                                        # frames per LDS scan of pitch_process_kernel


def edge_process_inputs(raw):
    """{input name: [raw matrices of one call]} cut from the tool's [598 x 2] output on EDGE_SOURCE: its first T rows, and three
    utterances of which the second and third start their prefix sums behind a long one."""
    assert raw.shape == (598, 2)
    ins = {f"rows{T}": [raw[:T]] for T in EDGE_LENGTHS}
    ins[EDGE_THREE] = [raw, raw[100:101], raw[298:]]
    return ins


EDGE_INPUT_NAMES = [f"rows{T}" for T in EDGE_LENGTHS] + [EDGE_THREE]
EDGE_PROCESS_PAIRS = ([(p, i) for p in ("defaults", "all_delay2", "ctx_10_3") for i in EDGE_INPUT_NAMES] +
                      [("delta_window3", "rows598"), ("raw_only", "rows598")])


def long_and_short():
    """(options, waveforms): the 6 s waveform whole (598 frames), then behind it a one-frame slice, a slice without a frame and a
    300-frame slice -- real utterance lengths and the shortest ones in one launch."""
    c = next(c for c in CASES if c["name"] == EDGE_SOURCE)
    w, o = c["waves"][0], c["opts"]
    one, many = samples_for(1, o), samples_for(300, o)
    waves = [w, w[16000:16000 + one], w[9000:9000 + one - 4], w[20000:20000 + many]]
    assert [num_frames(len(x), o)[1] for x in waves] == [598, 1, 0, 300]
    return o, waves


def frames_of(case):
    return [num_frames(len(w), case["opts"])[1] for w in case["waves"]]


def load_golden():
    """({case: dict(opts, kind, waves, refs [matrix or None], taken)}, {process case: {input case: [matrix or None]}},
    {(rate, snip_edges): {samples: frames}})"""
    z = np.load(GOLDEN)
    cases = {}
    for name in json.loads(str(z["names"])):
        n = int(z[name + "/count"])
        cases[name] = dict(opts=json.loads(str(z[name + "/opts"])), kind=str(z[name + "/kind"]), taken=bool(z[name + "/taken"]),
                           waves=[z[f"{name}/wave{i}"] for i in range(n)],
                           refs=[z[f"{name}/ref{i}"] if f"{name}/ref{i}" in z.files else None for i in range(n)])
    proc = {}
    for p in json.loads(str(z["process_names"])):
        proc[p] = {}
        for src in PROCESS_INPUTS:
            n = int(z[src + "/count"])
            proc[p][src] = [z[f"process/{p}/{src}/{i}"] if f"process/{p}/{src}/{i}" in z.files else None for i in range(n)]
    sweep = {}
    for row in z["sweep"]:
        sweep.setdefault((float(row[0]), bool(row[1])), {})[int(row[2])] = int(row[3])
    return cases, proc, sweep


# ---------------------------------------------------------------------------------------------- how the fixture was made
OPTION_FLAGS = dict(samp_freq="sample-frequency", frame_shift_ms="frame-shift", frame_length_ms="frame-length",
                    preemph_coeff="preemphasis-coefficient", min_f0="min-f0", max_f0="max-f0", soft_min_f0="soft-min-f0",
                    penalty_factor="penalty-factor", lowpass_cutoff="lowpass-cutoff", resample_freq="resample-frequency",
                    delta_pitch="delta-pitch", nccf_ballast="nccf-ballast", nccf_ballast_online="nccf-ballast-online",
                    lowpass_filter_width="lowpass-filter-width", upsample_filter_width="upsample-filter-width",
                    frames_per_chunk="frames-per-chunk", simulate_first_pass_online="simulate-first-pass-online",
                    recompute_frame="recompute-frame", max_frames_latency="max-frames-latency", snip_edges="snip-edges")
PROCESS_FLAGS = dict(pitch_scale="pitch-scale", pov_scale="pov-scale", pov_offset="pov-offset", delta_pitch_scale="delta-pitch-scale",
                     delta_pitch_noise_stddev="delta-pitch-noise-stddev", normalization_left_context="normalization-left-context",
                     normalization_right_context="normalization-right-context", delta_window="delta-window", delay="delay",
                     add_pov_feature="add-pov-feature", add_normalized_log_pitch="add-normalized-log-pitch",
                     add_delta_pitch="add-delta-pitch", add_raw_log_pitch="add-raw-log-pitch")


def flags(opts, table=OPTION_FLAGS):
    return ["--%s=%s" % (table[k], ("true" if v else "false") if isinstance(v, bool) else v) for k, v in opts.items() if k in table]


def _run_compute(compute, tmp, tag, opts, waves, verbose=False):
    """compute-kaldi-pitch-feats on `waves` written as wav files under `tmp`: (path of the archive, the tool's log)."""
    scp, ark = os.path.join(tmp, tag + ".scp"), os.path.join(tmp, tag + ".ark")
    with open(scp, "w") as f:
        for i, w in enumerate(waves):
            p = os.path.join(tmp, f"{tag}_{i}.wav")
            write_wav(p, w, full(opts)["samp_freq"])
            f.write(f"utt{i:03d} {p}\n")
    r = subprocess.run([compute] + (["--verbose=3"] if verbose else []) + flags(opts) + ["scp:" + scp, "ark:" + ark], check=True,
                       capture_output=True, text=True)
    return ark, r.stderr


def write_golden(bindir, path=GOLDEN):
    """Runs the reference's compute-kaldi-pitch-feats and process-kaldi-pitch-feats (in `bindir`) on every case."""
    from eesen_amd import kaldi_io
    compute, process = os.path.join(bindir, "compute-kaldi-pitch-feats"), os.path.join(bindir, "process-kaldi-pitch-feats")
    data = {"names": json.dumps(CASE_NAMES), "process_names": json.dumps([p["name"] for p in PROCESS_CASES])}
    with tempfile.TemporaryDirectory() as tmp:
        def run_compute(tag, opts, waves, verbose=False):
            return _run_compute(compute, tmp, tag, opts, waves, verbose)

        for c in CASES:
            name = c["name"]
            data[name + "/opts"] = json.dumps(c["opts"])
            data[name + "/kind"] = c["kind"]
            data[name + "/count"] = len(c["waves"])
            for i, w in enumerate(c["waves"]):
                data[f"{name}/wave{i}"] = w
            ark, log = run_compute(name, c["opts"], c["waves"], verbose=True)
            data[name + "/taken"] = "Forward-cost per frame changed from" in log
            for key, m in kaldi_io.read_mat_table("ark:" + ark):
                if np.asarray(m).size:
                    data[f"{name}/ref{int(key[3:])}"] = np.asarray(m, np.float32)
            if name in PROCESS_INPUTS:
                for p in PROCESS_CASES:
                    out = os.path.join(tmp, f"{name}_{p['name']}.ark")
                    # an empty matrix cannot be post-processed by the tool (NumFramesReady of nothing): filter through a table
                    keep = os.path.join(tmp, f"{name}_{p['name']}_in.ark")
                    kaldi_io.write_mat_ark(keep, [(k, np.asarray(m, np.float32)) for k, m in kaldi_io.read_mat_table("ark:" + ark) if np.asarray(m).size])
                    subprocess.run([process] + flags(p["opts"], PROCESS_FLAGS) + ["ark:" + keep, "ark:" + out], check=True, capture_output=True)
                    for key, m in kaldi_io.read_mat_table("ark:" + out):
                        data[f"process/{p['name']}/{name}/{int(key[3:])}"] = np.asarray(m, np.float32)
        rows = []
        for rate in SWEEP_RATES:
            for snip in (True, False):
                o = dict(samp_freq=rate, snip_edges=snip)
                ark, _ = run_compute(f"sweep_{int(rate)}_{int(snip)}", o, [np.zeros(n, np.int16) for n in SWEEP_LENGTHS])
                got = {int(key[3:]): np.asarray(m).shape[0] if np.asarray(m).size else 0 for key, m in kaldi_io.read_mat_table("ark:" + ark)}
                rows += [(rate, int(snip), n, got.get(i, 0)) for i, n in enumerate(SWEEP_LENGTHS)]
        data["sweep"] = np.array(rows, np.float64)
    np.savez_compressed(path, **data)


def load_golden_edges():
    """({edge case: dict(opts, kind, waves, refs, taken)} as load_golden gives them,
    {(process case, input name): ([raw matrices of the call], [the tool's output on each])})"""
    z = np.load(GOLDEN_EDGES)
    cases = {}
    for name in json.loads(str(z["names"])):
        n = int(z[name + "/count"])
        cases[name] = dict(opts=json.loads(str(z[name + "/opts"])), kind=str(z[name + "/kind"]), taken=bool(z[name + "/taken"]),
                           waves=[z[f"{name}/wave{i}"] for i in range(n)],
                           refs=[z[f"{name}/ref{i}"] if f"{name}/ref{i}" in z.files else None for i in range(n)])
    inputs = edge_process_inputs(np.load(GOLDEN)[EDGE_SOURCE + "/ref0"])
    proc = {(p, src): (inputs[src], [z[f"process/{p}/{src}/{i}"] for i in range(len(inputs[src]))])
            for p, src in (tuple(k) for k in json.loads(str(z["process_pairs"])))}
    return cases, proc


def write_golden_edges(bindir, path=GOLDEN_EDGES):
    """Runs the two reference tools (in `bindir`) on every edge case.  The post-processing inputs come from pitch.npz."""
    from eesen_amd import kaldi_io
    compute, process = os.path.join(bindir, "compute-kaldi-pitch-feats"), os.path.join(bindir, "process-kaldi-pitch-feats")
    data = {"names": json.dumps(EDGE_NAMES), "process_pairs": json.dumps(EDGE_PROCESS_PAIRS)}
    with tempfile.TemporaryDirectory() as tmp:
        for c in EDGE_CASES:
            name = c["name"]
            data[name + "/opts"] = json.dumps(c["opts"])
            data[name + "/kind"] = c["kind"]
            data[name + "/count"] = len(c["waves"])
            for i, w in enumerate(c["waves"]):
                data[f"{name}/wave{i}"] = w
            ark, log = _run_compute(compute, tmp, name, c["opts"], c["waves"], verbose=True)
            data[name + "/taken"] = "Forward-cost per frame changed from" in log
            for key, m in kaldi_io.read_mat_table("ark:" + ark):
                data[f"{name}/ref{int(key[3:])}"] = np.asarray(m, np.float32)
        inputs = edge_process_inputs(np.load(GOLDEN)[EDGE_SOURCE + "/ref0"])
        by_name = {p["name"]: p["opts"] for p in PROCESS_CASES}
        for pname, src in EDGE_PROCESS_PAIRS:
            raw, out = os.path.join(tmp, f"{pname}_{src}_in.ark"), os.path.join(tmp, f"{pname}_{src}.ark")
            kaldi_io.write_mat_ark(raw, [(f"utt{i:03d}", np.asarray(m, np.float32)) for i, m in enumerate(inputs[src])])
            subprocess.run([process] + flags(by_name[pname], PROCESS_FLAGS) + ["ark:" + raw, "ark:" + out], check=True, capture_output=True)
            for key, m in kaldi_io.read_mat_table("ark:" + out):
                data[f"process/{pname}/{src}/{int(key[3:])}"] = np.asarray(m, np.float32)
    np.savez_compressed(path, **data)


if __name__ == "__main__":      # python -m tests.pitch_cases [bindir]: remakes pitch_edges.npz after `make -C oracle/ref_build pitchbin`
    import sys
    write_golden_edges(sys.argv[1] if len(sys.argv) > 1 else
                       os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "pitchbin"))
