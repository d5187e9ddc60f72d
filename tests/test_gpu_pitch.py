"""-m gpu: Kaldi pitch features on the device (eesen_pitch_*, csrc/pitch.hip) against tests/golden/pitch.npz and tests/pitch_restatement.py.

* stages (eesen_pitch_nccf), per case: the down-sampled signal (distance relative to the waveform's peak) and both up-sampled NCCF
  matrices (absolute distance) against the float64 restatement, each within 3 x the float32-mode restatement's own distance from the
  float64 mode on that case -- the project's margin for an equally valid float32 order; silence is exact zeros;
* search: forward costs of the last frame, back pointers, track and output equal the float32 restatement of the search run on the
  device's own NCCF matrices, bit for bit, on every case; the re-estimate flag equals the reference tool's;
* end to end against the reference tool's output: the chosen lag is the tool's on every frame but at most 2 % of a case's frames
  (rounded up; the reference itself leaves out none, this is the room NCCF round-off gets), and on the rest the NCCF column is within
  3 x the case's reference floor (the float64 restatement's own distance from the tool); shapes are equal and a too-short waveform
  gives no matrix;
* post-processing against the tool per column within 3 x the reference floor; process = 1 inside compute equals process on compute's
  raw output exactly; the noise reproduces per seed and has the mean and deviation asked for; a launch of 33 equals 33 launches of 1;
* both native tools and both Python mirrors against api.Pitch.

The edge cases of tests/golden/pitch_edges.npz go through the same checks with the same bounds, at the sizes where the kernels take
another path (tests/pitch_cases.py lists why each is there):
* stages, search and end to end on lag grids of 63, 64, 65, 448, 449, 1023 and 1024 states -- one wavefront, a full last wavefront,
  one state in the last wavefront, the sixteen-wavefront maximum -- and on down-sampling ratios 16:3, 441:40 and 16:5; 1025 states
  are refused with EESEN_ERR_INVALID;
* post-processing against the tool on 255, 256, 257, 512, 513 and 598 rows and on 598, 1 and 300 rows in one call: the prefix-sum
  scan's chunks of 256 frames and the carry between them, and an utterance whose sums start behind a long one's;
* the 6 s waveform with a one-frame, a no-frame and a 300-frame slice behind it in one launch: the same bits as each alone, raw and
  processed, and process = 1 inside compute equals process on compute's raw output.

Measured figures of one run are in profiles/pitch.md.
"""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import pitch_cases as pc
from tests import pitch_restatement as pr

pytestmark = pytest.mark.gpu
GOLD, PROC, SWEEP = pc.load_golden()
EDGE, EDGE_PROC = pc.load_golden_edges()
ALL = {**GOLD, **EDGE}
COMPUTE_NAMES = pc.CASE_NAMES + pc.EDGE_NAMES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def restated(name, mode):
    c = ALL[name]
    return tuple(pr.compute(w.astype(mode), c["opts"], mode) for w in c["waves"])


@functools.lru_cache(maxsize=None)
def device_stages(name):
    from eesen_amd.api import Pitch
    c = ALL[name]
    pt = Pitch(**c["opts"])
    return tuple(pt.stages(w) for w in c["waves"])


def lag_index(mat, lags):
    """The lag state of every row of an (NCCF, pitch) matrix."""
    return np.argmin(np.abs(1.0 / lags.astype(np.float64)[None, :] - np.asarray(mat, np.float64)[:, 1:2]), axis=1)


@functools.lru_cache(maxsize=None)
def nccf_floor(name):
    """The float64 restatement's distance from the reference tool in the NCCF column (the lags agree on every frame: CPU test)."""
    c = ALL[name]
    return max([float(np.abs(ref[:, 0].astype(np.float64) - r["out"][:, 0]).max()) for ref, r in zip(c["refs"], restated(name, np.float64))
                if ref is not None] + [0.0])


@pytest.mark.parametrize("name", COMPUTE_NAMES)
def test_stages_against_restatement(gpu, name):
    c = ALL[name]
    r64, r32, dev = restated(name, np.float64), restated(name, np.float32), device_stages(name)
    worst = dict(down=0.0, nccf_pitch=0.0, nccf_pov=0.0)
    own = dict(worst)
    for w, a, b, d in zip(c["waves"], r64, r32, dev):
        assert d["frames"] == a["frames"] and d["down"].shape == a["down"].shape
        peak = max(float(np.abs(w.astype(np.float64)).max()), 1.0)
        worst["down"] = max(worst["down"], float(np.abs(d["down"] - a["down"]).max(initial=0.0)) / peak)
        own["down"] = max(own["down"], float(np.abs(b["down"].astype(np.float64) - a["down"]).max(initial=0.0)) / peak)
        if not a["frames"]:
            continue
        for k in ("nccf_pitch", "nccf_pov"):
            assert d[k].shape == a[k].shape and np.all(np.isfinite(d[k]))
            worst[k] = max(worst[k], float(np.abs(d[k] - a[k]).max()))
            own[k] = max(own[k], float(np.abs(b[k].astype(np.float64) - a[k]).max()))
        if c["kind"] == "zero":
            assert not d["down"].any() and not d["nccf_pitch"].any() and not d["nccf_pov"].any()
    print(f"pitch stages {name}: " + ", ".join(f"{k} device {worst[k]:.3e} float32 restatement {own[k]:.3e}" for k in worst))
    for k in worst:
        assert worst[k] <= 3.0 * own[k], (name, k, worst[k], own[k])


@pytest.mark.parametrize("name", COMPUTE_NAMES)
def test_search_bit_for_bit(gpu, name):
    c = ALL[name]
    taken_any = False
    for d in device_stages(name):
        if not d["frames"]:
            continue
        taken, scale = pr.reestimate(d["avg_norm_prod"], d["mean_square"][0], d["mean_square"][1], d["first_pass_frames"], d["frames"], c["opts"])
        assert taken == d["taken"]
        taken_any |= taken
        fwd, bp, track, out = pr.search(d["nccf_pitch"], d["nccf_pov"], scale if taken else None, c["opts"])
        assert np.array_equal(fwd.view(np.uint32), d["fwd"].view(np.uint32))
        assert np.array_equal(bp, d["backptr"])
        assert np.array_equal(track, d["track"])
        assert np.array_equal(out.view(np.uint32), d["raw"].view(np.uint32))
    assert taken_any == c["taken"], (name, taken_any, c["taken"])


@pytest.mark.parametrize("name", COMPUTE_NAMES)
def test_end_to_end_against_the_tool(gpu, name):
    from eesen_amd.api import Pitch
    c = ALL[name]
    pt = Pitch(**c["opts"])
    got = pt.compute(c["waves"])                       # one launch for the whole case
    lags = pr.lags(c["opts"])
    assert np.array_equal(lags, pt.lags())
    frames = left_out = 0
    worst = 0.0
    for w, g, ref in zip(c["waves"], got, c["refs"]):
        if ref is None:
            assert g.shape == (0, 0) and pt.shape(len(w))[0] == 0
            continue
        assert g.dtype == np.float32 and g.shape == ref.shape == (pt.shape(len(w))[0], 2)
        gi, ri = lag_index(g, lags), lag_index(ref, lags)
        assert np.array_equal(g[:, 1], (1.0 / lags.astype(np.float64)[gi]).astype(np.float32))
        same = gi == ri
        frames += len(gi)
        left_out += int((~same).sum())
        worst = max(worst, float(np.abs(g[same, 0].astype(np.float64) - ref[same, 0]).max(initial=0.0)))
    floor = nccf_floor(name)
    print(f"pitch end to end {name}: frames {frames}, left out {left_out}, NCCF device {worst:.3e}, reference floor {floor:.3e}")
    assert left_out <= max(1, math.ceil(0.02 * frames)), (name, left_out, frames)
    assert worst <= 3.0 * floor, (name, worst, floor)
    if c["kind"] == "zero":
        for g in got:
            assert not g[:, 0].any() and np.all(g[:, 1] == np.float32(pr.full(c["opts"])["max_f0"]))


@pytest.mark.parametrize("pname", [p["name"] for p in pc.PROCESS_CASES])
def test_process_against_the_tool(gpu, pname):
    from eesen_amd.api import Pitch
    popts = next(p["opts"] for p in pc.PROCESS_CASES if p["name"] == pname)
    pt = Pitch(**popts)
    for src in pc.PROCESS_INPUTS:
        raws = [m for m in GOLD[src]["refs"] if m is not None]
        refs = [m for m in PROC[pname][src] if m is not None]
        check_process(pt, pname, popts, src, raws, refs)


def check_process(pt, pname, popts, src, raws, refs):
    """One call of eesen_pitch_process on `raws` against the tool's `refs`: per column within 3 x the reference floor."""
    dim = pr.process_dim(popts)
    got = pt.process(raws)
    worst, floor = np.zeros(dim), np.zeros(dim)
    for raw, ref, g in zip(raws, refs, got):
        assert g.shape == ref.shape == (raw.shape[0] + popts.get("delay", 0), dim)
        worst = np.maximum(worst, np.abs(g.astype(np.float64) - ref).max(axis=0))
        floor = np.maximum(floor, np.abs(pr.process(raw, popts) - ref).max(axis=0))
    print(f"pitch process {pname} on {src}: device {worst}, reference floor {floor}")
    assert np.all(worst <= 3.0 * floor), (pname, src, worst, floor)


@pytest.mark.parametrize("pname,src", pc.EDGE_PROCESS_PAIRS)
def test_process_against_the_tool_at_length(gpu, pname, src):
    """The same rule past the 256-frame chunk of the prefix-sum scan: 255 .. 598 rows, and 598, 1 and 300 rows in one call."""
    from eesen_amd.api import Pitch
    popts = next(p["opts"] for p in pc.PROCESS_CASES if p["name"] == pname)
    raws, refs = EDGE_PROC[(pname, src)]
    check_process(Pitch(**popts), pname, popts, src, raws, refs)


def test_lag_grid_bound(gpu):
    """1024 lag states (a workgroup of 16 wavefronts) are accepted and run; one more is refused."""
    from eesen_amd.api import Pitch, EesenError, pitch_lags, pitch_opts
    c = EDGE[f"grid_{pc.MAX_STATES}"]
    pt = Pitch(**c["opts"])
    assert len(pt.lags()) == pc.MAX_STATES and pt.compute(c["waves"][2:])[0].shape == c["refs"][2].shape
    over = dict(delta_pitch=pc.delta_pitch_for(pc.MAX_STATES + 1))
    assert len(pr.lags(over)) == pc.MAX_STATES + 1
    for refused in (lambda: Pitch(**over), lambda: pitch_lags(pitch_opts(**over))):
        with pytest.raises(EesenError, match="more than 1024 lag states") as e:
            refused()
        assert e.value.code == -1                       # EESEN_ERR_INVALID


def test_long_and_short_in_one_launch(gpu):
    """At lengths past the scan's chunk, with noise 0: compute(process=True) on the four together equals each alone bit for bit, so a
    short utterance's prefix sums start clean behind a long one's; and process = 1 inside compute equals process on compute's raw
    output bit for bit."""
    from eesen_amd.api import Pitch
    o, waves = pc.long_and_short()
    for more in (dict(), dict(add_raw_log_pitch=True, delay=2), dict(normalization_left_context=10, normalization_right_context=3)):
        pt = Pitch(delta_pitch_noise_stddev=0.0, **o, **more)
        raw = pt.compute(waves)
        both = pt.compute(waves, process=True)
        assert [m.shape[0] for m in raw] == [598, 1, 0, 300]
        for i, w in enumerate(waves):
            for process, together in ((False, raw), (True, both)):
                alone = pt.compute([w], process=process)[0]
                assert alone.shape == together[i].shape and np.array_equal(alone.view(np.uint32), together[i].view(np.uint32)), (more, i, process)
        keep = [i for i, m in enumerate(raw) if m.shape[0]]
        after = pt.process([raw[i] for i in keep], utt_ids=keep)
        for i, m in zip(keep, after):
            assert m.shape == (raw[i].shape[0] + more.get("delay", 0), pt.shape(0)[2])
            assert np.array_equal(both[i].view(np.uint32), m.view(np.uint32)), (more, i)
        assert both[2].shape == (0, 0)


def test_process_inside_compute(gpu):
    from eesen_amd.api import Pitch
    c = GOLD["s33_ragged"]
    for o in (dict(delta_pitch_noise_stddev=0.0), dict(add_raw_log_pitch=True, delay=2, noise_seed=5)):
        pt = Pitch(**c["opts"], **o)
        raw = pt.compute(c["waves"])
        both = pt.compute(c["waves"], process=True)
        keep = [i for i, m in enumerate(raw) if m.shape[0]]
        after = pt.process([raw[i] for i in keep], utt_ids=keep)
        for i, m in zip(keep, after):
            assert m.shape == (raw[i].shape[0] + o.get("delay", 0), pt.shape(0)[2])
            assert np.array_equal(both[i].view(np.uint32), m.view(np.uint32))
        assert all(both[i].shape == (0, 0) for i in range(len(raw)) if i not in keep)


def test_noise(gpu):
    from eesen_amd.api import Pitch
    n, std, scale = 2400, 0.05, 10.0
    rng = np.random.default_rng(3)
    raw = np.stack([rng.uniform(0.0, 1.0, n), 100.0 * np.exp(np.cumsum(rng.normal(0.0, 0.01, n)))], 1).astype(np.float32)
    only = dict(add_pov_feature=False, add_normalized_log_pitch=False, delta_pitch_scale=scale)
    clean = Pitch(delta_pitch_noise_stddev=0.0, **only).process([raw])[0]
    a = Pitch(delta_pitch_noise_stddev=std, noise_seed=1, **only)
    x = a.process([raw], utt_ids=[9])[0]
    assert x.shape == clean.shape == (n, 1)
    assert np.array_equal(x, a.process([raw], utt_ids=[9])[0])                                   # a seed reproduces
    assert not np.array_equal(x, Pitch(delta_pitch_noise_stddev=std, noise_seed=2, **only).process([raw], utt_ids=[9])[0])
    assert not np.array_equal(x, a.process([raw], utt_ids=[10])[0])                              # the utterance id is part of the key
    term = (x.astype(np.float64) - clean)[:, 0]
    sd = std * scale
    print(f"pitch noise: mean {term.mean():.4e} (allowed {5 * sd / math.sqrt(n):.4e}), deviation {term.std():.5f} (wanted {sd}, allowed +-{5 * sd / math.sqrt(2 * n):.5f})")
    assert abs(term.mean()) <= 5.0 * sd / math.sqrt(n)
    assert abs(term.std() - sd) <= 5.0 * sd / math.sqrt(2 * n)


def test_batching_gives_identical_bits(gpu):
    from eesen_amd.api import Pitch
    c = GOLD["s33_ragged"]
    assert len(c["waves"]) == 33
    pt = Pitch(delta_pitch_noise_stddev=0.0, **c["opts"])
    for process in (False, True):
        together = pt.compute(c["waves"], process=process)
        for i, w in enumerate(c["waves"]):
            alone = pt.compute([w], process=process)[0]
            assert alone.shape == together[i].shape and np.array_equal(alone.view(np.uint32), together[i].view(np.uint32)), i


# ------------------------------------------------------------------------------------------------ the tools
TOOL_CASE = "voiced_8k_s3"


@pytest.fixture(scope="module")
def wav_scp(gpu, tmp_path_factory):
    from eesen_amd.api import Pitch
    c = GOLD[TOOL_CASE]
    tmp = tmp_path_factory.mktemp("pitch_tools")
    sf = pr.full(c["opts"])["samp_freq"]
    scp = tmp / "wav.scp"
    with open(scp, "w") as f:
        for i, w in enumerate(c["waves"]):
            pc.write_wav(str(tmp / f"u{i}.wav"), w, sf)
            f.write(f"utt{i} {tmp}/u{i}.wav\n")
    pc.write_wav(str(tmp / "stereo.wav"), np.repeat(c["waves"][1], 2), sf, channels=2)
    with open(tmp / "stereo.scp", "w") as f:
        f.write(f"st {tmp}/stereo.wav\n")
    pc.write_wav(str(tmp / "short.wav"), c["waves"][0][:100], sf)
    with open(tmp / "short.scp", "w") as f:
        f.write(f"sh {tmp}/short.wav\n")
    popts = dict(delta_pitch_noise_stddev=0.0, add_raw_log_pitch=True)
    pt = Pitch(**c["opts"], **popts)
    raw = pt.compute(c["waves"])
    return tmp, raw, pt.process(raw)


def _tool(kind, name):
    if kind == "native":
        return [os.path.join(ROOT, "eesen_amd", "bin", name)]
    return [sys.executable, "-m", "eesen_amd." + name.replace("-", "_")]


def _run(cmd, **kw):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, **kw)


@pytest.mark.parametrize("kind", ["native", "python"])
def test_tools(wav_scp, kind):
    from eesen_amd import kaldi_io
    tmp, raw, processed = wav_scp
    compute, process = _tool(kind, "compute-kaldi-pitch-feats"), _tool(kind, "process-kaldi-pitch-feats")
    rate = ["--sample-frequency=8000"]
    for tag, wspec in (("bin", "ark:{d}/{k}_raw.ark"), ("txt", "ark,t:{d}/{k}_raw.txt"), ("scp", "ark,scp:{d}/{k}_raw2.ark,{d}/{k}_raw.scp")):
        r = _run(compute + rate + [f"scp:{tmp}/wav.scp", wspec.format(d=tmp, k=kind)])
        assert r.returncode == 0, r.stderr
    for rspec in (f"ark:{tmp}/{kind}_raw.ark", f"ark:{tmp}/{kind}_raw.txt", f"scp:{tmp}/{kind}_raw.scp"):
        got = dict(kaldi_io.read_mat_table(rspec))
        assert sorted(got) == ["utt0", "utt1", "utt2"]
        for i in range(3):
            if rspec.endswith(".txt"):
                np.testing.assert_allclose(got[f"utt{i}"], raw[i], rtol=1e-6)
            else:
                assert np.array_equal(got[f"utt{i}"], raw[i])
    r = _run(process + ["--delta-pitch-noise-stddev=0", "--add-raw-log-pitch=true", f"ark:{tmp}/{kind}_raw.ark", f"ark,scp:{tmp}/{kind}_proc.ark,{tmp}/{kind}_proc.scp"])
    assert r.returncode == 0, r.stderr
    got = dict(kaldi_io.read_mat_table(f"scp:{tmp}/{kind}_proc.scp"))
    for i in range(3):
        assert np.array_equal(got[f"utt{i}"], processed[i])
    # a two-channel file: the reference's warning, channel 0
    r = _run(compute + rate + [f"scp:{tmp}/stereo.scp", f"ark:{tmp}/{kind}_st.ark"])
    assert r.returncode == 0 and "Channel not specified but you have data with 2 channels; defaulting to zero" in r.stderr, r.stderr
    assert np.array_equal(dict(kaldi_io.read_mat_table(f"ark:{tmp}/{kind}_st.ark"))["st"], raw[1])
    # nothing succeeded: exit status 1; a rate mismatch and a refused option are errors
    r = _run(compute + rate + [f"scp:{tmp}/short.scp", f"ark:{tmp}/{kind}_sh.ark"])
    assert r.returncode == 1, r.stderr
    r = _run(compute + [f"scp:{tmp}/wav.scp", f"ark:{tmp}/{kind}_bad.ark"])
    assert r.returncode not in (0, 1) and "Sample frequency mismatch" in r.stderr, r.stderr
    r = _run(compute + rate + ["--frames-per-chunk=10", f"scp:{tmp}/wav.scp", f"ark:{tmp}/{kind}_bad.ark"])
    assert r.returncode not in (0, 1) and "frames-per-chunk" in r.stderr, r.stderr
    assert _run(compute).returncode == 1 and _run(process).returncode == 1
