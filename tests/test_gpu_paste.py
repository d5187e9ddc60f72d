"""-m gpu: filterbank + pitch from audio in one pipeline (EESEN_FEAT_FBANK_PITCH, feat_paste_kernel, eesen_paste_feats) against
tests/golden/paste.npz, the two stand-alone extractors and numpy.

* bit equality: the feeder with the combined head alone, read back through acquire, equals numpy.hstack of api.Fbank.compute and
  api.Pitch.compute(process=True) on the same waveforms and ids, trimmed by the row rule, on every case; a dropped utterance has no
  rows, pad columns are zero, and a slot reused by a smaller batch shows nothing of the larger one; the same on a 6 s waveform with a
  one-frame, a no-frame and a 300-frame slice behind it (the fixture's waveforms are at most 0.6 s);
* against the reference's pasted matrices: rows and kept set exact.  Filterbank columns by the rule of tests/test_gpu_fbank.py: the
  distance from the float64 restatement is at most 3 x the case's reference floor (the reference tool's own distance from it).  Pitch
  columns by the rule of tests/test_gpu_pitch.py: the device picks the lag of the float64 restatement -- which picks the reference
  tool's on every frame, a condition write_golden checked -- on all but at most 2 % of a case's frames (rounded up), and its processed
  columns are within 3 x the reference floor (the float64 restatement of the post-processing against the tool's columns).  A frame whose
  lag differs spoils its neighbours in the moving-window columns, so an utterance with such a frame is compared in the POV column
  alone, on its other frames;
* behind the head, CMVN with variance normalisation and deltas (129 columns) equal the existing stage kernels run on the pasted
  matrix submitted as plain features, bit for bit;
* eesen_paste_feats / api.paste_feats on 2, 3 and 4 tables of widths 1, 3, 40 and 43, S = 1 and 33, against numpy;
* the refusals return their error codes: the stage without set_pitch, mismatched rates, the stage not first, a batch over the frame
  bound (refused before a byte of it is read);
* the tools: bin/paste-feats and its Python mirror on the fused path against the same tool's host join of this project's extractor
  tools' tables, byte for byte; ctc-decode from a `paste-feats ... | apply-cmvn ... |` rspecifier against the pasted table on disk.
"""
import ctypes as C
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fbank_restatement as fr
from tests import paste_cases as pc
from tests import pitch_restatement as pr

pytestmark = pytest.mark.gpu
GOLD = pc.load_golden()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FBANK_PITCH, CMVN, DELTAS, SPLICE = 6, 1, 4, 2


def as_columns(waves):
    return [np.asarray(w, np.float32).reshape(-1, 1) for w in waves]


@functools.lru_cache(maxsize=None)
def parts(name):
    """The two stand-alone extractors on the case (ids 0 .. S-1): ([filterbank matrices], [processed pitch matrices])."""
    from eesen_amd.api import Fbank, Pitch
    c = GOLD[name]
    return tuple(Fbank(**c["fbank"]).compute(c["waves"])), tuple(Pitch(**c["pitch"]).compute(c["waves"], process=True))


def pasted(fb, pt, tolerance):
    """numpy.hstack of the two parts trimmed by the rule; [0 x D] for a dropped utterance."""
    from eesen_amd.frontend import paste_frames
    D = next(m.shape[1] for m in fb if m.shape[0]) + next(m.shape[1] for m in pt if m.shape[0])
    out = []
    for a, b in zip(fb, pt):
        r = paste_frames([a.shape[0], b.shape[0]], tolerance)
        out.append(np.hstack([a[:r], b[:r]]) if r else np.zeros((0, D), np.float32))
    return out


def assembled(mats, ld):
    """The feeder's [T*S x ld] matrix of these utterances: row t*S + s, zeros past an utterance's end and in the pad columns."""
    T, S = max(m.shape[0] for m in mats), len(mats)
    out = np.zeros((T, S, ld), np.float32)
    for s, m in enumerate(mats):
        out[:m.shape[0], s, :m.shape[1]] = m
    return out.reshape(T * S, ld)


def read_slot(f, slot):
    """The whole assembled matrix of a slot, pad columns included."""
    from eesen_amd.api import CuMatrix
    got = f.acquire(slot)
    host = CuMatrix.view(got.ptr, got.rows, got.stride, got.stride, got.device, keepalive=f).numpy()
    f.release(slot)
    return host, got.cols


def head_feeder(c, slots=2, **more):
    from eesen_amd.api import Feeder
    f = Feeder(slots=slots)
    f.set_fbank(**dict(c["fbank"], **more.get("fbank", {})))
    f.set_pitch(**dict(c["pitch"], **more.get("pitch", {})))
    f.set_pipeline([(FBANK_PITCH, c["tolerance"], 0)] + more.get("stages", []))
    return f


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_feeder_equals_the_two_extractors(gpu, name):
    c = GOLD[name]
    fb, pt = parts(name)
    want = pasted(fb, pt, c["tolerance"])
    f = head_feeder(c)
    D = want[0].shape[1]
    for w, m, ref in zip(c["waves"], want, c["refs"]):
        assert f.pipeline_shape(1, len(w)) == (m.shape[0], D)
        assert (ref is None) == (m.shape[0] == 0), "the kept set is the reference's"
    host, cols = read_slot(f, f.submit_raw(as_columns(c["waves"])))
    assert cols == D and host.shape[1] == (D + 3) // 4 * 4
    exp = assembled(want, host.shape[1])
    assert host.shape == exp.shape
    assert np.array_equal(host.view(np.uint32), exp.view(np.uint32))


def test_feeder_equals_the_two_extractors_at_utterance_length(gpu):
    """The same equality at real lengths: the 6 s waveform of the pitch tests (598 frames, past the 256-frame chunks of the pitch
    post-processing's scan) with a one-pitch-frame slice, a slice without a frame and a 300-frame slice behind it, at 8 kHz.  Device
    against device, bit for bit, zero rows of the two dropped utterances and pad columns included."""
    from eesen_amd.api import Fbank, Pitch
    from tests import pitch_cases
    popts, waves = pitch_cases.long_and_short()
    c = dict(GOLD["s33_8k"], waves=waves)
    assert pr.full(c["pitch"])["samp_freq"] == pr.full(popts)["samp_freq"] == 8000.0
    assert [r[2] for r in pc.rows_of(c)] == [598, 0, 0, 299]
    fb, pt = Fbank(**c["fbank"]).compute(waves), Pitch(**c["pitch"]).compute(waves, process=True)
    assert [m.shape[0] for m in pt] == [598, 1, 0, 300]
    want = pasted(fb, pt, c["tolerance"])
    assert [m.shape[0] for m in want] == [598, 0, 0, 299]
    f = head_feeder(c)
    D = want[0].shape[1]
    for w, m in zip(waves, want):
        assert f.pipeline_shape(1, len(w)) == (m.shape[0], D)
    host, cols = read_slot(f, f.submit_raw(as_columns(waves)))
    assert cols == D and host.shape[1] == (D + 3) // 4 * 4
    exp = assembled(want, host.shape[1])
    assert host.shape == exp.shape
    assert np.array_equal(host.view(np.uint32), exp.view(np.uint32))


def test_slot_reuse_and_noise_ids(gpu):
    """One slot: a smaller batch after a larger one shows nothing of it.  With dither and delta-pitch noise on, a waveform's key is the
    feeder's counter for both extractors: the second batch has the keys S .. S + 1."""
    from eesen_amd.api import Fbank, Pitch
    c = GOLD["tol2_16k"]
    noisy = dict(fbank=dict(dither=1.0, dither_seed=3), pitch=dict(delta_pitch_noise_stddev=0.005, noise_seed=4))
    f = head_feeder(c, slots=1, **noisy)
    fbx, ptx = Fbank(**dict(c["fbank"], **noisy["fbank"])), Pitch(**dict(c["pitch"], **noisy["pitch"]))
    S = len(c["waves"])
    for waves, ids in ((c["waves"], list(range(S))), ([c["waves"][3], c["waves"][2]], [S, S + 1])):
        want = pasted(fbx.compute(waves, utt_ids=ids), ptx.compute(waves, process=True, utt_ids=ids), c["tolerance"])
        host, _ = read_slot(f, f.submit_raw(as_columns(waves)))
        exp = assembled(want, host.shape[1])
        assert host.shape == exp.shape and np.array_equal(host.view(np.uint32), exp.view(np.uint32))
    clean = pasted(*parts("tol2_16k"), c["tolerance"])
    assert not np.array_equal(want[1], clean[2]), "the noise is on"


@functools.lru_cache(maxsize=None)
def restated(name):
    """Per kept waveform index: (float64 filterbank restatement, float64 raw pitch restatement, its post-processing)."""
    c = GOLD[name]
    out = {}
    for i, (w, ref) in enumerate(zip(c["waves"], c["refs"])):
        if ref is not None:
            raw = pr.compute(w.astype(np.float64), c["pitch"])["out"]
            out[i] = (fr.compute(w, c["fbank"]), raw, pr.process(raw, c["pitch"]))
    return out


def lag_index(mat, lags):
    return np.argmin(np.abs(1.0 / lags.astype(np.float64)[None, :] - np.asarray(mat, np.float64)[:, 1:2]), axis=1)


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_against_the_reference_pasted_matrices(gpu, name):
    from eesen_amd.api import Pitch
    c = GOLD[name]
    f = head_feeder(c)
    host, D = read_slot(f, f.submit_raw(as_columns(c["waves"])))
    S = len(c["waves"])
    host = host.reshape(-1, S, host.shape[1])[:, :, :D]
    dev_raw = Pitch(**c["pitch"]).compute(c["waves"])
    lags = pr.lags(c["pitch"])
    nfb = fr.full(c["fbank"])["num_bins"] + int(bool(fr.full(c["fbank"])["use_energy"]))
    npt = pr.process_dim(c["pitch"])
    assert D == nfb + npt
    fb_worst = fb_floor = 0.0
    frames = left_out = 0
    pt_worst, pt_floor = np.zeros(npt), np.zeros(npt)
    for s, ref in enumerate(c["refs"]):
        rows = f.pipeline_shape(1, len(c["waves"][s]))[0]
        if ref is None:
            assert rows == 0 and not host[:, s].any()
            continue
        assert ref.shape == (rows, D) and not host[rows:, s].any()
        got = host[:rows, s]
        fb64, raw64, proc64 = restated(name)[s]
        fb_worst = max(fb_worst, fr.distance(got[:, :nfb], fb64[:rows], c["fbank"]))
        fb_floor = max(fb_floor, fr.distance(ref[:, :nfb], fb64[:rows], c["fbank"]))
        same = lag_index(dev_raw[s], lags) == lag_index(raw64, lags)
        frames += len(same)
        left_out += int((~same).sum())
        pt_floor = np.maximum(pt_floor, np.abs(proc64[:rows] - ref[:, nfb:]).max(axis=0))
        err = np.abs(got[:, nfb:].astype(np.float64) - proc64[:rows])
        if same.all():
            pt_worst = np.maximum(pt_worst, err.max(axis=0))
        elif pr.full_process(c["pitch"])["add_pov_feature"]:
            delay = pr.full_process(c["pitch"])["delay"]
            keep = np.concatenate([np.ones(delay, bool), same])[:rows]      # row t + delay holds frame t
            pt_worst[0] = max(pt_worst[0], err[keep, 0].max(initial=0.0))
    print(f"paste {name}: filterbank device {fb_worst:.3e} reference floor {fb_floor:.3e}; pitch frames {frames} left out {left_out}, "
          f"columns device {pt_worst} reference floor {pt_floor}")
    assert fb_worst <= 3.0 * fb_floor, (name, fb_worst, fb_floor)
    assert left_out <= max(1, math.ceil(0.02 * frames)), (name, left_out, frames)
    assert np.all(pt_worst <= 3.0 * pt_floor), (name, pt_worst, pt_floor)


def test_stages_behind_the_head(gpu):
    """FBANK_PITCH -> CMVN(norm_vars) -> DELTAS(2, 2) against CMVN -> DELTAS on the pasted matrices submitted as plain features."""
    from eesen_amd.api import Feeder
    c = GOLD["tol0"]                                    # two utterances kept, two dropped
    want = pasted(*parts("tol0"), c["tolerance"])
    D = want[0].shape[1]
    rng = np.random.default_rng(5)
    norm = [np.stack([rng.normal(0.0, 3.0, D), rng.uniform(0.2, 2.0, D)]).astype(np.float32) for _ in want]
    tail = [(CMVN, 1, 0), (DELTAS, 2, 2)]
    f = head_feeder(c, stages=tail)
    assert f.pipeline_shape(1, len(c["waves"][0])) == (want[0].shape[0], 129)
    a, cols = read_slot(f, f.submit_raw(as_columns(c["waves"]), norm))
    g = Feeder()
    g.set_pipeline(tail)
    b, cols_b = read_slot(g, g.submit_raw(want, norm))
    assert cols == cols_b == 129 and a.shape == b.shape and a.shape[1] == 132
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert a[:, :129].any() and not a[:, 129:].any()


@pytest.mark.parametrize("S", [1, 33])
@pytest.mark.parametrize("widths", [(1, 3), (40, 3), (3, 43, 1), (43, 1, 40, 3)])
def test_paste_feats_against_numpy(gpu, S, widths):
    from eesen_amd.api import paste_feats
    rng = np.random.default_rng(100 * S + len(widths))
    tol = 2
    base = rng.integers(1, 40, S)
    frames = np.stack([base + rng.integers(0, tol + 1, S) for _ in widths])          # within the tolerance ...
    dropped = [0] if S == 1 else [0, S // 2, S - 1]
    if S > 1:
        frames[-1, 0] = 0                          # ... but for: an empty matrix first,
        frames[0, S // 2] = frames[1:, S // 2].max() + tol + 1      # too long a one in the middle,
        frames[1, S - 1] = 0                       # and an empty one last
    else:
        frames[0, 0] = frames[1:, 0].max() + tol + 1
    tabs = [[rng.normal(0.0, 1.0, (int(frames[j, s]), w)).astype(np.float32) for s in range(S)] for j, w in enumerate(widths)]
    got = paste_feats(tabs, tol)
    assert len(got) == S
    for s in range(S):
        if s in dropped:
            assert got[s] is None
            continue
        r = int(frames[:, s].min())
        want = np.hstack([t[s][:r] for t in tabs])
        assert got[s].shape == want.shape and np.array_equal(got[s].view(np.uint32), want.view(np.uint32)), s


def test_refusals(gpu):
    from eesen_amd.api import Feeder, EesenError
    c = GOLD["tol2_16k"]
    f = Feeder()
    f.set_fbank(**c["fbank"])
    with pytest.raises(EesenError, match="eesen_feeder_set_pitch") as e:
        f.set_pipeline([(FBANK_PITCH, 2, 0)])
    assert e.value.code == -3
    f.set_pitch(**dict(c["pitch"], samp_freq=8000.0))
    with pytest.raises(EesenError, match="sample-frequency") as e:
        f.set_pipeline([(FBANK_PITCH, 2, 0)])
    assert e.value.code == -1
    f.set_pitch(**c["pitch"])
    with pytest.raises(EesenError, match="first stage") as e:
        f.set_pipeline([(SPLICE, 1, 1), (FBANK_PITCH, 2, 0)])
    assert e.value.code == -1
    with pytest.raises(EesenError, match="tolerance"):
        f.set_pipeline([(FBANK_PITCH, -1, 0)])
    with pytest.raises(EesenError):
        f.set_pitch(frames_per_chunk=10)            # the plan's own refusals
    f.set_pipeline([(FBANK_PITCH, 2, 0)])
    with pytest.raises(EesenError, match="samples x 1"):
        f.submit_raw([np.zeros((1000, 2), np.float32)])
    # a batch over the pitch tracker's frame bound (2^28 frames: 24 waveforms of 2^31 - 1 samples claimed) is refused on its counts
    # alone, before a sample is read: every pointer names the same 16 floats
    S = 24
    small = np.zeros(16, np.float32)
    ptrs = (C.c_void_p * S)(*[small.ctypes.data] * S)
    frames = np.full(S, 2 ** 31 - 1, np.int32)
    slot = C.c_int(-1)
    rc = f.lib.eesen_feeder_submit_raw(f.h, ptrs, frames.ctypes.data_as(C.POINTER(C.c_int)), None, None, S, 1, C.byref(slot))
    msg = f.lib.eesen_last_error().decode(errors="replace")
    assert rc == -1 and "too many frames" in msg, (rc, msg)
    host, _ = read_slot(f, f.submit_raw(as_columns(c["waves"])))         # and the feeder works on
    assert np.array_equal(host, assembled(pasted(*parts("tol2_16k"), 2), host.shape[1]))


# ------------------------------------------------------------------------------------------------ the tools
ENV = dict(os.environ, PATH="/usr/bin:/bin", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))   # no featbin tool on PATH
TOOL_CASE = "snip_mixed"          # two kept, two over the tolerance, one without a pitch frame


def _tool(kind, name):
    if kind == "native":
        return [os.path.join(ROOT, "bin", name)]
    return [sys.executable, "-m", "eesen_amd." + name.replace("-", "_")]


def _run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300, env=ENV)


def _inner_pipes(c, scp):
    cflags, pflags = pc.pitch_flags(c)
    return (f"ark:compute-fbank-feats {' '.join(pc.fbank_flags(c))} scp,p:{scp} ark:- |",
            f"ark,s,cs:compute-kaldi-pitch-feats {' '.join(cflags)} scp,p:{scp} ark:- | process-kaldi-pitch-feats {' '.join(pflags)} ark:- ark:- |")


@pytest.mark.parametrize("kind", ["native", "python"])
def test_paste_feats_fused_against_its_host_path(gpu, tmp_path, kind):
    """paste-feats handed the two pipes (run by nobody: PATH holds no featbin tool) against the same tool's host join of the tables
    this project's extractor tools write, byte for byte; and against the feeder."""
    from eesen_amd import kaldi_io
    c = GOLD[TOOL_CASE]
    scp = pc.write_waves(c, str(tmp_path))
    tol = f"--length-tolerance={c['tolerance']}"
    cflags, pflags = pc.pitch_flags(c)
    for cmd in (_tool(kind, "compute-fbank-feats") + pc.fbank_flags(c) + [f"scp:{scp}", f"ark:{tmp_path}/fbank.ark"],
                _tool(kind, "compute-kaldi-pitch-feats") + cflags + [f"scp:{scp}", f"ark:{tmp_path}/raw.ark"],
                _tool(kind, "process-kaldi-pitch-feats") + pflags + [f"ark:{tmp_path}/raw.ark", f"ark:{tmp_path}/pitch.ark"]):
        r = _run(cmd)
        assert r.returncode == 0, r.stderr[-2000:]
    r = _run(_tool(kind, "paste-feats") + [tol, f"ark:{tmp_path}/fbank.ark", f"ark,s,cs:{tmp_path}/pitch.ark", f"ark:{tmp_path}/host.ark"])
    assert r.returncode == 0 and f"Done {c['done']} utts, errors on {c['err']}" in r.stderr, r.stderr[-2000:]
    r = _run(_tool(kind, "paste-feats") + [tol] + list(_inner_pipes(c, scp)) + [f"ark:{tmp_path}/fused.ark"])
    assert r.returncode == 0 and f"Done {c['done']} utts, errors on {c['err']}" in r.stderr, r.stderr[-2000:]
    assert sum("exceeds tolerance" in w for w in pc.warnings_of(r.stderr)) == c["err"]
    fused = open(tmp_path / "fused.ark", "rb").read()
    assert len(fused) > 0 and fused == open(tmp_path / "host.ark", "rb").read()
    want = pasted(*parts(TOOL_CASE), c["tolerance"])
    got = dict(kaldi_io.read_mat_table(f"ark:{tmp_path}/fused.ark"))
    assert sorted(got) == [f"utt{i:03d}" for i, m in enumerate(want) if m.shape[0]]
    for i, m in enumerate(want):
        if m.shape[0]:
            assert np.array_equal(np.asarray(got[f"utt{i:03d}"], np.float32).view(np.uint32), m.view(np.uint32))


def test_ctc_decode_from_audio_through_both_extractors(gpu, tmp_path):
    """ctc-decode (native and Python) handed `paste-feats ... | apply-cmvn ... |` against itself handed apply-cmvn over the pasted
    table on disk: the same hypotheses, byte for byte, in one process and with no featbin tool on PATH."""
    import struct
    from eesen_amd import kaldi_io, nnet_io, synth
    c = GOLD["tol2_16k"]
    scp = pc.write_waves(c, str(tmp_path))
    feats = pasted(*parts("tol2_16k"), c["tolerance"])
    keys = [f"utt{i:03d}" for i in range(len(feats))]
    kaldi_io.write_mat_ark(str(tmp_path / "pasted.ark"), list(zip(keys, feats)))
    D = feats[0].shape[1]
    st = np.zeros((2, D + 1))
    for m in feats:
        st[0, :D] += m.astype(np.float64).sum(0); st[1, :D] += (m.astype(np.float64) ** 2).sum(0); st[0, D] += m.shape[0]
    with open(tmp_path / "cmvn.mat", "wb") as f:
        f.write(b"\x00BDM \x04" + struct.pack("<i", 2) + b"\x04" + struct.pack("<i", st.shape[1]) + st.astype("<f8").tobytes())
    K = 7
    cfg = synth.config("tiny_bi"); cfg.update(D=D, K=K)
    net = str(tmp_path / "net.nnet")
    nnet_io.write_nnet(net, synth.make_model(**cfg), binary=True)
    fbp, ptp = _inner_pipes(c, scp)
    pipe = f'ark,s,cs:paste-feats --length-tolerance={c["tolerance"]} "{fbp}" "{ptp}" ark:- | apply-cmvn --norm-vars=true {tmp_path}/cmvn.mat ark:- ark:- |'
    pre = f"ark:apply-cmvn --norm-vars=true {tmp_path}/cmvn.mat ark:{tmp_path}/pasted.ark ark:- |"
    got = {}
    for kind in ("native", "python"):
        for src, spec in (("pipe", pipe), ("pre", pre)):
            out = str(tmp_path / f"hyp_{kind}_{src}.ark")
            r = _run(_tool(kind, "ctc-decode") + ["--beam=4", net, spec, "ark:" + out])
            assert r.returncode == 0, r.stderr[-2000:]
            got[(kind, src)] = open(out, "rb").read()
    assert len(got[("native", "pipe")]) > 0
    assert got[("native", "pipe")] == got[("native", "pre")] == got[("python", "pipe")] == got[("python", "pre")]
