"""The filterbank extractor's fixture, restatement and host-side pieces, without a GPU (the device side: tests/test_gpu_fbank.py).

* tests/golden/fbank.npz is what tests/fbank_cases.py describes, and the float64 restatement (tests/fbank_restatement.py) reproduces
  every matrix the reference's own tool wrote: same shape, and a distance that is float32 FFT round-off (the case's reference floor,
  listed in profiles/fbank.md) -- below 1e-4 on white noise, a few 1e-3 at most under a tone or a chirp, exact silence at log(FLT_MIN);
* eesen_fbank_mel_banks against the restatement's filters, eesen_fbank_shape against NumFrames in both edge modes;
* the wave reader and the wav.scp table reader; the pipeline parser with a compute-fbank-feats head.
"""
import io
import os
import struct
import wave as wavmod

import numpy as np
import pytest

from tests import fbank_cases as fc
from tests import fbank_restatement as fr

GOLD = fc.load_golden()
# what the fixture's floors may be, by kind of signal: the reference's float32 FFT leaves round-off relative to the frame's PEAK bin
FLOOR_CEILING = {"noise": 1e-4, "tone": 1e-2, "chirp": 1e-2, "zero": 1e-5}


def test_fixture_is_the_case_list():
    assert list(GOLD) == fc.CASE_NAMES
    for c in fc.CASES:
        g = GOLD[c["name"]]
        assert g["opts"] == c["opts"] and g["kind"] == c["kind"] and len(g["waves"]) == len(c["waves"])
        for a, b, t, r in zip(g["waves"], c["waves"], fc.frames_of(c), g["refs"]):
            assert a.dtype == np.int16 and np.array_equal(a, b) and len(a) <= 0.4 * fr.full(c["opts"])["samp_freq"] + 1
            assert (r is None) == (t == 0)
    assert os.path.getsize(fc.GOLDEN) < 512 * 1024


def test_case_list_covers_what_the_kernel_can_get_wrong():
    geo = {fr.geometry(c["opts"])[2] for c in fc.CASES}
    assert geo == {256, 512, 1024, 2048}
    opts = [fr.full(c["opts"]) for c in fc.CASES]
    assert {o["num_bins"] for o in opts} >= {23, 40, 80}
    assert {o["window_type"] for o in opts} == {"hamming", "hanning", "povey", "rectangular"}
    assert any(o["preemph_coeff"] == 0.0 for o in opts) and any(not o["remove_dc_offset"] for o in opts)
    assert any(o["high_freq"] == -200.0 for o in opts) and any(o["low_freq"] == 0.0 for o in opts)
    assert any(not o["use_log_fbank"] for o in opts) and any(not o["snip_edges"] for o in opts)
    assert any(o["use_energy"] and o["raw_energy"] and o["energy_floor"] > 0 for o in opts)
    assert any(o["use_energy"] and not o["raw_energy"] and o["htk_compat"] for o in opts)
    assert {o["vtln_warp"] for o in opts} >= {0.9, 1.0, 1.1}
    assert all(o["dither"] == 0.0 for o in opts)
    assert {len(c["waves"]) for c in fc.CASES} >= {1, 3, 33}
    frames = [fc.frames_of(c) for c in fc.CASES]
    assert any(0 in f for f in frames) and any(1 in f for f in frames)
    totals = {sum(f) % fc.FRAMES_PER_BLOCK for f in frames}
    assert {1, fc.FRAMES_PER_BLOCK - 1} <= totals
    short = [c for c in fc.CASES if not fr.full(c["opts"])["snip_edges"]]
    assert any(len(w) < fr.geometry(c["opts"])[1] for c in short for w in c["waves"])


@pytest.mark.parametrize("name", fc.CASE_NAMES)
def test_restatement_against_the_reference_tool(name):
    c = GOLD[name]
    worst = 0.0
    for w, r in zip(c["waves"], c["refs"]):
        m = fr.compute(w, c["opts"])
        assert m.shape[0] == fr.num_frames(len(w), c["opts"])
        if r is None:
            assert m.shape[0] == 0
            continue
        assert m.shape == r.shape and r.dtype == np.float32
        worst = max(worst, fr.distance(r, m, c["opts"]))
    print(f"fbank case {name}: reference floor {worst:.3e}")
    assert worst <= FLOOR_CEILING[c["kind"]], (name, worst)
    if c["kind"] == "zero":
        assert all(np.all(r == np.log(np.float32(np.finfo(np.float32).tiny))) for r in c["refs"])
        assert abs(float(c["refs"][0][0, 0]) + 87.3366) < 1e-4


def _opts(**kw):
    from eesen_amd.api import fbank_opts
    return fbank_opts(**kw)


@pytest.mark.parametrize("warp", [1.0, 0.9, 1.1])
@pytest.mark.parametrize("cfg", [dict(num_bins=23), dict(num_bins=40), dict(num_bins=80, samp_freq=32000.0), dict(num_bins=40, samp_freq=8000.0),
                                 dict(num_bins=40, low_freq=0.0, high_freq=-200.0), dict(num_bins=40, samp_freq=44100.0)])
def test_mel_banks_against_the_restatement(cfg, warp):
    """first_index and size equal the float64 filters' support, except where the float64 weight at a foot is below the tolerance (the
    strict inequality at a foot is decided by the last bits of a float32 mel value there); weights within the tolerance.  float32 mel
    values up to ~2840 carry ~2e-4 absolute error, over a bin width of (mel_high - mel_low) / (bins + 1) mel: 68 mel or more at 40 bins
    gives 2e-5, with and without VTLN.  Narrower bins (80 bins: 44 mel at 32 kHz) divide the same error by a smaller width, and there
    a warped foot counts: it went through expf, the warp and logf again, three roundings of that size where an unwarped foot has one, so
    a weight's numerator and denominator carry 1 + 3 + 3 such errors instead of 1 + 1 + 1."""
    from eesen_amd.api import mel_banks
    o = dict(cfg, vtln_warp=warp)
    first, size, weights = mel_banks(_opts(**o))
    filt = fr.mel_filters(o)
    nb, half = filt.shape
    assert len(first) == len(size) == len(weights) == nb
    full = fr.full(o)
    nyq = 0.5 * full["samp_freq"]
    width = float(fr.mel(full["high_freq"] if full["high_freq"] > 0 else nyq + full["high_freq"]) - fr.mel(full["low_freq"])) / (nb + 1)
    tol = 2e-5 if width >= 68.0 else 2e-5 * (68.0 / width) * (7.0 / 3.0 if warp != 1.0 else 1.0)
    for b in range(nb):
        dense = np.zeros(half)
        assert 0 <= first[b] and first[b] + size[b] <= half and len(weights[b]) == size[b]
        dense[first[b]:first[b] + size[b]] = weights[b]
        assert np.max(np.abs(dense - filt[b])) <= tol, (b, np.max(np.abs(dense - filt[b])), tol)
        support = np.nonzero(filt[b] >= tol)[0]
        assert first[b] <= support[0] and first[b] + size[b] - 1 >= support[-1]
        wide = np.nonzero(filt[b] > 0)[0]
        assert first[b] >= wide[0] - 1 and first[b] + size[b] - 1 <= wide[-1] + 1


def test_mel_banks_option_checks():
    from eesen_amd.api import mel_banks, EesenError
    for bad, msg in ((dict(num_bins=2), "at least 3 mel bins"), (dict(num_bins=400), "num-mel-bins too large"), (dict(low_freq=-1.0), "Bad values"),
                     (dict(high_freq=9000.0), "Bad values"), (dict(low_freq=5000.0, high_freq=4000.0), "Bad values"),
                     (dict(vtln_warp=1.1, vtln_low=10.0), "vtln-low"), (dict(vtln_warp=0.9, vtln_high=8000.0), "vtln-low"),
                     (dict(round_to_power_of_two=False), "round-to-power-of-two"), (dict(htk_mode=True), "htk_mode"),
                     (dict(frame_length_ms=5.0), "256, 512, 1024 or 2048"), (dict(samp_freq=96000.0), "256, 512, 1024 or 2048")):
        with pytest.raises(EesenError, match=msg):
            mel_banks(_opts(**bad))
    o = _opts()
    assert (o.samp_freq, o.frame_shift_ms, o.frame_length_ms, o.dither, o.num_bins, o.low_freq, o.high_freq, o.vtln_low, o.vtln_high) == \
        (16000.0, 10.0, 25.0, 1.0, 23, 20.0, 0.0, 100.0, -500.0)
    assert abs(o.preemph_coeff - 0.97) < 1e-7 and (o.window_type, o.remove_dc_offset, o.round_to_power_of_two, o.snip_edges) == (2, 1, 1, 1)
    assert (o.use_energy, o.energy_floor, o.raw_energy, o.htk_compat, o.use_log_fbank, o.vtln_warp, o.dither_seed, o.htk_mode) == (0, 0.0, 1, 0, 1, 1.0, 0, 0)


@pytest.mark.parametrize("snip", [True, False])
@pytest.mark.parametrize("cfg", [dict(), dict(samp_freq=8000.0, use_energy=True), dict(samp_freq=44100.0, num_bins=40), dict(frame_shift_ms=12.5, num_bins=40)])
def test_shape_against_num_frames(cfg, snip):
    from eesen_amd.api import Fbank
    o = dict(cfg, snip_edges=snip, dither=0.0)
    fb = Fbank(**o)                     # options, shapes and filters need no device
    shift, length, _ = fr.geometry(o)
    dim = fr.full(o)["num_bins"] + int(fr.full(o)["use_energy"])
    for n in (0, 1, shift // 2 - 1, shift // 2, shift // 2 + 1, length - 1, length, length + shift - 1, length + shift, 10 * shift + 3, 160000):
        assert fb.shape(n) == (fr.num_frames(n, o), dim), n
    if snip:
        assert [fb.shape(n)[0] for n in (0, length - 1, length, length + shift - 1, length + shift)] == [0, 0, 1, 1, 2]


# ---------------------------------------------------------------------------------------------- wave input
def _write(path, data, rate=16000, channels=1, width=2):
    with wavmod.open(str(path), "wb") as w:
        w.setnchannels(channels); w.setsampwidth(width); w.setframerate(rate)
        w.writeframes(np.asarray(data).tobytes())


def test_wave_reader(tmp_path):
    from eesen_amd import kaldi_io
    rng = np.random.default_rng(3)
    mono = rng.integers(-32768, 32767, 1000).astype("<i2")
    stereo = rng.integers(-32768, 32767, (700, 2)).astype("<i2")
    _write(tmp_path / "mono.wav", mono)
    _write(tmp_path / "stereo.wav", stereo, rate=8000, channels=2)
    _write(tmp_path / "eight.wav", rng.integers(0, 255, 500).astype(np.uint8), width=1)
    with open(tmp_path / "wav.scp", "w") as f:
        f.write(f"a {tmp_path}/mono.wav\nb cat {tmp_path}/stereo.wav |\n")
    table = list(kaldi_io.read_wav_table(f"scp:{tmp_path}/wav.scp"))
    assert [k for k, _ in table] == ["a", "b"]
    (ra, da), (rb, db) = table[0][1], table[1][1]
    assert ra == 16000.0 and da.dtype == np.float32 and da.shape == (1, 1000) and np.array_equal(da[0], mono.astype(np.float32))
    assert rb == 8000.0 and db.shape == (2, 700) and np.array_equal(db.T, stereo.astype(np.float32))
    warned = []
    assert np.array_equal(kaldi_io.select_channel("b", db, 0, warned.append), stereo[:, 0]) and not warned
    assert np.array_equal(kaldi_io.select_channel("b", db, 1, warned.append), stereo[:, 1]) and not warned
    assert np.array_equal(kaldi_io.select_channel("b", db, -1, warned.append), stereo[:, 0]) and "defaulting to zero" in warned[0]
    assert kaldi_io.select_channel("a", da, 1, warned.append) is None and "producing no output" in warned[1]
    assert np.array_equal(kaldi_io.select_channel("a", da, -1, warned.append), mono) and len(warned) == 2
    raw = open(tmp_path / "mono.wav", "rb").read()
    with pytest.raises(kaldi_io.KaldiIOError, match="unexpected end of file"):
        kaldi_io.read_wave(io.BytesIO(raw[:30]))                       # a truncated header
    with pytest.raises(kaldi_io.KaldiIOError, match="16-bit"):
        kaldi_io.read_wave(open(tmp_path / "eight.wav", "rb"))
    with pytest.raises(kaldi_io.KaldiIOError, match="RIFF"):
        kaldi_io.read_wave(io.BytesIO(b"RIFX" + raw[4:]))
    # a data chunk cut short gives the samples that are there; a size of 0 or 0xFFFFFFFF (a pipe) reads to the end; extra chunks are skipped
    assert np.array_equal(kaldi_io.read_wave(io.BytesIO(raw[:-100]))[1][0], mono[:-50])
    at = raw.index(b"data")
    for size in (0, 0xFFFFFFFF):
        piped = raw[:at + 4] + struct.pack("<I", size) + raw[at + 8:]
        assert np.array_equal(kaldi_io.read_wave(io.BytesIO(piped))[1][0], mono)
    listed = raw[:at] + b"LIST" + struct.pack("<I", 6) + b"abcdef" + raw[at:]
    assert np.array_equal(kaldi_io.read_wave(io.BytesIO(listed))[1][0], mono)


# ---------------------------------------------------------------------------------------------- the pipeline parser
def test_pipeline_parser_with_a_filterbank_head():
    from eesen_amd import frontend as fe
    p = fe.parse_feature_pipeline("ark,s,cs:compute-fbank-feats --dither=0 --num-mel-bins=40 --use-energy=true --channel=1 --min-duration=0.1 "
                                  "--window-type=hamming --snip-edges=false scp:data/wav.scp ark:- | apply-cmvn --norm-vars=true --utt2spk=ark:u2s "
                                  "scp:cmvn.scp ark:- ark:- | splice-feats --left-context=1 --right-context=1 ark:- ark:- | "
                                  "subsample-feats --n=3 ark:- ark:- | add-deltas ark:- ark:- |")
    assert p is not None and p.source == "scp:data/wav.scp" and (p.channel, p.min_duration) == (1, 0.1)
    assert p.fbank == dict(dither=0.0, num_bins=40, use_energy=True, window_type="hamming", snip_edges=False)
    assert p.stages == [(fe.FBANK, 0, 0), (fe.CMVN, 1, 0), (fe.SPLICE, 1, 1), (fe.SUBSAMPLE, 3, 0), (fe.DELTAS, 2, 2)]
    assert (p.cmvn, p.utt2spk, p.norm_vars) == ("scp:cmvn.scp", "ark:u2s", True)
    assert p.out_dim(1) == 41 * 3 * 3 and p.cmvn_dim(1) == 41
    for n in (0, 100, 399, 400, 16000, 16079, 16080):
        t = fr.num_frames(n, p.fbank)
        assert fe.fbank_num_frames(n, p.fbank) == t and p.out_frames(n) == (t + 2) // 3
    p = fe.parse_feature_pipeline("ark:compute-fbank-feats scp:wav.scp ark:- |")
    assert p is not None and p.stages == [(fe.FBANK, 0, 0)] and p.fbank == {} and p.out_dim(1) == 23 and p.out_frames(16000) == 98
    # what the device extractor does not implement, or what is not this tool's command line, stays a pipe for the shell
    for bad in ("ark:compute-fbank-feats --vtln-map=ark:warps scp:wav.scp ark:- |", "ark:compute-fbank-feats --subtract-mean=true scp:wav.scp ark:- |",
                "ark:compute-fbank-feats --output-format=htk scp:wav.scp ark:- |", "ark:compute-fbank-feats --round-to-power-of-two=false scp:wav.scp ark:- |",
                "ark:compute-fbank-feats --window-type=blackman scp:wav.scp ark:- |", "ark:compute-fbank-feats --num-mel-bins=x scp:wav.scp ark:- |",
                "ark:compute-fbank-feats --config=conf/fbank.conf scp:wav.scp ark:- |", "ark:compute-fbank-feats scp:wav.scp ark:feats.ark |",
                "ark:compute-fbank-feats scp:wav.scp ark:- | compute-fbank-feats scp:wav.scp ark:- |",
                "ark:compute-fbank-feats scp:wav.scp ark:- | apply-cmvn scp:cmvn.scp scp:other.scp ark:- |",
                "ark:add-deltas ark:- ark:- | compute-fbank-feats scp:wav.scp ark:- |"):
        assert fe.parse_feature_pipeline(bad) is None, bad
    # a pipeline without the head is what it was
    q = fe.parse_feature_pipeline("ark,s,cs:apply-cmvn --norm-vars=true scp:cmvn.scp scp:train.scp ark:- | add-deltas ark:- ark:- |")
    assert q.fbank is None and q.stages == [(fe.CMVN, 1, 0), (fe.DELTAS, 2, 2)] and q.out_dim(40) == 120 and q.out_frames(77) == 77
