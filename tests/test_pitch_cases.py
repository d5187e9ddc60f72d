"""CPU: the pitch fixture (tests/golden/pitch.npz), the numpy restatement (tests/pitch_restatement.py) and the host side of
eesen_pitch_* (options, shapes, lag grid) -- no device needed.

The fixture is the case list; the case list covers what the kernels can get wrong; the float64 restatement picks the reference tool's
lag on EVERY frame of every case, takes the energy re-estimate exactly where the tool's log says it did, and counts the tool's frames
on the whole sweep.  Its remaining distance from the tool, in the NCCF column and in every processed column, is the case's REFERENCE
FLOOR, printed here and listed in profiles/pitch.md; tests/test_gpu_pitch.py allows the device three of them.
"""
import functools

import numpy as np
import pytest

from tests import pitch_cases as pc
from tests import pitch_restatement as pr

GOLD, PROC, SWEEP = pc.load_golden()


def test_fixture_is_the_case_list():
    assert list(GOLD) == pc.CASE_NAMES
    for c in pc.CASES:
        g = GOLD[c["name"]]
        assert g["opts"] == c["opts"] and g["kind"] == c["kind"] and len(g["waves"]) == len(c["waves"])
        for a, b, ref, t in zip(g["waves"], c["waves"], g["refs"], pc.frames_of(c)):
            assert a.dtype == np.int16 and np.array_equal(a, b)
            assert (ref is None) == (t == 0)
            if ref is not None:
                assert ref.shape == (t, 2) and ref.dtype == np.float32
    assert sorted(PROC) == sorted(p["name"] for p in pc.PROCESS_CASES)
    import os
    assert os.path.getsize(pc.GOLDEN) < 512 * 1024


def test_case_list_covers_what_the_kernels_can_get_wrong():
    by = {c["name"]: c for c in pc.CASES}
    frames = {n: pc.frames_of(c) for n, c in by.items()}
    rates = {pr.full(c["opts"])["samp_freq"] for c in pc.CASES}
    assert {8000.0, 11025.0, 16000.0} <= rates
    assert len(pr.downsample_tables(by["rate_11025"]["opts"])[2]) == 160                      # many filter phases
    assert {c["kind"] for c in pc.CASES} >= {"voiced", "noise", "zero", "tail", "mixed"}
    assert all(len(w) <= 0.6 * pr.full(c["opts"])["samp_freq"] for c in pc.CASES for w in c["waves"] if c["name"] != "long_6s")
    for n in ("voiced_16k_s3", "voiced_8k_s3"):
        assert len(by[n]["waves"]) == 3 and len(set(frames[n])) == 3
        assert sum(frames[n]) % pc.NCCF_FRAMES_PER_BLOCK == 1                                   # one above a multiple
    s33 = frames["s33_ragged"]
    assert len(s33) == 33 and 0 in s33 and 1 in s33 and len(set(s33)) > 8
    assert sum(s33) % pc.NCCF_FRAMES_PER_BLOCK == pc.NCCF_FRAMES_PER_BLOCK - 1                  # one below
    assert by["snip_false"]["opts"]["snip_edges"] is False
    grid, dflt = pr.lags(by["grid"]["opts"]), pr.lags({})
    assert len(dflt) == 417 and len(grid) != 417 and len(grid) % 64 != 0 and len(dflt) % 64 != 0   # a partly filled wavefront
    assert by["grid"]["opts"] == dict(min_f0=60.0, max_f0=500.0, delta_pitch=0.01, upsample_filter_width=3, lowpass_filter_width=2,
                                      penalty_factor=0.3, soft_min_f0=20.0, nccf_ballast=1000.0)
    for n, want in pc.TAIL_TAKEN.items():
        assert GOLD[n]["taken"] == want and len(by[n]["waves"][0]) == int(n.split("_")[1]) + int(n.split("_")[2])
        assert np.abs(by[n]["waves"][0]).max() < 32767                                          # under clipping
    assert frames["long_6s"] == [598] and 598 >= pr.DEFAULTS["recompute_frame"] and not GOLD["long_6s"]["taken"]
    assert all(np.abs(w.astype(np.int32)).max() < 32767 for c in pc.CASES for w in c["waves"])
    pnames = {p["name"]: p["opts"] for p in pc.PROCESS_CASES}
    assert all(p["delta_pitch_noise_stddev"] == 0.0 for p in pnames.values())
    assert pnames["all_delay2"]["delay"] == 2 and pr.process_dim(pnames["all_delay2"]) == 4
    assert pr.process_dim(pnames["raw_only"]) == 1 and pnames["delta_window3"]["delta_window"] == 3
    ctx = pnames["ctx_10_3"]
    assert (ctx["normalization_left_context"], ctx["normalization_right_context"]) == (10, 3)
    assert any(0 < t < 14 for t in frames["s33_ragged"])                                        # an utterance shorter than that window


@functools.lru_cache(maxsize=None)
def restated(name):
    c = GOLD[name]
    return tuple(pr.compute(w.astype(np.float64), c["opts"]) for w in c["waves"])


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_restatement_picks_the_tools_lag_on_every_frame(name):
    c = GOLD[name]
    lags = pr.lags(c["opts"]).astype(np.float64)
    floor, taken = 0.0, False
    for r, ref in zip(restated(name), c["refs"]):
        if ref is None:
            assert r["frames"] == 0
            continue
        assert r["frames"] == ref.shape[0]
        ref_idx = np.argmin(np.abs(1.0 / lags[None, :] - ref[:, 1:2].astype(np.float64)), axis=1)
        assert np.array_equal(ref[:, 1], (1.0 / lags[ref_idx]).astype(np.float32))              # the tool's pitch IS a grid value
        assert np.array_equal(ref_idx, r["track"]), np.nonzero(ref_idx != r["track"])[0]
        floor = max(floor, float(np.abs(ref[:, 0].astype(np.float64) - r["out"][:, 0]).max()))
        taken |= r["taken"]
    print(f"pitch reference floor {name}: NCCF {floor:.3e}")
    assert taken == c["taken"]
    if c["kind"] == "zero":
        for ref in c["refs"]:
            assert not ref[:, 0].any() and np.all(ref[:, 1] == np.float32(400.0))
    assert floor <= 1e-5          # float32 dot products of a hundred terms: a sanity check on the restatement, not a bound on the device


@pytest.mark.parametrize("pname", [p["name"] for p in pc.PROCESS_CASES])
def test_process_restatement_against_the_tool(pname):
    popts = next(p["opts"] for p in pc.PROCESS_CASES if p["name"] == pname)
    for src in pc.PROCESS_INPUTS:
        floor = np.zeros(pr.process_dim(popts))
        for raw, ref in zip(GOLD[src]["refs"], PROC[pname][src]):
            assert (raw is None) == (ref is None)
            if raw is None:
                continue
            mine = pr.process(raw, popts)
            assert mine.shape == ref.shape
            floor = np.maximum(floor, np.abs(mine - ref).max(axis=0))
        print(f"pitch reference floor, process {pname} on {src}: {floor}")
        assert np.all(floor <= 2e-5)      # float32 logarithms and sums scaled by up to 10: sanity, as above


def test_frame_counts_against_the_sweep():
    from eesen_amd.api import Pitch
    assert sorted({r for r, _ in SWEEP}) == [8000.0, 11025.0, 16000.0]
    for (rate, snip), table in SWEEP.items():
        pt = Pitch(samp_freq=rate, snip_edges=snip)
        for n, frames in table.items():
            assert pt.shape(n) == (frames, 2, 3), (rate, snip, n)
            assert pr.num_frames(n, dict(samp_freq=rate, snip_edges=snip))[1] == frames
    t = SWEEP[(16000.0, True)]
    assert [t[n] for n in (399, 400, 401, 559, 560, 561, 720, 1000)] == [1, 1, 1, 2, 2, 2, 3, 4]
    t = SWEEP[(16000.0, False)]
    assert [t[n] for n in (400, 560, 720, 1000)] == [3, 4, 5, 6]
    for c in pc.CASES:                                   # and the library against the restatement on every case length
        pt = Pitch(**c["opts"])
        assert [pt.shape(len(w))[0] for w in c["waves"]] == pc.frames_of(c)


def test_lags_against_restatement():
    from eesen_amd.api import Pitch, pitch_lags, pitch_opts
    for o in ({}, dict(samp_freq=8000.0), GOLD["grid"]["opts"], dict(min_f0=20.0, max_f0=600.0, delta_pitch=0.004)):
        want = pr.lags(o)
        assert np.array_equal(Pitch(**o).lags(), want) and np.array_equal(pitch_lags(pitch_opts(**o)), want)
    assert len(pr.lags({})) == 417


def test_defaults_are_the_references():
    from eesen_amd.api import pitch_opts
    o = pitch_opts()
    for k, v in {**pr.DEFAULTS, **pr.PROCESS_DEFAULTS}.items():
        assert getattr(o, k) == pytest.approx(float(v)), k
    assert o.noise_seed == 0


def test_refused_options():
    from eesen_amd.api import Pitch, EesenError
    for bad, why in ((dict(preemph_coeff=0.97), "deprecated"), (dict(frames_per_chunk=10), "online"), (dict(simulate_first_pass_online=True), "online"),
                     (dict(nccf_ballast_online=True), "online"), (dict(resample_freq=2000.0), "twice"), (dict(lowpass_cutoff=2000.0), "twice"),
                     (dict(soft_min_f0=60.0), "soft-min-f0"), (dict(delta_pitch=0.001), "lag states"),
                     (dict(add_pov_feature=False, add_normalized_log_pitch=False, add_delta_pitch=False), "At least one"),
                     (dict(samp_freq=16000.5), "whole"), (dict(delta_window=0), "delta-window")):
        with pytest.raises(EesenError, match=why):
            Pitch(**bad)
    Pitch(max_frames_latency=7)          # accepted, no effect offline


def test_python_tools_know_the_references_option_names():
    from eesen_amd.compute_kaldi_pitch_feats import PITCH_OPTIONS
    from eesen_amd.process_kaldi_pitch_feats import PROCESS_OPTIONS
    from eesen_amd import _lib
    assert set(PITCH_OPTIONS) == set(pc.OPTION_FLAGS.values())
    assert set(PROCESS_OPTIONS) == set(pc.PROCESS_FLAGS.values()) | {"noise-seed"}
    fields = {f[0] for f in _lib.PitchOpts._fields_}
    for table, flags, defaults in ((PITCH_OPTIONS, pc.OPTION_FLAGS, pr.DEFAULTS), (PROCESS_OPTIONS, pc.PROCESS_FLAGS, pr.PROCESS_DEFAULTS)):
        for field, flag in flags.items():
            assert table[flag][0] == field and field in fields and table[flag][1] == defaults[field], flag
    assert fields == set(pr.DEFAULTS) | set(pr.PROCESS_DEFAULTS) | {"noise_seed"}
