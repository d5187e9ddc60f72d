"""CPU: the pitch fixture (tests/golden/pitch.npz), the numpy restatement (tests/pitch_restatement.py) and the host side of
eesen_pitch_* (options, shapes, lag grid) -- no device needed.

The fixture is the case list; the case list covers what the kernels can get wrong; the float64 restatement picks the reference tool's
lag on EVERY frame of every case, takes the energy re-estimate exactly where the tool's log says it did, and counts the tool's frames
on the whole sweep.  Its remaining distance from the tool, in the NCCF column and in every processed column, is the case's REFERENCE
FLOOR, printed here and listed in profiles/pitch.md; tests/test_gpu_pitch.py allows the device three of them.

The edge fixture (tests/golden/pitch_edges.npz) is held to the same conditions, and its own promises are asserted: lag grids of exactly
63 .. 1024 states, down-sampling units of 3, 40 and 5 output samples, post-processing inputs on both sides of 256 and of 512 rows, all
long enough for an unclamped default window.  A post-processing that loses the carry between its 256-row scans is caught on every
input past 256 rows and on none up to it, so those lengths test what they are there for.
"""
import functools

import numpy as np
import pytest

from tests import pitch_cases as pc
from tests import pitch_restatement as pr

GOLD, PROC, SWEEP = pc.load_golden()
EDGE, EDGE_PROC = pc.load_golden_edges()
ALL = {**GOLD, **EDGE}


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


def test_edge_fixture_is_the_edge_case_list():
    import os
    assert list(EDGE) == pc.EDGE_NAMES and not set(EDGE) & set(GOLD)
    for c in pc.EDGE_CASES:
        g = EDGE[c["name"]]
        assert g["opts"] == c["opts"] and g["kind"] == c["kind"] and len(g["waves"]) == len(c["waves"]) == 3
        for a, b, ref, t in zip(g["waves"], c["waves"], g["refs"], pc.frames_of(c)):
            assert a.dtype == np.int16 and np.array_equal(a, b)
            assert ref is not None and ref.shape == (t, 2) and ref.dtype == np.float32
    assert sorted(EDGE_PROC) == sorted(pc.EDGE_PROCESS_PAIRS)
    for (pname, src), (raws, refs) in EDGE_PROC.items():
        popts = next(p["opts"] for p in pc.PROCESS_CASES if p["name"] == pname)
        assert len(raws) == len(refs)
        for raw, ref in zip(raws, refs):
            assert ref.dtype == np.float32 and ref.shape == (raw.shape[0] + popts.get("delay", 0), pr.process_dim(popts))
    assert os.path.getsize(pc.GOLDEN_EDGES) < 512 * 1024


def test_edge_case_list_covers_the_sizes_the_kernels_branch_on():
    by = {c["name"]: c for c in pc.EDGE_CASES}
    # the search: one thread per state, ceil(states / 64) wavefronts of which the last is padded with +inf, float4 reads up to ns4
    states = [len(pr.lags(by[n]["opts"])) for n in pc.GRID_NAMES]
    assert states == pc.GRID_STATES == [63, 64, 65, 448, 449, 1023, 1024]
    assert all(set(by[n]["opts"]) == {"delta_pitch"} for n in pc.GRID_NAMES)                     # the default 50 .. 400 Hz
    assert [-(-s // 64) for s in states] == [1, 1, 2, 7, 8, 16, 16] and pc.MAX_STATES == 1024
    assert {s % 64 for s in states} >= {0, 1, 63} and {s % 4 for s in states} == {0, 1, 3}
    assert len(pr.lags(dict(delta_pitch=pc.delta_pitch_for(pc.MAX_STATES + 1)))) == pc.MAX_STATES + 1    # the refused grid exists
    # the down-sampler: a few phases, more than one output sample per unit
    for n, unit in pc.RESAMPLE_OUT_UNITS.items():
        in_unit, out_unit, first, weights = pr.downsample_tables(by[n]["opts"])
        assert out_unit == unit == len(first) == len(weights)
    assert sorted(pc.RESAMPLE_OUT_UNITS.values()) == [3, 5, 40] and list(pc.RESAMPLE_OPTS) == pc.EDGE_NAMES[len(pc.GRID_NAMES):]
    assert pr.downsample_tables(by["rate_44100"]["opts"])[0] == 441 and pr.downsample_tables(by["resample_3000"]["opts"])[0] == 16
    for c in pc.EDGE_CASES:
        sf = pr.full(c["opts"])["samp_freq"]
        assert [len(w) for w in c["waves"]] == [int(round(s * sf)) for s in pc.EDGE_SECONDS] and max(pc.EDGE_SECONDS) <= 0.3
        assert all(t > 0 for t in pc.frames_of(c))
        assert all(np.abs(w.astype(np.int32)).max() < 32767 for w in c["waves"])                 # under clipping
    # the post-processing: the scan's chunk of 256 frames and its carry
    assert pc.frames_of(next(c for c in pc.CASES if c["name"] == pc.EDGE_SOURCE)) == [598]
    T = pc.EDGE_LENGTHS
    for edge in (pc.SCAN_CHUNK, 2 * pc.SCAN_CHUNK):
        assert edge in T and edge + 1 in T and any(t <= edge for t in T) and any(t > edge for t in T)                            # both sides of 256 and of 512
    assert {255, 256, 257, 512, 513, 598} == set(T)
    dflt = pr.PROCESS_DEFAULTS
    assert all(t >= dflt["normalization_left_context"] + dflt["normalization_right_context"] + 2 == 152 for t in T)   # an unclamped interior
    o, waves = pc.long_and_short()                                                               # and through compute and the feeder
    assert o == dict(samp_freq=8000.0) and [pr.num_frames(len(w), o)[1] for w in waves] == [598, 1, 0, 300]
    assert np.array_equal(waves[0], GOLD[pc.EDGE_SOURCE]["waves"][0])
    three = EDGE_PROC[("defaults", pc.EDGE_THREE)][0]
    assert [m.shape[0] for m in three] == [598, 1, 300]
    pairs = pc.EDGE_PROCESS_PAIRS
    for p in ("defaults", "all_delay2", "ctx_10_3"):
        assert [s for q, s in pairs if q == p] == pc.EDGE_INPUT_NAMES
    assert [s for q, s in pairs if q in ("delta_window3", "raw_only")] == ["rows598", "rows598"] and len(pairs) == 3 * 7 + 2
    for (pname, src), (raws, _) in EDGE_PROC.items():
        want = [598, 1, 300] if src == pc.EDGE_THREE else [int(src[4:])]
        assert [m.shape[0] for m in raws] == want
        assert np.array_equal(raws[0], GOLD[pc.EDGE_SOURCE]["refs"][0][:want[0]])                # the tool's own rows


@functools.lru_cache(maxsize=None)
def restated(name):
    c = ALL[name]
    return tuple(pr.compute(w.astype(np.float64), c["opts"]) for w in c["waves"])


@pytest.mark.parametrize("name", pc.CASE_NAMES + pc.EDGE_NAMES)
def test_restatement_picks_the_tools_lag_on_every_frame(name):
    c = ALL[name]
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


def edge_floor(pname, src, prefix=pr.prefix_sums):
    """Per utterance of the call: the float64 restatement's distance from the tool per column ([utterances x columns])."""
    popts = next(p["opts"] for p in pc.PROCESS_CASES if p["name"] == pname)
    raws, refs = EDGE_PROC[(pname, src)]
    out = []
    for raw, ref in zip(raws, refs):
        mine = pr.process(raw, popts, prefix=prefix)
        assert mine.shape == ref.shape
        out.append(np.abs(mine - ref).max(axis=0))
    return np.array(out)


@pytest.mark.parametrize("pname,src", pc.EDGE_PROCESS_PAIRS)
def test_process_restatement_against_the_tool_at_length(pname, src):
    floor = edge_floor(pname, src).max(axis=0)
    print(f"pitch reference floor, process {pname} on {src}: {floor}")
    assert np.all(floor <= 2e-5)          # the same sanity cap as on the short inputs


@pytest.mark.parametrize("pname,src", [(p, s) for p, s in pc.EDGE_PROCESS_PAIRS if p != "raw_only"])
def test_a_dropped_scan_carry_is_caught_past_256_rows_only(pname, src):
    """The teeth of the lengths: a post-processing whose prefix sums start again from zero every 256 rows (the kernel's scan with its
    carry lost) is the restatement itself up to 256 rows, and on every longer utterance its normalised column is more than the
    3 x reference floor the device gets away from the tool."""
    popts = next(p["opts"] for p in pc.PROCESS_CASES if p["name"] == pname)
    col = int(pr.full_process(popts)["add_pov_feature"])                    # the normalised column follows the POV one
    floor = edge_floor(pname, src)[:, col]
    wrong = edge_floor(pname, src, prefix=pr.prefix_sums_without_carry)[:, col]
    rows = [m.shape[0] for m in EDGE_PROC[(pname, src)][0]]
    print(f"pitch process without the carry, {pname} on {src}: rows {rows}, distance {wrong}, reference floor {floor}")
    for t, w, f in zip(rows, wrong, floor):
        if t <= pc.SCAN_CHUNK:
            assert w <= f
        else:
            assert w > 3.0 * floor.max(), (t, w, floor)           # the pair's floor, as the device test takes it
    assert any(t > pc.SCAN_CHUNK for t in rows) or src in ("rows255", "rows256")


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


def test_edge_lag_grids_on_the_host():
    """The library's lag grid equals the restatement's at every edge size; 1024 states are accepted and one more is refused."""
    from eesen_amd.api import Pitch, EesenError, pitch_lags, pitch_opts
    for c in pc.EDGE_CASES:
        want = pr.lags(c["opts"])
        assert np.array_equal(Pitch(**c["opts"]).lags(), want) and np.array_equal(pitch_lags(pitch_opts(**c["opts"])), want)
        assert [Pitch(**c["opts"]).shape(len(w))[0] for w in c["waves"]] == pc.frames_of(c)
    over = dict(delta_pitch=pc.delta_pitch_for(pc.MAX_STATES + 1))
    for refused in (lambda: Pitch(**over), lambda: pitch_lags(pitch_opts(**over))):
        with pytest.raises(EesenError, match="more than 1024 lag states") as e:
            refused()
        assert e.value.code == -1                       # EESEN_ERR_INVALID


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
