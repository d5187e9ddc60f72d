"""What tests/test_gpu_recurrence_dropout.py relies on, held without a GPU: the case table reaches every DROP = true row of the
recurrence kernel table, the generated inputs have the lengths, planted sequences and mask values the GPU bars assume, and the
oracle itself satisfies the exact properties the kernels are held to."""
import os
import re

import numpy as np
import pytest

from tests import dropout_cases as dc

KERNELS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eesen_amd", "csrc", "lstm_persistent.hip")
SMALLEST = [v for v in dc.VARIANTS if v[0] in ("bi64_s8", "bi64_s12", "bi128_s8")]


def test_every_dropout_row_of_the_kernel_table_is_run_by_a_case():
    src = open(KERNELS).read()
    fwd = re.findall(r"EESEN_FWD_F32\((\d+),(\d+),(\d+),(true|false),(true|false)\)", src)
    bwd = re.findall(r"EESEN_BWD_GEN\((\d+),(\d+),(true|false)\)", src)
    rows = ["lstm_fwd_persistent_kernel<%s>" % ",".join(r) for r in fwd if r[3] == "true"]
    rows += ["lstm_bwd_persistent_kernel<%s>" % ",".join(r) for r in bwd if r[2] == "true"]
    assert len(rows) == len(set(rows)) == 18, rows            # 8 forward, 10 backward
    named = {dc.fwd_row(c) for c in dc.CASES} | {dc.bwd_row(c) for c in dc.CASES}
    assert named <= set(rows), sorted(named - set(rows))       # the table names no row that is not compiled
    assert not named & set(dc.UNREACHED)
    missing = [r for r in rows if r not in named and r not in dc.UNREACHED]
    print(f"{len(named)} of {len(rows)} DROP = true rows are run by a named case; unreached: {sorted(dc.UNREACHED)}")
    assert not missing, missing
    assert len(named) >= 17 and all(dc.UNREACHED.values())


def test_the_recipes_run_where_the_table_says():
    by = {}
    for c, r in dc.VARIANTS:
        by.setdefault(c, []).append(r)
    assert list(by) == list(dc.CASES)
    for c in ("bi64_s12", "bi320_s10", "bi512_s32", "bi1024_s64"):
        assert {"rnndrop", "nml"} <= set(by[c])
    rest = [by[c][0] for c in dc.CASES if c not in ("bi64_s12", "bi320_s10", "bi512_s32", "bi1024_s64")]
    assert rest == ["rnndrop", "nml"] * 4
    assert "rnndrop_seq" in by["bi320_s10"] and {"nml_fwd", "generated"} <= set(by["bi512_s64"])
    assert len(dc.VARIANTS) == len(set(dc.VARIANTS)) == 19


@pytest.mark.parametrize("case", list(dc.CASES))
def test_lengths_and_planted_sequences(case):
    c = dc.CASES[case]; S, T, H = c["S"], c["T"], c["H"]
    lens = dc.lengths(case)
    assert lens.shape == (S,) and lens.min() >= 1 and lens.max() == T and T // 2 >= 2 and T // 2 + 1 < T
    for z in range(0, S, 16):                                  # every 16-sequence tile: lengths T, 1 and 2
        assert {T, 1, 2} <= set(lens[z:z + 16].tolist()), (case, z)
    if c["launches"] == 2:                                     # the two sequence windows differ
        assert not np.array_equal(lens[:S // 2], lens[S // 2:])
        assert np.flatnonzero(lens[:S // 2] == 1).tolist() != np.flatnonzero(lens[S // 2:] == 1).tolist()
    keep, drop = dc.planted(case)
    assert keep != drop and lens[keep] == T and lens[drop] == T and keep < 16 and drop >= 16 * ((S - 1) // 16)
    x = dc.features(case, lens).reshape(T, S, dc.D)
    ods, zero = dc.top_gradients(case, lens)
    assert zero and [p for p, _ in ods] == ["a", "b"]
    pad = np.arange(T)[:, None] >= lens[None, :]
    assert np.all(x[pad] == 0) and np.all(x[~pad].any(axis=-1))
    for _, od in ods:
        assert np.all(od.reshape(T, S, 2 * H)[pad] == 0)
    b = ods[1][1].reshape(T, S, 2 * H)
    assert all(np.all(b[:, s] == 0) for s in zero) and all(s % 4 == 1 and (s // 4) % 2 == 1 for s in zero)
    a = ods[0][1].reshape(T, S, 2 * H)
    for s in set(range(S)) - set(zero):
        assert np.array_equal(b[:, s], a[:, s] * np.float32(2.0 ** (-8 * (s % 4))))
    for recipe in [r for cc, r in dc.VARIANTS if cc == case and r != "generated"]:
        mk = dc.masks(case, recipe)
        kept = np.float32(1.0 / (1.0 - dc.P_REC))
        seq = bool(dc.RECIPES[recipe].get("rec_seq"))
        assert mk["rec"].shape == ((S if seq else (T + 2) * S), 2 * H) and mk["rec"].dtype == np.float32
        assert set(np.unique(mk["rec"])) == {np.float32(0), kept}
        assert abs((mk["rec"] > 0).mean() - (1 - dc.P_REC)) < 0.05
        m = dc.step_mask(case, mk["rec"])
        assert m.shape == (T, S, 2 * H) and np.all(m[:, keep] == kept)
        if not seq:
            assert np.all(m[T // 2, drop] == 0) and m[T // 2 - 1, drop].any() and m[T // 2 + 1, drop].any()
            assert not np.array_equal(m[0], m[1])
        if dc.RECIPES[recipe].get("forward"):
            assert mk["fwd"].shape == (T * S, 2 * H) and set(np.unique(mk["fwd"])) == {np.float32(0), np.float32(1.0 / (1.0 - dc.P_FWD))}
        else:
            assert mk["fwd"] is None


@pytest.mark.parametrize("variant", SMALLEST, ids=[f"{c}-{r}" for c, r in SMALLEST])
def test_the_oracle_satisfies_the_exact_checks(variant):
    """... and the fp32 oracle's distance to the fp64 one, the first yardstick of the GPU bars, is finite and not zero."""
    case, recipe = variant
    c = dc.CASES[case]; S, T, H = c["S"], c["T"], c["H"]
    lens = dc.lengths(case); x = dc.features(case, lens); ods, zero = dc.top_gradients(case, lens)
    mk = dc.masks(case, recipe)
    L = dc.layer(case, recipe)
    out64, back64 = dc.oracle_run(L, x, lens, ods, "f64", mk)
    out32, back32 = dc.oracle_run(L, x, lens, ods, "f32", mk)
    pad = np.arange(T)[:, None] >= lens[None, :]
    m = dc.step_mask(case, mk["rec"])
    for out, back in ((out64, back64), (out32, back32)):
        o = out.reshape(T, S, 2 * H)
        # (padding rows: the reference masks only its backward direction's (bilstm-parallel-layer.h:201-204); its forward direction runs on
        # over them, after every valid frame, and the library's kernels write zeros there -- the GPU test holds THEM to exact zeros)
        assert np.isfinite(o).all() and np.all(o[pad][:, H:] == 0)
        if dc.RECIPES[recipe].get("rnndrop"):                  # c = 0 where the mask is 0, so tanh(c) * o = 0
            assert np.all(o[(m == 0) & ~pad[:, :, None]] == 0)
            assert np.count_nonzero(o[~pad]) > 0.5 * o[~pad].size
        for (prof, _), (ind, g) in zip(ods, back):
            i = ind.reshape(T, S, dc.D)
            assert np.isfinite(i).all() and np.isfinite(g).all() and np.all(i[pad] == 0)
            if prof == "b":
                assert all(np.all(i[:, s] == 0) for s in zero)
    w = dc.seq_worst(out32.reshape(T, S, 2 * H), out64.reshape(T, S, 2 * H), lens, blocks=2)
    assert 0 < w["maxnorm"] < 1e-5 and 0 < w["p999"] < 1e-3, w
    for (_, _), (i32, _), (i64, _) in zip(ods, back32, back64):
        w = dc.seq_worst(i32.reshape(T, S, dc.D), i64.reshape(T, S, dc.D), lens)
        assert 0 < w["maxnorm"] < 1e-4 and np.isfinite(w["p999"]) and w["p999"] > 0, w
    # the dropout did something: the same layer without it gives another output
    plain, _ = dc.oracle_run(dc.layer(case), x, lens, [], "f64")
    assert np.abs(plain - out64).max() > 1e-3
