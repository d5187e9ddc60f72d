"""What tests/test_gpu_recurrence_rows.py relies on, held without a GPU: every row of the recurrence kernel table is accounted for --
run by a named case, held by another module, or written down as unreachable -- the generated inputs have the lengths and gradient
profiles the GPU bars assume, and the fp32 oracle's distance to the fp64 one, the yardstick of those bars, is finite and not zero."""
import os
import re

import numpy as np
import pytest

from tests import dropout_cases as dc
from tests import recurrence_cases as rc

KERNELS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eesen_amd", "csrc", "lstm_persistent.hip")
MACROS = {"EESEN_FWD_F32": "lstm_fwd_persistent_kernel", "EESEN_FWD_BF": "lstm_fwd_persistent_bf_kernel",
          "EESEN_BWD_GEN": "lstm_bwd_persistent_kernel", "EESEN_BWD_Q4": "lstm_bwd_persistent_q4_kernel"}
# the three smallest cases (cells x sequences x frames x directions) and bi36_s8
_size = lambda n: rc.ALL[n]["H"] * rc.ALL[n]["S"] * rc.ALL[n]["T"] * rc.ndir(n)
SMALLEST = list(dict.fromkeys(sorted(rc.CASES, key=_size)[:3] + ["bi36_s8"]))


def table_rows():
    """The rows of kRecKernels, named as the EESEN_ROW macro stringises them (and as Plan() prints them): kernel<arguments>."""
    src = open(KERNELS).read()
    body = src[src.index("const RecKernel kRecKernels[] = {"):]
    body = re.sub(r"//[^\n]*", "", body[:body.index("};")])
    rows = []
    for macro, args in re.findall(r"\b(EESEN_ROW|EESEN_FWD_F32|EESEN_FWD_BF|EESEN_BWD_GEN|EESEN_BWD_Q4)\(([^()]*)\)", body):
        a = [x.strip() for x in args.split(",")]
        if macro == "EESEN_ROW":                       # (family, kind, kernel, arguments...)
            rows.append("%s<%s>" % (a[2], ",".join(a[3:])))
        else:
            rows.append("%s<%s>" % (MACROS[macro], ",".join(a)))
    assert body.count("EESEN_") == len(rows), "a row of the table was not parsed"
    return rows


def test_every_row_of_the_kernel_table_is_accounted_for_once():
    rows = table_rows()
    # The table compiles 71 instantiations: 21 fp32 forward tiles, 12 on the bf16 pipe, 2 multiplexed forward, 20 generic backward,
    # 8 of the 4 x 32 backward tile, 3 + 2 + 3 K-split ones -- 18 of them DROP = true (tests/test_dropout_cases.py), 53 not.
    assert len(rows) == len(set(rows)) == 71, (len(rows), sorted(r for r in set(rows) if rows.count(r) > 1))
    per_family = {k: sum(r.startswith(k + "<") for r in rows) for k in sorted({r.split("<")[0] for r in rows})}
    assert per_family == {"lstm_fwd_persistent_kernel": 21, "lstm_fwd_persistent_bf_kernel": 12, "lstm_fwd_persistent_mux_kernel": 2,
                          "lstm_bwd_persistent_kernel": 20, "lstm_bwd_persistent_q4_kernel": 8, "lstm_bwd_persistent_ksplit_kernel": 3,
                          "lstm_bwd_persistent_ksplit_h_kernel": 2, "lstm_bwd_persistent_ksplit_mux_kernel": 3}, per_family
    named = {c["fwd"] for c in rc.CASES.values()} | {c["bwd"] for c in rc.CASES.values()}
    held, unreached = set(rc.HELD_ELSEWHERE), set(rc.UNREACHED)
    for what, names in (("CASES", named), ("HELD_ELSEWHERE", held), ("UNREACHED", unreached),
                        ("PER_STEP", {c[p] for c in rc.PER_STEP.values() for p in ("fwd", "bwd")} - {rc.PER_STEP_KERNELS})):
        assert names <= set(rows), (what, "names a row that is not compiled", sorted(names - set(rows)))
    assert all(r.strip() for r in rc.UNREACHED.values()) and all(rc.HELD_ELSEWHERE.values())
    assert not unreached & (named | held)
    # A case runs two rows; where one of them is held by another module it stays that module's (the product path's narrow forward
    # tile under the two-tile backward arm at 320 cells: the only one)
    assert named & held == {rc.fwd_bf(2, 2, 2, 2, True)}, sorted(named & held)
    own = named - held
    print(f"{len(rows)} rows: {len(own)} run by a case of recurrence_cases.CASES, {len(held)} held elsewhere "
          f"({sum('dropout' in v for v in rc.HELD_ELSEWHERE.values())} of them DROP = true), {len(unreached)} unreached")
    missing = [r for r in rows if r not in own | held | unreached]
    assert not missing, missing
    assert len(own) + len(held) + len(unreached) == len(rows)      # ... each once
    assert (len(own), len(held), len(unreached)) == (42, 25, 4)
    print(f"all {len(rows)} rows are accounted for, each once")
    # the DROP = true rows are exactly what the dropout table answers for
    assert {r for r in rows if re.search(r"kernel<[\d,]+,true(,false)?>$", r) and "_bf_" not in r and "_mux_" not in r} == \
        {r for r, v in rc.HELD_ELSEWHERE.items() if "dropout" in v}


def test_the_case_table_is_well_formed():
    tuning = open(os.path.join(os.path.dirname(KERNELS), "tuning.h")).read()
    ab = tuning[tuning.index("A/B arms of the tests"):tuning.index("---- diagnostics")]
    for name, c in rc.ALL.items():
        assert name == rc.case_name(c["kind"], c["H"], c["S"], c["env"])
        assert c["kind"] in ("BiLstmParallel", "LstmParallel") and c["T"] == (6 if c["S"] >= 64 else 8)
        for k in c["env"]:                       # only the A/B switches of tuning.h
            assert re.search(r"//\s+%s\s" % k, ab), (name, k)
        assert not {"EESEN_SPIN_LIMIT", "EESEN_POLL_NS", "EESEN_PERSISTENT"} & set(c["env"])
    for name, c in rc.CASES.items():
        assert rc.line_aligned(name), name
        assert c["fwd"].startswith("lstm_fwd_persistent_") and c["bwd"].startswith("lstm_bwd_persistent_")
        assert all(n in (1, 2) for n in c["launches"])
    assert not rc.line_aligned("bi20_s17")
    assert all(rc.line_aligned(n) for n in rc.PER_STEP if n != "bi20_s17")
    for name in ("bi1280_s8", "uni2048_s8"):
        assert rc.PER_STEP[name]["H"] > 1024 and rc.PER_STEP[name]["fwd"] == rc.PER_STEP[name]["bwd"] == rc.PER_STEP_KERNELS
    assert all(c["fwd"] == rc.PER_STEP_KERNELS for c in rc.PER_STEP.values())
    # widths no other module runs: between 512 and 1024 cells, above 1024, and no multiple of 32 above 150
    H = {c["H"] for c in rc.ALL.values()}
    assert {528, 640} <= H and {1280, 2048} <= H and {200, 264, 300, 400, 516, 520} <= H


@pytest.mark.parametrize("name", list(rc.ALL))
def test_lengths_features_and_top_gradients(name):
    check_lengths_features_and_top_gradients(name)


def check_lengths_features_and_top_gradients(name, rc=rc):
    """(rc: the module of the case table -- tests/test_share_cases.py holds its own table's inputs to the same checks)"""
    c = rc.ALL[name]; S, T, H, nd = c["S"], c["T"], c["H"], rc.ndir(name)
    lens = rc.lengths(name)
    assert lens.shape == (S,) and lens.dtype == np.int32 and lens.min() >= 1 and lens.max() == T
    tiles = [sorted(lens[z:z + 16].tolist()) for z in range(0, S, 16)]
    for z in range(0, S, 16):                                  # every 16-sequence tile: lengths T, 1 and 2 ...
        assert set((T, 1, 2)[:S - z]) <= set(lens[z:z + 16].tolist()), (name, z)
    if S >= 32:                                                # ... at places that differ between tiles
        where = [tuple(np.flatnonzero(lens[z:z + 16] <= 2).tolist()) for z in range(0, S - 15, 16)]
        assert len(set(where)) > 1, (name, where, tiles)
    x = rc.features(name, lens).reshape(T, S, rc.D)
    ods, zero = rc.top_gradients(name, lens)
    assert [p for p, _ in ods] == ["a", "b"] and x.dtype == np.float32
    assert bool(zero) == (S >= 8) and all(s % 4 == 1 and (s // 4) % 2 == 1 and s < S for s in zero)
    pad = np.arange(T)[:, None] >= lens[None, :]
    assert np.all(x[pad] == 0) and np.all(x[~pad].any(axis=-1))
    for _, od in ods:
        assert od.shape == (T * S, nd * H) and od.dtype == np.float32 and np.all(od.reshape(T, S, nd * H)[pad] == 0)
    a, b = (od.reshape(T, S, nd * H) for _, od in ods)
    assert np.all(a[~pad].any(axis=-1))
    assert all(np.all(b[:, s] == 0) for s in zero)
    for s in set(range(S)) - set(zero):
        assert np.array_equal(b[:, s], a[:, s] * np.float32(2.0 ** (-8 * (s % 4))))
    L = rc.layer(name)
    assert len(L) == 1 and L[0]["type"] == c["kind"] and L[0]["input_dim"] == rc.D and L[0]["output_dim"] == nd * H
    # a function of the shape alone: two cases of one shape get the same inputs, and the dropout module's are those
    assert np.array_equal(lens, dc.shape_lengths(H, S, T, nd))


def test_the_generalised_generators_are_the_dropout_modules():
    for case in ("bi64_s8", "bi128_s32"):
        c = dc.CASES[case]
        lens = dc.lengths(case)
        assert np.array_equal(lens, dc.shape_lengths(c["H"], c["S"], c["T"], 2))
        assert np.array_equal(dc.features(case, lens), dc.shape_features(c["H"], c["S"], c["T"], 2, lens))
        for (_, o1), (_, o2) in zip(dc.top_gradients(case, lens)[0], dc.shape_top_gradients(c["H"], c["S"], c["T"], 2, lens)[0]):
            assert np.array_equal(o1, o2)
    # ... and this module's bi128_s32 has that module's inputs (the same shape)
    lens = rc.lengths("bi128_s32")
    assert np.array_equal(rc.features("bi128_s32", lens), dc.features("bi128_s32", dc.lengths("bi128_s32")))


@pytest.mark.parametrize("name", SMALLEST)
def test_the_fp32_oracle_is_a_yardstick_and_both_oracles_satisfy_the_exact_checks(name):
    check_the_yardstick(name)


def check_the_yardstick(name, rc=rc):
    c = rc.ALL[name]; S, T, H, nd = c["S"], c["T"], c["H"], rc.ndir(name)
    lens = rc.lengths(name); x = rc.features(name, lens); ods, zero = rc.top_gradients(name, lens)
    L = rc.layer(name)
    out64, back64 = rc.oracle_run(L, x, lens, ods, "f64", rc.masks(name))
    out32, back32 = rc.oracle_run(L, x, lens, ods, "f32", rc.masks(name))
    pad = np.arange(T)[:, None] >= lens[None, :]
    for out, back in ((out64, back64), (out32, back32)):
        o = out.reshape(T, S, nd * H)
        # (padding rows of the output: the reference masks only its backward direction's; its forward direction runs on over them,
        # after every valid frame -- the library's kernels write zeros there, and the GPU test holds THEM to exact zeros)
        assert np.isfinite(o).all() and (nd == 1 or np.all(o[pad][:, H:] == 0))
        for (prof, _), (ind, g) in zip(ods, back):
            i = ind.reshape(T, S, rc.D)
            assert np.isfinite(i).all() and np.isfinite(g).all() and np.all(i[pad] == 0)
            if prof == "b":
                assert zero and all(np.all(i[:, s] == 0) for s in zero)
    w = rc.seq_worst(out32.reshape(T, S, nd * H), out64.reshape(T, S, nd * H), lens, blocks=nd)
    assert 0 < w["maxnorm"] < 1e-5 and 0 < w["p999"] < 1e-3, w
    for (i32, _), (i64, _) in zip(back32, back64):
        w = rc.seq_worst(i32.reshape(T, S, rc.D), i64.reshape(T, S, rc.D), lens)
        assert 0 < w["maxnorm"] < 1e-4 and np.isfinite(w["p999"]) and w["p999"] > 0, w
