"""What tests/test_gpu_recurrence_share.py relies on, held without a GPU: tests/share_cases.py is well formed, every plan it names
satisfies the planner's own conditions on sequence windows, the table covers 2, 4 and 8 launches of every kernel family that runs in
windows, the generated inputs have the lengths and gradient profiles the GPU bars assume at the new batch sizes, and the fp32 oracle's
distance to the fp64 one, the yardstick of those bars, is finite and not zero."""
import os
import re

import pytest

from tests import recurrence_cases as rc
from tests import share_cases as sc
from tests import test_recurrence_cases as trc

# the three smallest cases (cells x sequences x frames x directions)
_size = lambda n: sc.ALL[n]["H"] * sc.ALL[n]["S"] * sc.ALL[n]["T"] * sc.ndir(n)
SMALLEST = sorted(sc.TABLE, key=_size)[:3]
# one case per shape (kind, cells, sequences): the inputs are a function of the shape alone
SHAPES = list({(c["kind"], c["H"], c["S"]): n for n, c in reversed(list(sc.TABLE.items()))}.values())[::-1]


def test_the_case_table_is_well_formed():
    tuning = open(os.path.join(os.path.dirname(trc.KERNELS), "tuning.h")).read()
    ab = tuning[tuning.index("A/B arms of the tests"):tuning.index("---- diagnostics")]
    rows = set(trc.table_rows())
    for name, c in sc.TABLE.items():
        assert name == rc.case_name(c["kind"], c["H"], c["S"], c["env"]) + (f"-{c['recipe']}" if c["recipe"] else "") + f"@share{c['share']}"
        assert c["share"] in (2, 4, 8) and c["share"] in sc.SHARES
        assert c["kind"] in ("BiLstmParallel", "LstmParallel") and c["T"] == (6 if c["S"] >= 64 else 8)
        for k in c["env"]:                       # only the A/B switches of tuning.h
            assert re.search(r"//\s+%s\s" % k, ab), (name, k)
        assert not {"EESEN_SPIN_LIMIT", "EESEN_POLL_NS", "EESEN_PERSISTENT", "EESEN_GPU_SHARE"} & set(c["env"])
        assert c["recipe"] is None or (c["recipe"] in sc.dc.RECIPES and c["kind"] == "BiLstmParallel")
        for p, n in zip(("fwd", "bwd"), c["launches"]):
            assert (c[p] == sc.PER_STEP_KERNELS) == (n == 0), (name, p)
            assert c[p] == sc.PER_STEP_KERNELS or c[p] in rows, (name, p, "names a row that is not compiled")
            assert n in (0, 1, 2, 4, 8), (name, p, n)
        # a dropout layer runs the DROP = true rows, any other the DROP = false ones
        for p in ("fwd", "bwd"):
            if sc.family(c[p]) in ("f32", "generic"):
                assert ("true" in c[p].split("<")[1].split(",")[3 if p == "fwd" else 2]) == bool(c["recipe"]), (name, c[p])
        assert sc.twin(name) in sc.SHARE1 and sc.ALL[sc.twin(name)]["share"] == 1
        tw = sc.ALL[sc.twin(name)]
        assert all(tw[k] == c[k] for k in ("kind", "H", "S", "T", "env", "recipe"))
    assert set(sc.CASES) | set(sc.PER_STEP) == set(sc.TABLE) and not set(sc.CASES) & set(sc.PER_STEP)
    assert sorted(n for s in (1, 2, 4, 8) for n in sc.at_share(s)) == sorted(sc.ALL) and sc.at_share(1) == list(sc.SHARE1)
    assert sc.STEP["cfg"]["S"] == 64 and sc.STEP["cfg"]["T"] == 12 and sc.STEP["cfg"]["H"] == 512 and sc.STEP["shares"] == (2, 4)


def test_every_plan_satisfies_the_planners_conditions_on_windows():
    """rec_plan.cpp, restated: pick_windows takes n equal windows only where S is divisible by n and a window is a whole number of
    sequence tiles; a frame's rows of the whole batch and of a window are whole 128-byte lines (line_aligned)."""
    for name, c in sc.TABLE.items():
        H, S, nd = c["H"], c["S"], sc.ndir(name)
        for p, n, cols in (("fwd", c["launches"][0], nd * H), ("bwd", c["launches"][1], nd * 4 * H)):
            if n == 0:
                continue
            assert S % n == 0 and (S // n) % sc.seq_tile(c[p]) == 0, (name, p, n, sc.seq_tile(c[p]))
            assert (S * cols * 4) % 128 == 0 and (S // n * cols * 4) % 128 == 0, (name, p)
            if sc.family(c[p]) == "q4":          # the 4 x 32 tile walks the whole batch itself
                assert n == 1


def test_the_table_covers_every_window_count_of_every_family():
    seen = {}
    for name, c in sc.TABLE.items():
        for p, n in zip(("fwd", "bwd"), c["launches"]):
            seen.setdefault(sc.family(c[p]), set()).add(n)
    print({k: sorted(v) for k, v in seen.items() if k})
    assert {2, 4, 8} <= seen["plane"]         # the forward plane rows
    assert {2, 4, 8} <= seen["f32"]           # the fp32 forward rows
    assert {2, 4, 8} <= seen["generic"]       # the generic backward tile
    # the K-split rows: 2 and 4.  (Eight windows of them need 128 sequences at 768 cells or more -- one 16-sequence tile is 96 to 128
    # workgroups -- which is twice the largest case here, in the oracles' time as well; the window loop itself is the launcher's, the
    # same for every family, and runs 8 times on the generic tile)
    assert {2, 4} <= seen["ksplit"]
    assert 1 in seen["q4"]
    both_ksplit = {c["bwd"].split("<")[0] for c in sc.TABLE.values() if sc.family(c["bwd"]) == "ksplit" and c["launches"][1] > 1}
    assert both_ksplit == {"lstm_bwd_persistent_ksplit_kernel", "lstm_bwd_persistent_ksplit_h_kernel"}
    assert any(c["recipe"] and c["launches"] == (2, 2) for c in sc.TABLE.values())                       # DROP = true in two windows
    assert {c["recipe"] for c in sc.TABLE.values()} >= {"nml", "rnndrop"}
    assert any(c["kind"] == "LstmParallel" and c["launches"] == (2, 2) for c in sc.TABLE.values())       # one direction in two windows
    assert sum(c["fwd"] == c["bwd"] == sc.PER_STEP_KERNELS for c in sc.PER_STEP.values()) >= 2
    # the multiplexed rows are never the table's: under a share they are taken at exactly two windows only, and no case has them there
    assert not any("_mux_" in c[p] for c in sc.TABLE.values() for p in ("fwd", "bwd"))
    assert {c["share"] for c in sc.TABLE.values()} == {2, 4, 8}
    assert 128 in {c["S"] for c in sc.TABLE.values()}


@pytest.mark.parametrize("name", SHAPES)
def test_lengths_features_and_top_gradients(name):
    trc.check_lengths_features_and_top_gradients(name, sc)
    # ... and the share-1 twin has the same inputs, as has the rows module's case of the same shape
    c = sc.TABLE[name]
    lens = sc.lengths(name)
    assert (sc.lengths(sc.twin(name)) == lens).all() and (sc.features(sc.twin(name), lens) == sc.features(name, lens)).all()
    same = [n for n, r in rc.ALL.items() if (r["kind"], r["H"], r["S"], r["T"]) == (c["kind"], c["H"], c["S"], c["T"])]
    for n in same[:1]:
        assert (rc.features(n, rc.lengths(n)) == sc.features(name, lens)).all()


def test_the_planted_masks_are_the_dropout_modules():
    for name, c in sc.TABLE.items():
        mk = sc.masks(name)
        assert (mk is None) == (c["recipe"] is None)
        if mk is not None:
            want = sc.dc.masks(f"bi{c['H']}_s{c['S']}", c["recipe"])
            assert (mk["rec"] == want["rec"]).all() and mk["fwd"] is None and want["fwd"] is None
            assert mk["rec"].shape == ((c["T"] + 2) * c["S"], 2 * c["H"])
            assert sc.layer(name)[0]["dropout"] == sc.dc.RECIPES[c["recipe"]] and "dropout" not in sc.layer("bi512_s64@share2")[0]


@pytest.mark.parametrize("name", SMALLEST)
def test_the_fp32_oracle_is_a_yardstick_and_both_oracles_satisfy_the_exact_checks(name):
    trc.check_the_yardstick(name, sc)
