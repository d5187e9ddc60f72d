"""CPU: the restatement of the exact CTC scores and of the second pass (tests/ctc_rescore_restatement.py) against the restatements that
exist, and the properties of tests/ctc_rescore_cases.py's inputs the GPU tests rely on."""
import numpy as np
import pytest

from tests import ctc_beam_restatement as R
from tests import ctc_cases as cc
from tests import ctc_rescore_cases as Z
from tests import ctc_rescore_restatement as Q


def _all_entries():
    """(name, logp64 of the utterance, labels) of every labelling the cases hold."""
    lens, probs, S = Z.reorder_batch()
    for s in range(S):
        p = Z.utt(probs, s, S, int(lens[s]))
        for lab in Z.reorder_facts(p)["labels"]:
            yield f"reorder {s}", p, lab
    for name, (lens, probs, labels, T, S) in Z.quirk_cases().items():
        yield name, probs, list(labels[0])
    for name in Z.BITWISE:
        lens, probs, labels, T, S = Z.bitwise_case(name)
        for s in range(S):
            yield f"{name} {s}", Z.utt(probs, s, S, int(lens[s])), list(labels[s])


def test_fp64_restatement_is_lnp64_on_every_case():
    seen = 0
    for name, p, lab in _all_entries():
        l64 = R.log64(p)
        assert abs(Q.lnp(l64, lab) - R.lnp64(l64, lab)) <= 1e-12 * max(1.0, abs(R.lnp64(l64, lab))), name
        seen += 1
    assert seen >= 20
    # the conventions: the empty labelling, no frames, too few frames, a zero on every path
    l64 = R.log64(np.full((4, 3), 1.0 / 3, np.float32))
    for dt in (np.float64, np.float32):
        assert Q.lnp(l64, [], dt) == pytest.approx(4 * np.log(1.0 / 3), rel=1e-6) and Q.lnp(l64[:0], [], dt) == 0.0
        assert Q.lnp(l64[:0], [1], dt) == Q.NEG and Q.lnp(l64, [1, 1, 1], dt) == Q.NEG and Q.lnp(l64, [1, 1], dt) > Q.DEAD
        z = l64.copy()
        z[2, :] = Q.NEG
        assert Q.lnp(z, [1], dt) == Q.NEG and R.lnp64(z, [1]) == Q.NEG
    assert R.lnp64(l64, []) == pytest.approx(Q.lnp(l64, []), abs=1e-12)


def test_restatement_is_the_path_sum_for_every_labelling():
    """K = 3, n = 6: all 729 paths."""
    rng = np.random.default_rng(9501)
    p = cc.softmax32((2.0 * rng.standard_normal((6, 3))).astype(np.float32))
    l64 = R.log64(p)
    sums = R.enumerate_paths(l64)
    assert len(sums) > 30
    for lab, v in sums.items():
        assert abs(Q.lnp(l64, list(lab)) - v) < 1e-12 * max(1.0, abs(v)), lab
        assert Q.figure(Q.lnp(l64.astype(np.float32), list(lab), np.float32), v) < 1e-5, lab
    assert Q.lnp(l64, [1, 1, 1, 1]) == Q.NEG and (1, 1, 1, 1) not in sums          # 4 labels + 3 repeats on 6 frames: no path


def test_ordering_rule_on_lists():
    am = [np.float32(-3.0), np.float32(-2.0), None, np.float32(-2.0), np.float32(-1e30)]
    totals, order = Q.rescore(am, [0.0] * 5, [1] * 5, 1.0, 0.0)
    assert order == [1, 3, 0, 2, 4]                                   # the tie keeps the first-pass order; no score: last, by rank
    assert totals[2] == np.float32(-1e30) and totals[4] == np.float32(-1e30)
    totals, order = Q.rescore(am[:2], [-4.0, -9.0], [2, 5], 0.5, 0.25)
    assert totals[0] == np.float32(-3.0 + 0.5 * -4.0 + 0.25 * 2) and totals[1] == np.float32(-2.0 + 0.5 * -9.0 + 0.25 * 5)
    assert order == [0, 1]
    # weight and bonus are the float32 values the C call receives
    assert Q.total_of(-1.0, -7.0, 3, 0.1, 0.3) == np.float32(-1.0 + float(np.float32(0.1)) * -7.0 + float(np.float32(0.3)) * 3)


def test_reorder_case_preconditions():
    assert Z.search_reorder(len(Z.REORDER_SEEDS)) == Z.REORDER_SEEDS
    assert Z.REORDER["n"] <= 16 and Z.REORDER["K"] <= 6 and Z.REORDER["B"] <= 4
    lens, probs, S = Z.reorder_batch()
    for s in range(S):
        f = Z.reorder_facts(Z.utt(probs, s, S, int(lens[s])))
        assert f["ok"] and f["order64"] != [0, 1, 2, 3] and f["order64"][0] != 0, s
        assert Q.min_gap(f["exact"]) > 1e-3 and Q.min_gap(f["beam"]) > 1e-3, s
        for lab, total, exact in zip(f["labels"], f["beam"], f["exact"]):
            assert exact >= total - R.bar_of(total, int(lens[s])), (s, lab)      # the exact score is never below the beam's


def test_quirk_case_preconditions():
    cases = Z.quirk_cases()
    assert set(cases) == {"no_final_blank", "no_final_blank_h12", "last_frame_spike"}
    for name, (lens, probs, labels, T, S) in cases.items():
        lab = list(labels[0])
        if name.startswith("no_final_blank"):
            assert int(lens[0]) == len(lab) + cc.num_repeats(lab), name
        o32, _ = cc.oracle_pair(lens, probs, labels, T, S)
        bar, floor, a64 = Q.bar(R.log64(probs), lab)
        assert a64 > Q.DEAD, name
        assert o32["pzx"][0] < -1e29 or abs(float(o32["pzx"][0]) - a64) > 1.0, (name, o32["pzx"][0], a64)
        a32 = Q.lnp(R.log32(probs), lab, np.float32)
        assert Q.figure(a32, a64) < bar, (name, a32, a64, bar)


@pytest.mark.parametrize("name", sorted(Z.BITWISE))
def test_bitwise_case_preconditions(name):
    lens, probs, labels, T, S = Z.bitwise_case(name)
    longest = max(2 * len(l) + 1 for l in labels)
    assert Z.BITWISE[name]["positions"] // 2 < longest <= Z.BITWISE[name]["positions"]
    for s in range(S):
        n = int(lens[s])
        assert n > len(labels[s]) + cc.num_repeats(labels[s])
        b, l = Q.final_cells(R.log32(Z.utt(probs, s, S, n)), list(labels[s]), np.float32)
        assert float(b) >= float(l) + 1.0 and float(b) > Q.DEAD, (s, b, l)
