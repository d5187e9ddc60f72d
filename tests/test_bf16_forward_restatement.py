"""CPU: the fp64 restatement of the "bf16 forward" variant (tests/layer_restatement.py: gemm(bf16_operands=True);
tests/bf16_forward_restatement.py: one step of the recurrence) and its bounds, on the very arrays tests/test_gpu_bf16_forward_fp64.py
gives the kernels (tests/bf16_forward_cases.py):
  * an fp32 evaluation of the variant's arithmetic -- operands rounded to nearest even, fp32 accumulation in k order in 16-wide blocks,
    the device's activation formulas -- stays inside EVERY bound of every case;
  * every listed fault leaves the bound on an element of a NAMED case and quantity (SHOWS);
  * each direction's recurrent product is within reach of the bounds at every tile: a fault confined to one direction shows there;
  * the bounds hold something: per sequence and quantity, at most half of the live elements have a bound above their own magnitude."""
import functools

import numpy as np
import pytest

from tests import bf16_forward_cases as BC
from tests import bf16_forward_restatement as BR
from tests import layer_restatement as R
from tests import lstm_gemm_restatement as LR
from tests.layer_cases import affine_case, affine_input

wr = BC.worst_ratio
# fault -> (case, quantity) on which it must leave the bound.  GEMM cases: the held layer's gate activations; affine:<name>: the output.
SHOWS = {"truncated": ("ends", "gates"), "only_a_rounded": ("interior", "gates"), "only_b_rounded": ("affine:tile", "out"),
         "unrounded": ("affine:big", "out"), "bf16_accumulator": ("ends", "gates"), "k_tail_dropped": ("ragged", "gates"),
         "wm_one_plane": ("bi256_s20", "gates"), "m_unrounded": ("bi1024_s32", "m"), "m_truncated": ("bi768_s16", "c"),
         "c_two_steps_back": ("bi256_s20", "c"), "shifts_swapped": ("bi256_s20", "m"),
         # confined to one direction
         "wm_one_plane_forward": ("bi768_s16", "c"), "wm_one_plane_backward": ("bi768_s16", "gates"),
         "stale_m_backward": ("bi1024_s32", "m"), "no_product_backward": ("bi512_tiny", "gates")}
ORDINARY_BI = [n for n, c in BC.RECURRENCE.items() if c[0] == BC.BI and c[5] is None]       # both directions of ordinary size


# ------------------------------------------------------------------------------------------------------------ GEMM
@functools.lru_cache(maxsize=None)
def _gemm_operands(name):
    """(a, b, bias, value, bound of the held quantity, fp32 result -> held quantity)."""
    if name.startswith("affine:"):
        case = affine_case(name[7:])
        xa = affine_input(case)
        v, b = R.affine_forward(xa, case["W"], case["b"], 0, bf16_operands=True)
        return xa, case["W"], case["b"], v, b, lambda c32: c32
    case = BC.gemm_case(name)
    L = case["layers"][case["hold"]]
    P = LR.unpack(L)
    xa = BC.held_input(case)
    v, b, _, _ = LR.gates_restated(L, xa, case["lens"], case["S"], case["T"], 0, False, bf16_operands=True)
    return xa, P["Wx"], P["b"], v, b, lambda c32: LR.gates_fp32(P, c32, case["lens"], case["S"], case["T"])


GEMM_NAMES = [n for n in BC.GEMM if n != "quadrants"] + ["affine:" + n for n in BC.AFFINE_LAST]      # (quadrants: the arrays of ends)


@pytest.mark.parametrize("name", GEMM_NAMES)
def test_fp32_evaluation_of_the_gemm_stays_inside_every_bound(name):
    a, b, bias, v, bound, through = _gemm_operands(name)
    r = wr(through(BR.gemm_fp32(a, b, bias)), v, bound)
    print(name, "worst error / bound", r)
    assert r < 1.0
    # the mode argument is ignored, and the rounded operands restate themselves
    v2, b2 = R.gemm(R.round_bf16(a), R.round_bf16(b), 2, bias=bias, bf16_operands=True)
    v0, b0 = R.gemm(a, b, 0, bias=bias, bf16_operands=True)
    assert np.array_equal(v2, v0) and np.array_equal(b2, b0)


@pytest.mark.parametrize("mutation", BR.GEMM_MUTATIONS)
def test_every_gemm_fault_leaves_the_bound_on_its_named_case(mutation):
    name, _ = SHOWS[mutation]
    a, b, bias, v, bound, through = _gemm_operands(name)
    r = wr(through(BR.gemm_fp32(a, b, bias, mutation)), v, bound)
    print(mutation, SHOWS[mutation], "worst error / bound", r)
    assert r > 1.0


def test_the_k_tail_is_only_a_fault_where_there_is_one():
    """interior and ends have K = 64 and 512: whole 16-wide blocks, the unguarded kernel."""
    for name in ("interior", "ends"):
        a, b, bias, _, _, _ = _gemm_operands(name)
        assert a.shape[1] % 16 == 0 and np.array_equal(BR.gemm_fp32(a, b, bias, "k_tail_dropped"), BR.gemm_fp32(a, b, bias))
    assert _gemm_operands("ragged")[0].shape[1] % 16 != 0


# ------------------------------------------------------------------------------------------------------------ recurrence
@functools.lru_cache(maxsize=None)
def _free_running(name, mutation=None):
    case = BC.recurrence_case(name)
    return BR.layer_fp32(case["layers"][0], case["x"], case["lens"], case["S"], case["T"], mutation)


def _restated(name, dev, rec_round=True):
    case = BC.recurrence_case(name)
    return BR.step_restated(case["layers"][0], case["x"], case["lens"], case["S"], case["T"], dev["m"], dev["c"], rec_round)


@pytest.mark.parametrize("name", list(BC.RECURRENCE))
def test_fp32_evaluation_of_the_recurrence_stays_inside_every_bound(name):
    case = BC.recurrence_case(name)
    dev = _free_running(name)
    want = _restated(name, dev)
    live = LR.live_rows(case["lens"], case["S"], case["T"])
    assert not live.all()
    for q in BR.QUANTITIES:
        r = wr(dev[q], *want[q])
        print(name, q, "worst error / bound", r)
        assert r < 1.0
        assert np.all(want[q][0][~live] == 0) and np.all(want[q][1][~live] == 0)
    # what the bounds hold: per sequence and QUANTITY, at most half of the live elements have a bound above their own magnitude
    share = {q: float(BR.vacuous_share([want[q]], case["lens"], case["S"], case["T"]).max()) for q in BR.QUANTITIES}
    print(name, "largest share of a sequence's elements with bound > |value|", share)
    assert max(share.values()) <= 0.5
    # without the recurrence's roundings the restatement is another function: the bounds tell the two precisions apart
    other = _restated(name, dev, rec_round=False)
    assert max(wr(dev[q], *other[q]) for q in BR.QUANTITIES) > 1.0


@pytest.mark.parametrize("name", ORDINARY_BI)
def test_each_direction_s_recurrent_product_is_within_reach_at_every_tile(name):
    """W_m as ONE plane in one direction only leaves the bound on that direction's columns, of every quantity, and on no other: the
    kernel's code for the backward chain (t and tp, the exchange block of (tp, dir), the hi / lo planes of direction 1) is held as
    the forward chain's is."""
    H = BC.recurrence_case(name)["H"]
    for dirn, mutation in enumerate(("wm_one_plane_forward", "wm_one_plane_backward")):
        dev = _free_running(name, mutation)
        want = _restated(name, dev)
        for q in BR.QUANTITIES:
            w = (4 if q == "gates" else 1) * H
            hit, other = slice(dirn * w, (dirn + 1) * w), slice((1 - dirn) * w, (2 - dirn) * w)
            r_hit = wr(dev[q][:, hit], want[q][0][:, hit], want[q][1][:, hit])
            r_other = wr(dev[q][:, other], want[q][0][:, other], want[q][1][:, other])
            print(name, mutation, q, "worst error / bound in the direction", r_hit, "in the other", r_other)
            assert r_hit > 1.0 and r_other < 1.0


@pytest.mark.parametrize("name", GEMM_NAMES)
def test_gemm_bounds_hold_something(name):
    a, b, bias, v, bound, _ = _gemm_operands(name)
    if name.startswith("affine:"):
        assert (bound > np.abs(v)).mean(1).max() <= 0.5
    else:
        case = BC.gemm_case(name)
        assert BR.vacuous_share([(v, bound)], case["lens"], case["S"], case["T"]).max() <= 0.5


@pytest.mark.parametrize("mutation", [m for m in BR.REC_MUTATIONS if m != "wm_unrounded"])
def test_every_recurrence_fault_leaves_the_bound_on_its_named_case(mutation):
    name, q = SHOWS[mutation]
    dev = _free_running(name, mutation)
    r = wr(dev[q], *_restated(name, dev)[q])
    print(mutation, SHOWS[mutation], "worst error / bound", r)
    assert r > 1.0


def test_an_unrounded_w_m_cannot_leave_the_bound():
    """The one listed fault that no case can be made to show, by arithmetic: hi + lo keeps W_m to within 2^-17 |W_m| (17 significant
    bits: the second rounding is of a remainder below 2^-8 of the leading bit), so an unrounded W_m moves a pre-activation by at
    most 2^-17 sum |m||W_m| -- and that only where every product errs the same way -- which is under half of the accumulation term
    (H + 3) 2^-24 sum |m||W_m| at the smallest admitted H = 256, and less above.  Two planes ARE fp32-class at this bound; ONE plane
    (2^-9) is not, and that fault is shown above."""
    worst = 0.0
    for name in BC.RECURRENCE:
        for Wm in LR.unpack(BC.recurrence_case(name)["layers"][0])["Wm"]:
            hi, lo = BR.wm_planes(Wm)
            w = Wm.astype(np.float64)
            worst = max(worst, float(np.max(np.abs(w - hi.astype(np.float64) - lo) / np.abs(w))))
    assert 0 < worst <= 2.0 ** -17 and 2 * 2.0 ** -17 < (256 + 3) * BR.U
    dev = _free_running("bi256_s20", "wm_unrounded")
    assert not np.array_equal(dev["m"], _free_running("bi256_s20")["m"])
    assert max(wr(dev[q], *_restated("bi256_s20", dev)[q]) for q in BR.QUANTITIES) < 1.0


def test_case_tables():
    assert set(SHOWS) == set(BR.GEMM_MUTATIONS + BR.REC_MUTATIONS) - {"wm_unrounded"}
    assert {BC.recurrence_case(n)["H"] for n in ORDINARY_BI} == {256, 512, 768, 1024}
    assert sorted(c[5] for c in BC.RECURRENCE.values() if c[5] is not None) == [0, 1]
    assert [BC.bf16_layers(BC.gemm_case(n)["layers"]) for n in BC.GEMM] == [0, 0, 2, 2]
    assert BC.gemm_case("quadrants")["x"] is not None and np.array_equal(BC.gemm_case("quadrants")["x"], BC.gemm_case("ends")["x"])
    assert ("quadrants", 1) not in BC.GEMM_RUNS and len(BC.GEMM_RUNS) == 7
    for n in BC.GEMM:
        case = BC.gemm_case(n)
        P = LR.unpack(case["layers"][case["hold"]])
        assert not np.any(P["Wx"][P["Wx"].shape[0] // 3]) and case["lens"].min() < case["T"]
