"""CPU: what tests/test_gpu_lstm_gemms.py holds the GEMMs and reductions around an LSTM layer against (tests/lstm_gemm_restatement.py,
cases: tests/lstm_gemm_cases.py).  The intermediates the GPU test reads from the device -- gate gradients, m, c -- come from a plain
numpy recurrence here.
  (a) the plain recurrence agrees with OracleNet(layers, "f64") (output, input gradient, parameter gradients), so the CPU stand-ins
      are the quantities the device computes;
  (b) a numpy fp32 evaluation -- for the plane modes an emulation of gemm.hip's arithmetic with the scales net.cpp prescribes -- stays
      inside every DERIVED bound; the worst ratio per quantity is printed;
  (c) every listed mutation leaves the bound on at least one element of every quantity it concerns, in mode 2, in every case it
      applies to; the factor is printed (inf: an fp16 plane overflowed).  This is the condition on the INPUTS of the cases.
The bounds come from counting roundings (module docstring of the restatement); nothing in them was fitted to an observed error."""
import functools
import json
import os

import numpy as np
import pytest

from tests import layer_restatement as R
from tests import lstm_gemm_cases as LC
from tests import lstm_gemm_restatement as LR

hs, am = R.half_scale, R.amax
SCALE_MUTATIONS = ("per_tensor_word", "wrong_axis", "stale_bound", "fw_rows_for_bw", "dir0_cols_for_dir1", "word_for_measured")
PLANE_MUTATIONS = ("drop_hi_lo", "drop_lo_planes", "no_bias")


def mutated_scales(P, x, DG, bounded, mutation):
    """The scales of prescribed_scales -- or, mutated, what a wrong net.cpp would use."""
    H4 = 4 * P["H"]
    xm = np.ascontiguousarray(x[::-1, ::-1]) if mutation == "stale_bound" else x       # the measurements of ANOTHER minibatch
    s = LR.prescribed_scales(P, xm, DG, bounded)
    W = P["Wx"]
    take = lambda v, n: np.resize(v, n)
    if mutation == "per_tensor_word":
        if not bounded:
            s["fwd_a"] = hs(am(x, None))
        s["fwd_b"] = hs(am(W, None))
        if DG is not None:
            s.update(in_a=hs(am(DG, None)), in_b=hs(am(W, None)), wx_a=hs(am(DG, None)), wm_a=np.full(DG.shape[1], hs(am(DG, None))))
            if not bounded:
                s["wx_b"] = hs(am(x, None))
    elif mutation == "wrong_axis":           # rows where columns are due and the reverse, read at the index the kernel would use
        if not bounded:
            s["fwd_a"] = take(hs(am(x, 0)), x.shape[0])
        s["fwd_b"] = take(hs(am(W, 0)), W.shape[0])
        if DG is not None:
            s.update(in_a=take(hs(am(DG, 0)), DG.shape[0]), in_b=take(hs(am(W, 1)), W.shape[1]), wx_a=take(hs(am(DG, 1)), DG.shape[1]),
                     wm_a=take(hs(am(DG, 1)), DG.shape[1]))
            if not bounded:
                s["wx_b"] = take(hs(am(x, 1)), x.shape[1])
    elif mutation == "fw_rows_for_bw":       # w_hi.p += N4 forgotten: the backward direction's W_x rows under the forward rows' bounds
        s["fwd_b"] = np.concatenate([s["fwd_b"][:H4], s["fwd_b"][:H4]])
    elif mutation == "dir0_cols_for_dir1":   # bd.cols + dir 4H forgotten in the W_m gradient
        s["wm_a"] = np.concatenate([s["wm_a"][:H4], s["wm_a"][:H4]])
    elif mutation == "word_for_measured":    # the word 1.0 although the mask scales m by 1 / (1 - p)
        s["fwd_a"] = hs(1.0)
    return s


def gates_fp32(case, mode, x, mutation=None):
    L = case["layers"][case["hold"]]
    P = LR.unpack(L)
    s = mutated_scales(P, x, None, LC.x_bounded(case), mutation if mutation in SCALE_MUTATIONS else None)
    G = R.gemm_fp32(x, P["Wx"], mode, s["fwd_a"], s["fwd_b"], P["b"], mutation if mutation in PLANE_MUTATIONS else None)
    return LR.gates_fp32(P, G, case["lens"], case["S"], case["T"])


def backward_fp32(case, mode, x, buf, mutation=None):
    """Every backward quantity of the held layer in numpy fp32, from the same x, DG, m, c the restatement reads."""
    L = case["layers"][case["hold"]]
    P = LR.unpack(L)
    nd, H, S = P["nd"], P["H"], case["S"]
    DG, m, c = buf["DG"], buf["m"], buf["c"]
    s = mutated_scales(P, x, DG, LC.x_bounded(case), mutation if mutation in SCALE_MUTATIONS else None)
    pm = mutation if mutation in PLANE_MUTATIONS else None
    out = dict(in_diff=R.gemm_fp32(DG, P["Wx"].T, mode, s["in_a"], s["in_b"], None, pm), Wx_grad=R.gemm_fp32(DG.T, x.T, mode, s["wx_a"], s["wx_b"], None, pm),
               b_grad=LR.col_reduction_fp32(DG))
    for dirn in range(nd):
        cols = slice(dirn * 4 * H, (dirn + 1) * 4 * H)
        ms = m[:, dirn * H:(dirn + 1) * H] if mutation == "unshifted_m" else LR.shifted(m, S, dirn, H)
        out[f"Wm_grad{dirn}"] = R.gemm_fp32(DG[:, cols].T, ms.T, mode, s["wm_a"][cols], s["wm_b"], None, pm)
        terms = LR.peephole_terms(P, DG, c, S, dirn, swapped=mutation == "peephole_shift_swapped")
        out[f"peep_grad{dirn}"] = np.stack([LR.col_reduction_fp32(t.astype(np.float32)) for t in terms])
    return out


@functools.lru_cache(maxsize=None)
def cpu_buffers(name):
    """(the held layer's x, dict(gates, c, m, DG) of the held layer) from the plain recurrence."""
    case = LC.backward_case(name)
    S, T, lens = case["S"], case["T"], case["lens"]
    x = LC.held_input(case)
    return x, LR.recurrence(case["layers"][case["hold"]], x, lens, S, T, case["d"])


ALL_BACKWARD = list(LC.BACKWARD) + list(LC.UPPER)
ALL_FORWARD = list(LC.FORWARD) + list(LC.SINGLE)


# ------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("name", ["ragged", "uni", "upper"])
def test_the_plain_recurrence_equals_the_f64_oracle(name):
    from oracle import net as onet
    case = LC.backward_case(name)
    S, T, lens = case["S"], case["T"], case["lens"]
    ora = onet.OracleNet(case["layers"], "f64")
    ora.set_seq_lengths(lens)
    out = ora.propagate(case["x"])
    # (padded frames: the reference lets the forward direction run on and relies on a zero gradient there, the library zeroes both
    # directions' gates, state and gate gradients -- lstm.hip: t >= len --, as the plain recurrence does: compared on the real frames)
    live = LR.live_rows(lens, S, T)
    in_diff = ora.backpropagate(np.where(live[:, None], case["d"], np.float32(0)), update=False)
    x = case["x"] if case["hold"] == 0 else LR.recurrence(case["layers"][0], case["x"], lens, S, T, dtype=np.float64)["m"]
    L = case["layers"][case["hold"]]
    buf = LR.recurrence(L, x, lens, S, T, case["d"], dtype=np.float64)      # (uncast: gate gradients below the fp32 range stay what they are)
    if case["hold"] == 0:
        assert np.abs(buf["m"] - out)[live].max() <= 1e-12
    want = LR.backward_restated(L, x, buf["DG"], buf["m"], buf["c"], S, 0, LC.x_bounded(case))
    fresh = ora.fresh_grads_flat()
    n = sum(p.size for p in L["params"])
    got = LR.grads_by_quantity(L, fresh[fresh.size - n:])
    if case["hold"] == 0:
        got["in_diff"] = in_diff
    # (the mode-0 bound is (K + 3) 2^-24 sum |a||b| and up: 1e-6 of it is 1e-13 K of the magnitudes.  Plus 1e-12 of the quantity's
    # largest value: where a gate is all but saturated 1 - g g and o (1 - o) cancel in fp64 too, in the oracle and here alike, and a
    # gate gradient of 1e-17 of its neighbours carries an absolute error of their 1e-16)
    for q, g in got.items():
        v, b = want[q]
        err = np.abs(g - v)
        assert np.all(err <= 1e-6 * b + 1e-12 * np.abs(v).max()), (q, float(np.max(err / (1e-6 * b + 1e-12 * np.abs(v).max()))))


# ------------------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("mode", LC.MODES)
@pytest.mark.parametrize("name", ALL_BACKWARD)
def test_an_fp32_evaluation_of_the_backward_quantities_stays_inside_the_bounds(name, mode):
    case = LC.backward_case(name)
    x, buf = cpu_buffers(name)
    want = LR.backward_restated(case["layers"][case["hold"]], x, buf["DG"], buf["m"], buf["c"], case["S"], mode, LC.x_bounded(case))
    got = backward_fp32(case, mode, x, buf)
    worst = {q: LC.worst_ratio(got[q], *want[q]) for q in want}
    print(f"fp32 numpy / bound, {name} mode {mode}: " + ", ".join(f"{q} {v:.3f}" for q, v in worst.items()))
    assert all(v < 1.0 for v in worst.values()), worst
    # the inputs are what the module docstring of the cases says: DG is neither empty nor uniform
    DG = buf["DG"]
    nz = np.abs(DG[DG != 0])
    assert nz.size > DG.size // 8 and np.log2(float(nz.max()) / float(nz.min())) > 40
    live = LR.live_rows(case["lens"], case["S"], case["T"])
    assert not live.all() and not np.any(DG[~live]) and np.all(want["in_diff"][0][~live] == 0)


@pytest.mark.parametrize("mode", LC.MODES)
@pytest.mark.parametrize("name", ALL_FORWARD)
def test_an_fp32_evaluation_of_the_gates_stays_inside_the_bounds(name, mode):
    case = LC.forward_case(name)
    x = LC.held_input(case)
    val, bound, G, Gb = LR.gates_restated(case["layers"][case["hold"]], x, case["lens"], case["S"], case["T"], mode, LC.x_bounded(case))
    r = LC.worst_ratio(gates_fp32(case, mode, x), val, bound)
    live = LR.live_rows(case["lens"], case["S"], case["T"])
    mid = (np.abs(G[live]) > 0.25) & (np.abs(G[live]) < 4.0)
    print(f"fp32 numpy / bound, gates {name} mode {mode}: {r:.3f}; pre-activations in 0.25 < |G| < 4: {mid.mean():.3f}, log2 span "
          f"{np.log2(np.abs(G[live]).max() / np.abs(G[live][G[live] != 0]).min()):.0f}")
    assert r < 1.0
    assert mid.mean() > 0.03                       # a share of the gates is neither linear nor saturated
    if case["dropout"]:                            # the word 1.0 would overflow an fp16 plane: 2^14 |x| >= 65520
        assert np.abs(x).max() * 2.0 ** 14 >= 65520.0 and np.abs(x).max() <= 4.0


# ------------------------------------------------------------------------------------------------------------ (c)
def _factor(got, want_bound):
    r = LC.worst_ratio(got, *want_bound)
    return np.inf if np.isnan(r) else r


def _concerned(mutation, case, P, forward):
    """The quantities a mutation can reach in a case (empty: it does not apply there)."""
    nd, bounded, single = P["nd"], LC.x_bounded(case), case["hold"] == 0
    wm = [f"Wm_grad{d}" for d in range(nd)]
    if forward:
        return {"per_tensor_word": ["gates"], "wrong_axis": ["gates"], "stale_bound": ["gates"] if single else [], "drop_hi_lo": ["gates"],
                "drop_lo_planes": ["gates"], "no_bias": ["gates"], "fw_rows_for_bw": ["gates"] if nd == 2 else [],
                "word_for_measured": ["gates"] if case["dropout"] else []}.get(mutation, [])
    return {"per_tensor_word": ["in_diff", "Wx_grad"] + wm, "wrong_axis": ["in_diff", "Wx_grad"] + wm, "stale_bound": [] if bounded else ["Wx_grad"],
            "drop_hi_lo": ["in_diff", "Wx_grad"] + wm, "drop_lo_planes": ["in_diff", "Wx_grad"] + wm, "dir0_cols_for_dir1": wm[1:],
            "unshifted_m": wm, "peephole_shift_swapped": [f"peep_grad{d}" for d in range(nd)]}.get(mutation, [])


@pytest.mark.parametrize("mutation", LR.MUTATIONS)
def test_every_mutation_leaves_the_bounds(mutation):
    seen = 0
    for name in ALL_BACKWARD:
        case = LC.backward_case(name)
        L = case["layers"][case["hold"]]
        qs = _concerned(mutation, case, LR.unpack(L), False)
        if not qs:
            continue
        x, buf = cpu_buffers(name)
        want = LR.backward_restated(L, x, buf["DG"], buf["m"], buf["c"], case["S"], 2, LC.x_bounded(case))
        with np.errstate(over="ignore", invalid="ignore"):
            got = backward_fp32(case, 2, x, buf, mutation)
        fac = {q: _factor(got[q], want[q]) for q in qs}
        print(f"{mutation} {name}: error / bound " + ", ".join(f"{q} {v:.3g}" for q, v in fac.items()))
        assert all(v > 1.0 for v in fac.values()), (mutation, name, fac)
        seen += 1
    for name in ALL_FORWARD:
        case = LC.forward_case(name)
        L = case["layers"][case["hold"]]
        if not _concerned(mutation, case, LR.unpack(L), True):
            continue
        x = LC.held_input(case)
        val, bound, _, _ = LR.gates_restated(L, x, case["lens"], case["S"], case["T"], 2, LC.x_bounded(case))
        with np.errstate(over="ignore", invalid="ignore"):
            fac = _factor(gates_fp32(case, 2, x, mutation), (val, bound))
        print(f"{mutation} {name}: error / bound gates {fac:.3g}")
        assert fac > 1.0, (mutation, name, fac)
        seen += 1
    assert seen > 0, mutation


# ------------------------------------------------------------------------------------------------------------ the committed figures
def test_the_committed_mi355x_ratios_cover_every_case_and_stay_below_one():
    """profiles/lstm_gemms_fp64.json, as tests/test_gpu_lstm_gemms.py wrote it on an MI355X: every case, every quantity, every mode."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lstm_gemms_fp64.json")
    worst = json.load(open(path))["worst"]
    assert set(worst) == set(ALL_BACKWARD) | set(ALL_FORWARD)
    for name in ALL_BACKWARD:
        case = LC.backward_case(name)
        nd = LR.unpack(case["layers"][case["hold"]])["nd"]
        qs = {"Wx_grad", "b_grad"} | {f"{q}{d}" for q in ("Wm_grad", "peep_grad") for d in range(nd)} | ({"in_diff"} if case["hold"] == 0 else set())
        assert set(worst[name]) == qs, name
    for name in ALL_FORWARD:
        assert set(worst[name]) == {"gates", "gates above 2^-100"}, name
    for name, qs in worst.items():
        for q, modes in qs.items():
            assert set(modes) == {str(m) for m in LC.MODES} and all(0.0 <= r < 1.0 for r in modes.values()), (name, q, modes)
