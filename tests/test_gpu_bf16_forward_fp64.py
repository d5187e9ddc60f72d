"""-m gpu: the "bf16 forward" variant (eesen_net_set_forward_precision(1 | 2); BASELINE config 4) held ELEMENT BY ELEMENT against an fp64
restatement, within the rounding bound derived for each element -- the one-product body of gemm_split_body (gemm.hip: bf16_store,
rne_bf16_bits, its own k loop; guarded and unguarded, on the main stream and as the side stream's early middle with its token of
extra LDS), which only Net::forward_pass reaches, and lstm_fwd_persistent_bf_kernel<CPW,4,1,2,false> for CPW = 1..4.  No element is
excluded anywhere, padded rows included.

The GEMM is observed through the gate activations of a layer whose W_m and peepholes are zero (tests/lstm_gemm_restatement.py:
gates_restated, with layer_restatement.gemm's bf16_operands form) and as an AffineTransform's output; the recurrence ONE STEP DEEP in m
and c, from the buffers the device itself hands out (Net.DebugLayerBuffer; tests/bf16_forward_restatement.py).  Nets and inputs:
tests/bf16_forward_cases.py, shared with tests/test_bf16_forward_restatement.py, which shows on the CPU that an fp32 evaluation stays
inside these bounds and that the listed faults leave them.  The bounds are derived, not measured; the only measured figures are the
worst error / bound ratios per (case, quantity, precision), written to bf16_forward_fp64.json in $EESEN_PARITY_OUT (when set; committed
from an MI355X run as profiles/bf16_forward_fp64.json) and asserted < 1.  Both directions of a BiLSTM layer are within reach: the recurrence cases at the four
tiles give both ordinary weights, and the cross-check -- the OTHER precision's restatement must miss -- is asserted per direction.

Every case runs under GEMM mode 0 and under the default mode: the variant does not look at the mode, so the two answers are the same
bits.  (Not asserted for the recurrence cases under precision 2: there the recurrence is the fp32-class one, whose planes ARE the
mode's; both answers are held.)"""
import json
import os

import numpy as np
import pytest

from tests import bf16_forward_cases as BC
from tests import bf16_forward_restatement as BR
from tests import layer_restatement as R
from tests import lstm_gemm_restatement as LR
from tests.layer_cases import affine_case
from tests.test_gpu_layers import hold

pytestmark = pytest.mark.gpu
GEMM_MODES = (0, -1)                    # fp32 MFMA; the library's default
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def record():
    worst = {}

    def note(case, quantity, precision, ratio, below=True):
        assert (ratio < 1.0) == below, f"{case} {quantity} precision {precision}: worst error / bound {ratio:.3g}"
        q = worst.setdefault(case, {}).setdefault(quantity, {})
        q[str(precision)] = (max if below else min)(q.get(str(precision), float(ratio)), float(ratio))      # (of the two GEMM modes' runs)

    yield note
    out_dir = os.environ.get("EESEN_PARITY_OUT")
    if not out_dir:
        return
    try:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "bf16_forward_fp64.json"), "w") as f:
            json.dump(dict(what="worst |HIP - fp64 restatement| / derived bound of the bf16 forward variant, per case, quantity and forward "
                                "precision (1: GEMMs and recurrence, 2: GEMMs only); 'direction d, other precision's restatement': the "
                                "cross-check on that direction's columns, asserted > 1", worst=worst), f, indent=1)
    except OSError:
        pass


def forward(gpu, layers, lens, x, precision, mode, held=(), env=None, quadrants=False):
    """A fresh Net under GEMM mode `mode` and the switches `env` (read when the Net is created: tuning.h), one Propagate: (net, output,
    {(layer, which): buffer}, plan, info).  quadrants: the one case whose plan is the "needed quadrants" schedule."""
    from eesen_amd.api import Net
    try:
        assert gpu.eesen_set_gemm_mode(mode) == 0
        with pytest.MonkeyPatch.context() as mp:
            for k, v in (env or {}).items():
                mp.setenv(k, v)
            net = Net.from_layers(layers)
        net.SetForwardPrecision(precision)
        net.SetSeqLengths(lens)
        out = net.Propagate(x).numpy()
        net.Synchronize()
        bufs = {k: net.DebugLayerBuffer(*k) for k in held}
        plan, info = net.Plan()["layers"], net.RecurrenceInfo()
        # the plan: persistent kernels wherever it names one, no recovery; the bf16 recurrence where bf_plan_shape admits it, under 1 only
        assert info["lstm_layers"] == len(plan) and net.recoveries == 0, info
        assert info["fwd_persistent"] == sum(bool(L["forward"]["persistent"]) for L in plan), (info, plan)
        assert net.Bf16RecurrenceLayers() == (BC.bf16_layers(layers) if precision == 1 else 0)
        scheds = [L.get("input_gemm", BC.WHOLE) for L in plan]
        assert not any(s.startswith("gated") for s in scheds) and any("needed quadrants" in s for s in scheds) == quadrants, scheds
        for L in plan:
            if L["cells"] % 256 == 0 and L["cells"] <= 1024:
                assert (L["forward"]["kernel"] == BC.kernel_row(L["cells"])) == (precision == 1), L
    finally:
        gpu.eesen_set_gemm_mode(-1)
    assert np.all(np.isfinite(out)) and all(np.all(np.isfinite(b)) for b in bufs.values())
    return net, out, bufs, plan, info


def in_both_modes(gpu, layers, lens, x, precision, held, same_bits=True, **kw):
    """forward() under GEMM mode 0 and under the default mode; the same bits from both."""
    runs = [forward(gpu, layers, lens, x, precision, mode, held, **kw) for mode in GEMM_MODES]
    if same_bits:
        assert np.array_equal(bits(runs[0][1]), bits(runs[1][1])), "the output depends on the GEMM mode"
        for k in held:
            assert np.array_equal(bits(runs[0][2][k]), bits(runs[1][2][k])), f"buffer {k} depends on the GEMM mode"
    return runs


def same_on_rounded_operands(net, layers, h, x, want, buf, round_x=True):
    """Idempotence: round_bf16 applied to the net's input and to the held layer's W_x (W) beforehand changes no bit.  round_x=False:
    an activation layer stands between the net's input and the GEMM, so only the weights are rounded."""
    layers_r, x_r = BC.rounded_operands(layers, h, x)
    net.SetParams(np.concatenate([np.asarray(p, np.float32).ravel() for L in layers_r for p in L["params"]]))
    out = net.Propagate(x_r if round_x else x).numpy()
    net.Synchronize()
    got = out if buf is None else net.DebugLayerBuffer(*buf)
    assert np.array_equal(bits(got), bits(want)), "operands already rounded to bf16 give other bits"


# ------------------------------------------------------------------------------------------------------------ the GEMM, through the gates
@pytest.mark.parametrize("name,precision", BC.GEMM_RUNS)
def test_gemm_through_the_gates_holds_every_element(gpu, record, name, precision):
    case = BC.gemm_case(name)
    layers, h, S, T, lens = case["layers"], case["hold"], case["S"], case["T"], case["lens"]
    held = [(h, 0), (h, 2)] + ([(0, 2)] if h else [])
    (net, out, bufs, plan, info), _ = in_both_modes(gpu, layers, lens, case["x"], precision, held, env=BC.GEMM_ENV.get(name),
                                                    quadrants=name == "quadrants")
    gates = bufs[(h, 0)]
    assert np.array_equal(bits(bufs[(h, 2)]), bits(out))                  # (the held layer is the top one)
    if h:                     # the schedule the case is about (bf16_forward_cases)
        assert plan[1]["input_gemm"] == BC.GEMM_PLAN[name][precision], plan[1]["input_gemm"]
    live = LR.live_rows(lens, S, T)
    assert not live.all() and np.all(gates[~live] == 0)
    xa = BC.held_input(case, bufs.get((0, 2)))
    val, bound, G, _ = LR.gates_restated(layers[h], xa, lens, S, T, 0, False, bf16_operands=True)
    mid = (np.abs(G[live]) > 0.25) & (np.abs(G[live]) < 4.0)
    assert mid.mean() > 0.03
    r = BC.worst_ratio(gates, val, bound)
    print(name, "precision", precision, "gates: worst error / bound", r)
    record(name, "gates", precision, hold(gates, val, bound, f"{name} precision {precision} gates"))
    big = np.abs(val) > 2.0 ** -100       # (for the record: without the sigmoids the device flushes to 0, inside the bound's 2^-126)
    record(name, "gates above 2^-100", precision, BC.worst_ratio(gates[big], val[big], bound[big]))
    same_on_rounded_operands(net, layers, h, case["x"], gates, (h, 0))


# ------------------------------------------------------------------------------------------------------------ the GEMM of an Affine layer
@pytest.mark.parametrize("precision", BC.PRECISIONS)
@pytest.mark.parametrize("name", BC.AFFINE_LAST)
def test_affine_layer_as_the_last_one_holds_every_element(gpu, record, name, precision):
    case = affine_case(name)
    layers, lens, front = case["layers"], case["lens"], case["front"]
    (net, out, _, _, _), _ = in_both_modes(gpu, layers, lens, case["x"], precision, [])
    xa = case["x"]
    if front:                 # the Affine layer's input, bit for bit: the same kernel on the same matrix gives the same bits
        xa = forward(gpu, layers[:1], lens, case["x"], precision, -1)[1]
        assert np.abs(xa[:, case["tiny"]]).max() <= 2.0 ** -20 and np.abs(xa).max() <= 1.0
    want = R.affine_forward(xa, case["W"], case["b"], 0, bf16_operands=True)
    print(name, "precision", precision, "out: worst error / bound", BC.worst_ratio(out, *want))
    record(f"affine:{name}", "out", precision, hold(out, *want, f"affine {name} precision {precision} out"))
    same_on_rounded_operands(net, layers, len(layers) - 1, case["x"], out, None, round_x=not front)


@pytest.mark.parametrize("precision", BC.PRECISIONS)
@pytest.mark.parametrize("name", BC.AFFINE_BEHIND)
def test_affine_layer_behind_an_lstm_layer_holds_every_element(gpu, record, name, precision):
    case = BC.affine_behind_case(name)
    layers, lens = case["layers"], case["lens"]
    (net, out, bufs, _, _), _ = in_both_modes(gpu, layers, lens, case["x"], precision, [(0, 2)])
    want = R.affine_forward(bufs[(0, 2)], case["W"], case["b"], 0, bf16_operands=True)
    print(name, "precision", precision, "out: worst error / bound", BC.worst_ratio(out, *want))
    record(f"lstm+affine:{name}", "out", precision, hold(out, *want, f"lstm + affine {name} precision {precision} out"))
    same_on_rounded_operands(net, layers, 1, case["x"], out, None)


# ------------------------------------------------------------------------------------------------------------ the recurrence, one step deep
@pytest.mark.parametrize("name", list(BC.RECURRENCE))
def test_recurrence_holds_every_element_one_step_deep(gpu, record, name):
    case = BC.recurrence_case(name)
    layers, S, T, lens, x = case["layers"], case["S"], case["T"], case["lens"], case["x"]
    held = [(0, 0), (0, 1), (0, 2)]
    live = LR.live_rows(lens, S, T)
    for precision in BC.PRECISIONS:
        runs = in_both_modes(gpu, layers, lens, x, precision, held, same_bits=precision == 1)
        for net, out, bufs, plan, info in (runs if precision == 2 else runs[:1]):
            got = dict(gates=bufs[(0, 0)], c=bufs[(0, 1)], m=bufs[(0, 2)])
            assert np.array_equal(bits(got["m"]), bits(out))
            assert (plan[0]["forward"]["kernel"] == case["row"]) == (precision == 1) and plan[0]["forward"]["persistent"], plan
            assert not live.all() and all(np.all(got[q][~live] == 0) for q in got)
            mine = BR.step_restated(layers[0], x, lens, S, T, got["m"], got["c"], rec_round=precision == 1)
            other = BR.step_restated(layers[0], x, lens, S, T, got["m"], got["c"], rec_round=precision != 1)
            for q in BR.QUANTITIES:
                record(name, q, precision, hold(got[q], *mine[q], f"{name} precision {precision} {q}"))
            big = np.abs(mine["gates"][0]) > 2.0 ** -100       # (for the record, as above: without the flushed sigmoids)
            record(name, "gates above 2^-100", precision, BC.worst_ratio(got["gates"][big], mine["gates"][0][big], mine["gates"][1][big]))
            # the cross-check, PER DIRECTION: the other precision's restatement is another function of that direction's recurrent
            # product, and the bounds notice -- in the forward chain's columns and in the backward chain's (not in a direction whose
            # weights are 2^-20: its product lies under the bounds' absolute terms either way)
            nd, H = (2 if case["kind"] == BC.BI else 1), case["H"]
            for dirn in range(nd):
                cols = lambda q: slice(dirn * (4 if q == "gates" else 1) * H, (dirn + 1) * (4 if q == "gates" else 1) * H)
                r = max(BC.worst_ratio(got[q][:, cols(q)], other[q][0][:, cols(q)], other[q][1][:, cols(q)]) for q in BR.QUANTITIES)
                print(name, "precision", precision, "direction", dirn, "against the other precision's restatement", r)
                if dirn != case["small"]:
                    record(name, f"direction {dirn}, other precision's restatement", precision, r, below=False)
        if precision == 1:
            same_on_rounded_operands(runs[0][0], layers, 0, x, runs[0][2][(0, 0)], (0, 0))
