"""-m gpu: the dense GEMMs and reductions AROUND an LSTM layer -- the input->gates GEMM in each of its schedules (whole; both ends and an
early middle; needed quadrants; gated under the recurrence below, gemm_f32_nt_gated, in its fp32, bf16-plane and fp16-plane forms), the
input gradient, the W_x and W_m gradients, lstm_bias_peep_pass1/2 -- under all three GEMM modes, with the operand bounds Net itself
chooses in csrc/net.cpp (measured per row / column, the backward direction's half of a vector, the word 1.0 behind an LSTM layer, a
fresh measurement behind forward dropout), held ELEMENT BY ELEMENT against the fp64 restatement of tests/lstm_gemm_restatement.py
within the rounding bound it derives for each element.  No element is excluded anywhere, padded rows included.

The intermediates come from the device through the read-only test hook eesen_net_debug_layer_buffer (Net.DebugLayerBuffer): the
backward quantities are restated from the gate gradients DG, the output m and the cell state c the device handed out, bit for bit, so
nothing of the recurrences' own rounding enters (tests/test_gpu_recurrence_*.py hold those); the forward GEMM is observed through the
gate activations of a layer whose W_m and peepholes are zero, behind the real recurrence kernel on the real schedule.  Nets and
inputs: tests/lstm_gemm_cases.py, shared with tests/test_lstm_gemm_restatement.py, which shows on the CPU that an fp32 evaluation
stays inside these bounds and that every listed mutation leaves them.  The bounds are derived, not measured; the only measured figures
are the worst error / bound ratios per (case, quantity, mode), written to lstm_gemms_fp64.json in $EESEN_PARITY_OUT (when set;
committed from an MI355X run as profiles/lstm_gemms_fp64.json) and asserted < 1."""
import json
import os

import numpy as np
import pytest

from tests import lstm_gemm_cases as LC
from tests import lstm_gemm_restatement as LR
from tests.test_gpu_layers import SENTINEL, _filled, _with_pads, hold

pytestmark = pytest.mark.gpu
EESEN_ERR_STATE = -3                    # include/eesen_hip.h


@pytest.fixture(scope="module")
def record():
    worst = {}

    def note(case, quantity, mode, ratio):
        assert ratio < 1.0, f"{case} {quantity} mode {mode}: worst error / bound {ratio:.3g}"
        q = worst.setdefault(case, {}).setdefault(quantity, {})
        q[str(mode)] = max(q.get(str(mode), 0.0), float(ratio))

    yield note
    out_dir = os.environ.get("EESEN_PARITY_OUT")
    if not out_dir:
        return
    try:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "lstm_gemms_fp64.json"), "w") as f:
            json.dump(dict(what="worst |HIP - fp64 restatement| / derived bound of the GEMMs and reductions around an LSTM layer, per case, "
                                "quantity and GEMM mode (0 fp32 MFMA, 1 three bf16 planes, 2 two fp16 planes)", worst=worst), f, indent=1)
    except OSError:
        pass


def fresh_net(case, gpu, mode, monkeypatch, env=None):
    """A Net of the case's layers, created under GEMM mode `mode` and the case's switches (read when the Net is created: tuning.h)."""
    from eesen_amd.api import Net
    assert gpu.eesen_set_gemm_mode(mode) == 0
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    net = Net.from_layers(case["layers"])
    for k in (env or {}):
        monkeypatch.delenv(k)
    net.SetSeqLengths(case["lens"])
    return net


def persistent_as_planned(net):
    """RecurrenceInfo() of the last passes against the plan: every LSTM layer whose plan names a persistent kernel ran on it, no recovery."""
    plan, info = net.Plan()["layers"], net.RecurrenceInfo()
    assert info["lstm_layers"] == len(plan) and net.recoveries == 0, info
    assert info["fwd_persistent"] == sum(bool(L["forward"]["persistent"]) for L in plan), (info, plan)
    return plan, info


# ------------------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("mode", LC.MODES)
@pytest.mark.parametrize("name", list(LC.BACKWARD) + list(LC.UPPER))
def test_backward_gemms_and_reductions_hold_every_element(gpu, record, monkeypatch, name, mode):
    from eesen_amd.api import CuMatrix
    case = LC.backward_case(name)
    layers, h, S, T, x = case["layers"], case["hold"], case["S"], case["T"], case["x"]
    rows, D = x.shape
    try:
        net = fresh_net(case, gpu, mode, monkeypatch)
        out = net.Propagate(x).numpy()
        in_diff = _filled(rows, D)
        net.BackpropagateNoUpdate(CuMatrix.from_numpy(case["d"]), in_diff)
        net.Synchronize()
        full = _with_pads(in_diff)
        DG, m, c = (net.DebugLayerBuffer(h, which) for which in (3, 2, 1))
        xa = LC.held_input(case, net.DebugLayerBuffer(0, 2) if h else None)
        grads = net.GetGrads()
        plan, info = persistent_as_planned(net)
        assert info["bwd_persistent"] == sum(bool(L["backward"]["persistent"]) for L in plan), (info, plan)
    finally:
        gpu.eesen_set_gemm_mode(-1)
    L = layers[h]
    nd, H = (2 if L["type"] == LC.BI else 1), L["output_dim"] // (2 if L["type"] == LC.BI else 1)
    assert DG.shape == (rows, nd * 4 * H) and m.shape == c.shape == (rows, nd * H) and xa.shape == (rows, L["input_dim"])
    assert np.all(full[:, D:].view(np.uint32) == SENTINEL.view(np.uint32)), "in_diff: a pad column was written"
    in_diff = np.ascontiguousarray(full[:, :D])
    for a in (out, in_diff, grads, DG, m, c):
        assert np.all(np.isfinite(a))
    assert np.array_equal(m.view(np.uint32), out.view(np.uint32))          # the hook's m IS the net's output (the held layer is the top one)
    live = LR.live_rows(case["lens"], S, T)
    dead = ~live | (np.arange(rows) % S == case["zero_seq"])               # padded frames, and the sequence whose gradient is zero
    assert not live.all() and np.all(DG[dead] == 0) and np.all(in_diff[dead] == 0) and np.all(m[~live] == 0) and np.all(c[~live] == 0)
    assert np.any(DG[:, nd * 4 * H - H:]) and np.any(DG[rows - S]) and np.count_nonzero(DG) > DG.size // 8    # ... and the buffer is DG, whole
    want = LR.backward_restated(L, xa, DG, m, c, S, mode, LC.x_bounded(case))
    n = sum(p.size for p in L["params"])
    got = LR.grads_by_quantity(L, grads[grads.size - n:])
    if h == 0:                # (behind a lower layer the held layer's input gradient is not handed out: the net's is the lower layer's)
        got["in_diff"] = in_diff
        assert np.all(got["Wx_grad"][:, case["zero_col"]] == 0)
    for q in sorted(got):
        record(name, q, mode, hold(got[q], *want[q], f"{name} mode {mode} {q}"))


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("mode", LC.MODES)
@pytest.mark.parametrize("name", list(LC.FORWARD) + list(LC.SINGLE))
def test_gate_input_gemm_holds_every_element_on_every_schedule(gpu, record, monkeypatch, name, mode):
    case = LC.forward_case(name)
    layers, h, S, T = case["layers"], case["hold"], case["S"], case["T"]
    try:
        net = fresh_net(case, gpu, mode, monkeypatch, case["env"])
        out = net.Propagate(case["x"]).numpy()
        net.Synchronize()
        gates, m = net.DebugLayerBuffer(h, 0), net.DebugLayerBuffer(h, 2)
        m_lower = net.DebugLayerBuffer(0, 2) if h else None
        mask = net.GetDropoutMasks(0, T, S)["fwd"] if case["dropout"] else None
        plan, info = persistent_as_planned(net)
    finally:
        gpu.eesen_set_gemm_mode(-1)
    if h:                     # the schedule the case is about, on persistent kernels
        assert info["fwd_persistent"] == 2, info
        sched = plan[1]["input_gemm"]
        assert (sched.startswith("gated") if case["plan"] == "gated" else case["plan"] in sched), sched
        assert ("needed quadrants" in sched) == (name == "quadrants")
    if case["dropout"]:
        assert mask is not None and set(np.unique(mask)) == {0.0, 4.0}
    assert np.all(np.isfinite(gates)) and np.all(np.isfinite(out))
    assert np.array_equal(m.view(np.uint32), out.view(np.uint32))          # (the held layer is the top one; no dropout on it)
    live = LR.live_rows(case["lens"], S, T)
    assert not live.all() and np.all(gates[~live] == 0)
    xa = LC.held_input(case, m_lower, mask)
    if case["dropout"]:       # the word 1.0 would overflow an fp16 plane here
        assert np.abs(xa).max() * 2.0 ** 14 >= 65520.0
    val, bound, G, _ = LR.gates_restated(layers[h], xa, case["lens"], S, T, mode, LC.x_bounded(case))
    mid = (np.abs(G[live]) > 0.25) & (np.abs(G[live]) < 4.0)
    assert mid.mean() > 0.03
    record(name, "gates", mode, hold(gates, val, bound, f"{name} mode {mode} gates"))
    # (the worst ratios of all sit at sigmoid(-87.4) ~ 2^-126, which the device flushes to 0 and the bound's FLUSH term allows: for the
    # record, the same figure over the gates that are not down there)
    big = np.abs(val) > 2.0 ** -100
    record(name, "gates above 2^-100", mode, LC.worst_ratio(gates[big], val[big], bound[big]))


# ------------------------------------------------------------------------------------------------------------ the hook itself
def test_the_hook_refuses_what_it_does_not_have(gpu):
    """EESEN_ERR_STATE: nothing propagated; not an LSTM layer; no Backpropagate since the last Propagate; a gate-gradient slot that a
    lower layer has reused (two slots alternate between the LSTM layers: of three layers the top one's is gone)."""
    from eesen_amd import synth
    from eesen_amd.api import CuMatrix, EesenError, Net
    cfg = dict(kind="BiLstmParallel", layers=3, H=32, D=8, K=5, S=3, T=6)
    layers = synth.make_model(**cfg)
    batch = synth.make_batch(min_frac=0.5, **cfg)
    net = Net.from_layers(layers)
    net.SetSeqLengths(batch.lens)

    def refused(layer, which):
        with pytest.raises(EesenError) as e:
            net.DebugLayerBuffer(layer, which)
        assert e.value.code == EESEN_ERR_STATE, e.value

    refused(0, 0)                                           # nothing propagated
    out = net.Propagate(batch.feats)
    refused(3, 0)                                           # the AffineTransform layer
    refused(0, 3)                                           # no Backpropagate yet
    assert net.DebugLayerBuffer(1, 0).shape == (18, 256) and net.DebugLayerBuffer(1, 1).shape == (18, 64)
    d = np.random.default_rng(3).standard_normal((18, 5)).astype(np.float32)
    net.BackpropagateNoUpdate(CuMatrix.from_numpy(d))
    refused(2, 3)                                           # layer 0 wrote the slot layer 2 had
    a, b = net.DebugLayerBuffer(1, 3), net.DebugLayerBuffer(0, 3)
    assert a.shape == b.shape == (18, 256) and np.any(a) and np.any(b) and not np.array_equal(a, b)
    net.Propagate(batch.feats)
    refused(1, 3)                                           # ... and a new Propagate retires them all
    net.RecurrenceInfo()
    assert out.NumRows() == 18 and net.recoveries == 0
