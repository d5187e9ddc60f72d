"""net.cpp "only the needed quadrants first" (EESEN_FWD_QUAD): in front of a forward recurrence the main stream computes only the
gate-input rows the two chains read first -- rows [0, r0) of the forward columns, rows [r1, rows) of the backward columns --, the
other two quadrants follow on the side stream behind the middle rows, and the narrow forward kernel waits for them at a row guard
(LstmLayerDev::guard).  Every element of G is the same dot product from the same kernel: with the switch on and off one Propagate ->
CTC -> Backpropagate must agree BIT FOR BIT in the network output, the input gradient and every parameter gradient.  (The gradients
are functions of every layer's gate activations, which overwrite G.  That the schedules are RIGHT, not only equal -- every gate held
against an fp64 restatement through the gate buffer eesen_net_debug_layer_buffer hands out -- is tests/test_gpu_lstm_gemms.py.)

Shapes: 3-layer BiLSTM, D = 8, K = 5.  (H, S, T) = (64, 32, 33) is listed in the issue as "middle empty"; at that shape the middle is
rows [256, 768) of 1056 -- not empty -- so the schedule applies there and the case checks it as one more unequal split; (64, 4, 33)
is the shape whose middle IS empty (r0 = 256 > r1 = 0) and stands for the fall-back the issue asks for.
"""
import numpy as np
import pytest

from eesen_amd import synth

pytestmark = pytest.mark.gpu

QUAD = "needed quadrants"
ENDS = "both ends"
WHOLE = "whole, recurrence"


def middle(S, T):
    """rows [r0, r1) of the next layer's input GEMM that run under the end of a recurrence (net.cpp: fwd_early); (0, 0): none"""
    m = 3 * T // 4
    r0 = ((T - 1 - m) * S + 255) // 256 * 256
    r1 = (m + 1) * S // 256 * 256
    return (r0, r1) if T >= 32 and m + 1 < T and r1 > r0 else (0, 0)


def one_step(layers, batch, quad, monkeypatch, steps=1):
    from eesen_amd.api import Net, Ctc, CuMatrix
    monkeypatch.setenv("EESEN_FWD_QUAD", quad)
    net = Net.from_layers(layers); net.SetTrainOptions(1e-3, 0.9); ctc = Ctc()
    monkeypatch.delenv("EESEN_FWD_QUAD")
    res = []
    for _ in range(steps):
        net.SetSeqLengths(batch.lens)
        out = net.Propagate(batch.feats)
        diff = ctc.EvalParallel(batch.lens, out, batch.labels)
        in_diff = CuMatrix(out.NumRows(), net.InputDim())
        net.BackpropagateNoUpdate(diff, in_diff)
        res.append((out.numpy(), in_diff.numpy(), net.GetGrads()))
    info = net.RecurrenceInfo()
    assert info["fwd_persistent"] == info["lstm_layers"] == sum(1 for L in net.Plan()["layers"]) and net.recoveries == 0, info
    plan = net.Plan()["layers"]
    return res, [L.get("input_gemm") for L in plan], [L["forward"]["kernel"] for L in plan]   # (the key exists behind an LSTM layer)


CASES = [
    # H, S, T, kind, expected schedule of the upper layers with the switch on
    pytest.param(64, 32, 64, "BiLstmParallel", QUAD, id="aligned"),
    pytest.param(64, 32, 37, "BiLstmParallel", QUAD, id="ends-differ"),
    pytest.param(64, 20, 48, "BiLstmParallel", QUAD, id="partial-sequence-tile"),
    pytest.param(512, 32, 128, "BiLstmParallel", QUAD, id="workload-instantiation"),
    pytest.param(64, 32, 33, "BiLstmParallel", QUAD, id="T33-issue-shape"),
    pytest.param(64, 4, 33, "BiLstmParallel", WHOLE, id="middle-empty"),
    pytest.param(64, 32, 64, "LstmParallel", WHOLE, id="unidirectional"),
]


@pytest.mark.parametrize("H,S,T,kind,want", CASES)
def test_quadrant_schedule_is_bit_identical(gpu, monkeypatch, H, S, T, kind, want):
    cfg = dict(kind=kind, layers=3, H=H, D=8, K=5, S=S, T=T)
    layers = synth.make_model(**cfg)
    batch = synth.make_batch(min_frac=0.5, **cfg)
    r0, r1 = middle(S, T)
    assert (r1 > r0) == (want == QUAD or kind == "LstmParallel"), (r0, r1)
    if want == QUAD:
        assert 0 < r0 < r1 < T * S
    off, sched_off, _ = one_step(layers, batch, "0", monkeypatch)
    on, sched_on, kernels = one_step(layers, batch, "1", monkeypatch, steps=2)
    # the plan key: layer 0 has nothing below it; the upper layers take the new schedule exactly where the rule says, today's otherwise
    today = ENDS if (r1 > r0 and kind == "BiLstmParallel") else WHOLE
    assert sched_off[0] is None and sched_on[0] is None
    assert all(today in s and QUAD not in s for s in sched_off[1:]), sched_off
    assert all(want in s for s in sched_on[1:]), sched_on
    if H == 512:
        assert kernels[1] == kernels[2] == "lstm_fwd_persistent_bf_kernel<2,2,2,2,true>", kernels
    for step in on:     # (the second step reuses the guard words of the first)
        for name, a, b in zip(("output", "input gradient", "parameter gradients"), step, off[0]):
            assert np.all(np.isfinite(a)), name
            assert np.array_equal(a, b), (name, float(np.abs(a - b).max()))
    assert np.abs(off[0][2]).max() > 0


def test_recovery_from_a_timed_out_kernel_on_the_quadrant_schedule(gpu, monkeypatch, capfd):
    """EESEN_SPIN_LIMIT=0: every bounded wait of the forward kernels -- the row guards among them -- gives up at once.  As for any
    timed-out persistent kernel the step is dropped on the device, the parameters stay what they were, and the Net goes on: the next
    steps equal those of a Net that never took the schedule, from the same parameters."""
    from eesen_amd.api import Net, Ctc
    cfg = dict(kind="BiLstmParallel", layers=3, H=64, D=8, K=5, S=32, T=64)
    layers = synth.make_model(max_grad=1.0, **cfg)
    batch = synth.make_batch(min_frac=0.5, **cfg)

    def step(net, ctc):
        net.SetSeqLengths(batch.lens)
        out = net.Propagate(batch.feats)
        diff = ctc.EvalParallel(batch.lens, out, batch.labels)
        net.Backpropagate(diff)

    monkeypatch.setenv("EESEN_SPIN_LIMIT", "0")
    monkeypatch.setenv("EESEN_FWD_QUAD", "1")
    bad = Net.from_layers(layers); bad.SetTrainOptions(1e-3, 0.9); cb = Ctc()
    monkeypatch.delenv("EESEN_SPIN_LIMIT")
    good = Net.from_layers(layers)                 # (the plan of this shape, from a Net whose buffers exist: after a Propagate)
    good.SetSeqLengths(batch.lens); good.Propagate(batch.feats)
    assert all(QUAD in L["input_gemm"] for L in good.Plan()["layers"][1:])
    p0 = bad.GetParams()
    step(bad, cb)                                  # the kernels give up: update skipped on the device
    assert np.array_equal(bad.GetParams(), p0)     # (GetParams synchronises: the host notices and falls back here)
    bad.RecurrenceInfo()
    assert bad.recoveries == 1
    assert "NOT applied" in capfd.readouterr().err
    step(bad, cb)                                  # ... and goes on
    p1 = bad.GetParams()
    assert bad.RecurrenceInfo()["fwd_persistent"] == 0 and bad.recoveries == 1
    assert np.all(np.isfinite(p1)) and not np.array_equal(p1, p0)
    monkeypatch.setenv("EESEN_PERSISTENT", "0")
    ref = Net.from_layers(layers); ref.SetTrainOptions(1e-3, 0.9); cr = Ctc()
    step(ref, cr)
    assert np.array_equal(p1, ref.GetParams())
