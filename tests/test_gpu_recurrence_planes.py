"""-m gpu: the recurrences that hold their operands as two fp16 planes, against an fp64 layer, PER SEQUENCE, on inputs built to
stress the planes' power-of-two scales.

Two kernels multiply fp16 planes (three products per operand pair):
  lstm_fwd_persistent_bf_kernel<., ., 2, 2, true>   the forward recurrence of narrow and wide layers: W_m scaled by one power of
                                                    the layer's max |W_m|, m_t by a fixed 2^14
  lstm_bwd_persistent_ksplit_h_kernel               the backward recurrence of 1024-cell layers: the gate gradients scaled by their
                                                    producer, one power per (producer wave, sequence)
fp16 has 5 exponent bits, so what a scale is shared across decides whether a small operand keeps its low bits.  A sequence whose
gradients are 2^-24 of its neighbours' only shows in its own rows of in_diff: this module looks at every sequence on its own.

One LSTM layer is the whole Net; the test picks the top gradient `od`.  Reference: oracle.net.OracleNet(..., "f64") on the same
fp32 inputs.  Arms (a fresh Net each: the switches are read when a Net is created):
  P   the product path with EESEN_GEMM_MODE=f32 (the GEMMs' own planes: test_gpu_gemm.py; with the bounds Net chooses around an LSTM layer: test_gpu_lstm_gemms.py)
  Pd  the same with the default GEMM mode: the path that ships
  F   the same tiles and grids on the fp32-input MFMA (EESEN_FWD_SPLIT=0, EESEN_BWD_F16=0)
  S   the per-step fp32 kernels (EESEN_PERSISTENT=0)
Metric: rel_err (max-norm) and the p999 of err_metrics, per (sequence, direction) for the layer output and per sequence for in_diff,
each over that sequence's valid rows; rel_err per tensor for the gradients.  Bar, the rule test_gpu_gemm.py holds the GEMM's planes to:
  err_P <= max(1.5 * max(err_F, err_S), 4e-7)       max-norm of the output and of in_diff, per sequence
with two factors set by measurement (profiles/recurrence_planes.md, every case of this module, per-sequence power in ksplit_h):
  4 for the gradient tensors: the bias and peephole gradients sum a layer's gate gradients over every frame, and the planes' 22-bit
    operands leave them up to 3.1x the fp32 arms' distance to fp64 (1.0e-6 against 3.3e-7: bias_fw, 1024 cells, profile e; 2.9x
    bias_bw at S = 64, profile a); the weight gradients stay inside 1.5x
  3 for p999: within one sequence (<= 40 x 40 values above the floor) it is nearly the largest elementwise error; measured up to 2.3x
    (in_diff, 1024 cells, S = 64, profile c)
With ONE power per producer wave (the four sequences of a group sharing the largest one's), profile b put the 2^-24 sequences of
every 1024-cell shape at 14-35x the bar's reference on max-norm and up to 97x on p999.
Pd is recorded, not held to the bar: its GEMMs add their own planes, bounded per sum |a||b| in test_gpu_gemm.py.
A sequence whose `od` is zero has an in_diff of exact zeros.  Every number goes to $EESEN_PARITY_OUT/recurrence_planes.json.

Magnitude profiles (od: the top gradient; weights: synth.make_model unless named):
  a  baseline: od ~ N(0, 1) on valid rows, 0 on padding
  b  confident neighbours: in every aligned group of four sequences (a producer wave's group) od scaled by 1, 2^-8, 2^-16, 2^-24;
     every other group holds one sequence whose od is zero
  c  spread over time: row (t, s) of od scaled by 2^-u, u ~ U[0, 24]
  d  unbalanced W_m: one direction's W_m and W_x scaled by 2^-20, bias 0 ("dir"); one gate block of one direction the same way
     ("gate": the cell input g, whose tanh passes a small pre-activation straight through)
  e  tiny state: zero bias and inputs so small that |m_t| ~ 2^-20 ("tiny")
  f  range ends: max |W_m| near 1e4 ("big") and near 1e-30 ("small"): finite, and on "small" no value the fp32 arm keeps flushed to
     zero.  "big" is held to finiteness only: its gates saturate with a gain of ~1e4 per step, so the layer amplifies any rounding
     difference -- F and S themselves end 2e-3 from fp64 (max-norm of the output), and the planes' 22-bit operands flip saturated units.
Profiles e and the "gate" block of d cannot see the planes through the output: fp32's tanh of a pre-activation near 2^-20 (the
(e^2x - 1) / (e^2x + 1) form every arm shares with the reference) is itself 18-28 % off, and the bar is calibrated by those arms.
"""
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from eesen_amd import synth
from tests.util import err_metrics, rel_err, split_params, valid_mask

pytestmark = pytest.mark.gpu
# name -> (layer kind, cells, sequences, frames, the backward kernel the width selects).  Each is confirmed by Plan() below.
SHAPES = {
    "bi512_s32": ("BiLstmParallel", 512, 32, 24, None),          # narrow forward plane tile
    "bi320_s10": ("BiLstmParallel", 320, 10, 30, None),          # the recipes' shape
    "bi320_s20": ("BiLstmParallel", 320, 20, 30, None),
    "bi1024_s32": ("BiLstmParallel", 1024, 32, 16, "ksplit_h"),  # wide forward plane tile, ksplit_h
    "bi1024_s24": ("BiLstmParallel", 1024, 24, 16, "ksplit_h"),  # ragged last sequence tile
    "bi1024_s64": ("BiLstmParallel", 1024, 64, 12, "ksplit_h"),  # ksplit_h in two windows
    "uni1024_s48": ("LstmParallel", 1024, 48, 16, "ksplit_h"),   # one direction (at S = 32 the one-direction grid takes the 16 x 16 tile)
}
# weights -> the od profiles run on them
WEIGHTS = {"synth": ("a", "b", "c"), "dir": ("a",), "gate": ("a",), "tiny": ("a",), "big": ("a",), "small": ("a",)}
CASES = [("bi512_s32", w) for w in WEIGHTS] + [("bi320_s10", "synth"), ("bi320_s20", "synth")] + \
        [("bi1024_s32", w) for w in WEIGHTS] + [("bi1024_s24", "synth"), ("bi1024_s64", "synth"),
                                                ("uni1024_s48", "synth"), ("uni1024_s48", "gate")]
D = 40
ARM_ENV = {
    "P": {"EESEN_GEMM_MODE": "f32"},
    "Pd": {},
    "F": {"EESEN_GEMM_MODE": "f32", "EESEN_FWD_SPLIT": "0", "EESEN_BWD_F16": "0"},
    "S": {"EESEN_GEMM_MODE": "f32", "EESEN_PERSISTENT": "0"},
}
SWITCHES = sorted({k for e in ARM_ENV.values() for k in e})


# factor on max(err_F, err_S) per metric (see the module docstring for the measurements behind the last two)
FACTOR = {"maxnorm": 1.5, "grad": 4.0, "p999": 3.0}


def bar(err_f, err_s, factor=1.5):
    return max(factor * max(err_f, err_s), 4e-7)


def _case(shape, weights):
    """(layers, Batch, [(profile, od)], zero_seqs) of one case: deterministic."""
    kind, H, S, T, _ = SHAPES[shape]
    cfg = dict(kind=kind, layers=1, H=H, D=D, K=4, S=S, T=T)
    layers = synth.make_model(**cfg)[:1]; batch = synth.make_batch(**cfg)
    L = layers[0]; nd = 2 if kind.startswith("Bi") else 1
    p = [np.array(a, np.float32) for a in L["params"]]   # per direction: Wx [4H, D], Wm [4H, H], bias [4H], peepholes [H] x 3
    if weights == "dir":     # the last direction: W_x, W_m 2^-20, bias 0
        d = nd - 1
        p[6 * d] *= np.float32(2.0 ** -20); p[6 * d + 1] *= np.float32(2.0 ** -20); p[6 * d + 2][:] = 0.0
    elif weights == "gate":  # direction 0, gate block 0 (g): its rows of W_x, W_m 2^-20, bias 0
        p[0][:H] *= np.float32(2.0 ** -20); p[1][:H] *= np.float32(2.0 ** -20); p[2][:H] = 0.0
    elif weights == "tiny":  # zero bias, inputs 2^-20 of the baseline's: |m_t| ~ 2^-20
        for d in range(nd):
            p[6 * d + 2][:] = 0.0
        batch.feats[:] *= np.float32(2.0 ** -20)
    elif weights in ("big", "small"):
        target = 1e4 if weights == "big" else 1e-30
        for d in range(nd):
            p[6 * d + 1] = (p[6 * d + 1] * np.float32(target / float(np.abs(p[6 * d + 1]).max()))).astype(np.float32)
    L["params"] = p
    vm = valid_mask(batch.lens, T, S)
    rng = np.random.default_rng(H * 131 + S * 7 + T)
    base = rng.standard_normal((T * S, nd * H)).astype(np.float32)
    base[~vm] = 0.0
    ods, zero = [], []
    for prof in WEIGHTS[weights]:
        od = base.copy().reshape(T, S, nd * H)
        if prof == "b":
            od *= (2.0 ** (-8.0 * (np.arange(S) % 4))).astype(np.float32)[None, :, None]
            zero = [4 * g + 1 for g in range(S // 4) if g % 2 == 1]
            od[:, zero, :] = 0.0
        elif prof == "c":
            od *= np.exp2(-rng.uniform(0.0, 24.0, (T, S, 1))).astype(np.float32)
        ods.append((prof, od.reshape(T * S, nd * H)))
    return layers, batch, ods, zero


def _oracle(shape, weights):
    from oracle import net as onet
    layers, batch, ods, _ = _case(shape, weights)
    ora = onet.OracleNet(layers, "f64"); ora.set_train_options(1.0, 0.0); ora.set_seq_lengths(batch.lens)
    out = ora.propagate(batch.feats)
    res = []
    for _, od in ods:
        in_diff = ora.backpropagate(od, update=False)
        res.append((in_diff, ora.fresh_grads_flat()))
    return out, res


@pytest.fixture(scope="module")
def oracles(request):
    """The fp64 layers of every selected case, computed on a thread pool (the C oracle releases the GIL) while the GPU arms run."""
    ids = [it.callspec.params["case"] for it in request.session.items
           if it.module.__name__ == __name__ and hasattr(it, "callspec") and "case" in it.callspec.params]
    pool = ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1))
    futs = {c: pool.submit(_oracle, *c) for c in dict.fromkeys(ids)}
    yield futs
    pool.shutdown(wait=False, cancel_futures=True)


@pytest.fixture(scope="module")
def report():
    rows = []
    yield rows.append
    out = os.environ.get("EESEN_PARITY_OUT")   # (the per-case summary of a run is profiles/recurrence_planes.md)
    if not out:
        return
    try:
        os.makedirs(out, exist_ok=True)
        json.dump(rows, open(os.path.join(out, "recurrence_planes.json"), "w"), indent=1)
    except OSError:
        pass


def _arm(monkeypatch, arm, layers, batch, ods):
    from eesen_amd.api import Net, CuMatrix
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in ARM_ENV[arm].items():
        monkeypatch.setenv(k, v)
    net = Net.from_layers(layers)
    out, back = None, []
    for _, od in ods:
        net.SetSeqLengths(batch.lens)
        out = net.Propagate(batch.feats).numpy()
        idf = CuMatrix(batch.T * batch.S, D)
        net.BackpropagateNoUpdate(CuMatrix.from_numpy(od), idf)
        back.append((idf.numpy(), net.GetGrads()))
    info = net.RecurrenceInfo()
    plan = net.Plan()                  # (after a Propagate: the forward plan depends on the layer's input being there)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return plan, info, net.recoveries, out, back


@pytest.mark.parametrize("case", CASES, ids=[f"{s}-{w}" for s, w in CASES])
def test_plane_recurrences_hold_fp32_accuracy_per_sequence(gpu, oracles, report, monkeypatch, case):
    shape, weights = case
    kind, H, S, T, bwd_kernel = SHAPES[shape]
    layers, batch, ods, zero = _case(shape, weights)
    nd = 2 if kind.startswith("Bi") else 1
    arms = {a: _arm(monkeypatch, a, layers, batch, ods) for a in ARM_ENV}

    # what ran: P (and Pd) on the plane kernels, F on the same tiles without them, both persistent throughout; S per step
    for a in ("P", "Pd", "F"):
        plan, info, rec = arms[a][:3]
        fk, bk = plan["layers"][0]["forward"]["kernel"], plan["layers"][0]["backward"]["kernel"]
        assert info["fwd_persistent"] == info["bwd_persistent"] == info["lstm_layers"] == 1 and rec == 0, (a, info, rec)
        planes = fk.startswith("lstm_fwd_persistent_bf_kernel<") and fk.endswith(",true>")
        if a == "F":
            assert not planes and "ksplit_h" not in bk, (a, fk, bk)
        else:
            assert planes, (a, fk)
            assert bwd_kernel is None or bwd_kernel in bk, (a, bk)
    if bwd_kernel:
        assert "ksplit" in arms["F"][0]["layers"][0]["backward"]["kernel"]   # the same K-split tiles on the fp32-input MFMA
    assert arms["S"][0]["layers"][0]["forward"]["persistent"] is False

    want_out, want_back = oracles[case].result()
    vm = valid_mask(batch.lens, T, S).reshape(T, S)
    fails = []

    def check(quantity, index, got, ref):
        e = {a: rel_err(g, ref) for a, g in got.items()}
        p = {a: err_metrics(g, ref)["p999"] for a, g in got.items()}
        report(dict(case=f"{shape}-{weights}", quantity=quantity, index=index,
                    **{f"err_{a}": e[a] for a in e}, **{f"p999_{a}": p[a] for a in p}))
        if weights == "big":       # chaotic at max |W_m| = 1e4 (docstring): finiteness and no flush only
            return
        grad = quantity.startswith("grad")
        for name, m, f in (("maxnorm", e, FACTOR["grad" if grad else "maxnorm"]),) + ((("p999", p, FACTOR["p999"]),) if not grad else ()):
            b = bar(m["F"], m["S"], f)
            if m["P"] > b:
                fails.append(f"{quantity}[{index}] {name} {m['P']:.3g} > bar {b:.3g} (F {m['F']:.3g}, S {m['S']:.3g}, Pd {m['Pd']:.3g})")

    outs = {a: arms[a][3].reshape(T, S, nd * H) for a in arms}
    wo = want_out.reshape(T, S, nd * H)
    for s in range(S):
        for d in range(nd):
            sl = slice(d * H, (d + 1) * H)
            check("out", f"s{s}/d{d}", {a: outs[a][vm[:, s], s, sl] for a in arms}, wo[vm[:, s], s, sl])
    for k, (prof, od) in enumerate(ods):
        want_in, want_g = want_back[k]
        ins = {a: arms[a][4][k][0].reshape(T, S, D) for a in arms}
        wi = want_in.reshape(T, S, D)
        for s in range(S):
            check(f"in_diff/{prof}", f"s{s}", {a: ins[a][vm[:, s], s] for a in arms}, wi[vm[:, s], s])
        if prof == "b":
            for a in arms:                  # a sequence without a top gradient gets none below it
                assert all(np.all(ins[a][:, s] == 0.0) for s in zero), (a, zero)
        gs = {a: dict(((n, v) for _, n, v in split_params(layers, arms[a][4][k][1]))) for a in arms}
        for _, n, ref in split_params(layers, want_g):
            check(f"grad/{prof}", n, {a: gs[a][n] for a in arms}, ref)
        for a in arms:
            assert np.isfinite(arms[a][4][k][0]).all() and np.isfinite(arms[a][4][k][1]).all(), a
        if weights == "small":              # nothing the fp32 arm keeps is flushed to zero on the planes
            for a in ("P", "Pd"):
                for q in (0, 1):
                    f, g = arms["F"][4][k][q], arms[a][4][k][q]
                    assert np.all((f == 0) | (g != 0)), (a, q)
    for a in arms:
        assert np.isfinite(arms[a][3]).all(), a
    assert not fails, f"{len(fails)} over the bar:\n" + "\n".join(fails[:24])
