"""-m gpu: the recurrent-dropout recurrences, at every tile they ship in, against an fp64 layer, PER SEQUENCE.

With recurrent dropout on, rec_plan.cpp sends a BiLSTM layer to the DROP = true instantiations of lstm_fwd_persistent_kernel and
lstm_bwd_persistent_kernel (the plane, 4 x 32, K-split and multiplexed tiles refuse drop_mode): 8 forward and 10 backward rows of
the kernel table.  tests/test_gpu_dropout.py reaches three of them, at 32 cells and below, behind a whole net and its CTC; here every
row runs alone.  tests/dropout_cases.py holds the case table -- shape, the rows rec_plan.cpp takes there on a whole 256-CU device,
recipes -- and the input generators; tests/test_dropout_cases.py holds, without a GPU, that the table covers the rows and that the
inputs are what this module assumes.

One BiLstmParallel layer (40 inputs) is the whole Net; the test picks the top gradient `od`.  Masks are injected (they are one-shot:
injected again before every Propagate), identical for every arm and the oracle.  Arms, a fresh Net each:
  Dp  default switches: the persistent dropout rows.  Plan() must name exactly the case's two rows and its launches per pass, with
      fwd_persistent == bwd_persistent == 1 and no recovery
  Ds  EESEN_PERSISTENT=0: the per-step kernels of lstm.hip and their drop_mode branches
  N   the same layer and lengths WITHOUT dropout on the DROP = false rows of the same families (the plane, 4 x 32 and K-split tiles
      switched off; EESEN_FWD_MUX=0 as well, or the two windows of bi1024_s64 would run as one multiplexed launch of another kernel)
EESEN_GEMM_MODE=f32 in all three (the GEMMs' planes: test_gpu_gemm.py; with the bounds Net chooses around an LSTM layer: test_gpu_lstm_gemms.py).
Reference: oracle.net.OracleNet(layers, "f64") with the same masks, computed on a thread pool while the GPU arms run.

Accuracy, per sequence over its valid rows: rel_err (max-norm) and the p999 of err_metrics of the output per (sequence, direction)
and of in_diff per sequence; rel_err per gradient tensor.  Yardstick of a quantity: the larger of
  (i)  the fp32 oracle with the same masks against the fp64 layer (the reference's own arithmetic in fp32)
  (ii) arm N against ITS fp64 layer (no dropout)
each the worst over the case's sequences; neither is code under test.  Bar: max(factor * yardstick, 4e-7) with the factors of
tests/test_gpu_recurrence_planes.py (1.5 max-norm, 3 p999, 4 gradient tensors).  Dp and Ds are each held to it; no case is exempt.
Exact: padding rows of the output and of in_diff are zero; a sequence whose od is zero has an in_diff of zeros; under RNNDrop the
output is exactly 0.0 wherever the mask is 0 (c = 0 there, so tanh(c) * o = 0); two runs of Dp give the same bits; all is finite.
bi512_s64-generated is the production path: the masks are drawn on the device (SetDropoutSeed), read back (GetDropoutMasks: only
the values 0 and 1 / (1 - p) over all (T + 2) * S rows) and replayed through the oracles and the other arms.

od profiles: "a" N(0, 1) on valid rows; "b" in every aligned group of four sequences scaled by 1, 2^-8, 2^-16, 2^-24, and every other
group holds one sequence whose od is zero.  Every figure goes to $EESEN_PARITY_OUT/recurrence_dropout.json; the record of the first
run on the device is profiles/recurrence_dropout.json (.md).
"""
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import dropout_cases as dc
from tests.util import rel_err, split_params

pytestmark = pytest.mark.gpu
_OFF = {"EESEN_FWD_SPLIT": "0", "EESEN_FWD_F16": "0", "EESEN_BWD_Q4": "0", "EESEN_BWD_KSPLIT": "0", "EESEN_BWD_F16": "0", "EESEN_FWD_MUX": "0"}
ARM_ENV = {
    "Dp": {"EESEN_GEMM_MODE": "f32"},
    "Ds": {"EESEN_GEMM_MODE": "f32", "EESEN_PERSISTENT": "0"},
    "N": {"EESEN_GEMM_MODE": "f32", **_OFF},
}
SWITCHES = sorted({k for e in ARM_ENV.values() for k in e})
FACTOR = {"maxnorm": 1.5, "p999": 3.0, "grad": 4.0}
FLOOR = 4e-7
SEED = 5


def bar(yardstick, factor):
    return max(factor * yardstick, FLOOR)


def _inputs(case):
    lens = dc.lengths(case)
    ods, zero = dc.top_gradients(case, lens)
    return lens, dc.features(case, lens), ods, zero


def _oracle(case, recipe, prec, mk=None):
    """recipe None: the no-dropout twin's layer."""
    lens, x, ods, _ = _inputs(case)
    if recipe and mk is None:
        mk = dc.masks(case, recipe)
    return dc.oracle_run(dc.layer(case, recipe), x, lens, ods, prec, mk)


@pytest.fixture(scope="module")
def pool():
    p = ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1))
    yield p
    p.shutdown(wait=False, cancel_futures=True)


@pytest.fixture(scope="module")
def oracles(request, pool):
    """(case, recipe | None, precision) -> future of the oracle layer of every selected case, in the order the cases run (the C
    oracle releases the GIL): fp64 and fp32 with the case's masks, fp64 without dropout once per shape."""
    sel = [it.callspec.params["variant"] for it in request.session.items
           if it.module.__name__ == __name__ and hasattr(it, "callspec") and "variant" in it.callspec.params]
    futs = {}
    for case, recipe in dict.fromkeys(sel):
        for key in ((case, recipe, "f64"), (case, recipe, "f32"), (case, None, "f64")):
            if key not in futs and key[1] != "generated":
                futs[key] = pool.submit(_oracle, *key)
    return futs


@pytest.fixture(scope="module")
def report():
    rows = []
    yield rows.append
    out = os.environ.get("EESEN_PARITY_OUT")
    if not out:
        return
    try:
        os.makedirs(out, exist_ok=True)
        json.dump(rows, open(os.path.join(out, "recurrence_dropout.json"), "w"), indent=1)
    except OSError:
        pass


def _arm(monkeypatch, arm, case, recipe, mk, generate=False):
    """One fresh Net through Propagate and Backpropagate for every od.  generate: the first Propagate draws its masks on the device;
    they are read back into `mk` (and injected from then on).  Returns (plan, info, recoveries, out, [(in_diff, grads) per od])."""
    from eesen_amd.api import Net, CuMatrix
    c = dc.CASES[case]; S, T = c["S"], c["T"]
    lens, x, ods, _ = _inputs(case)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in ARM_ENV[arm].items():
        monkeypatch.setenv(k, v)
    net = Net.from_layers(dc.layer(case, None if arm == "N" else recipe))
    if generate:
        net.SetDropoutSeed(SEED)
    out, back = None, []
    for k, (_, od) in enumerate(ods):
        if arm != "N" and not (generate and k == 0):
            net.SetDropoutMasks(0, fwd=mk["fwd"], rec=mk["rec"])
        net.SetSeqLengths(lens)
        o = net.Propagate(x).numpy()
        if generate and k == 0:
            got = net.GetDropoutMasks(0, T, S)
            assert got["mode"] == 2 and got["fwd"] is None and got["rec"].shape == ((T + 2) * S, 2 * c["H"])
            mk.update(fwd=None, rec=got["rec"])
        assert out is None or np.array_equal(o, out), (arm, "the same masks gave another output")
        out = o
        idf = CuMatrix(T * S, dc.D)
        net.BackpropagateNoUpdate(CuMatrix.from_numpy(od), idf)
        back.append((idf.numpy(), net.GetGrads()))
    info = net.RecurrenceInfo()
    plan = net.Plan()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return plan, info, net.recoveries, out, back


@pytest.mark.parametrize("variant", dc.VARIANTS, ids=dc.IDS)
def test_dropout_recurrences_hold_fp32_accuracy_per_sequence(gpu, oracles, pool, report, monkeypatch, variant):
    case, recipe = variant
    c = dc.CASES[case]; H, S, T = c["H"], c["S"], c["T"]
    lens, x, ods, zero = _inputs(case)
    generated = recipe == "generated"
    mk = {} if generated else dc.masks(case, recipe)
    arms = {"Dp": _arm(monkeypatch, "Dp", case, recipe, mk, generate=generated)}
    if generated:      # the production path: the masks the device drew take only the two values, over every row; replay them
        kept = np.float32(1.0 / (1.0 - dc.P_REC))
        assert set(np.unique(mk["rec"])) == {np.float32(0), kept}
        assert abs((mk["rec"] > 0).mean() - (1 - dc.P_REC)) < 0.01
        want = {p: pool.submit(_oracle, case, recipe, p, mk) for p in ("f64", "f32")}
    else:
        want = {p: oracles[(case, recipe, p)] for p in ("f64", "f32")}
    arms["Dp2"] = _arm(monkeypatch, "Dp", case, recipe, mk)
    arms["Ds"] = _arm(monkeypatch, "Ds", case, recipe, mk)
    arms["N"] = _arm(monkeypatch, "N", case, recipe, mk)

    # what ran
    for a in ("Dp", "Dp2", "N"):
        plan, info, rec = arms[a][:3]
        f, b = plan["layers"][0]["forward"], plan["layers"][0]["backward"]
        print(f"{case}-{recipe} {a}: forward {f['kernel']} x{f['launches']}, backward {b['kernel']} x{b['launches']}")
        assert info["fwd_persistent"] == info["bwd_persistent"] == info["lstm_layers"] == 1 and rec == 0, (a, info, rec)
        if a == "N":   # the DROP = false rows of the same two families, the same tiles
            assert f["kernel"].startswith(dc.fwd_row(case).replace("true,false>", "false,")), (a, f["kernel"])
            assert b["kernel"] == dc.bwd_row(case).replace("true>", "false>"), (a, b["kernel"])
        else:
            assert f["kernel"] == dc.fwd_row(case) and b["kernel"] == dc.bwd_row(case), (a, f["kernel"], b["kernel"])
        assert f["launches"] == b["launches"] == c["launches"], (a, f["launches"], b["launches"])
    assert arms["Ds"][0]["layers"][0]["forward"]["persistent"] is False and arms["Ds"][0]["layers"][0]["backward"]["persistent"] is False
    assert arms["Ds"][1]["fwd_persistent"] == arms["Ds"][1]["bwd_persistent"] == 0

    # exact properties
    pad = np.arange(T)[:, None] >= lens[None, :]
    m = dc.step_mask(case, mk["rec"])
    for a, (_, _, _, out, back) in arms.items():
        o = out.reshape(T, S, 2 * H)
        assert np.isfinite(o).all() and np.all(o[pad] == 0), (a, "output: not finite, or padding rows not zero")
        if a != "N" and dc.RECIPES[recipe].get("rnndrop"):
            assert np.all(o[(m == 0) & ~pad[:, :, None]] == 0), (a, "RNNDrop: the output is not 0 where the mask is")
        for (prof, _), (ind, g) in zip(ods, back):
            i = ind.reshape(T, S, dc.D)
            assert np.isfinite(i).all() and np.isfinite(g).all(), (a, prof)
            assert np.all(i[pad] == 0), (a, prof, "in_diff: padding rows not zero")
            if prof == "b":
                assert all(np.all(i[:, s] == 0) for s in zero), (a, "a sequence without a top gradient got an in_diff")
    assert np.array_equal(arms["Dp"][3], arms["Dp2"][3]), "two runs of Dp: another output"
    for (i1, g1), (i2, g2) in zip(arms["Dp"][4], arms["Dp2"][4]):
        assert np.array_equal(i1, i2) and np.array_equal(g1, g2), "two runs of Dp: another in_diff or gradient"

    # accuracy
    ref_out, ref_back = want["f64"].result()
    f32_out, f32_back = want["f32"].result()
    refn_out, refn_back = oracles[(case, None, "f64")].result()
    fails = []

    def hold(quantity, figs):
        """figs: source -> {metric: worst figure}; "O" is the fp32 oracle.  The bar of each metric from O and N, Dp and Ds held to it."""
        row = dict(case=f"{case}-{recipe}", quantity=quantity)
        for metric in figs["O"]:
            f = FACTOR["grad" if quantity.startswith("grad") else metric]
            b = bar(max(figs["O"][metric], figs["N"][metric]), f)
            row.update({f"{metric}_{a}": figs[a][metric] for a in ("Dp", "Ds", "N", "O")}, **{f"{metric}_bar": b})
            for a in ("Dp", "Ds"):
                if not figs[a][metric] <= b:
                    fails.append(f"{quantity} {metric} {a} {figs[a][metric]:.3g} > bar {b:.3g} (fp32 oracle {figs['O'][metric]:.3g}, N {figs['N'][metric]:.3g})")
        print(json.dumps(row))
        report(row)

    r3 = lambda v, w: np.asarray(v).reshape(T, S, w)
    hold("out", {"Dp": dc.seq_worst(r3(arms["Dp"][3], 2 * H), r3(ref_out, 2 * H), lens, 2),
                 "Ds": dc.seq_worst(r3(arms["Ds"][3], 2 * H), r3(ref_out, 2 * H), lens, 2),
                 "O": dc.seq_worst(r3(f32_out, 2 * H), r3(ref_out, 2 * H), lens, 2),
                 "N": dc.seq_worst(r3(arms["N"][3], 2 * H), r3(refn_out, 2 * H), lens, 2)})
    L = dc.layer(case)
    names = lambda flat: {n: v for _, n, v in split_params(L, np.asarray(flat))}
    for k, (prof, _) in enumerate(ods):
        hold(f"in_diff/{prof}", {"Dp": dc.seq_worst(r3(arms["Dp"][4][k][0], dc.D), r3(ref_back[k][0], dc.D), lens),
                                 "Ds": dc.seq_worst(r3(arms["Ds"][4][k][0], dc.D), r3(ref_back[k][0], dc.D), lens),
                                 "O": dc.seq_worst(r3(f32_back[k][0], dc.D), r3(ref_back[k][0], dc.D), lens),
                                 "N": dc.seq_worst(r3(arms["N"][4][k][0], dc.D), r3(refn_back[k][0], dc.D), lens)})
        g = {"Dp": names(arms["Dp"][4][k][1]), "Ds": names(arms["Ds"][4][k][1]), "O": names(f32_back[k][1]), "N": names(arms["N"][4][k][1])}
        ref, refn = names(ref_back[k][1]), names(refn_back[k][1])
        for n in ref:
            hold(f"grad/{prof}/{n}", {a: {"maxnorm": rel_err(g[a][n], refn[n] if a == "N" else ref[n])} for a in g})
    assert not fails, f"{len(fails)} over the bar:\n" + "\n".join(fails[:24])
