"""-m gpu: every row of the recurrence kernel table that no other module holds, at its own tile, against an fp64 layer, PER SEQUENCE.

eesen_amd/csrc/lstm_persistent.hip compiles the LSTM time recurrence 71 times into one table; rec_plan.cpp takes one row per layer
and pass from the layer's shape and the switches of tuning.h.  tests/recurrence_cases.py holds, per case, a shape and switches and the
two rows the planner takes there on a whole 256-CU device, and the shapes that must fall to the one-launch-per-step kernels of
lstm.hip (more than 1024 cells, 260 forward workgroups, rows that are no whole 128-byte lines); tests/test_recurrence_cases.py holds,
without a GPU, that every row of the table is run by a case here, held by another module or written down as unreachable.

One recurrent layer (40 inputs) is the whole Net; the test picks the top gradient `od`.  Arms, a fresh Net each (the switches are
read when a Net is created):
  K   the case's switches and EESEN_GEMM_MODE=f32 (the GEMMs' planes: test_gpu_gemm.py; with the bounds Net chooses around an LSTM layer: test_gpu_lstm_gemms.py).  Plan() must name exactly the
      case's forward and backward rows and its launches per pass, RecurrenceInfo() both passes persistent, and nothing recovered.
      The same Net runs everything twice: the same bits
  St  EESEN_GEMM_MODE=f32, EESEN_PERSISTENT=0: the per-step kernels of lstm.hip at the same shape -- held like K, not a yardstick
A PER_STEP shape has one arm, D: the default recurrence switches (and EESEN_GEMM_MODE=f32); Plan() must answer the per-step kernels
for the passes the table names (and the table's row for the other), and nothing recovered.

Reference: oracle.net.OracleNet(layers, "f64") on the same fp32 inputs.  Yardstick of a quantity: the fp32 oracle (the reference's own
arithmetic) against the fp64 one, the worst over the case's sequences.  No GPU arm enters any bar.  Both oracles are computed on a
thread pool while the arms run.

Metrics (dropout_cases.seq_worst): rel_err (max-norm) and the p999 of err_metrics per (sequence, direction) for the output and per
sequence for in_diff, each over that sequence's valid rows; rel_err per gradient tensor.  Bar: max(factor * yardstick, 4e-7); K, St
and D are each held to it, no case exempt.  ONE factor per metric for the whole module: the larger of the project's factor (1.5
max-norm, 3 p999, 4 gradient tensors: calibrated against a yardstick that included a GPU arm) and 1.25 times the worst ratio arm /
yardstick of the first full run (profiles/recurrence_rows.json, .md), rounded up to the next half, with the caps 3 (max-norm:
tests/util.py diff_bound's margin over the fp32 oracle alone), 6 (p999) and 8 (gradient tensors).  A figure at or under the 4e-7 floor
passes whatever the factor and so does not enter the worst ratio.
The first full run (all 34 cases passed with the project's factors): worst ratios 1.49 on max-norm (bi64_s8-FWD_SPLIT=0, out, K:
6.2e-7 against 4.2e-7), 1.68 on p999 (bi128_s32-FWD_SPLIT=0, out, K) and 1.27 on a gradient tensor (bi40_s32, grad/a/Wm_fw, K).  So
the factors are 2 for max-norm (1.25 x 1.49 = 1.86, the next half), 3 for p999 and 4 for the gradient tensors (the project's: 1.25
x the worst ratio stays below them).

Exact, every arm: everything is finite; padding rows of the output and of in_diff are zero; a sequence whose od is zero has an
in_diff of zeros; the second run of K (D) on the same Net gives the same bits.

od profiles: "a" N(0, 1) on valid rows; "b" in every aligned group of four sequences scaled by 1, 2^-8, 2^-16, 2^-24, and every other
group holds one sequence whose od is zero.  Every figure goes to $EESEN_PARITY_OUT/recurrence_rows.json.
"""
import functools
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import recurrence_cases as rc
from tests.util import rel_err, split_params

pytestmark = pytest.mark.gpu
GEMM = {"EESEN_GEMM_MODE": "f32"}
# every switch a Net of this module may read: none leaks from one arm (or from the caller's environment) into the next
SWITCHES = ("EESEN_GEMM_MODE", "EESEN_PERSISTENT", "EESEN_FWD_SPLIT", "EESEN_FWD_F16", "EESEN_FWD_MUX", "EESEN_FWD_NARROW2",
            "EESEN_FWD_T16_SMALL", "EESEN_BWD_Q4", "EESEN_BWD_Q4_ST8", "EESEN_BWD_KSPLIT", "EESEN_BWD_MUX", "EESEN_BWD_F16")
FACTOR = {"maxnorm": 2.0, "p999": 3.0, "grad": 4.0}      # (the docstring; profiles/recurrence_rows.md)
FLOOR = 4e-7


def bar(yardstick, factor):
    return max(factor * yardstick, FLOOR)


# `cases`: the module that holds the case table and its generators -- tests/recurrence_cases.py, or tests/share_cases.py for
# tests/test_gpu_recurrence_share.py, which runs these same functions on its own table
@functools.lru_cache(maxsize=None)
def _inputs(name, cases=rc):
    """(lengths, features, [(profile, od)], zero sequences) of a case: computed once, shared by the arms and the oracles, never written."""
    lens = cases.lengths(name)
    ods, zero = cases.top_gradients(name, lens)
    x = cases.features(name, lens)
    for a in [lens, x] + [od for _, od in ods]:
        a.setflags(write=False)
    return lens, x, ods, zero


def _oracle(name, prec, cases=rc):
    lens, x, ods, _ = _inputs(name, cases)
    return cases.oracle_run(cases.layer(name), x, lens, ods, prec, cases.masks(name))


@pytest.fixture(scope="module")
def oracles(request):
    """(case, precision) -> future of the oracle layer of every selected case, in the order the cases run, on a thread pool (the C
    oracle releases the GIL) while the GPU arms run."""
    sel = [it.callspec.params["name"] for it in request.session.items
           if it.module.__name__ == __name__ and hasattr(it, "callspec") and "name" in it.callspec.params]
    pool = ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1))
    futs = {(n, p): pool.submit(_oracle, n, p) for n in dict.fromkeys(sel) for p in ("f64", "f32")}
    yield futs
    pool.shutdown(wait=False, cancel_futures=True)


@pytest.fixture(scope="module")
def report():
    rows = []
    yield rows.append
    out = os.environ.get("EESEN_PARITY_OUT")
    if not out:
        return
    try:
        os.makedirs(out, exist_ok=True)
        json.dump(rows, open(os.path.join(out, "recurrence_rows.json"), "w"), indent=1)
    except OSError:
        pass


def _arm(monkeypatch, env, name, runs=1, cases=rc):
    """One fresh Net through Propagate and Backpropagate for every od, `runs` times over (a case with recurrent dropout: its masks
    injected before every Propagate -- they are one-shot).
    Returns (plan, info, recoveries, [(out, [(in_diff, grads) per od]) per run])."""
    from eesen_amd.api import Net, CuMatrix
    c = cases.ALL[name]; S, T = c["S"], c["T"]
    lens, x, ods, _ = _inputs(name, cases)
    mk = cases.masks(name)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    net = Net.from_layers(cases.layer(name))
    passes = []
    for _ in range(runs):
        out, back = None, []
        for _, od in ods:
            if mk is not None:
                net.SetDropoutMasks(0, fwd=mk["fwd"], rec=mk["rec"])
            net.SetSeqLengths(lens)
            o = net.Propagate(x).numpy()
            assert out is None or np.array_equal(o, out), "the same input gave another output"
            out = o
            idf = CuMatrix(T * S, cases.D)
            net.BackpropagateNoUpdate(CuMatrix.from_numpy(od), idf)
            back.append((idf.numpy(), net.GetGrads()))
        passes.append((out, back))
    info = net.RecurrenceInfo()
    plan = net.Plan()                  # (after a Propagate: the forward plan depends on the layer's exchange buffer being there)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return plan, info, net.recoveries, passes


def _what_ran(tag, plan, info, recoveries, fwd, bwd, launches, fails):
    """Plan() names exactly `fwd` and `bwd` (rc.PER_STEP_KERNELS: that pass on lstm.hip) with `launches` per pass."""
    f, b = plan["layers"][0]["forward"], plan["layers"][0]["backward"]
    print(f"{tag}: forward {f['kernel']} x{f.get('launches', 0)}, backward {b['kernel']} x{b.get('launches', 0)}")
    if (f["kernel"], b["kernel"]) != (fwd, bwd):
        fails.append(f"{tag}: Plan() names {f['kernel']} / {b['kernel']}, the table {fwd} / {bwd}")
    if (f.get("launches", 0), b.get("launches", 0)) != tuple(launches):
        fails.append(f"{tag}: {f.get('launches', 0)} / {b.get('launches', 0)} launches, the table {tuple(launches)}")
    pers = (int(fwd != rc.PER_STEP_KERNELS), int(bwd != rc.PER_STEP_KERNELS))
    if (f["persistent"], b["persistent"]) != (bool(pers[0]), bool(pers[1])) or \
            (info["fwd_persistent"], info["bwd_persistent"], info["lstm_layers"]) != (pers[0], pers[1], 1):
        fails.append(f"{tag}: persistent passes {info}, the table {pers}")
    if recoveries != 0:
        fails.append(f"{tag}: {recoveries} recoveries")
    return dict(forward=f["kernel"], backward=b["kernel"], launches=[f.get("launches", 0), b.get("launches", 0)],
                workgroups=[f.get("workgroups", 0), b.get("workgroups", 0)], recoveries=recoveries)


def _exact(tag, name, passes, fails, cases=rc):
    c = cases.ALL[name]; H, S, T, nd = c["H"], c["S"], c["T"], cases.ndir(name)
    lens, _, ods, zero = _inputs(name, cases)
    pad = np.arange(T)[:, None] >= lens[None, :]
    for out, back in passes:
        o = out.reshape(T, S, nd * H)
        if not np.isfinite(o).all():
            fails.append(f"{tag}: the output is not finite")
        if not np.all(o[pad] == 0):
            fails.append(f"{tag}: padding rows of the output are not zero")
        for (prof, _), (ind, g) in zip(ods, back):
            i = ind.reshape(T, S, cases.D)
            if not (np.isfinite(i).all() and np.isfinite(g).all()):
                fails.append(f"{tag} {prof}: in_diff or a gradient is not finite")
            if not np.all(i[pad] == 0):
                fails.append(f"{tag} {prof}: padding rows of in_diff are not zero")
            if prof == "b" and not all(np.all(i[:, s] == 0) for s in zero):
                fails.append(f"{tag}: a sequence without a top gradient got an in_diff")
    if len(passes) == 2:
        (o1, b1), (o2, b2) = passes
        if not (np.array_equal(o1, o2) and all(np.array_equal(i1, i2) and np.array_equal(g1, g2) for (i1, g1), (i2, g2) in zip(b1, b2))):
            fails.append(f"{tag}: the second run on the same Net gave other bits")


def _accuracy(name, arms, oracles, report, fails, cases=rc):
    """arms: tag -> (out, back) of the arm's first run; each held to the bar of every quantity."""
    c = cases.ALL[name]; H, S, T, nd = c["H"], c["S"], c["T"], cases.ndir(name)
    lens, _, ods, _ = _inputs(name, cases)
    ref_out, ref_back = oracles[(name, "f64")].result()
    f32_out, f32_back = oracles[(name, "f32")].result()

    def hold(quantity, figs):
        """figs: source -> {metric: worst figure}; "O" is the fp32 oracle, the yardstick."""
        row = dict(case=name, quantity=quantity)
        for metric in figs["O"]:
            kind = "grad" if quantity.startswith("grad") else metric
            b = bar(figs["O"][metric], FACTOR[kind])
            row.update({f"{metric}_{a}": figs[a][metric] for a in figs}, **{f"{metric}_bar": b})
            for a in arms:
                row[f"{metric}_ratio_{a}"] = figs[a][metric] / figs["O"][metric] if figs["O"][metric] > 0 else None
                if not figs[a][metric] <= b:
                    fails.append(f"{quantity} {metric} {a} {figs[a][metric]:.3g} > bar {b:.3g} (fp32 oracle {figs['O'][metric]:.3g}: "
                                 f"{figs[a][metric] / max(figs['O'][metric], 1e-300):.2f} x)")
        print(json.dumps(row))
        report(row)

    r3 = lambda v, w: np.asarray(v).reshape(T, S, w)
    hold("out", {**{a: cases.seq_worst(r3(out, nd * H), r3(ref_out, nd * H), lens, nd) for a, (out, _) in arms.items()},
                 "O": cases.seq_worst(r3(f32_out, nd * H), r3(ref_out, nd * H), lens, nd)})
    L = cases.layer(name)
    names = lambda flat: {n: v for _, n, v in split_params(L, np.asarray(flat))}
    for k, (prof, _) in enumerate(ods):
        hold(f"in_diff/{prof}", {**{a: cases.seq_worst(r3(back[k][0], cases.D), r3(ref_back[k][0], cases.D), lens) for a, (_, back) in arms.items()},
                                 "O": cases.seq_worst(r3(f32_back[k][0], cases.D), r3(ref_back[k][0], cases.D), lens)})
        g = {**{a: names(back[k][1]) for a, (_, back) in arms.items()}, "O": names(f32_back[k][1])}
        ref = names(ref_back[k][1])
        for n in ref:
            hold(f"grad/{prof}/{n}", {a: {"maxnorm": rel_err(g[a][n], ref[n])} for a in g})


@pytest.mark.parametrize("name", list(rc.CASES))
def test_recurrence_rows_hold_fp32_accuracy_per_sequence(gpu, oracles, report, monkeypatch, name):
    c = rc.CASES[name]
    fails = []
    K = _arm(monkeypatch, {**c["env"], **GEMM}, name, runs=2)
    St = _arm(monkeypatch, {**GEMM, "EESEN_PERSISTENT": "0"}, name)
    ran = {"K": _what_ran(f"{name} K", *K[:3], c["fwd"], c["bwd"], c["launches"], fails),
           "St": _what_ran(f"{name} St", *St[:3], rc.PER_STEP_KERNELS, rc.PER_STEP_KERNELS, (0, 0), fails)}
    report(dict(case=name, switches=c["env"], plan=ran))
    _exact(f"{name} K", name, K[3], fails)
    _exact(f"{name} St", name, St[3], fails)
    _accuracy(name, {"K": K[3][0], "St": St[3][0]}, oracles, report, fails)
    assert not fails, f"{len(fails)} findings:\n" + "\n".join(fails[:24])


@pytest.mark.parametrize("name", list(rc.PER_STEP))
def test_shapes_without_a_persistent_tile_run_per_step_and_hold_fp32_accuracy(gpu, oracles, report, monkeypatch, name):
    c = rc.PER_STEP[name]
    fails = []
    Dd = _arm(monkeypatch, {**c["env"], **GEMM}, name, runs=2)
    report(dict(case=name, switches=c["env"], plan={"D": _what_ran(f"{name} D", *Dd[:3], c["fwd"], c["bwd"], c["launches"], fails)}))
    _exact(f"{name} D", name, Dd[3], fails)
    _accuracy(name, {"D": Dd[3][0]}, oracles, report, fails)
    assert not fails, f"{len(fails)} findings:\n" + "\n".join(fails[:24])
