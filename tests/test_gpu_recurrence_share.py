"""-m gpu: the recurrence kernels on a device the process SHARES, against an fp64 layer, PER SEQUENCE.

With EESEN_GPU_SHARE=n (or a communicator that finds n of its ranks on one device) rec_plan.cpp sizes every grid against 1/n of the
CUs.  It then answers sequence windows -- the same kernel 2, 4 or 8 times with LstmLayerDev::s_begin / s_count set, and every buffer
a kernel indexes by sequence (G, C, Y, the exchange copy X, rmask, DG, the K-split tiles' PX, DGH and EX, the arrival counters) goes
through that offset -- takes the multiplexed kernels at exactly two windows only, has no residency census, leaves the narrow forward
tile and the 8-sequence backward tile at smaller shapes, and sends shapes that are persistent on a whole device to the per-step
kernels.  The other recurrence modules run on a whole device, where all but three plans have one window.  tests/share_cases.py holds
the cases: shape, switches, share, and the rows and launches Plan() answered under that share on an MI355X.

The share is read once per process, so the cases run in CHILD processes (tests/_share_worker.py), one per share, one after the other:
all selected cases of a share in one child, and their twins on a whole device (share 1) in a fourth.  A child is a fresh
subprocess.run under its own time limit (120 s and 20 s per case); its environment is this process's without the rows module's
SWITCHES and without EESEN_GPU_SHARE, plus the share (unset for share 1).  A child that ends on a signal, with 134, 139, 124 or 137,
or at its limit is not retried, no further child is started, and every remaining test fails at once with its stderr.

A child runs the rows module's own arm (test_gpu_recurrence_rows._arm: a fresh Net, the case's switches and EESEN_GEMM_MODE=f32,
both top-gradient profiles, twice over) and this module holds what it wrote with the rows module's own checks:
  exact     Plan() names exactly the table's rows and launches and the share; RecurrenceInfo() agrees; nothing recovered; all is
            finite; padding rows of the output and of in_diff are zero; a sequence without a top gradient gets an in_diff of zeros; the
            second run gives the same bits (_what_ran, _exact) -- the share-1 twin likewise, but for its plan (tests/test_gpu_plans.py)
  windows   sequences are independent chains and a window is a whole number of sequence tiles, so a sequence keeps its place in
            its tile: where a pass's row under the share is the row of the share-1 twin, that pass's results are BIT-IDENTICAL per
            sequence -- the output for the forward pass; in_diff (both profiles) for the backward pass, where the forward rows are
            equal too.  A wrong window offset is named outright, by sequence and frame
  accuracy  _accuracy unchanged: reference oracle.net.OracleNet(layers, "f64"), yardstick the fp32 oracle against it, the bar
            max(FACTOR * yardstick, 4e-7) with that module's FACTOR, per (sequence, direction) for the output, per sequence for in_diff,
            per tensor for the gradients; the arm under the share ("K") and its share-1 twin ("W") are each held to it
One whole training step (share_cases.STEP: 2 x BiLSTM(512) + affine + softmax + CTC, S = 64, T = 12, the default GEMM mode) runs in
the same children at share 2 and 4, where Net::forward_pass / backpropagate take the other branches of one_window, leaves_room and
light: held to the fp32 oracle's train_step as tests/test_gpu_gemm.py test_training_step_in_split_mode_meets_the_same_parity_bar
holds its step (rel_err of pzx, diff and the fresh gradients below 1e-4, nothing recovered), and within that test's 2e-5 of the
EESEN_PERSISTENT=0 arm's gradients.

Every figure goes to $EESEN_PARITY_OUT/recurrence_share.json; the first full run is profiles/recurrence_share.json (.md).
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import share_cases as sc
from tests import test_gpu_recurrence_rows as rows
from tests.util import rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FATAL = (134, 139, 124, 137)
_DEAD = {}            # set once by a worker that died: {"share", "why", "stderr"}; no worker is started after that


def child_env(share):
    env = {k: v for k, v in os.environ.items() if k not in rows.SWITCHES and k != "EESEN_GPU_SHARE"}
    if share > 1:
        env["EESEN_GPU_SHARE"] = str(share)
    return env


def _dead():
    return f"the worker of share {_DEAD['share']} {_DEAD['why']}; no further worker is started.  Its stderr ended:\n{_DEAD['stderr']}"


class Worker:
    """What one child wrote."""

    def __init__(self, out):
        self.out = out

    def load(self, name):
        what = json.load(open(os.path.join(self.out, name + ".json")))
        z = np.load(os.path.join(self.out, name + ".npz"))
        profs = [p for p, _ in rows._inputs(name, sc)[2]]
        passes = [(z[f"out_r{k}"], [(z[f"in_diff_{p}_r{k}"], z[f"grads_{p}_r{k}"]) for p in profs]) for k in (0, 1)]
        return what["plan"], what["info"], what["recoveries"], passes

    def step(self):
        return json.load(open(os.path.join(self.out, "step.json"))), np.load(os.path.join(self.out, "step.npz"))


@pytest.fixture(scope="module")
def workers(request):
    """share -> Worker: the child of a share is started when its first case asks for it, with every selected case of that share (share
    1: the twins of every selected case) and the training step where that is selected; run once, never again."""
    mine = [it for it in request.session.items if it.module.__name__ == __name__ and hasattr(it, "callspec")]
    names = list(dict.fromkeys(it.callspec.params["name"] for it in mine if "name" in it.callspec.params))
    steps = {it.callspec.params["step_share"] for it in mine if "step_share" in it.callspec.params}
    todo = {s: [n for n in names if sc.TABLE[n]["share"] == s] for s in sc.SHARES}
    todo[1] = list(dict.fromkeys(sc.twin(n) for n in names))
    tmp = tempfile.mkdtemp(prefix="eesen_share_")
    done = {}

    def get(share):
        if share in done:
            if isinstance(done[share], str):
                pytest.fail(done[share], pytrace=False)
            return done[share]
        if _DEAD:
            pytest.fail(_dead(), pytrace=False)
        out = os.path.join(tmp, f"share{share}")
        args = ["--out", out] + (["--cases", ",".join(todo[share])] if todo[share] else []) + (["--step"] if share in steps else [])
        limit = 120 + 20 * (len(todo[share]) + (2 if share in steps else 0))
        cmd = [sys.executable, "-m", "tests._share_worker"] + args
        try:
            r = subprocess.run(cmd, env=child_env(share), cwd=ROOT, capture_output=True, text=True, timeout=limit)
            rc_, err, why = r.returncode, r.stderr, None
            print(r.stdout, end="")
        except subprocess.TimeoutExpired as e:      # (subprocess.run has killed the child and waited for it)
            err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
            rc_, why = None, f"was killed at its limit of {limit} s"
        if why is None and (rc_ < 0 or rc_ in FATAL):
            why = f"ended on signal {-rc_}" if rc_ < 0 else f"exited with {rc_}"
        if why is not None:
            _DEAD.update(share=share, why=why, stderr=err[-3000:])
            done[share] = _dead()
        elif rc_ != 0:
            done[share] = f"the worker of share {share} exited with {rc_}:\n{err[-3000:]}"
        else:
            done[share] = Worker(out)
        return get(share)

    yield get
    shutil.rmtree(tmp, ignore_errors=True)


@pytest.fixture(scope="module")
def pool():
    p = ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1))
    yield p
    p.shutdown(wait=False, cancel_futures=True)


@pytest.fixture(scope="module")
def oracles(request, pool):
    """(case, precision) -> future of the oracle layer, computed once per shape and recipe (the switches and the share are not the
    oracle's) in the order the cases run, on a thread pool (the C oracle releases the GIL) while the children run."""
    sel = [it.callspec.params["name"] for it in request.session.items
           if it.module.__name__ == __name__ and hasattr(it, "callspec") and "name" in it.callspec.params]
    by_shape, futs = {}, {}
    for n in dict.fromkeys(sel):
        c = sc.TABLE[n]
        for p in ("f64", "f32"):
            key = (c["kind"], c["H"], c["S"], c["T"], c["recipe"], p)
            if key not in by_shape:
                by_shape[key] = pool.submit(rows._oracle, n, p, sc)
            futs[(n, p)] = by_shape[key]
    return futs


@pytest.fixture(scope="module")
def report():
    rows_ = []
    yield rows_.append
    out = os.environ.get("EESEN_PARITY_OUT")
    if not out:
        return
    try:
        os.makedirs(out, exist_ok=True)
        json.dump(rows_, open(os.path.join(out, "recurrence_share.json"), "w"), indent=1)
    except OSError:
        pass


def _same_bits(what, got, ref, lens, T, S, fails):
    """got, ref [T*S x C]: bit-identical over every sequence's valid frames; the first (sequence, frame) that is not, named."""
    g, r = got.reshape(T, S, -1), ref.reshape(T, S, -1)
    bad = [(s, t) for s in range(S) for t in range(int(lens[s])) if not np.array_equal(g[t, s], r[t, s])]
    if bad:
        seqs = sorted({s for s, _ in bad})
        fails.append(f"{what}: {len(seqs)} sequences differ from the share-1 run, the first at sequence {bad[0][0]}, frame {bad[0][1]} "
                     f"(sequences {seqs[:16]}{'...' if len(seqs) > 16 else ''})")
    return not bad


@pytest.mark.parametrize("name", list(sc.TABLE))
def test_recurrences_under_a_share_hold_fp32_accuracy_and_windows_keep_a_sequences_bits(gpu, workers, oracles, report, name):
    if _DEAD:
        pytest.fail(_dead(), pytrace=False)
    c = sc.TABLE[name]; S, T = c["S"], c["T"]
    one = sc.twin(name)
    K, W = workers(c["share"]).load(name), workers(1).load(one)
    fails = []
    ran = {"K": rows._what_ran(f"{name} K", *K[:3], c["fwd"], c["bwd"], c["launches"], fails)}
    if K[0]["gpu_share"] != c["share"] or W[0]["gpu_share"] != 1:
        fails.append(f"Plan() says share {K[0]['gpu_share']} and {W[0]['gpu_share']}, the table {c['share']} and 1")
    f1, b1 = W[0]["layers"][0]["forward"], W[0]["layers"][0]["backward"]
    ran["W"] = dict(forward=f1["kernel"], backward=b1["kernel"], launches=[f1.get("launches", 0), b1.get("launches", 0)],
                    workgroups=[f1.get("workgroups", 0), b1.get("workgroups", 0)], recoveries=W[2])
    print(f"{one} W: forward {f1['kernel']} x{f1.get('launches', 0)}, backward {b1['kernel']} x{b1.get('launches', 0)}")
    if W[2] != 0:
        fails.append(f"{one}: {W[2]} recoveries")
    rows._exact(f"{name} K", name, K[3], fails, cases=sc)
    rows._exact(f"{one} W", one, W[3], fails, cases=sc)

    # windows do not change a sequence's arithmetic
    lens, _, ods, _ = rows._inputs(name, sc)
    same_fwd = ran["K"]["forward"] != sc.PER_STEP_KERNELS and ran["K"]["forward"] == f1["kernel"]
    same_bwd = same_fwd and ran["K"]["backward"] != sc.PER_STEP_KERNELS and ran["K"]["backward"] == b1["kernel"]
    bits = dict(forward=None, backward=None)
    if same_fwd:
        bits["forward"] = _same_bits(f"{name} output ({c['launches'][0]} launches against {ran['W']['launches'][0]})",
                                     K[3][0][0], W[3][0][0], lens, T, S, fails)
    if same_bwd:
        bits["backward"] = all([_same_bits(f"{name} in_diff/{prof} ({c['launches'][1]} launches against {ran['W']['launches'][1]})",
                                           K[3][0][1][k][0], W[3][0][1][k][0], lens, T, S, fails) for k, (prof, _) in enumerate(ods)])
    print(f"{name}: bit-identical to share 1: forward {bits['forward']}, backward {bits['backward']} (None: another row, not compared)")
    report(dict(case=name, switches=c["env"], recipe=c["recipe"], share=c["share"], plan=ran, bit_identical_to_share1=bits))

    rows._accuracy(name, {"K": K[3][0], "W": W[3][0]}, oracles, report, fails, cases=sc)
    assert not fails, f"{len(fails)} findings:\n" + "\n".join(fails[:24])


@pytest.fixture(scope="module")
def step_oracle(pool):
    def run():
        from eesen_amd import synth
        from oracle import net as onet
        cfg = sc.STEP["cfg"]
        ora = onet.OracleNet(synth.make_model(**cfg), "f32"); ora.set_train_options(1.0, 0.0)
        o = onet.train_step(ora, synth.make_batch(**cfg), "f32")
        return o["pzx"], o["diff"], ora.fresh_grads_flat()
    return pool.submit(run)


@pytest.mark.parametrize("step_share", sc.STEP["shares"])
def test_training_step_under_a_share_meets_the_parity_bar(gpu, workers, step_oracle, report, step_share):
    if _DEAD:
        pytest.fail(_dead(), pytrace=False)
    what, z = workers(step_share).step()
    pzx, diff, grads = step_oracle.result()
    assert what["share"] == step_share and all(what[a]["plan"]["gpu_share"] == step_share for a in ("P", "S"))
    figs = {}
    for a in ("P", "S"):
        figs[a] = dict(pzx=rel_err(z[f"pzx_{a}"], pzx), diff=rel_err(z[f"diff_{a}"], diff), grads=rel_err(z[f"grads_{a}"], grads))
    figs["P_to_S"] = rel_err(z["grads_P"], z["grads_S"])
    layers = {a: [dict(forward=l["forward"]["kernel"], backward=l["backward"]["kernel"],
                       launches=[l["forward"].get("launches", 0), l["backward"].get("launches", 0)]) for l in what[a]["plan"]["layers"]]
              for a in ("P", "S")}
    print(json.dumps(dict(step_share=step_share, figures=figs, layers=layers["P"])))
    report(dict(case=f"step@share{step_share}", figures=figs, plan={a: what[a]["plan"] for a in ("P", "S")},
                recoveries={a: what[a]["recoveries"] for a in ("P", "S")}))
    # the arm under test runs persistent kernels in windows; the other arm none
    assert all(l["forward"].startswith("lstm_fwd_persistent") and l["backward"].startswith("lstm_bwd_persistent") for l in layers["P"]), layers["P"]
    assert any(n > 1 for l in layers["P"] for n in l["launches"]), layers["P"]
    assert what["P"]["info"]["fwd_persistent"] == what["P"]["info"]["bwd_persistent"] == what["P"]["info"]["lstm_layers"] == 2
    assert what["S"]["info"]["fwd_persistent"] == what["S"]["info"]["bwd_persistent"] == 0
    assert what["P"]["recoveries"] == 0 and what["S"]["recoveries"] == 0
    for a in ("P", "S"):
        assert figs[a]["pzx"] < 1e-4 and figs[a]["diff"] < 1e-4 and figs[a]["grads"] < 1e-4, (a, figs[a])
    assert figs["P_to_S"] < 2e-5, figs
