"""One process of tests/test_gpu_recurrence_share.py: the cases of tests/share_cases.py that run under ONE share of the device.

rec_plan.cpp reads EESEN_GPU_SHARE once per process (gpu_share(): a function-local static), so every share needs a process of its
own; the parent starts this module once per share, with the share in the child's environment and nowhere else.  TEST INFRASTRUCTURE
(no test_ prefix: not collected).

  python -m tests._share_worker --out DIR --cases name,name,...     one recurrent layer per case
  python -m tests._share_worker --out DIR --step                    one whole training step (share_cases.STEP)

Per case: a fresh Net with the case's switches and EESEN_GEMM_MODE=f32 through Propagate and BackpropagateNoUpdate for both
top-gradient profiles, twice over on the same Net -- the rows module's own arm (test_gpu_recurrence_rows._arm).  DIR/<case>.npz holds
out_r<k>, in_diff_<profile>_r<k> and grads_<profile>_r<k> of both runs k, DIR/<case>.json Plan(), RecurrenceInfo() and the
recoveries.  --step: DIR/step.npz holds pzx, diff and the fresh gradients of the default arm ("P") and of EESEN_PERSISTENT=0 ("S"),
DIR/step.json both arms' Plan(), RecurrenceInfo() and recoveries.  Plan()["gpu_share"] must be the share of the environment.
"""
import argparse
import json
import os
import sys

import numpy as np
import pytest

from tests import share_cases as sc
from tests import test_gpu_recurrence_rows as rows


def env_share():
    v = os.environ.get("EESEN_GPU_SHARE", "")
    return int(v) if v else 1


def run_case(out_dir, name, mp):
    c = sc.ALL[name]
    assert c["share"] == env_share(), (name, "started under share", env_share())
    plan, info, recoveries, passes = rows._arm(mp, {**c["env"], **rows.GEMM}, name, runs=2, cases=sc)
    assert plan["gpu_share"] == env_share(), (plan["gpu_share"], env_share())
    arrays = {}
    for k, (out, back) in enumerate(passes):
        arrays[f"out_r{k}"] = out
        for (prof, _), (in_diff, grads) in zip(rows._inputs(name, sc)[2], back):
            arrays[f"in_diff_{prof}_r{k}"] = in_diff
            arrays[f"grads_{prof}_r{k}"] = grads
    np.savez(os.path.join(out_dir, name + ".npz"), **arrays)
    with open(os.path.join(out_dir, name + ".json"), "w") as f:
        json.dump(dict(case=name, share=env_share(), plan=plan, info=info, recoveries=recoveries), f)
    f, b = plan["layers"][0]["forward"], plan["layers"][0]["backward"]
    print(f"{name}: forward {f['kernel']} x{f.get('launches', 0)}, backward {b['kernel']} x{b.get('launches', 0)}", flush=True)


def run_step(out_dir, mp):
    """One training step of share_cases.STEP's net in the default GEMM mode: the default recurrence switches, and EESEN_PERSISTENT=0."""
    from eesen_amd import synth
    from eesen_amd.api import Ctc, Net
    cfg = sc.STEP["cfg"]
    layers, batch = synth.make_model(**cfg), synth.make_batch(**cfg)
    arrays, what = {}, dict(share=env_share())
    for arm, env in (("P", {}), ("S", {"EESEN_PERSISTENT": "0"})):
        for k in rows.SWITCHES:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        net = Net.from_layers(layers); net.SetTrainOptions(1.0, 0.0); ctc = Ctc()
        net.SetSeqLengths(batch.lens)
        out = net.Propagate(batch.feats)
        diff = ctc.EvalParallel(batch.lens, out, batch.labels)
        net.BackpropagateNoUpdate(diff)
        arrays.update({f"pzx_{arm}": np.asarray(ctc.pzx), f"diff_{arm}": diff.numpy(), f"grads_{arm}": net.GetGrads()})
        info = net.RecurrenceInfo()
        plan = net.Plan()
        assert plan["gpu_share"] == env_share(), (plan["gpu_share"], env_share())
        what[arm] = dict(plan=plan, info=info, recoveries=net.recoveries)
        print(f"step {arm}: " + "; ".join(f"{l['forward']['kernel']} x{l['forward'].get('launches', 0)} / "
                                          f"{l['backward']['kernel']} x{l['backward'].get('launches', 0)}" for l in plan["layers"]), flush=True)
    for k in rows.SWITCHES:
        mp.delenv(k, raising=False)
    np.savez(os.path.join(out_dir, "step.npz"), **arrays)
    with open(os.path.join(out_dir, "step.json"), "w") as f:
        json.dump(what, f)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default="")
    ap.add_argument("--step", action="store_true")
    a = ap.parse_args(argv)
    os.makedirs(a.out, exist_ok=True)
    mp = pytest.MonkeyPatch()
    for name in [n for n in a.cases.split(",") if n]:
        run_case(a.out, name, mp)
    if a.step:
        run_step(a.out, mp)
    return 0


if __name__ == "__main__":
    sys.exit(main())
