#!/usr/bin/env python3
"""The frame-level cross-entropy step at a senone-sized output layer, next to the CTC step, on one GPU: cfg2's network
(4 x 512 BiLSTM, D = 40, S = 32, T = 1000) with a K = 4000 output layer (CE) and with K = 51 (CTC).

    python scripts/ce_step.py                       # every leg, each in a process of its own; one JSON line
    python scripts/ce_step.py --leg ce|ctc          # one leg in this process (what the driver runs)

A leg times `steps` steps (Propagate -> loss -> Backpropagate + update) after `warmup` between two device synchronisations,
and, with the loss's own phase timer summed over the same steps, the loss kernel's share.  The CE kernel's bytes: it reads the
valid rows of the posteriors and writes the whole diff, 2 x rows x K x 4 bytes when every row is valid (lengths = T here).
The kernel table (and the output-layer GEMMs / softmax) come from `rocprofv3 --kernel-trace --stats -- python
scripts/ce_step.py --leg ce` -- see profiles/ce_step.md for the exact commands."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = dict(kind="BiLstmParallel", layers=4, H=512, D=40, S=32, T=1000)


def leg(name: str, steps: int, warmup: int) -> dict:
    from eesen_amd import synth, _lib
    from eesen_amd.api import Net, Ctc, CE
    K = 4000 if name == "ce" else 51
    cfg = dict(CFG, K=K)
    layers = synth.make_model(**cfg)
    batch = synth.make_batch(min_frac=1.0, **cfg)
    net = Net.from_layers(layers)
    net.SetTrainOptions(1e-5, 0.9)
    rng = np.random.default_rng(1)
    rows = cfg["S"] * cfg["T"]
    if name == "ce":
        loss = CE()
        tg = rng.integers(0, K, size=rows).astype(np.int32)
    else:
        loss = Ctc()
    diff = None

    def step():
        nonlocal diff
        net.SetSeqLengths(batch.lens)
        out = net.Propagate(batch.feats)
        if name == "ce":
            diff = loss.EvalParallel(out, tg, diff, batch.lens, want_obj=False)
        else:
            diff = loss.EvalParallel(batch.lens, out, batch.labels, diff, want_pzx=False)
        net.Backpropagate(diff)

    for _ in range(warmup):
        step()
    net.Synchronize()
    loss.SetProfiling(True)
    loss.PhaseTimes()
    _lib.check(_lib.load().eesen_device_synchronize(0))
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    _lib.check(_lib.load().eesen_device_synchronize(0))
    ms = (time.perf_counter() - t0) * 1e3 / steps
    ph = loss.PhaseTimes()
    loss_ms = sum(ph.values()) * 1e3 / steps
    r = dict(leg=name, K=K, S=cfg["S"], T=cfg["T"], steps=steps, warmup=warmup, step_ms=round(ms, 3), loss_ms=round(loss_ms, 4))
    if name == "ce":
        nbytes = 2.0 * rows * K * 4
        r.update(ce_bytes=nbytes, ce_tbps=round(nbytes / (loss_ms * 1e-3) / 1e12, 3), obj=loss.stats()["obj"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["ce", "ctc"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per leg process")
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(leg(a.leg, a.steps, a.warmup)), flush=True)
        return 0
    out = {}
    for name in ("ce", "ctc"):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--leg", name,
               "--steps", str(a.steps), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if r.returncode != 0:   # a faulted or timed-out leg ends the run: nothing more is started on the GPU
            out[name] = dict(returncode=r.returncode, stderr=r.stderr[-2000:])
            break
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out), flush=True)
    return 0 if all("returncode" not in v for v in out.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
