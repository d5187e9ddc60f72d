#!/usr/bin/env python3
"""Measures Ctc.RescoreNbest (INTEGRATION.md "Rescoring") at the decode profile's shape and writes the rows of profiles/ctc_rescore.md.

    python scripts/ctc_rescore_profile.py [--out DIR] [--reps 5]

Shape: profiles/ctc_decode.md's -- S = 32, T = 1000, K = 46, tests/ctc_cases.peaky_case(32, 1000, 46, 100, (4, 12, 30), 101), posteriors
(is_log = 0), beam 16, max_classes 20 -- with nbest 4 and 16.  Three legs per nbest, each in a process of its own (this script starts
itself with --leg), after one warm-up call of everything the leg times:

    decode    Ctc.DecodeParallel: wall clock around the call (it waits for its results) and eesen_ctc_get_decode_times
    rescore   Ctc.RescoreNbest on that call's entries, no second LM: wall clock and eesen_ctc_get_rescore_times
    eval      what the parent commit could do: per rank i one Ctc.EvalParallel over the 32 utterances with each utterance's i-th
              labelling (one without that rank, or with an empty one, takes a one-label stand-in: the call refuses empty labellings);
              wall clock over the nbest calls and the sum of eesen_ctc_get_phase_times

Every leg prints one JSON line; the parent collects them into DIR/ctc_rescore.json and prints a markdown table.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = dict(S=32, T=1000, K=46, U=100, heights=(4, 12, 30), seed=101, beam=16, max_classes=20)


def leg(name, nbest, reps):
    import numpy as np
    from eesen_amd import _lib
    from eesen_amd.api import Ctc, CuMatrix
    from tests import ctc_cases as cc
    assert _lib.device_count() > 0, "this measurement needs a GPU"
    lens, probs, _ = cc.peaky_case(SHAPE["S"], SHAPE["T"], SHAPE["K"], SHAPE["U"], SHAPE["heights"], SHAPE["seed"])
    dev = CuMatrix.from_numpy(np.ascontiguousarray(probs, np.float32))
    ctc = Ctc()
    decode = lambda: ctc.DecodeParallel(lens, dev, beam=SHAPE["beam"], max_classes=SHAPE["max_classes"], nbest=nbest)
    hyps, _ = decode()
    out = dict(leg=name, nbest=nbest, reps=reps, lattices=int(np.sum(ctc.hyp_len >= 0)), longest=int(ctc.hyp_len.max()))
    wall, phases = [], []
    if name == "decode":
        decode()
        for _ in range(reps):
            t0 = time.perf_counter()
            decode()
            wall.append(time.perf_counter() - t0)
            phases.append(ctc.DecodeTimes())
    elif name == "rescore":
        res = ctc.RescoreNbest(lens, dev)
        for _ in range(reps):
            t0 = time.perf_counter()
            res = ctc.RescoreNbest(lens, dev)
            wall.append(time.perf_counter() - t0)
            phases.append(ctc.RescoreTimes())
        out["reranked"] = int(sum(res.order[s, 0] != 0 for s in range(len(lens))))
        out["reordered"] = int(sum(res.order[s, :len(hyps[s])].tolist() != list(range(len(hyps[s]))) for s in range(len(lens))))
    elif name == "eval":
        pick = lambda s, i: (hyps[s][i] if i < len(hyps[s]) and hyps[s][i] else [1])
        ranks = [[pick(s, i) for s in range(len(lens))] for i in range(nbest)]
        diff = ctc.EvalParallel(lens, dev, ranks[0])
        for _ in range(reps):
            acc = dict(log=0.0, alpha_beta=0.0, error_diff=0.0)
            t0 = time.perf_counter()
            for labels in ranks:
                ctc.EvalParallel(lens, dev, labels, diff=diff)
                for k, v in ctc.PhaseTimes().items():
                    acc[k] = acc.get(k, 0.0) + v
            wall.append(time.perf_counter() - t0)
            phases.append(acc)
    else:
        raise SystemExit(f"unknown leg {name}")
    out["wall_ms"] = [round(1e3 * w, 4) for w in wall]
    out["phases_ms"] = {k: round(1e3 * sum(p[k] for p in phases) / len(phases), 4) for k in phases[0]}
    print("LEG " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--leg")
    ap.add_argument("--nbest", type=int)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.nbest, a.reps)
    rows = []
    for nbest in (4, 16):
        for name in ("decode", "rescore", "eval"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--nbest", str(nbest), "--reps", str(a.reps)],
                               capture_output=True, text=True, cwd=ROOT, timeout=900)
            if r.returncode != 0:      # nothing more is started on the device after a leg that failed
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"leg {name} nbest {nbest} ended with {r.returncode}")
            rows.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("LEG ")][-1][4:]))
            print(json.dumps(rows[-1]), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ctc_rescore.json"), "w") as f:
        json.dump(dict(shape=SHAPE, rows=rows), f, indent=1)
    print("| nbest | leg | lattices | phases (ms) | wall (ms, min - max) |\n|---|---|---|---|---|")
    for r in rows:
        ph = ", ".join(f"{k} {v:.3f}" for k, v in r["phases_ms"].items())
        print(f"| {r['nbest']} | {r['leg']} | {r['lattices']} | {ph} | {min(r['wall_ms']):.2f} - {max(r['wall_ms']):.2f} |")


if __name__ == "__main__":
    main()
