#!/usr/bin/env python3
"""Measures Ctc.MbrNbest (INTEGRATION.md "Minimum Bayes risk") next to the decode call it follows and next to the same distances on one
host thread, and writes the rows of profiles/ctc_mbr.md.

    python scripts/ctc_mbr_profile.py [--out DIR] [--reps 5]

Shapes: S = 32, T = 1000, K = 46, posteriors (is_log = 0), max_classes 20, beam = nbest = 16 and 64.
    plain     profiles/ctc_decode.md's posteriors, tests/ctc_cases.peaky_case(32, 1000, 46, 100, (4, 12, 30), 101); tokens are labels
    lexicon   profiles/ctc_decode_lex.md's: tests/ctc_lex_cases.random_entries(seed=5601, K=46, space=1, V=20000, max_len=8) and
              lex_case(lexicon, 32, 1000, 8.0, 5602, fill=0.25), no word LM; level 0 (word ids) and level 1 (labels, spaces included)
One process per (mode, nbest) (this script starts itself with --leg), after one warm-up call of everything that is timed:
    decode    Ctc.DecodeParallel: wall clock around the call (it waits for its results) and eesen_ctc_get_decode_times
    mbr       Ctc.MbrNbest on that call's entries: wall clock and eesen_ctc_get_mbr_times (job build + uploads, kernel, host)
    host      the yardstick: the same pairs i < k of every list through eesen_edit_distance, one call at a time on one thread, from
              pointers prepared beforehand; `host_empty` is the same number of calls on empty sequences -- what the loop itself costs
Every leg prints one JSON line; the parent collects them into DIR/ctc_mbr.json and prints a markdown table.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = dict(S=32, T=1000, K=46, U=100, heights=(4, 12, 30), seed=101, max_classes=20)
LEXICON = dict(seed=5601, K=46, space=1, V=20000, max_len=8)


def leg(mode, nbest, reps):
    import tempfile
    import numpy as np
    from eesen_amd import _lib
    from eesen_amd.api import Ctc, CuMatrix, Lexicon
    from tests import ctc_cases as cc
    from tests import ctc_lex_cases as xc
    from tests.ctc_lex_restatement import Lex
    assert _lib.device_count() > 0, "this measurement needs a GPU"
    lib = _lib.load()
    trie = None
    if mode == "plain":
        lens, probs, _ = cc.peaky_case(SHAPE["S"], SHAPE["T"], SHAPE["K"], SHAPE["U"], SHAPE["heights"], SHAPE["seed"])
    else:
        lex = Lex(LEXICON["K"], LEXICON["space"], xc.random_entries(**LEXICON))
        lens, probs, _ = xc.lex_case(lex, SHAPE["S"], SHAPE["T"], 8.0, 5602, fill=0.25)
        with tempfile.TemporaryDirectory() as d:
            trie = Lexicon(lex.write(d, "lex"), None, K=lex.K, space=lex.space)
    dev = CuMatrix.from_numpy(np.ascontiguousarray(probs, np.float32))
    ctc = Ctc()
    decode = lambda: ctc.DecodeParallel(lens, dev, beam=nbest, max_classes=SHAPE["max_classes"], nbest=nbest, lexicon=trie)
    decode()
    decode()
    out = dict(mode=mode, nbest=nbest, reps=reps, entries=int(np.sum(ctc.hyp_len >= 0)))
    wall, phases = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        decode()
        wall.append(time.perf_counter() - t0)
        phases.append(ctc.DecodeTimes())
    ms = lambda ws: [round(1e3 * w, 4) for w in ws]
    mean = lambda ps: {k: round(1e3 * sum(p[k] for p in ps) / len(ps), 4) for k in ps[0]}
    out["decode"] = dict(wall_ms=ms(wall), phases_ms=mean(phases))
    S, N = ctc.hyp_len.shape
    for level in ([0] if mode == "plain" else [0, 1]):
        words = level == 0 and ctc.words is not None
        tok = [[np.ascontiguousarray((ctc.words if words else ctc.hyp)[s, i, :int((ctc.words_len if words else ctc.hyp_len)[s, i])], np.int32)
                if ctc.hyp_len[s, i] >= 0 else None for i in range(N)] for s in range(S)]
        res = ctc.MbrNbest(level=level)
        wall, phases = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            res = ctc.MbrNbest(level=level)
            wall.append(time.perf_counter() - t0)
            phases.append(ctc.MbrTimes())
        pairs = [(s, i, k) for s in range(S) for i in range(N) for k in range(i + 1, N) if tok[s][i] is not None and tok[s][k] is not None]
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        calls = [(ptr(tok[s][i]), int(tok[s][i].size), ptr(tok[s][k]), int(tok[s][k].size)) for s, i, k in pairs]
        err = C.c_int(0)
        ref = C.byref(err)
        fn = lib.eesen_edit_distance
        host, empty, got = [], [], None
        for _ in range(max(1, min(reps, 3))):
            got, sink = np.empty(len(calls), np.int32), np.empty(len(calls), np.int32)
            t0 = time.perf_counter()
            for j, (pa, la, pb, lb) in enumerate(calls):
                fn(pa, la, pb, lb, ref)
                got[j] = err.value
            host.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            for j, (pa, la, pb, lb) in enumerate(calls):
                fn(pa, 0, pb, 0, ref)
                sink[j] = err.value
            empty.append(time.perf_counter() - t0)
        same = all(res.dist[s, i, k] == d for (s, i, k), d in zip(pairs, got.tolist()))
        lengths = [c[1] for c in calls] + [c[3] for c in calls]
        out[f"level{level}"] = dict(pairs=len(pairs), cells=int(sum(c[1] * c[3] for c in calls)), longest=int(max(lengths) if lengths else 0),
                                    mean_len=round(float(np.mean(lengths)) if lengths else 0.0, 1), equal_to_host=bool(same),
                                    moved=int(sum(res.order[s, 0] != 0 for s in range(S))), mbr=dict(wall_ms=ms(wall), phases_ms=mean(phases)),
                                    host_ms=ms(host), host_empty_ms=ms(empty))
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
    for mode in ("plain", "lexicon"):
        for nbest in (16, 64):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", mode, "--nbest", str(nbest), "--reps", str(a.reps)],
                               capture_output=True, text=True, cwd=ROOT, timeout=900)
            if r.returncode != 0:      # nothing more is started on the device after a leg that failed
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"leg {mode} nbest {nbest} ended with {r.returncode}")
            rows.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("LEG ")][-1][4:]))
            print(json.dumps(rows[-1]), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ctc_mbr.json"), "w") as f:
        json.dump(dict(shape=SHAPE, lexicon=LEXICON, rows=rows), f, indent=1)
    print("| mode | nbest | level | pairs | DP cells | decode wall (ms) | MBR wall (ms) | build / kernel / host (ms) | host loop (ms) | of which the loop itself | host loop : MBR wall |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        for level in (0, 1):
            v = r.get(f"level{level}")
            if not v:
                continue
            p = v["mbr"]["phases_ms"]
            w, h, e = min(v["mbr"]["wall_ms"]), min(v["host_ms"]), min(v["host_empty_ms"])
            print(f"| {r['mode']} | {r['nbest']} | {level} | {v['pairs']} | {v['cells']} | {min(r['decode']['wall_ms']):.2f} | {w:.2f} | "
                  f"{p['build']:.2f} / {p['kernel']:.3f} / {p['host']:.2f} | {h:.1f} | {e:.1f} | {h / w:.1f} ({(h - e) / w:.1f} without the loop) |")


if __name__ == "__main__":
    main()
