"""Generates tests/golden/frontend_edges.npz: the outputs of THE REFERENCE'S OWN add-deltas and splice-feats (oracle/_ref/featbin,
`make -C oracle/ref_build featbin`) at the limits eesen_feeder_set_pipeline accepts -- order 8, window 16, 64 frames of context -- on the
`limits` utterances of tests/feeder_cases.py.  No CMVN is involved.  TEST INFRASTRUCTURE; runs only where the reference exists.

    python -m oracle.make_golden_frontend_edges

The inputs are regenerated from seeds; the file holds a hash of them and, per pipeline and utterance, the tools' output.  Before it
writes, every output is held to oracle/frontend.py the way tests/test_feeder_cases.py holds the file afterwards: splices exactly, deltas
within feeder_cases.deltas_bound.  A reference that misses the bound is not written down.
"""
from __future__ import annotations

import json
import os
import tempfile

import numpy as np

from oracle import frontend as ofe
from oracle import make_golden_frontend as mg
from tests import feeder_cases as fc


def worst_ratio(stages, raw, got):
    """max |oracle - got| / bound over the elements of one utterance (0 where both are exact); asserts shape, exactness and the bound."""
    mine = ofe.run_pipeline(stages, raw)
    assert mine is not None and got.shape == mine.shape and got.dtype == np.float32, (stages, got.shape)
    bound = fc.limit_bound(stages, raw)
    if bound is None:
        assert np.array_equal(mine.view(np.uint32), got.view(np.uint32)), (stages, "splices are copies: bit-exact")
        return 0.0
    diff = np.abs(mine.astype(np.float64) - got.astype(np.float64))
    assert np.all(diff <= bound), (stages, float(np.max(diff / np.maximum(bound, 1e-300))))
    return float(np.max(diff[bound > 0] / bound[bound > 0], initial=0.0))


def main():
    assert os.path.isfile(os.path.join(mg.BIN, "add-deltas")), "build oracle/_ref first: make -C oracle/ref_build featbin"
    utts = fc.limit_utts()
    blob = {"hash": fc.input_hash([m for _, m in utts]), "names": json.dumps(sorted(fc.LIMIT_PIPELINES))}
    worst = 0.0
    for name, stages in sorted(fc.LIMIT_PIPELINES.items()):
        with tempfile.TemporaryDirectory() as tmp:
            outs, _ = mg.run_reference_tail(utts, fc.reference_tail(stages), tmp)
        assert sorted(outs) == sorted(k for k, _ in utts), (name, sorted(outs))
        ratio = max(worst_ratio(stages, raw, np.asarray(outs[k], np.float32)) for k, raw in utts)
        worst = max(worst, ratio)
        for k, _ in utts:
            blob[f"out/{name}/{k}"] = np.asarray(outs[k], np.float32)
        print(f"{name}: {[outs[k].shape for k, _ in utts]}, worst |oracle - reference| / bound {ratio:.4f}")
    np.savez_compressed(fc.GOLDEN, **blob)
    print("wrote", fc.GOLDEN, os.path.getsize(fc.GOLDEN), "bytes; worst ratio to the bound", f"{worst:.4f}")


if __name__ == "__main__":
    main()
