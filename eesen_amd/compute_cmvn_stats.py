#!/usr/bin/env python3
"""compute-cmvn-stats on MI355X: CMVN statistics per utterance, per speaker or global (/root/reference/src/featbin/compute-cmvn-stats.cc).

Usage: python -m eesen_amd.compute_cmvn_stats [options] feats-rspecifier (stats-wspecifier|stats-wxfilename)
e.g.:  python -m eesen_amd.compute_cmvn_stats --spk2utt=ark:data/spk2utt scp:data/feats.scp ark,scp:cmvn.ark,cmvn.scp
       python -m eesen_amd.compute_cmvn_stats --spk2utt=ark:data/spk2utt "ark:compute-fbank-feats --num-mel-bins=40 scp:data/wav.scp ark:- |" ark,scp:cmvn.ark,cmvn.scp

The reference's options, three modes, warnings, final log line and exit status (0 if and only if an utterance was accumulated).  One
sequential pass over the feature rspecifier: utterances are batched by total floats and every batch is one call of the device
kernel (api.cmvn_stats), or, where the rspecifier is a pipe the front end recognises (eesen_amd.frontend), a feeder pipeline with
the statistics tap on its last boundary, so the features never come back to the host.  Every utterance's [2 x (D+1)] doubles are
kept; speakers are summed on the host in fp64 in the order of each spk2utt list, the global matrix in table order and rounded to
float once (INTEGRATION.md "CMVN statistics").  Deviations: --device is new; --weights with a pipeline rspecifier is refused.
"""
from __future__ import annotations

import os
import sys

import numpy as np

BATCH_FLOATS = 1 << 23      # 8 M floats (32 MB) per launch, as compute-fbank-feats batches its samples
WSPECIFIER_OPTIONS = ("t", "b", "f", "nf", "p")


def is_wspecifier(name: str) -> bool:
    """ClassifyWspecifier (util/kaldi-table.cc): options in front of the first ':' with `ark` or `scp` among them."""
    head, sep, _ = name.partition(":")
    opts = head.split(",")
    return bool(sep) and all(o in ("ark", "scp") + WSPECIFIER_OPTIONS for o in opts) and any(o in ("ark", "scp") for o in opts)


def main(argv=None) -> int:
    from eesen_amd.parse_options import ParseOptions, ParseError
    ap = ParseOptions("Compute cepstral mean and variance normalization statistics\n"
                      "If wspecifier provided: per-utterance by default, or per-speaker if\n"
                      "spk2utt option provided; if wxfilename: global\n"
                      "Usage: compute-cmvn-stats  [options] feats-rspecifier (stats-wspecifier|stats-wxfilename)\n", prog="compute-cmvn-stats")
    ap.register("spk2utt", "", "rspecifier for speaker to utterance-list map")
    ap.register("binary", True, "write in binary mode (applies only to global CMN/CVN)")
    ap.register("weights", "", "rspecifier for a vector of floats for each utterance, that's a per-frame weight.")
    ap.register("device", 0, "GPU index")
    try:
        o = ap.read(argv)
    except ParseError as e:
        print(str(e), file=sys.stderr)
        return 255
    if len(o.args) != 2:
        ap.print_usage()
        return 1
    rspecifier, out_name = o.args

    def warn(msg):
        print(f"WARNING (compute-cmvn-stats:main()) {msg}", file=sys.stderr)

    try:
        from eesen_amd import kaldi_io, frontend
        from eesen_amd.compute_fbank_feats import parse_wspecifier
        to_table = is_wspecifier(out_name)
        if not to_table and o.spk2utt:
            raise kaldi_io.KaldiIOError("--spk2utt option not compatible with wxfilename as output (did you forget ark:?)")
        pipe = None if os.environ.get("EESEN_HOST_FEATURE_PIPES") else frontend.parse_feature_pipeline(rspecifier)
        if pipe is not None and o.weights:
            raise kaldi_io.KaldiIOError("--weights is not supported with a feature pipeline computed on the device (the statistics tap is "
                                        "unweighted): write the features to an archive first")
        from eesen_amd import api
        weights = kaldi_io.read_vec_float_table(o.weights) if o.weights else None

        # ---- the one pass: (key, status, dim, rows, weight count, stats or None) of every utterance, in table order
        utts = []
        OK, NO_WEIGHTS, BAD_WEIGHTS = 0, 1, 2

        def flush(batch):
            if not batch:
                return
            if pipe is not None:
                slot = feeder.submit_raw([m.raw for _, m in batch], [m.cmvn for _, m in batch] if batch[0][1].cmvn is not None else None)
                stats = feeder.stats(slot)
            else:
                stats = api.cmvn_stats([m for _, m in batch], [weights[utts[i][0]] for i, _ in batch] if weights is not None else None, device=o.device)
            for (i, _), st in zip(batch, stats):
                utts[i][2] = st.shape[1] - 1
                utts[i][5] = st

        batch, total = [], 0
        if pipe is not None:
            feeder = api.Feeder(o.device, slots=2)
            pipe.configure(feeder)
            feeder.set_stats_tap(len(pipe.stages))
            for key, raw in frontend.read_raw(pipe, warn=warn):
                if batch and (total + raw.raw.size > BATCH_FLOATS or batch[0][1].raw.shape[1] != raw.raw.shape[1] or len(batch) == 65535):
                    flush(batch)
                    batch, total = [], 0
                utts.append([key, OK, raw.shape[1], raw.shape[0], 0, None])
                batch.append((len(utts) - 1, raw))
                total += raw.raw.size
        else:
            for key, m in kaldi_io.read_mat_table(rspecifier):
                m = np.ascontiguousarray(m, np.float32)
                if m.ndim != 2 or m.shape[1] == 0:
                    raise kaldi_io.KaldiIOError(f"feature matrix without columns for utterance {key}")
                status, wdim = OK, 0
                if weights is not None:
                    if key not in weights:
                        status = NO_WEIGHTS
                    elif len(weights[key]) != m.shape[0]:
                        status, wdim = BAD_WEIGHTS, len(weights[key])
                utts.append([key, status, m.shape[1], m.shape[0], wdim, None])
                if status != OK:
                    continue
                if batch and (total + m.size > BATCH_FLOATS or batch[0][1].shape[1] != m.shape[1] or len(batch) == 65535):    # a batch holds one width
                    flush(batch)
                    batch, total = [], 0
                batch.append((len(utts) - 1, m))
                total += m.size
        flush(batch)

        # ---- the three modes over the kept matrices
        num_done = num_err = 0

        def usable(u) -> bool:      # AccCmvnStatsWrapper's two warnings
            if u[1] == NO_WEIGHTS:
                warn(f"No weights available for utterance {u[0]}")
            if u[1] == BAD_WEIGHTS:
                warn(f"Weights for utterance {u[0]} have wrong dimension {u[4]} vs. {u[3]}")
            return u[1] == OK

        def add(acc, u):
            if acc.shape[1] != u[2] + 1:
                raise kaldi_io.KaldiIOError(f"feature dimension of utterance {u[0]} differs from the statistics it is added to")
            if u[1] == OK:
                acc += u[5]

        if to_table:
            ark, scp, text = parse_wspecifier(out_name)

            def produce():
                nonlocal num_done, num_err
                if o.spk2utt:
                    index = {u[0]: u for u in utts}
                    for spk, uttlist in kaldi_io.read_token_lists(o.spk2utt):
                        acc = None
                        for utt in uttlist:
                            u = index.get(utt)
                            if u is None:
                                warn(f"Did not find features for utterance {utt}")
                                num_err += 1
                                continue
                            if acc is None:     # InitCmvnStats on the first utterance found
                                acc = np.zeros((2, u[2] + 1), np.float64)
                            add(acc, u)
                            if usable(u):
                                num_done += 1
                            else:
                                num_err += 1
                        if acc is None:
                            warn(f"No stats accumulated for speaker {spk}")
                        else:
                            yield spk, acc
                else:
                    for u in utts:
                        if not usable(u):
                            num_err += 1
                            continue
                        num_done += 1
                        yield u[0], u[5]

            kaldi_io.write_mat64_ark(ark, produce(), text=text, scp_path=scp)
        else:
            acc = None
            for u in utts:
                if acc is None:
                    acc = np.zeros((2, u[2] + 1), np.float64)
                add(acc, u)
                if usable(u):
                    num_done += 1
                else:
                    num_err += 1
            stats_float = (acc if acc is not None else np.zeros((0, 0))).astype(np.float32)     # Matrix<float> stats_float(stats): rounded once
            with kaldi_io._open_out(out_name) as f:
                if o.binary:
                    f.write(kaldi_io._matrix_bytes(stats_float, False))
                else:
                    f.write(kaldi_io._matrix64_bytes(stats_float.astype(np.float64), True))     # the same 7 digits
                f.flush()
            print(f"LOG (compute-cmvn-stats:main()) Wrote global CMVN stats to {'standard output' if out_name == '-' else out_name}", file=sys.stderr)
        print(f"LOG (compute-cmvn-stats:main()) Done accumulating CMVN stats for {num_done} utterances; {num_err} had errors.", file=sys.stderr)
        return 0 if num_done else 1
    except Exception as e:
        print(f"ERROR (compute-cmvn-stats:main()) {e}", file=sys.stderr)
        return 255


if __name__ == "__main__":
    sys.exit(main())
