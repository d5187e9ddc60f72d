#!/usr/bin/env python3
"""paste-feats: feature tables side by side (the reference's src/featbin/paste-feats.cc), from audio on MI355X.

Usage: python -m eesen_amd.paste_feats [options] <in-rspecifier1> <in-rspecifier2> [<in-rspecifier3> ...] <out-wspecifier>
   or: python -m eesen_amd.paste_feats [options] <in-rxfilename1> <in-rxfilename2> [<in-rxfilename3> ...] <out-wxfilename>
e.g.:  python -m eesen_amd.paste_feats --length-tolerance=2 "ark:compute-fbank-feats --num-mel-bins=40 scp,p:wav.scp ark:- |" \\
       "ark,s,cs:compute-kaldi-pitch-feats scp,p:wav.scp ark:- | process-kaldi-pitch-feats ark:- ark:- |" ark,scp:feats.ark,feats.scp

Two paths.  When the inputs are exactly the two pipes above (what eesen_amd.frontend.parse_feature_pipeline recognises as a
paste-feats head) neither pipe is run: the wav table is read once, batched by total samples, and every batch is one pass of the
feeder's EESEN_FEAT_FBANK_PITCH stage -- one upload, the filterbank, the pitch tracker and the join on the device, one copy back
(INTEGRATION.md "Fbank + pitch").  Any other inputs are joined on the host and need no device: the first table is read
sequentially, the others by key, as in the reference.  The reference's warnings, "Done N utts, errors on M" and exit status.
"""
from __future__ import annotations

import shlex
import sys

import numpy as np

BATCH_SAMPLES = 1 << 22      # as compute-kaldi-pitch-feats: the pitch tracker's scratch is what bounds a batch


def length_warning(frames, utt: str, tolerance: int) -> str:
    return f"Length mismatch {max(frames)} vs. {min(frames)}{' for utt ' + utt if utt else ''} exceeds tolerance {tolerance}"


def append_feats(mats, utt: str, tolerance: int, warn):
    """AppendFeats (paste-feats.cc:30-65): the matrices side by side, trimmed to the shortest; None (and the warning) when they differ
    by more than the tolerance or one is empty."""
    from eesen_amd.frontend import paste_frames
    frames = [m.shape[0] for m in mats]
    rows = paste_frames(frames, tolerance)
    if rows == 0:
        warn(length_warning(frames, utt, tolerance), "AppendFeats")
        return None
    return np.hstack([np.asarray(m, np.float32)[:rows] for m in mats])


class _ByKey:
    """RandomAccessBaseFloatMatrixReader: a sorted table (ark,s: / ark,s,cs:) is walked forward, any other is read whole."""

    def __init__(self, spec: str):
        from eesen_amd import kaldi_io
        opts = spec.partition(":")[0].split(",")
        self.sorted = opts[0] == "ark" and "s" in opts[1:]
        self.it = kaldi_io.read_mat_table(spec)
        self.cur = None
        self.table = None if self.sorted else dict(self.it)

    def get(self, key: str):
        if self.table is not None:
            return self.table.get(key)
        while True:
            if self.cur is None:
                self.cur = next(self.it, None)
                if self.cur is None:
                    return None
            if self.cur[0] == key:
                return self.cur[1]
            if self.cur[0] > key:
                return None
            self.cur = None


def _fused(pipe, tolerance: int, device: int, warn):
    """(key, pasted matrix or None) for every waveform of the wav table, the features computed on the device."""
    from eesen_amd import frontend
    from eesen_amd.api import Feeder
    feeder = Feeder(device, slots=1)
    pipe.configure(feeder)

    def flush(batch):
        rows = [feeder.pipeline_shape(1, w.shape[0])[0] for _, w in batch]
        keep = [i for i, r in enumerate(rows) if r]
        host = None
        if keep:
            slot = feeder.submit_raw([batch[i][1] for i in keep])
            got = feeder.acquire(slot)
            host = got.numpy().reshape(-1, len(keep), got.cols)
            feeder.release(slot)
        at = {i: k for k, i in enumerate(keep)}
        for i, (key, w) in enumerate(batch):
            if not rows[i]:
                n = w.shape[0]
                warn(length_warning([frontend.fbank_num_frames(n, pipe.fbank), pipe.pitch_rows(n)[0]], key, tolerance), "AppendFeats")
                yield key, None
            else:
                yield key, np.ascontiguousarray(host[:rows[i], at[i], :])

    batch, total = [], 0
    for key, wave in frontend._read_waves(pipe, pipe.source, lambda m: warn(m, "main")):
        if batch and total + wave.shape[0] > BATCH_SAMPLES:
            yield from flush(batch)
            batch, total = [], 0
        batch.append((key, wave))
        total += wave.shape[0]
    if batch:
        yield from flush(batch)


def main(argv=None) -> int:
    from eesen_amd.parse_options import ParseOptions, ParseError
    from eesen_amd.compute_fbank_feats import parse_wspecifier
    ap = ParseOptions("Paste feature files (assuming they have the same lengths);  think of the\n"
                      "unix command paste a b.\n"
                      "Usage: paste-feats <in-rspecifier1> <in-rspecifier2> [<in-rspecifier3> ...] <out-wspecifier>\n"
                      " or: paste-feats <in-rxfilename1> <in-rxfilename2> [<in-rxfilename3> ...] <out-wxfilename>\n"
                      " e.g. paste-feats ark:feats1.ark \"ark:select-feats 0-3 ark:feats2.ark ark:- |\" ark:feats-out.ark\n"
                      "  or: paste-feats foo.mat bar.mat baz.mat\n"
                      "See also: copy-feats, copy-matrix, append-vector-to-feats, concat-feats\n", prog="paste-feats")
    ap.register("length-tolerance", 0, "If length is different, trim as shortest up to a frame  difference of length-tolerance, otherwise exclude segment.")
    ap.register("binary", True, "If true, output files in binary (only relevant for single-file operation, i.e. no tables)")
    ap.register("device", 0, "GPU index (only when the inputs are the two recognised pipes from audio)")
    try:
        o = ap.read(argv)
    except ParseError as e:
        print(str(e), file=sys.stderr)
        return 255
    if len(o.args) < 3:
        ap.print_usage()
        return 1

    def warn(msg, where="main"):
        print(f"WARNING (paste-feats:{where}()) {msg}", file=sys.stderr)

    try:
        from eesen_amd import frontend, kaldi_io
        ins, out = o.args[:-1], o.args[-1]
        tol = o.length_tolerance
        if ins[0].partition(":")[0].split(",")[0] not in ("ark", "scp") or ":" not in ins[0]:
            mats = [kaldi_io.read_mat_file(a) for a in ins]        # rxfilenames: one matrix each
            m = append_feats(mats, "", tol, warn)
            if m is None:
                return 1
            kaldi_io.write_mat_file(out, m, o.binary)
            print(f"LOG (paste-feats:main()) Wrote appended features to {out}", file=sys.stderr)
            return 0
        ark, scp, text = parse_wspecifier(out)
        pipe = None
        if len(ins) == 2:
            pipe = frontend.parse_feature_pipeline(f"ark:paste-feats --length-tolerance={tol} {shlex.quote(ins[0])} {shlex.quote(ins[1])} ark:- |")
        num_done = num_err = 0

        def produce():
            nonlocal num_done, num_err
            if pipe is not None:
                for key, m in _fused(pipe, tol, o.device, warn):
                    if m is None:
                        num_err += 1
                        continue
                    num_done += 1
                    yield key, m
                return
            others = [_ByKey(a) for a in ins[1:]]
            for key, first in kaldi_io.read_mat_table(ins[0]):
                mats = [np.asarray(first, np.float32)]
                for a, rd in zip(ins[1:], others):
                    m = rd.get(key)
                    if m is None:
                        warn(f"Missing utt {key} from input {a}")
                        break
                    mats.append(np.asarray(m, np.float32))
                if len(mats) != len(ins):
                    num_err += 1
                    continue
                m = append_feats(mats, key, tol, warn)
                if m is None:
                    num_err += 1
                    continue
                num_done += 1
                yield key, m

        kaldi_io.write_mat_ark(ark, produce(), text=text, scp_path=scp)
        print(f"LOG (paste-feats:main()) Done {num_done} utts, errors on {num_err}", file=sys.stderr)
        return 0 if num_done else 255
    except Exception as e:
        print(f"ERROR (paste-feats:main()) {e}", file=sys.stderr)
        return 255


if __name__ == "__main__":
    sys.exit(main())
