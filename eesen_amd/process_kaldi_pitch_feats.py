#!/usr/bin/env python3
"""process-kaldi-pitch-feats on MI355X: (NCCF, pitch) pairs to ASR features (the reference's src/featbin/process-kaldi-pitch-feats.cc).

Usage: python -m eesen_amd.process_kaldi_pitch_feats [options] <feat-rspecifier> <feats-wspecifier>

The option names of the reference's ProcessPitchOptions; matrices are batched by total frames and every batch is one launch
(eesen_pitch_process, INTEGRATION.md "Pitch").  Deviations: the delta-pitch noise is a counter-based generator keyed by --noise-seed,
the utterance's number in the table and the frame, so a run reproduces (--srand is accepted and unused;
--delta-pitch-noise-stddev=0 is the path held to the reference); an empty input matrix is skipped with a warning.
"""
from __future__ import annotations

import sys

BATCH_FRAMES = 1 << 20

# flag -> (field of eesen_pitch_opts_t, default, doc): ProcessPitchOptions::Register (pitch-functions.h:247-284), plus --noise-seed
PROCESS_OPTIONS = {
    "pitch-scale": ("pitch_scale", 2.0, "Scaling factor for the final normalized log-pitch value"),
    "pov-scale": ("pov_scale", 2.0, "Scaling factor for final POV (probability of voicing) feature"),
    "pov-offset": ("pov_offset", 0.0, "This can be used to add an offset to the POV feature. Intended for use in online decoding as a substitute for  CMN."),
    "delta-pitch-scale": ("delta_pitch_scale", 10.0, "Term to scale the final delta log-pitch feature"),
    "delta-pitch-noise-stddev": ("delta_pitch_noise_stddev", 0.005, "Standard deviation for noise we add to the delta log-pitch (before scaling); should be "
                                                                   "about the same as delta-pitch option to pitch creation."),
    "normalization-left-context": ("normalization_left_context", 75, "Left-context (in frames) for moving window normalization"),
    "normalization-right-context": ("normalization_right_context", 75, "Right-context (in frames) for moving window normalization"),
    "delta-window": ("delta_window", 2, "Number of frames on each side of central frame, to use for delta window."),
    "delay": ("delay", 0, "Number of frames by which the pitch information is delayed."),
    "add-pov-feature": ("add_pov_feature", True, "If true, the warped NCCF is added to output features"),
    "add-normalized-log-pitch": ("add_normalized_log_pitch", True, "If true, the log-pitch with POV-weighted mean subtraction over 1.5 second window is added to output features"),
    "add-delta-pitch": ("add_delta_pitch", True, "If true, time derivative of log-pitch is added to output features"),
    "add-raw-log-pitch": ("add_raw_log_pitch", False, "If true, log(pitch) is added to output features"),
    "noise-seed": ("noise_seed", 0, "Seed of the delta-pitch noise's counter-based generator (a seed reproduces its features)"),
}


def main(argv=None) -> int:
    from eesen_amd.parse_options import ParseOptions, ParseError
    from eesen_amd.compute_fbank_feats import parse_wspecifier
    ap = ParseOptions("Post-process Kaldi pitch features, consisting of pitch and NCCF, into\n"
                      "features suitable for input to ASR system.  Default setup produces\n"
                      "3-dimensional features consisting of (pov-feature, pitch-feature,\n"
                      "delta-pitch-feature); select from (pov-feature, pitch-feature,\n"
                      "delta-pitch-feature, raw-log-pitch), produced in that order.\n"
                      "Usage: process-kaldi-pitch-feats [options...] <feat-rspecifier> <feats-wspecifier>\n", prog="process-kaldi-pitch-feats")
    for flag, (_, default, doc) in PROCESS_OPTIONS.items():
        ap.register(flag, default, doc)
    ap.register("srand", 0, "Seed for random number generator [accepted and unused: see --noise-seed]")
    ap.register("device", 0, "GPU index")
    try:
        o = ap.read(argv)
    except ParseError as e:
        print(str(e), file=sys.stderr)
        return 255
    if len(o.args) != 2:
        ap.print_usage()
        return 1
    feat_rspecifier, output_wspecifier = o.args
    try:
        from eesen_amd import kaldi_io
        from eesen_amd.api import Pitch
        ark, scp, text = parse_wspecifier(output_wspecifier)
        pt = Pitch(o.device, **{field: getattr(o, flag.replace("-", "_")) for flag, (field, _, _) in PROCESS_OPTIONS.items()})
        num_done = 0

        def flush(batch):
            nonlocal num_done
            for (key, _, _), m in zip(batch, pt.process([m for _, _, m in batch], utt_ids=[i for _, i, _ in batch])):
                num_done += 1
                yield key, m

        def produce():
            batch, total = [], 0
            for n, (key, m) in enumerate(kaldi_io.read_mat_table(feat_rspecifier)):
                if m.shape[0] == 0:
                    print(f"WARNING (process-kaldi-pitch-feats:main()) Empty matrix for utterance {key}: producing no output.", file=sys.stderr)
                    continue
                if m.shape[1] != 2:
                    raise kaldi_io.KaldiIOError(f"Input feature must be pitch feature (should have dimension 2): utterance {key}")
                if batch and total + m.shape[0] > BATCH_FRAMES:
                    yield from flush(batch)
                    batch, total = [], 0
                batch.append((key, n, m))          # the utterance's number in the table keys its noise
                total += m.shape[0]
            if batch:
                yield from flush(batch)

        kaldi_io.write_mat_ark(ark, produce(), text=text, scp_path=scp)
        print(f"LOG (process-kaldi-pitch-feats:main()) Post-processed pitch for {num_done} utterances.", file=sys.stderr)
        return 0 if num_done else 1
    except Exception as e:
        print(f"ERROR (process-kaldi-pitch-feats:main()) {e}", file=sys.stderr)
        return 255


if __name__ == "__main__":
    sys.exit(main())
