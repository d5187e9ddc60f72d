#!/usr/bin/env python3
"""compute-kaldi-pitch-feats on MI355X: (NCCF, pitch) pairs from a wav table (the reference's src/featbin/compute-kaldi-pitch-feats.cc).

Usage: python -m eesen_amd.compute_kaldi_pitch_feats [options] <wav-rspecifier> <feats-wspecifier>
e.g.:  python -m eesen_amd.compute_kaldi_pitch_feats --sample-frequency=8000 scp:data/wav.scp ark:- | \\
       python -m eesen_amd.process_kaldi_pitch_feats ark:- ark,scp:pitch.ark,pitch.scp

Every option name of the reference's PitchExtractionOptions; utterances are batched by total samples and every batch is one minibatch
of the device extractor (eesen_pitch_compute, INTEGRATION.md "Pitch").  Deviations: --frames-per-chunk, --simulate-first-pass-online,
--nccf-ballast-online and --preemphasis-coefficient are refused when set; a waveform too short for a frame gets the reference's
warning and no matrix (the reference writes an empty one).
"""
from __future__ import annotations

import sys

import numpy as np

BATCH_SAMPLES = 1 << 22      # 4 M samples per minibatch: 26 k frames of 16 kHz audio, 90 MB of NCCF rows on the device

# flag -> (field of eesen_pitch_opts_t, default, doc): PitchExtractionOptions::Register (pitch-functions.h:133-196)
PITCH_OPTIONS = {
    "sample-frequency": ("samp_freq", 16000.0, "Waveform data sample frequency (must match the waveform file, if specified there)"),
    "frame-length": ("frame_length_ms", 25.0, "Frame length in milliseconds"),
    "frame-shift": ("frame_shift_ms", 10.0, "Frame shift in milliseconds"),
    "preemphasis-coefficient": ("preemph_coeff", 0.0, "Coefficient for use in signal preemphasis (deprecated) [must be 0]"),
    "min-f0": ("min_f0", 50.0, "min. F0 to search for (Hz)"),
    "max-f0": ("max_f0", 400.0, "max. F0 to search for (Hz)"),
    "soft-min-f0": ("soft_min_f0", 10.0, "Minimum f0, applied in soft way, must not exceed min-f0"),
    "penalty-factor": ("penalty_factor", 0.1, "cost factor for FO change."),
    "lowpass-cutoff": ("lowpass_cutoff", 1000.0, "cutoff frequency for LowPass filter (Hz) "),
    "resample-frequency": ("resample_freq", 4000.0, "Frequency that we down-sample the signal to.  Must be more than twice lowpass-cutoff"),
    "delta-pitch": ("delta_pitch", 0.005, "Smallest relative change in pitch that our algorithm measures"),
    "nccf-ballast": ("nccf_ballast", 7000.0, "Increasing this factor reduces NCCF for quiet frames"),
    "nccf-ballast-online": ("nccf_ballast_online", False, "This is useful mainly for debug; it affects how the NCCF ballast is computed. [not supported]"),
    "lowpass-filter-width": ("lowpass_filter_width", 1, "Integer that determines filter width of lowpass filter, more gives sharper filter"),
    "upsample-filter-width": ("upsample_filter_width", 5, "Integer that determines filter width when upsampling NCCF"),
    "frames-per-chunk": ("frames_per_chunk", 0, "Only relevant for offline pitch extraction with online compatibility [not supported: must be 0]"),
    "simulate-first-pass-online": ("simulate_first_pass_online", False, "If true, output the features an online decoder would see in the first pass [not supported]"),
    "recompute-frame": ("recompute_frame", 500, "The frame below which an utterance's NCCF is re-scaled once the whole signal's energy is known"),
    "max-frames-latency": ("max_frames_latency", 0, "Maximum number of frames of latency that we allow pitch tracking to introduce (no effect offline)"),
    "snip-edges": ("snip_edges", True, "If this is set to false, the incomplete frames near the ending edge won't be snipped, so that the number of "
                                       "frames is the file size divided by the frame-shift. This makes different types of features give the same number of frames."),
}


def main(argv=None) -> int:
    from eesen_amd.parse_options import ParseOptions, ParseError
    from eesen_amd.compute_fbank_feats import parse_wspecifier
    ap = ParseOptions("Apply Kaldi pitch extractor, starting from wav input.  Output is 2-dimensional\n"
                      "features consisting of (NCCF, pitch in Hz), where NCCF is between -1 and 1, and\n"
                      "higher for voiced frames.  You will typically pipe this into\n"
                      "process-kaldi-pitch-feats.\n"
                      "Usage: compute-kaldi-pitch-feats [options...] <wav-rspecifier> <feats-wspecifier>\n", prog="compute-kaldi-pitch-feats")
    for flag, (_, default, doc) in PITCH_OPTIONS.items():
        ap.register(flag, default, doc)
    ap.register("device", 0, "GPU index")
    try:
        o = ap.read(argv)
    except ParseError as e:
        print(str(e), file=sys.stderr)
        return 255
    if len(o.args) != 2:
        ap.print_usage()
        return 1
    wav_rspecifier, output_wspecifier = o.args

    def warn(msg, where="main"):
        print(f"WARNING (compute-kaldi-pitch-feats:{where}()) {msg}", file=sys.stderr)

    try:
        from eesen_amd import kaldi_io
        from eesen_amd.api import Pitch
        ark, scp, text = parse_wspecifier(output_wspecifier)
        pt = Pitch(o.device, **{field: getattr(o, flag.replace("-", "_")) for flag, (field, _, _) in PITCH_OPTIONS.items()})
        want = float(np.float32(o.sample_frequency))
        num_done = 0

        def flush(batch):
            nonlocal num_done
            for (key, _), m in zip(batch, pt.compute([w for _, w in batch])):
                if m.shape[0] == 0:
                    warn(f"No frames output in pitch extraction for utterance {key}", "ComputeKaldiPitch")
                    continue
                num_done += 1
                yield key, m

        def produce():
            batch, total = [], 0
            for key, (rate, data) in kaldi_io.read_wav_table(wav_rspecifier):
                chan = kaldi_io.select_channel(key, data, -1, warn)
                if rate != want:
                    raise kaldi_io.KaldiIOError(f"Sample frequency mismatch: you specified {want:g} but data has {rate:g} (use --sample-frequency "
                                                f"option).  Utterance is {key}")
                if batch and total + chan.size > BATCH_SAMPLES:
                    yield from flush(batch)
                    batch, total = [], 0
                batch.append((key, chan))
                total += chan.size
            if batch:
                yield from flush(batch)

        kaldi_io.write_mat_ark(ark, produce(), text=text, scp_path=scp)
        print(f"LOG (compute-kaldi-pitch-feats:main()) Done {num_done} utterances, 0 with errors.", file=sys.stderr)
        return 0 if num_done else 1
    except Exception as e:
        print(f"ERROR (compute-kaldi-pitch-feats:main()) {e}", file=sys.stderr)
        return 255


if __name__ == "__main__":
    sys.exit(main())
