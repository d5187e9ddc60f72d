#!/usr/bin/env python3
"""compute-fbank-feats on MI355X: log-mel filterbank features from a wav table (/root/reference/src/featbin/compute-fbank-feats.cc).

Usage: python -m eesen_amd.compute_fbank_feats [options] <wav-rspecifier> <feats-wspecifier>
e.g.:  python -m eesen_amd.compute_fbank_feats --num-mel-bins=40 scp:data/wav.scp ark,scp:fbank.ark,fbank.scp

The reference's option names and defaults; utterances are batched by total samples and every batch is one launch of the device
extractor (eesen_fbank_compute, INTEGRATION.md "Fbank").  Deviations: --dither-seed is new (the dither is a counter-based generator
keyed by seed, utterance number, frame and sample, so a run reproduces; --dither=0 is the path held to the reference);
--vtln-map, --utt2spk, --output-format=htk and --round-to-power-of-two=false are refused.
"""
from __future__ import annotations

import sys

import numpy as np

BATCH_SAMPLES = 1 << 23      # 8 M samples (32 MB of float32, nine minutes of 16 kHz audio) per launch


def parse_wspecifier(spec: str):
    """(archive path, scp path or None, text) of `ark:`, `ark,t:`, `scp:` is not a writer; `ark,scp:a.ark,a.scp` writes both."""
    head, sep, rest = spec.partition(":")
    opts = head.split(",")
    if not sep or "ark" not in opts:
        raise ValueError(f"unsupported wspecifier '{spec}' (expected ark:..., ark,t:... or ark,scp:...,...)")
    text = "t" in opts
    if "scp" in opts:
        a, comma, b = rest.partition(",")
        if not comma:
            raise ValueError(f"wspecifier '{spec}' names one file for an archive and a script")
        ark, scp = (a, b) if opts.index("ark") < opts.index("scp") else (b, a)
        return ark, scp, text
    return rest, None, text


def main(argv=None) -> int:
    from eesen_amd.parse_options import ParseOptions, ParseError
    from eesen_amd.frontend import FBANK_OPTIONS
    ap = ParseOptions("Create Mel-filter bank (FBANK) feature files.\n"
                      "Usage:  compute-fbank-feats [options...] <wav-rspecifier> <feats-wspecifier>\n", prog="compute-fbank-feats")
    docs = {"sample-frequency": (16000.0, "Waveform data sample frequency (must match the waveform file, if specified there)"),
            "frame-length": (25.0, "Frame length in milliseconds"), "frame-shift": (10.0, "Frame shift in milliseconds"),
            "preemphasis-coefficient": (0.97, "Coefficient for use in signal preemphasis"),
            "remove-dc-offset": (True, "Subtract mean from waveform on each frame"), "dither": (1.0, "Dithering constant (0.0 means no dither)"),
            "window-type": ("povey", 'Type of window ("hamming"|"hanning"|"povey"|"rectangular")'),
            "round-to-power-of-two": (True, "If true, round window size to power of two."),
            "snip-edges": (True, "If true, end effects will be handled by outputting only frames that completely fit in the file, and the number of "
                                 "frames depends on the frame-length.  If false, the number of frames depends only on the frame-shift, and we "
                                 "reflect the data at the ends."),
            "num-mel-bins": (23, "Number of triangular mel-frequency bins"), "low-freq": (20.0, "Low cutoff frequency for mel bins"),
            "high-freq": (0.0, "High cutoff frequency for mel bins (if < 0, offset from Nyquist)"),
            "vtln-low": (100.0, "Low inflection point in piecewise linear VTLN warping function"),
            "vtln-high": (-500.0, "High inflection point in piecewise linear VTLN warping function (if negative, offset from high-mel-freq"),
            "use-energy": (False, "Add an extra dimension with energy to the FBANK output."),
            "energy-floor": (0.0, "Floor on energy (absolute, not relative) in FBANK computation"),
            "raw-energy": (True, "If true, compute energy before preemphasis and windowing"),
            "htk-compat": (False, "If true, put energy last.  Warning: not sufficient to get HTK compatible features (need to change other parameters)."),
            "use-log-fbank": (True, "If true, produce log-filterbank, else produce linear."),
            "vtln-warp": (1.0, "Vtln warp factor (only applicable if vtln-map not specified)"),
            "dither-seed": (0, "Seed of the dither's counter-based generator (a seed reproduces its features)")}
    for name, (default, doc) in docs.items():
        ap.register(name, default, doc)
    ap.register("subtract-mean", False, "Subtract mean of each feature file [CMS]; not recommended to do it this way. ")
    ap.register("vtln-map", "", "Map from utterance or speaker-id to vtln warp factor (rspecifier) [not supported]")
    ap.register("utt2spk", "", "Utterance to speaker-id map (if doing VTLN and you have warps per speaker) [not supported]")
    ap.register("channel", -1, "Channel to extract (-1 -> expect mono, 0 -> left, 1 -> right)")
    ap.register("min-duration", 0.0, "Minimum duration of segments to process (in seconds).")
    ap.register("output-format", "kaldi", "Format of the output files [kaldi only]")
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

    def warn(msg):
        print(f"WARNING (compute-fbank-feats:main()) {msg}", file=sys.stderr)

    try:
        from eesen_amd import kaldi_io
        from eesen_amd.api import Fbank
        if o.vtln_map or o.utt2spk:
            raise kaldi_io.KaldiIOError("--vtln-map / --utt2spk are not supported: one --vtln-warp per run")
        if o.output_format != "kaldi":
            raise kaldi_io.KaldiIOError(f"--output-format={o.output_format} is not supported (kaldi only)")
        ark, scp, text = parse_wspecifier(output_wspecifier)
        fb = Fbank(o.device, **{field: getattr(o, flag.replace("-", "_")) for flag, (field, _) in FBANK_OPTIONS.items()})
        want = float(np.float32(o.sample_frequency))
        num_utts = num_success = 0

        def flush(batch):
            nonlocal num_success
            feats = fb.compute([w for _, _, w in batch], utt_ids=[i for _, i, _ in batch])
            for (key, _, _), m in zip(batch, feats):
                if m.shape[0] == 0:             # (the reference fails on a waveform shorter than a frame)
                    warn(f"Failed to compute features for utterance {key}")
                    continue
                if o.subtract_mean:             # compute-fbank-feats.cc:150-156, on the host behind the copy back
                    mean = (m.sum(axis=0, dtype=np.float32) * np.float32(1.0 / m.shape[0])).astype(np.float32)
                    m = m - mean[None, :]
                num_success += 1
                yield key, m

        def produce():
            nonlocal num_utts
            batch, total = [], 0
            for key, (rate, data) in kaldi_io.read_wav_table(wav_rspecifier):
                num_utts += 1
                if data.shape[1] / rate < o.min_duration:
                    warn(f"File: {key} is too short ({data.shape[1] / rate:g} sec): producing no output.")
                    continue
                chan = kaldi_io.select_channel(key, data, o.channel, warn)
                if chan is None:
                    continue
                if rate != want:
                    raise kaldi_io.KaldiIOError(f"Sample frequency mismatch: you specified {want:g} but data has {rate:g} (use --sample-frequency "
                                                f"option).  Utterance is {key}")
                if batch and total + chan.size > BATCH_SAMPLES:
                    yield from flush(batch)
                    batch, total = [], 0
                batch.append((key, num_utts - 1, chan))
                total += chan.size
            if batch:
                yield from flush(batch)

        kaldi_io.write_mat_ark(ark, produce(), text=text, scp_path=scp)
        print(f"LOG (compute-fbank-feats:main())  Done {num_success} out of {num_utts} utterances.", file=sys.stderr)
        return 0 if num_success else 1
    except Exception as e:
        print(f"ERROR (compute-fbank-feats:main()) {e}", file=sys.stderr)
        return 255


if __name__ == "__main__":
    sys.exit(main())
