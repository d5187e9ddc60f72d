#!/usr/bin/env python3
"""ctc-align on MI355X: best-path CTC alignment of utterances against their transcripts (the Python mirror of
eesen_amd/csrc/tools/ctc_align.cc: the same library calls in the same order, byte-identical tables).

Usage: python -m eesen_amd.ctc_align [options] <model-in> <feature-rspecifier> <labels-rspecifier> <alignment-wspecifier>
e.g.:  python -m eesen_amd.ctc_align --num-sequence=20 final.nnet scp:feats.scp ark:labels.ark ark:ali.ark

The reference has no such tool: it aligns ONE utterance per invocation through a TLG graph compiled for it and the WFST decoder
(asr_egs/wsj/steps/align_ctc_single_utt.sh:67-85).  Per group of --num-sequence utterances: forward pass as
net-output-extract -> optional log + prior subtraction (net-output-extract's options) -> Ctc.AlignParallel.  Written: one int32
vector per utterance, the class id of every frame (blank = 0) -- the targets table of train-ce-parallel.
"""
from __future__ import annotations

import math
import os
import sys


def main(argv=None) -> int:
    from eesen_amd.parse_options import ParseOptions, ParseError
    ap = ParseOptions("Align utterances against their label sequences: the best (Viterbi) CTC path through the network's outputs.\n"
                      "Writes the class id of every frame (blank = 0), the targets table of train-ce-parallel.\n"
                      "\n"
                      "Usage:  ctc-align [options] <model-in> <feature-rspecifier> <labels-rspecifier> <alignment-wspecifier>\n"
                      "e.g.: \n"
                      "ctc-align net ark:features.ark ark:labels.ark ark:ali.ark\n", prog="ctc-align")
    ap.register("class-frame-counts", "", "Vector with frame-counts of classes to compute log-priors; the alignment then runs on log-posteriors "
                                          "minus the scaled log-priors")
    ap.register("prior-scale", 1.0, "Scaling factor to be applied on class-log-priors")
    ap.register("prior-cutoff", 1e-10, "Classes with priors lower than cutoff will have 0 likelihood")
    ap.register("blank-scale", 1.0, "Scale probability of class 0 (blank) by this factor")
    ap.register("positions-wspecifier", "", "Also write the lattice position of every frame (position j of the labels interleaved with blanks: "
                                            "label j/2 when j is odd, a blank otherwise)")
    ap.register("use-gpu", "yes", "yes|no|optional (accepted for the recipes' command lines; this tool always runs on the GPU)")
    ap.register("num-sequence", 1, "Utterances forwarded and aligned together")
    ap.register("frame-limit", 1e5, "Max number of frames forwarded together", kind="double")
    ap.register("device", 0, "GPU index")
    try:
        o = ap.read(argv)
    except ParseError as e:
        print(str(e), file=sys.stderr)
        return 255
    if len(o.args) != 4:
        ap.print_usage()
        return 1
    model_filename, feature_rspecifier, labels_rspecifier, alignment_wspecifier = o.args

    def warn(msg):
        print(f"WARNING (ctc-align:main()) {msg}", file=sys.stderr)

    try:
        import ctypes as C
        import numpy as np
        from eesen_amd import kaldi_io, _lib, frontend
        from eesen_amd.api import Net, Ctc
        from eesen_amd.batching import interleave
        from eesen_amd.net_output_extract import class_log_priors

        def out_of(wspecifier):
            kind, path, text = kaldi_io._parse_specifier(wspecifier)
            if kind != "ark":
                raise kaldi_io.KaldiIOError("only ark: output is supported")
            return path, text

        ali_out = out_of(alignment_wspecifier)
        pos_out = out_of(o.positions_wspecifier) if o.positions_wspecifier else None
        net = Net(o.device).Read(model_filename)
        net.SetTestMode()
        ctc = Ctc(o.device)
        ctc.SetGuard(net)           # an alignment of a timed-out forward pass comes back as NaN, never as a table entry
        log_pri = class_log_priors(o.class_frame_counts, o.prior_cutoff, o.blank_scale) if o.class_frame_counts else None
        K = net.OutputDim()
        if log_pri is not None and log_pri.size != K:
            raise kaldi_io.KaldiIOError(f"Dimensionality mismatch, class_frame_counts {log_pri.size} class_output_llk {K}")
        labels = kaldi_io.read_vec_int_table(labels_rspecifier)
        pipe = frontend.parse_feature_pipeline(feature_rspecifier) if not os.environ.get("EESEN_HOST_FEATURE_PIPES") else None
        feeder = None
        if pipe is not None:
            from eesen_amd.api import Feeder
            feeder = Feeder(o.device, slots=1)
            pipe.configure(feeder)
        n = dict(done=0, no_labels=0, infeasible=0, frames=0, score=0.0)
        positions = []              # (key, positions) of the utterances written, for --positions-wspecifier

        def flush(group):
            for _, m in group:
                if m.shape[1] != net.InputDim():
                    raise kaldi_io.KaldiIOError(f"feature dimension {m.shape[1]} does not match the net's InputDim {net.InputDim()}")
            if pipe is not None:    # raw matrices: the filters of the rspecifier pipe run on the device (eesen_amd.frontend)
                lens = np.array([m.shape[0] for _, m in group], np.int32)
                slot = feeder.submit([m for _, m in group])
                net.SetSeqLengths(lens)
                out = net.Propagate(feeder.acquire(slot))
                feeder.release(slot)
            else:
                feats, lens, _ = interleave([m for _, m in group], net.InputDim())
                net.SetSeqLengths(lens)
                out = net.Propagate(feats)
            if log_pri is not None:
                _lib.check(_lib.load().eesen_op_log_sub_prior(o.device, None, C.c_void_p(out.ptr), out.rows, out.cols, out.stride, 1,
                                                              log_pri.ctypes.data_as(C.c_void_p), o.prior_scale))
            ali, pos, score = ctc.AlignParallel(lens, out, [labels[key] for key, _ in group], is_log=log_pri is not None)
            for s, (key, m) in enumerate(group):
                frames = int(lens[s])
                if math.isnan(score[s]):
                    raise RuntimeError(f"the forward pass of {key} timed out on the device: no alignment")
                if not score[s] > -1e29:
                    warn(f"{key}, no feasible alignment of {len(labels[key])} labels on {frames} frames, producing no output for this utterance")
                    n["infeasible"] += 1
                    continue
                n["done"] += 1; n["frames"] += frames; n["score"] += float(score[s])
                if pos_out:
                    positions.append((key, pos[:frames, s].copy()))
                yield key, ali[:frames, s]

        def produce():
            group, max_len = [], 0
            table = frontend.read_raw(pipe, warn=warn) if pipe is not None else kaldi_io.read_mat_table(feature_rspecifier)
            for key, mat in table:
                if key not in labels or len(labels[key]) == 0:
                    warn(f"{key}, missing labels")
                    n["no_labels"] += 1
                    continue
                if group and (len(group) == o.num_sequence or max(max_len, mat.shape[0]) * (len(group) + 1) > o.frame_limit):
                    yield from flush(group)
                    group, max_len = [], 0
                group.append((key, mat)); max_len = max(max_len, mat.shape[0])
            if group:
                yield from flush(group)

        kaldi_io.write_vec_int_ark(ali_out[0], produce(), text=ali_out[1])
        if pos_out:
            kaldi_io.write_vec_int_ark(pos_out[0], positions, text=pos_out[1])
        avg = n["score"] / n["frames"] if n["frames"] else 0.0
        print(f"LOG (ctc-align:main()) Done {n['done']} utterances, {n['no_labels']} without labels, {n['infeasible']} infeasible; "
              f"average best-path log-score per frame {avg:g}", file=sys.stderr)
        return 0 if n["done"] else 255
    except Exception as e:
        print(f"ERROR (ctc-align:main()) {e}", file=sys.stderr)
        return 255


if __name__ == "__main__":
    sys.exit(main())
