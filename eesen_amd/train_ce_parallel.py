#!/usr/bin/env python3
"""train-ce-parallel on MI355X: the command-line contract of the reference's src/netbin/train-ce-parallel.cc.

Usage: python -m eesen_amd.train_ce_parallel [options] <feature-rspecifier> <labels-rspecifier> <model-in> [<model-out>]
e.g.:  python -m eesen_amd.train_ce_parallel --learn-rate=4e-5 --num-sequence=10 scp:feature.scp ark:ali_pdf.ark nnet.init nnet.iter1

Frame-level cross-entropy training on aligned frame targets (one int32 class id per frame, e.g. the output of ali-to-pdf)
with the same <Nnet> files as train-ctc-parallel.  Same options, same stderr contract (`FRAME_ACCURACY >> x% <<`), exit
code 0 / 255 (the reference returns -1).  One GPU: the reference's CE trainer has no multi-job mode.  The Python mirror of
eesen_amd/bin/train-ce-parallel: the same library calls in the same order, so both write the same model bytes.
"""
from __future__ import annotations

import os
import sys
import time

USAGE = ("Perform one iteration of Cross-entropy (CE) training by SGD.\n"
         "The updates are done per-utternace and by processing multiple utterances in parallel.\n"
         "\n"
         "Usage: train-ce-parallel [options] <feature-rspecifier> <labels-rspecifier> <model-in> [<model-out>]\n"
         "e.g.: \n"
         "train-ce-parallel scp:feature.scp ark:labels.ark nnet.init nnet.iter1\n")


def log(msg: str, level: str = "LOG", where: str = "main():eesen_amd/train_ce_parallel.py"):
    print(f"{level} (train-ce-parallel:{where}) {msg}", file=sys.stderr, flush=True)


def build_parser():
    """Options and help texts of train-ce-parallel.cc:40-61 and NetTrainOptions::Register (src/net/train-opts.h:45-51), then
    what the CTC trainer registers for one job."""
    from eesen_amd.parse_options import ParseOptions
    po = ParseOptions(USAGE, prog="train-ce-parallel")
    po.register("learn-rate", 0.008, "Learning rate")
    po.register("momentum", 0.0, "Momentum")
    po.register("adagrad-epsilon", 1e-6, "Epsilon for numerical stability for all adaptive optimizers (Adagrad, RMSProp)")
    po.register("rms-prop-rho", 0.9, "Rho parameter for RMSProp")
    po.register("binary", True, "Write model  in binary mode")
    po.register("cross-validate", False, "Perform cross-validation (no backpropagation)")
    po.register("num-sequence", 5, "Number of sequences processed in parallel")
    po.register("frame-limit", 100000.0, "Max number of frames to be processed", kind="double")
    po.register("report-step", 100, "Step (number of sequences) for status reporting")
    po.register("use-gpu", "yes", "yes|no|optional, only has effect if compiled with CUDA")
    po.register("opt-algorithm", "SGD", "Optimization algorithm (SGD|Adagrad|RMSProp)")
    po.register("device", -1, "GPU index (default: $LOCAL_RANK, else 0)")
    return po


class Counts:
    def __init__(self):
        self.num_no_tgt_mat = 0
        self.num_other_error = 0


def ce_groups(table, targets, num_sequence: int, frame_limit: float, feat_dim: int, counts: Counts, warn=lambda m: None):
    """The grouping of train-ce-parallel.cc:114-137: utterances are added until there are num_sequence of them or the
    padded frame count EXCEEDS frame_limit -- the test comes after the add, so a group may be larger than the limit.
    Yields [(key, feats [T_s x D], targets [T_s])] per group.  An utterance whose target vector differs in length from its
    features is skipped as an "other error" (undefined behaviour in the reference); an empty group is never yielded."""
    import numpy as np
    group, max_frame_num = [], 0
    for utt, mat in table:
        tg = targets.get(utt)
        if tg is None:                                       # :117-122
            warn(f"{utt}, missing targets")
            counts.num_no_tgt_mat += 1
            continue
        if len(tg) != mat.shape[0]:
            warn(f"{utt}, length mismatch of targets {len(tg)} and features {mat.shape[0]}")
            counts.num_other_error += 1
            continue
        if mat.shape[1] != feat_dim:
            raise ValueError(f"feature dimension {mat.shape[1]} does not match the net's InputDim {feat_dim}")
        max_frame_num = max(max_frame_num, mat.shape[0])     # :127
        group.append((utt, np.ascontiguousarray(mat, np.float32), np.asarray(tg, np.int32)))
        if len(group) == num_sequence or len(group) * max_frame_num > frame_limit:   # :132-136
            yield group
            group, max_frame_num = [], 0
    if group:
        yield group


def interleave_targets(group):
    """target_host of :143-151: row t*S + s = frame t of utterance s, 0 on padded rows; returns (targets, lens, T)."""
    import numpy as np
    lens = [len(g[2]) for g in group]
    T, S = max(lens), len(group)
    tg = np.zeros(T * S, np.int32)
    for s, (_, _, t) in enumerate(group):
        tg[s:len(t) * S:S] = t
    return tg, lens, T


def main(argv=None) -> int:
    from eesen_amd.parse_options import ParseError
    ap = build_parser()
    try:
        o = ap.read(argv)
    except ParseError as e:
        print(str(e), file=sys.stderr)
        return 255
    if len(o.args) != (3 if o.cross_validate else 4):      # :64-67
        ap.print_usage()
        return 1
    feature_rspecifier, targets_rspecifier, model_filename = o.args[:3]
    target_model_filename = None if o.cross_validate else o.args[3]
    try:
        from eesen_amd import kaldi_io
        from eesen_amd.api import Net, CE, CuMatrix, Feeder
        dev = o.device if o.device >= 0 else int(os.environ.get("LOCAL_RANK", "0"))
        net = Net(dev).Read(model_filename)                                       # :88
        net.SetTrainOptions(o.learn_rate, o.momentum)                             # :89
        net.SetUpdateAlgorithm(o.opt_algorithm, o.adagrad_epsilon, o.rms_prop_rho)
        ce = CE(dev)
        ce.SetReportStep(o.report_step)                                           # :99
        ce.SetGuard(net)       # a minibatch computed from a timed-out forward pass never reaches the statistics
        feeder = Feeder(dev, slots=2)
        feat_dim = net.InputDim()
        table = kaldi_io.read_mat_table(feature_rspecifier)                       # :94-95
        targets = kaldi_io.read_vec_int_table(targets_rspecifier)
        log(("CROSS-VALIDATION" if o.cross_validate else "TRAINING") + " STARTED")   # :103
        t0 = time.time()
        counts = Counts()
        num_done, total_frames = 0, 0
        groups = ce_groups(table, targets, o.num_sequence, o.frame_limit, feat_dim, counts, warn=lambda m: log(m, "WARNING"))

        def stage():
            g = next(groups, None)
            return (g, feeder.submit([m for _, m, _ in g])) if g is not None else (None, -1)

        def print_progress(wait):           # the KALDI_LOG of CE::EvalParallel (ce-loss.cc:153-167)
            for line in ce.Progress(wait):
                log(line, where="EvalParallel():eesen_amd/csrc/ce_host.cpp")

        diff_buf = None
        g, slot = stage()
        while g is not None:
            tg, lens, T = interleave_targets(g)
            S = len(g)
            net.SetSeqLengths(lens)                                               # :154
            net_out = net.Propagate(feeder.acquire(slot))                         # :157
            feeder.release(slot)
            if diff_buf is None or diff_buf.rows * diff_buf.stride < net_out.rows * net_out.stride:
                # (grows by half, as the native trainer's buffer: the list is sorted by length)
                if diff_buf is not None:
                    net.Synchronize()
                old = 0 if diff_buf is None else diff_buf.rows * diff_buf.stride
                need = max(net_out.rows * net_out.stride, old + old // 2)
                diff_buf = CuMatrix(-(-need // net_out.stride), net_out.cols, dev, zero=False)
            diff = CuMatrix.view(diff_buf.ptr, net_out.rows, net_out.cols, net_out.stride, dev, keepalive=diff_buf)
            ce.EvalParallel(net_out, tg, diff, lens, want_obj=False)              # :158
            if not o.cross_validate:                                              # :161-163
                net.Backpropagate(diff)
            print_progress(False)
            num_done += S                                                         # :165-166
            total_frames += T * S
            g, slot = stage()          # next batch: read and staged while the GPU runs this one's backward pass
        net.Synchronize()
        print_progress(True)
        if not o.cross_validate:                                                  # :172-174
            log(net.InfoGradient(o.opt_algorithm != "SGD"))
            net.Write(target_model_filename, o.binary)                            # :176-178
        el = max(time.time() - t0, 1e-9)
        log(f"Done {num_done} files, {counts.num_no_tgt_mat} with no targets, {counts.num_other_error} with other errors. "
            f"[{'CROSS-VALIDATION' if o.cross_validate else 'TRAINING'}, {el / 60:g} min, fps{total_frames / el:g}]")   # :180-185
        if ce.Dropped():
            log(f"{ce.Dropped()} minibatch(es) were computed from a timed-out forward pass and are not in the statistics", "WARNING")
        log(ce.Report())                                                          # :186
        return 0
    except Exception as e:      # :193-196
        print(str(e), file=sys.stderr)
        return 255


if __name__ == "__main__":
    sys.exit(main())
