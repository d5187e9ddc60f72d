#!/usr/bin/env python3
"""ctc-decode on MI355X: lexicon-free CTC prefix beam search of utterances (the Python mirror of eesen_amd/csrc/tools/ctc_decode.cc:
the same library calls in the same order, byte-identical tables).

Usage: python -m eesen_amd.ctc_decode [options] <model-in> <feature-rspecifier> <hyp-wspecifier>
e.g.:  python -m eesen_amd.ctc_decode --num-sequence=20 --beam=16 final.nnet scp:feats.scp ark:hyp.ark

The reference has no such tool: it decodes ONE utterance per process through a TLG graph and its WFST decoder.  Per group of
--num-sequence utterances: forward pass as net-output-extract -> optional log + prior subtraction (net-output-extract's options) ->
Ctc.DecodeParallel.  Written: one int32 vector per hypothesis, the labels (blank-free); with --nbest > 1 under the keys utt-1, utt-2, ...
With --lm a token n-gram LM (an ARPA file over the net's tokens) is fused into the search (api.TokenLm).
With --lexicon the labellings are held to lexicon words separated by --space-unit, scored by an optional word n-gram LM (--word-lm):
api.Lexicon; the word ids go to --words-wspecifier and word errors are counted against --word-ref-rspecifier.
With --word-boundary=none the lexicon has no boundary unit (the phoneme systems: nothing but CTC's blank between words, homophones
allowed): api.Lexicon(space=None); the word ends go to --word-ends-wspecifier.
With --ctm-out the best hypothesis of every utterance is aligned to the frames (Ctc.DecodeStamps) and written as CTM lines
`key 1 start duration word [confidence]`, the file sclite scores.
With --rescore=true every returned hypothesis gets its exact acoustic score and the list is ranked again, optionally with a second LM
(--rescore-lm): Ctc.RescoreNbest.  Everything is then written in the new order and speaks of the new best hypothesis.
With --mbr=true every list is ranked by expected errors under its own posterior (over the second pass's totals with --rescore):
Ctc.MbrNbest.  Everything is written in that order, the errors against the references come back with it, and the summary adds the
errors of the N-best oracle.
"""
from __future__ import annotations

import math
import os
import sys


def _space_class(unit: str, units_path: str) -> int:
    """The class id of --space-unit: a symbol of the units table, or a decimal id without one."""
    if not units_path:
        if not (unit.isascii() and unit.isdigit() and len(unit) <= 9):
            raise ValueError(f"--space-unit={unit} is no decimal class id (give --lexicon-units to name it by its symbol)")
        return int(unit)
    try:
        lines = open(units_path).read().splitlines()
    except OSError:
        raise ValueError(f"cannot open {units_path}")
    for line in lines:
        f = line.split()
        if len(f) >= 2 and f[0] == unit and f[1].isascii() and f[1].isdigit() and len(f[1]) <= 9:
            return int(f[1])
    raise ValueError(f"--space-unit={unit} is not in {units_path}")


def _id_symbols(path: str) -> dict:
    """`symbol id` lines -> id -> symbol (the first symbol of an id wins)."""
    try:
        lines = open(path).read().splitlines()
    except OSError:
        raise ValueError(f"cannot open {path}")
    out = {}
    for line in lines:
        f = line.split()
        if len(f) >= 2 and f[1].isascii() and f[1].isdigit() and len(f[1]) <= 9:
            out.setdefault(int(f[1]), f[0])
    return out


def main(argv=None) -> int:
    from eesen_amd.parse_options import ParseOptions, ParseError
    ap = ParseOptions("Decode utterances without a lexicon: CTC prefix beam search over the network's outputs.\n"
                      "Writes the most probable label sequences (blank-free int32 vectors); with --nbest > 1 under the keys utt-1, utt-2, ...\n"
                      "\n"
                      "Usage:  ctc-decode [options] <model-in> <feature-rspecifier> <hyp-wspecifier>\n"
                      "e.g.: \n"
                      "ctc-decode --beam=16 net ark:features.ark ark:hyp.ark\n", prog="ctc-decode")
    ap.register("class-frame-counts", "", "Vector with frame-counts of classes to compute log-priors; the search then runs on log-posteriors "
                                          "minus the scaled log-priors")
    ap.register("prior-scale", 1.0, "Scaling factor to be applied on class-log-priors")
    ap.register("prior-cutoff", 1e-10, "Classes with priors lower than cutoff will have 0 likelihood")
    ap.register("blank-scale", 1.0, "Scale probability of class 0 (blank) by this factor")
    ap.register("beam", 16, "Prefixes kept per frame (1 .. 64)")
    ap.register("max-classes", 20, "Non-blank classes a prefix is extended by per frame: the best of the frame (1 .. 64; beam * max-classes <= 2048)")
    ap.register("nbest", 1, "Hypotheses written per utterance (1 .. beam)")
    ap.register("scores-out", "", "Also write `key log-probability` text lines, one per hypothesis, to this file")
    ap.register("ref-rspecifier", "", "Reference label sequences: the token errors of the best hypotheses against them are counted")
    ap.register("lm", "", "ARPA file of a token n-gram LM (its words: the symbols of --lm-units, or class ids) fused into the search")
    ap.register("lm-units", "", "units.txt of the LM's words: `symbol id` per line; without it the ARPA's words are decimal class ids")
    ap.register("lm-weight", 1.0, "Weight of the LM's log-probability of every label")
    ap.register("insertion-bonus", 0.0, "Added per label, in nats")
    ap.register("lm-eos", False, "Add the weighted log-probability of </s> at the end of every hypothesis")
    ap.register("lexicon", "", "Lexicon, `word unit unit ...` per spelling: the hypotheses are its words separated by --space-unit")
    ap.register("lexicon-units", "", "units.txt of the lexicon's units: `symbol id` per line; without it they are decimal class ids")
    ap.register("space-unit", "<SPACE>", "The unit between words: a symbol of --lexicon-units, or a decimal class id without it")
    ap.register("word-boundary", "unit", "unit: words are separated by --space-unit; none: nothing but CTC's blank stands between words and "
                                         "several words may share a spelling (the phoneme systems)")
    ap.register("word-ends-wspecifier", "", "With --word-boundary=none: also write, per hypothesis, the number of labels up to and "
                                            "including each word's last (int32 vectors)")
    ap.register("word-lm", "", "ARPA file of a word n-gram LM over the lexicon's words, stepped once per word (weight: --lm-weight)")
    ap.register("word-bonus", 0.0, "Added per word, in nats")
    ap.register("lm-skip-oov", False, "Drop the n-grams of --word-lm that hold a word outside the lexicon instead of refusing the file")
    ap.register("lm-lookahead", False, "Rank the candidates of a frame as if the most probable word (by --word-lm's unigrams) that the "
                                       "lexicon still allows had been paid already: a narrow --beam prunes better")
    ap.register("words-wspecifier", "", "Also write the word ids of every hypothesis (int32 vectors, the keys of <hyp-wspecifier>)")
    ap.register("words-table-out", "", "Write the lexicon's `word id` table to this file")
    ap.register("word-ref-rspecifier", "", "Reference word-id sequences: the word errors of the best hypotheses against them are counted")
    ap.register("ctm-out", "", "Also write the best hypothesis of every utterance as CTM lines `key 1 start duration word` to this file: "
                               "its words aligned to the frames")
    ap.register("frame-shift", 0.01, "Seconds per frame of the network's output (the recipes subsample by 3: 0.03)", kind="double")
    ap.register("ctm-precision", 2, "Digits behind the point of the CTM's times and confidences")
    ap.register("ctm-conf", False, "A sixth CTM column: the word's posterior over the --nbest hypotheses")
    ap.register("conf-scale", 1.0, "Scale of the hypotheses' log-probabilities in that posterior (>= 0)", kind="double")
    ap.register("ctm-units", "", "units.txt naming the CTM's words without a lexicon: `symbol id` per line (default: --lm-units; else class ids)")
    ap.register("rescore", False, "Second pass: score every hypothesis exactly, rank the list again and write everything in the new order")
    ap.register("rescore-lm", "", "ARPA file of the second pass's LM: over --lm-units' tokens, or over the lexicon's words with --lexicon "
                                  "(default: the first pass's LM scores)")
    ap.register("rescore-lm-weight", "", "Weight of the LM score in the second pass (default: --lm-weight)")
    ap.register("rescore-bonus", "", "Added per label or, with --lexicon, per word in the second pass (default: --insertion-bonus or --word-bonus)")
    ap.register("rescore-lm-eos", "", "true|false: --rescore-lm's log-probability of </s> joins at the end (default: --lm-eos)")
    ap.register("mbr", False, "Minimum Bayes risk: rank every list by its hypotheses' expected errors under the list's own posterior and write "
                              "everything in that order")
    ap.register("mbr-scale", "", "Scale of the hypotheses' log-probabilities in that posterior, >= 0 (default: 1.0)")
    ap.register("mbr-units", False, "Count the expected errors in labels even with --lexicon (default: in labels, or in words with --lexicon)")
    ap.register("use-gpu", "yes", "yes|no|optional (accepted for the recipes' command lines; this tool always runs on the GPU)")
    ap.register("num-sequence", 1, "Utterances forwarded and decoded together")
    ap.register("frame-limit", 1e5, "Max number of frames forwarded together", kind="double")
    ap.register("device", 0, "GPU index")
    try:
        o = ap.read(argv)
    except ParseError as e:
        print(str(e), file=sys.stderr)
        return 255
    if len(o.args) != 3:
        ap.print_usage()
        return 1
    model_filename, feature_rspecifier, hyp_wspecifier = o.args

    def warn(msg):
        print(f"WARNING (ctc-decode:main()) {msg}", file=sys.stderr)

    def log(msg):
        print(f"LOG (ctc-decode:main()) {msg}", file=sys.stderr)

    def number_option(name, text):      # a --rescore-* value kept as text so that "not given" can stand for the first pass's value
        from eesen_amd.parse_options import _strtod
        v = _strtod(text)
        if v is None:
            raise ValueError(f'Invalid floating-point option "{text}" of --{name}')
        return v

    def bool_option(name, text):
        if text.lower() in ("true", "t", "1"):
            return True
        if text.lower() in ("false", "f", "0"):
            return False
        raise ValueError(f"Invalid format for boolean argument [expected true or false] of --{name}: {text.lower()}")

    try:
        if not o.rescore and (o.rescore_lm or o.rescore_lm_weight or o.rescore_bonus or o.rescore_lm_eos):
            raise ValueError("--rescore-lm, --rescore-lm-weight, --rescore-bonus and --rescore-lm-eos need --rescore=true")
        if not o.mbr and (o.mbr_scale or o.mbr_units):
            raise ValueError("--mbr-scale and --mbr-units need --mbr=true")
        mbr_c = number_option("mbr-scale", o.mbr_scale) if o.mbr_scale else 1.0
        second_weight = number_option("rescore-lm-weight", o.rescore_lm_weight) if o.rescore_lm_weight else o.lm_weight
        second_bonus = number_option("rescore-bonus", o.rescore_bonus) if o.rescore_bonus else (o.word_bonus if o.lexicon else o.insertion_bonus)
        second_eos = bool_option("rescore-lm-eos", o.rescore_lm_eos) if o.rescore_lm_eos else o.lm_eos
        import ctypes as C
        import numpy as np
        from eesen_amd import kaldi_io, _lib, frontend
        from eesen_amd.api import Net, Ctc, TokenLm, Lexicon
        from eesen_amd.batching import interleave
        from eesen_amd.net_output_extract import class_log_priors

        kind, out_path, out_text = kaldi_io._parse_specifier(hyp_wspecifier)
        if kind != "ark":
            raise kaldi_io.KaldiIOError("only ark: output is supported")
        net = Net(o.device).Read(model_filename)
        net.SetTestMode()
        ctc = Ctc(o.device)
        ctc.SetGuard(net)           # hypotheses of a timed-out forward pass come back as NaN, never as table entries
        log_pri = class_log_priors(o.class_frame_counts, o.prior_cutoff, o.blank_scale) if o.class_frame_counts else None
        K = net.OutputDim()
        lm = None
        if o.lexicon and o.lm:
            raise kaldi_io.KaldiIOError("--lexicon together with --lm: the token LM and the word LM cannot be combined")
        if o.lm:
            lm = TokenLm(o.lm, o.lm_units or None, K=K)
        elif o.lm_units and not o.rescore_lm:
            raise kaldi_io.KaldiIOError("--lm-units without --lm")
        second_lm = None
        lex = None
        if o.word_boundary not in ("unit", "none"):
            raise kaldi_io.KaldiIOError(f"--word-boundary={o.word_boundary} is neither unit nor none")
        unspaced = o.word_boundary == "none"
        if unspaced and not o.lexicon:
            raise kaldi_io.KaldiIOError("--word-boundary=none needs --lexicon")
        if unspaced and o.space_unit != "<SPACE>":
            raise kaldi_io.KaldiIOError(f"--space-unit={o.space_unit} together with --word-boundary=none: there is no unit between words")
        if not unspaced and o.word_ends_wspecifier:
            raise kaldi_io.KaldiIOError("--word-ends-wspecifier needs --word-boundary=none")
        if o.lexicon:
            if unspaced:
                lex = Lexicon(o.lexicon, o.lexicon_units or None, K=K, space=None)
                log(f"the largest homophone set of {o.lexicon} holds {lex.MaxHomophones()} words")
            else:
                lex = Lexicon(o.lexicon, o.lexicon_units or None, K=K, space=_space_class(o.space_unit, o.lexicon_units))
            if o.words_table_out:
                lex.WriteWords(o.words_table_out)
            def word_lm_of(arpa):          # a word LM reads its words through the lexicon's table
                table = o.words_table_out
                if not table:          # a file of our own, created exclusively, gone as soon as the LM has read it
                    import tempfile
                    fd, table = tempfile.mkstemp(prefix="ctc-decode-words.")
                    os.close(fd)
                try:
                    if not o.words_table_out:
                        lex.WriteWords(table)
                    made = TokenLm(arpa, table, K=lex.Info()["words"] + 1, skip_oov=o.lm_skip_oov)
                finally:
                    if not o.words_table_out:
                        os.remove(table)
                if o.lm_skip_oov:
                    log(f"{made.OovDropped()} n-grams of {arpa} hold a word outside the lexicon and were dropped")
                return made
            if o.word_lm:
                lm = word_lm_of(o.word_lm)
            if o.rescore_lm:
                second_lm = word_lm_of(o.rescore_lm)
        elif o.lexicon_units or o.word_lm or o.words_wspecifier or o.words_table_out or o.word_ref_rspecifier or o.word_bonus != 0.0 or o.lm_skip_oov:
            raise kaldi_io.KaldiIOError("--lexicon-units, --word-lm, --word-bonus, --lm-skip-oov, --words-wspecifier, --words-table-out and "
                                        "--word-ref-rspecifier need --lexicon")
        if lex is None and o.rescore_lm:
            second_lm = TokenLm(o.rescore_lm, o.lm_units or None, K=K)
        if o.lm_lookahead:
            if lex is None:
                raise kaldi_io.KaldiIOError("--lm-lookahead needs --lexicon and --word-lm")
            ctc.SetLmLookahead(1)          # (without --word-lm the library refuses the first decode call)
            if lm is not None:
                la = lex.Lookahead(lm)
                log(f"unigram look-ahead over {la.size} lexicon nodes, la in [{float(la.min()):.9g}, {float(la[0]):.9g}]")
        # the CTM's word symbols: the lexicon's words, else the units of --ctm-units / --lm-units, else decimal class ids
        ctm_symbols, ctm = {}, None
        if o.ctm_out:
            if not 0 <= o.ctm_precision <= 17:
                raise kaldi_io.KaldiIOError(f"--ctm-precision={o.ctm_precision} is outside [0, 17]")
            if not (math.isfinite(o.frame_shift) and o.frame_shift > 0):
                raise kaldi_io.KaldiIOError("--frame-shift must be positive")
            if lex is not None:
                if o.words_table_out:
                    ctm_symbols = _id_symbols(o.words_table_out)
                else:
                    import tempfile
                    fd, table = tempfile.mkstemp(prefix="ctc-decode-words.")
                    os.close(fd)
                    try:
                        lex.WriteWords(table)
                        ctm_symbols = _id_symbols(table)
                    finally:
                        os.remove(table)
            elif o.ctm_units or o.lm_units:
                ctm_symbols = _id_symbols(o.ctm_units or o.lm_units)
            try:
                ctm = open(o.ctm_out, "w")
            except OSError:
                raise kaldi_io.KaldiIOError(f"cannot open {o.ctm_out}")
        elif o.ctm_units or o.ctm_conf:
            raise kaldi_io.KaldiIOError("--ctm-units and --ctm-conf need --ctm-out")
        if log_pri is not None and log_pri.size != K:
            raise kaldi_io.KaldiIOError(f"Dimensionality mismatch, class_frame_counts {log_pri.size} class_output_llk {K}")
        refs = kaldi_io.read_vec_int_table(o.ref_rspecifier) if o.ref_rspecifier else {}
        word_refs = kaldi_io.read_vec_int_table(o.word_ref_rspecifier) if o.word_ref_rspecifier else {}
        words_writer = None     # the word ids of every hypothesis, written as the hypotheses are
        if o.words_wspecifier:
            wkind, words_path, words_text = kaldi_io._parse_specifier(o.words_wspecifier)
            if wkind != "ark":
                raise kaldi_io.KaldiIOError("only ark: output is supported")
            words_writer = kaldi_io.VecIntArkWriter(words_path, text=words_text)
        ends_writer = None
        if o.word_ends_wspecifier:
            ekind, ends_path, ends_text = kaldi_io._parse_specifier(o.word_ends_wspecifier)
            if ekind != "ark":
                raise kaldi_io.KaldiIOError("only ark: output is supported")
            ends_writer = kaldi_io.VecIntArkWriter(ends_path, text=ends_text)
        pipe = frontend.parse_feature_pipeline(feature_rspecifier) if not os.environ.get("EESEN_HOST_FEATURE_PIPES") else None
        feeder = None
        if pipe is not None:
            from eesen_amd.api import Feeder
            feeder = Feeder(o.device, slots=1)
            pipe.configure(feeder)
        n = dict(done=0, empty=0, dead=0, frames=0, score=0.0, tok_err=0, tok_ref=0, scored=0, lm=0.0, labels=0, word_err=0, word_ref=0, word_scored=0, ctm=0, reranked=0, tok_oracle=0, word_oracle=0, mbr_moved=0)
        scores = open(o.scores_out, "w") if o.scores_out else None
        lib = _lib.load()

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
                _lib.check(lib.eesen_op_log_sub_prior(o.device, None, C.c_void_p(out.ptr), out.rows, out.cols, out.stride, 1,
                                                      log_pri.ctypes.data_as(C.c_void_p), o.prior_scale))
            hyps, score = ctc.DecodeParallel(lens, out, beam=o.beam, max_classes=o.max_classes, nbest=o.nbest, is_log=log_pri is not None,
                                             lm=lm, lm_weight=o.lm_weight, insertion_bonus=o.insertion_bonus, lm_eos=o.lm_eos, lexicon=lex,
                                             word_bonus=o.word_bonus)
            lm_score, words, words_len, word_ends = ctc.lm_score, ctc.words, ctc.words_len, ctc.word_ends
            stamps = ctc.DecodeStamps(lens, out, is_log=log_pri is not None, conf_scale=o.conf_scale) if ctm is not None else None
            second = ctc.RescoreNbest(lens, out, is_log=log_pri is not None, lm=second_lm, lm_weight=second_weight, bonus=second_bonus,
                                      lm_eos=second_eos) if o.rescore else None
            hlen = ctc.hyp_len
            mbr = tok_dist = word_dist = None
            if o.mbr:
                # the references in the level's tokens ride along (an utterance without one: an empty reference, never read back)
                level = 1 if o.mbr_units else 0
                words_level = lex is not None and not o.mbr_units
                totals = second.total if second is not None else None
                pack = lambda table: [table.get(key, []) for key, _ in group]
                mbr = ctc.MbrNbest(level=level, scale=mbr_c, totals=totals, refs=pack(word_refs if words_level else refs))
                tok_dist, word_dist = (None, mbr.ref_dist) if words_level else (mbr.ref_dist, None)
                if lex is not None and (refs if words_level else word_refs):   # the other kind of reference: distances alone, at the other level
                    other = ctc.MbrNbest(level=1 - level, scale=mbr_c, totals=totals, refs=pack(refs if words_level else word_refs), ref_only=True).ref_dist
                    tok_dist, word_dist = (other, word_dist) if words_level else (tok_dist, other)
            for s, (key, m) in enumerate(group):
                frames = int(lens[s])
                if math.isnan(score[s, 0]) or (second is not None and math.isnan(second.total[s, 0])) or (mbr is not None and math.isnan(mbr.posterior[s, 0])):
                    raise RuntimeError(f"the forward pass of {key} timed out on the device: no hypotheses")
                if not hyps[s]:
                    why = "no surviving prefix ends a lexicon word" if lex is not None else "every prefix has probability zero"
                    warn(f"{key}, {why} on {frames} frames, producing no output for this utterance")
                    n["dead"] += 1
                    continue
                # the first-pass ranks of the returned entries in the order they are written: by expected errors, the second pass's, or the beam's
                second_ranks = [int(r) for r in (second.order[s] if second is not None else range(o.nbest)) if 0 <= r < o.nbest and hlen[s, r] >= 0]
                ranks = [int(r) for r in mbr.order[s] if 0 <= r < o.nbest and hlen[s, r] >= 0] if mbr is not None else second_ranks
                n["reranked"] += second_ranks != list(range(len(second_ranks)))
                n["mbr_moved"] += mbr is not None and ranks[0] != second_ranks[0]
                for i, r in enumerate(ranks):
                    k = f"{key}-{i + 1}" if o.nbest > 1 else key
                    if scores:
                        if second is not None:
                            scores.write(f"{k} {float(second.total[s, r]):.9g} {float(second.am_score[s, r]):.9g} {float(second.lm_score[s, r]):.9g}\n")
                        else:
                            scores.write(f"{k} {float(score[s, r]):.9g}" + (f" {float(lm_score[s, r]):.9g}" if lm is not None else "") + "\n")
                    yield k, np.asarray(hyps[s][r], np.int32)
                    if words_writer is not None:          # (after the hypothesis is out, as the native tool orders its writes)
                        words_writer.write(k, words[s, r, :words_len[s, r]])
                    if ends_writer is not None:
                        ends_writer.write(k, word_ends[s, r, :words_len[s, r]])
                b0 = ranks[0]             # the best hypothesis: what is scored against the references and written to the CTM
                # with --mbr the distances came back with the list (an entry that does not count has none: the host routine); the oracle
                # is the list's best
                def errors_of(dist, ref, best):
                    err = int(dist[s, b0]) if dist is not None else -1
                    if err < 0:
                        e = C.c_int(0)
                        _lib.check(lib.eesen_edit_distance(ref.ctypes.data_as(C.c_void_p), ref.size, best.ctypes.data_as(C.c_void_p), best.size, C.byref(e)))
                        err = e.value
                    found = [int(dist[s, r]) for r in ranks if dist[s, r] >= 0] if dist is not None else []
                    return err, min(found) if found else err
                if key in refs:
                    ref, best = np.ascontiguousarray(refs[key], np.int32), np.asarray(hyps[s][b0], np.int32)
                    err, oracle = errors_of(tok_dist, ref, best)
                    n["tok_err"] += err; n["tok_ref"] += int(ref.size); n["scored"] += 1; n["tok_oracle"] += oracle
                if key in word_refs:
                    ref, best = np.ascontiguousarray(word_refs[key], np.int32), np.ascontiguousarray(words[s, b0, :words_len[s, b0]], np.int32)
                    err, oracle = errors_of(word_dist, ref, best)
                    n["word_err"] += err; n["word_ref"] += int(ref.size); n["word_scored"] += 1; n["word_oracle"] += oracle
                if ctm is not None:       # the best hypothesis' words: a label each without a lexicon
                    if math.isnan(stamps.word_conf[s, 0, 0]):
                        raise RuntimeError(f"the forward pass of {key} timed out on the device: no time stamps")
                    ids = words[s, b0, :words_len[s, b0]] if lex is not None else hyps[s][b0]
                    conf = stamps.word_conf[s]
                    if second is not None and o.ctm_conf:   # the posterior over the list by the second pass's totals (the stamps' own is by the beam's)
                        from eesen_amd.api import word_confidence
                        wl = np.where(hlen[s] < 0, -1, words_len[s] if lex is not None else hlen[s])
                        conf = word_confidence(second.total[s], wl, words[s] if lex is not None else ctc.hyp[s], stamps.word_start[s], stamps.word_end[s],
                                               o.conf_scale).astype(np.float32)
                    for j, w in enumerate(ids):
                        b, e = int(stamps.word_start[s, b0, j]), int(stamps.word_end[s, b0, j])
                        if b < 0:             # (a labelling too long to align)
                            continue
                        line = f"{key} 1 {o.frame_shift * b:.{o.ctm_precision}f} {o.frame_shift * (e - b):.{o.ctm_precision}f} {ctm_symbols.get(int(w), str(int(w)))}"
                        if o.ctm_conf:
                            line += f" {float(conf[b0, j]):.{o.ctm_precision}f}"
                        ctm.write(line + "\n")
                        n["ctm"] += 1
                n["done"] += 1; n["frames"] += frames; n["score"] += float(second.total[s, b0] if second is not None else score[s, b0])
                n["empty"] += len(hyps[s][b0]) == 0
                if lm is not None or second_lm is not None:
                    n["lm"] += float(second.lm_score[s, b0] if second is not None else lm_score[s, b0])
                    n["labels"] += int(words_len[s, b0]) if lex is not None else len(hyps[s][b0])

        def produce():
            group, max_len = [], 0
            table = frontend.read_raw(pipe, warn=warn) if pipe is not None else kaldi_io.read_mat_table(feature_rspecifier)
            for key, mat in table:
                if group and (len(group) == o.num_sequence or max(max_len, mat.shape[0]) * (len(group) + 1) > o.frame_limit):
                    yield from flush(group)
                    group, max_len = [], 0
                group.append((key, mat)); max_len = max(max_len, mat.shape[0])
            if group:
                yield from flush(group)

        try:
            kaldi_io.write_vec_int_ark(out_path, produce(), text=out_text)
        finally:
            if words_writer is not None:
                words_writer.close()
            if ends_writer is not None:
                ends_writer.close()
        if scores:
            scores.close()
        if ctm is not None:
            ctm.close()
        if o.ref_rspecifier:
            log(f"{n['tok_err']} token errors on {n['tok_ref']} reference tokens of {n['scored']} utterances")
            if o.mbr:
                log(f"{n['tok_oracle']} token errors of the N-best oracle (the best of up to {o.nbest} hypotheses per utterance)")
            log(f"\nTOKEN_ACCURACY >> {100.0 * (1.0 - n['tok_err'] / max(n['tok_ref'], 1)):g}% <<")
        if o.word_ref_rspecifier:
            log(f"{n['word_err']} word errors on {n['word_ref']} reference words of {n['word_scored']} utterances")
            if o.mbr:
                log(f"{n['word_oracle']} word errors of the N-best oracle (the best of up to {o.nbest} hypotheses per utterance)")
            log(f"\nWORD_ACCURACY >> {100.0 * (1.0 - n['word_err'] / max(n['word_ref'], 1)):g}% <<")
        if n["dead"]:
            log(f"{n['dead']} utterances without a hypothesis")
        avg = n["score"] / n["frames"] if n["frames"] else 0.0
        tail = f"; average LM log-probability per {'word' if lex is not None else 'label'} {(n['lm'] / n['labels'] if n['labels'] else 0.0):g}" if lm is not None or second_lm is not None else ""
        if o.ctm_out:
            tail += f"; {n['ctm']} CTM words"
        if o.rescore:
            tail += f"; {n['reranked']} utterances re-ranked"
        if o.mbr:
            tail += f"; {n['mbr_moved']} utterances whose hypothesis of least expected errors is not the most probable"
        log(f"Done {n['done']} utterances, {n['empty']} empty hypotheses; average log-probability per frame {avg:g}{tail}")
        return 0 if n["done"] else 255
    except Exception as e:
        print(f"ERROR (ctc-decode:main()) {e}", file=sys.stderr)
        return 255


if __name__ == "__main__":
    sys.exit(main())
