"""Host side of the device feature front end (include/eesen_hip.h `eesen_feeder_set_pipeline`).

The recipes hand `train-ctc-parallel` / `net-output-extract` their features as an rspecifier that is a pipe of host filters
(/root/reference/asr_egs/wsj/steps/train_ctc_parallel.sh:95-110, decode_ctc_lat.sh:92-95,
librispeech/steps/train_ctc_parallel_mult.sh:110-133), e.g.

    ark,s,cs:apply-cmvn --norm-vars=true --utt2spk=ark:data/utt2spk scp:data/cmvn.scp scp:exp/train.scp ark:- | \
             splice-feats --left-context=1 --right-context=1 ark:- ark:- | subsample-feats --n=3 --offset=0 ark:- ark:- | \
             add-deltas ark:- ark:- |

`parse_feature_pipeline` recognises exactly such command lines (the option sets of the reference's featbin tools): the
trainers then read the RAW table themselves (here `scp:exp/train.scp`), look the CMVN statistics up per utterance, and
the filters run on the GPU inside the batch assembly -- same command line, no filter processes.  Anything it does not
recognise (another tool, an option it does not implement such as --skip-dims) returns None and the rspecifier is opened
as the pipe it is.

The pipe may start at the audio: `compute-fbank-feats [options] scp:wav.scp ark:- | apply-cmvn ... ark:- ark:- | add-deltas ark:- ark:- |`.
The tools then read the wav table themselves and the features are computed on the device too (EESEN_FEAT_FBANK, the head stage of
the feeder's pipeline); options the device extractor does not implement (--vtln-map, --subtract-mean, htk output, ...) leave the
rspecifier unrecognised.

Or at the audio through both extractors, the tonal recipes' features (asr_egs/wsj/steps/make_fbank_pitch.sh:117-121):
`paste-feats --length-tolerance=2 "ark:compute-fbank-feats [options] scp,p:wav.scp ark:- |" "ark,s,cs:compute-kaldi-pitch-feats [options]
scp,p:wav.scp ark:- | process-kaldi-pitch-feats [options] ark:- ark:- |" ark:- | apply-cmvn ... ark:- ark:- | ...`.  Both inner pipes must name
the same wav table and every option must be one of the device extractors' (--config files are read as the tools read them); the head
stage is then EESEN_FEAT_FBANK_PITCH and `paste_frames` the row count of an utterance.  The inputs in the other order, a third input,
--binary or extract-segments leave the rspecifier unrecognised (INTEGRATION.md "Fbank + pitch").
"""
from __future__ import annotations

import os
import shlex
from dataclasses import dataclass, field
from typing import Dict, Iterator, List, Optional, Tuple

import numpy as np

from . import kaldi_io

CMVN, SPLICE, SUBSAMPLE, DELTAS, FBANK = 1, 2, 3, 4, 5    # EESEN_FEAT_* of include/eesen_hip.h
FBANK_PITCH = 6

# compute-fbank-feats' options that map onto eesen_fbank_opts_t: flag -> (field, type); FrameExtractionOptions / MelBanksOptions /
# FbankOptions::Register, plus --vtln-warp of the tool and --dither-seed of this project
FBANK_OPTIONS = {"sample-frequency": ("samp_freq", float), "frame-length": ("frame_length_ms", float), "frame-shift": ("frame_shift_ms", float),
                 "preemphasis-coefficient": ("preemph_coeff", float), "remove-dc-offset": ("remove_dc_offset", bool), "dither": ("dither", float),
                 "window-type": ("window_type", str), "round-to-power-of-two": ("round_to_power_of_two", bool), "snip-edges": ("snip_edges", bool),
                 "num-mel-bins": ("num_bins", int), "low-freq": ("low_freq", float), "high-freq": ("high_freq", float),
                 "vtln-low": ("vtln_low", float), "vtln-high": ("vtln_high", float), "use-energy": ("use_energy", bool),
                 "energy-floor": ("energy_floor", float), "raw-energy": ("raw_energy", bool), "htk-compat": ("htk_compat", bool),
                 "use-log-fbank": ("use_log_fbank", bool), "vtln-warp": ("vtln_warp", float), "dither-seed": ("dither_seed", int)}
WINDOW_TYPES = ("hamming", "hanning", "povey", "rectangular")


def fbank_geometry(opts: dict) -> Tuple[int, int]:
    """(WindowShift, WindowSize) in samples (feature-functions.h:119-124: a double product of the float options, truncated)."""
    sf = float(np.float32(opts.get("samp_freq", 16000.0)))
    return (int(sf * 0.001 * float(np.float32(opts.get("frame_shift_ms", 10.0)))),
            int(sf * 0.001 * float(np.float32(opts.get("frame_length_ms", 25.0)))))


def fbank_num_frames(nsamp: int, opts: dict) -> int:
    """NumFrames (feature-functions.cc:29-48); equals eesen_fbank_shape."""
    shift, length = fbank_geometry(opts)
    if opts.get("snip_edges", True):
        return 0 if nsamp < length else 1 + (nsamp - length) // shift
    return int(np.float32(np.float32(nsamp) / np.float32(shift)) + np.float32(0.5))


def paste_frames(frames, tolerance: int = 0) -> int:
    """Rows of an utterance behind paste-feats, from its row counts in the inputs (AppendFeats, paste-feats.cc:35-56): the shortest,
    or 0 -- no output -- when the longest exceeds it by more than `tolerance` or an input is empty; equals eesen_feat_paste_frames."""
    frames = [int(f) for f in frames]
    if not frames or tolerance < 0 or min(frames) < 0:
        raise ValueError("paste_frames: at least one row count, none of them negative, and a tolerance >= 0")
    lo, hi = min(frames), max(frames)
    return 0 if hi - lo > tolerance or lo == 0 else lo


def _pitch_flags():
    """(compute-kaldi-pitch-feats', process-kaldi-pitch-feats'): flag -> (field of eesen_pitch_opts_t, type), as the tools register them."""
    from .compute_kaldi_pitch_feats import PITCH_OPTIONS
    from .process_kaldi_pitch_feats import PROCESS_OPTIONS
    return ({k: (f, type(d)) for k, (f, d, _) in PITCH_OPTIONS.items()}, {k: (f, type(d)) for k, (f, d, _) in PROCESS_OPTIONS.items()})


def _split_pipe(cmd: str) -> Optional[List[str]]:
    """The commands of a shell pipe line, split at the `|` that stand outside quotes (an inner rspecifier such as
    "ark:compute-fbank-feats ... |" keeps its own); None when a quote is left open."""
    segs, cur, quote, i = [], [], None, 0
    while i < len(cmd):
        ch = cmd[i]
        if quote is None and ch == "\\" and i + 1 < len(cmd):
            cur.append(cmd[i:i + 2])
            i += 2
            continue
        if quote is None and ch in "'\"":
            quote = ch
        elif quote == ch:
            quote = None
        elif quote == '"' and ch == "\\" and i + 1 < len(cmd):
            cur.append(cmd[i:i + 2])
            i += 2
            continue
        elif quote is None and ch == "|":
            segs.append("".join(cur))
            cur, ch = [], ""
        cur.append(ch)
        i += 1
    if quote is not None:
        return None
    segs.append("".join(cur))
    return segs


def _with_config(argv: List[str]) -> Optional[List[str]]:
    """--config=<file> as the tools read it (one --x=y per line, # comments; read first, so the command line overrides it): the
    file's options in front of the others.  None when a file cannot be read or a line is no option."""
    head, rest = [], []
    for a in argv:
        if a.startswith("--config="):
            try:
                lines = open(a[len("--config="):].strip()).read().splitlines()
            except OSError:
                return None
            for line in lines:
                line = line.split("#", 1)[0].strip()
                if line and not line.startswith("--"):
                    return None
                if line:
                    head.append(line)
        else:
            rest.append(a)
    return head + rest


def _wav_source(src: str) -> Optional[str]:
    """A wav table rspecifier without its options (scp,p:x -> scp:x); None for anything that is not a plain table."""
    head, sep, path = src.partition(":")
    if not sep or head.split(",")[0] not in ("ark", "scp") or src.rstrip().endswith("|"):
        return None
    return head.split(",")[0] + ":" + path.strip()


def _bool(v: str) -> Optional[bool]:
    """ParseOptions::ToBool (/root/reference/src/util/parse-options.cc): true/t/1 and false/f/0, and the empty string = true."""
    v = v.strip().lower()
    if v in ("", "true", "t", "1"):
        return True
    if v in ("false", "f", "0"):
        return False
    return None


def _options(argv: List[str], known: Dict[str, type]):
    """Splits `--name=value` options from positional arguments; None if an option is unknown or malformed."""
    opts, pos = {}, []
    for a in argv:
        if a.startswith("--"):
            name, _, val = a[2:].partition("=")
            name = name.replace("_", "-")
            if name not in known:
                return None
            if known[name] is bool:
                b = _bool(val)
                if b is None:
                    return None
                opts[name] = b
            elif known[name] is int:
                try:
                    opts[name] = int(val)
                except ValueError:
                    return None
            elif known[name] is float:
                try:
                    opts[name] = float(val)
                except ValueError:
                    return None
            else:
                opts[name] = val
        else:
            pos.append(a)
    return opts, pos


@dataclass
class FeaturePipeline:
    source: str                                   # rspecifier of the raw features
    stages: List[Tuple[int, int, int]] = field(default_factory=list)   # (EESEN_FEAT_*, a, b) in order
    cmvn: Optional[str] = None                    # stats rspecifier (per utterance / speaker) or rxfilename (global)
    utt2spk: Optional[str] = None
    norm_vars: bool = False
    # with a compute-fbank-feats head: `source` is the wav table, `fbank` the extractor's options (fields of eesen_fbank_opts_t)
    fbank: Optional[dict] = None
    channel: int = -1
    min_duration: float = 0.0
    # with a paste-feats head over compute-fbank-feats and the two pitch tools: `pitch` holds fields of eesen_pitch_opts_t and
    # `tolerance` paste-feats' --length-tolerance (the stage is (FBANK_PITCH, tolerance, 0))
    pitch: Optional[dict] = None
    tolerance: int = 0
    _pitch_shape: object = field(default=None, compare=False, repr=False)

    def configure(self, feeder) -> None:
        """Sets this pipeline on an api.Feeder (the extractors' options first, when it starts at the audio)."""
        if self.fbank is not None:
            feeder.set_fbank(**self.fbank)
        if self.pitch is not None:
            feeder.set_pitch(**self.pitch)
        feeder.set_pipeline(self.stages)

    def _fbank_dim(self) -> int:
        return self.fbank.get("num_bins", 23) + int(self.fbank.get("use_energy", False))

    def pitch_rows(self, nsamp: int) -> Tuple[int, int]:
        """(rows, columns) of the processed pitch matrix of a waveform: eesen_pitch_shape (host only), frames + delay rows."""
        if self._pitch_shape is None:
            from .api import Pitch
            self._pitch_shape = Pitch(**self.pitch)       # no device is touched before a compute call
        frames, _, dim = self._pitch_shape.shape(nsamp)
        return (frames + int(self.pitch.get("delay", 0)) if frames else 0), dim

    def cmvn_dim(self, D: int) -> int:
        """Feature dimension in front of the CMVN stage."""
        if self.pitch is not None:
            return self._fbank_dim() + self.pitch_rows(0)[1]
        return self._fbank_dim() if self.fbank is not None else D

    def out_dim(self, D: int) -> int:
        for k, a, b in self.stages:
            if k == FBANK:
                D = self._fbank_dim()
            elif k == FBANK_PITCH:
                D = self._fbank_dim() + self.pitch_rows(0)[1]
            elif k == SPLICE:
                D *= 1 + a + b
            elif k == DELTAS:
                D *= 1 + a
        return D

    def out_frames(self, T: int) -> int:
        for k, a, b in self.stages:
            if k == FBANK:
                T = fbank_num_frames(T, self.fbank)
            elif k == FBANK_PITCH:
                T = paste_frames([fbank_num_frames(T, self.fbank), self.pitch_rows(T)[0]], a)
            elif k == SUBSAMPLE:
                T = T * -a if a < 0 else (max(0, (T - b + a - 1) // a) if T > b else 0)
        return T


def _inner_pipe(spec: str) -> Optional[List[List[str]]]:
    """The argument vectors of an input of paste-feats that is itself a pipe, "ark[,s,cs]:tool ... | tool ... |"; None otherwise."""
    head, sep, cmd = spec.partition(":")
    if not sep or head.split(",")[0] != "ark" or any(o not in ("s", "cs") for o in head.split(",")[1:]) or not cmd.rstrip().endswith("|"):
        return None
    segs = _split_pipe(cmd.rstrip()[:-1])
    if segs is None or any(not s.strip() for s in segs):
        return None
    try:
        return [shlex.split(s) for s in segs]
    except ValueError:
        return None


def _parse_paste_head(argv: List[str]) -> Optional[FeaturePipeline]:
    """paste-feats [--length-tolerance=N] "<fbank pipe>" "<pitch pipe>" ark:- (asr_egs/wsj/steps/make_fbank_pitch.sh:117-121): both
    inner pipes over one wav table, every option one of the device extractors'.  None leaves the rspecifier to the shell."""
    r = _options(argv, {"length-tolerance": int})
    if r is None or len(r[1]) != 3 or r[1][2] != "ark:-" or r[0].get("length-tolerance", 0) < 0:
        return None
    fb, pt = _inner_pipe(r[1][0]), _inner_pipe(r[1][1])
    if fb is None or pt is None or len(fb) != 1 or len(pt) != 2:
        return None
    if [os.path.basename(a[0]) for a in fb + pt] != ["compute-fbank-feats", "compute-kaldi-pitch-feats", "process-kaldi-pitch-feats"]:
        return None
    args = [_with_config(a[1:]) for a in fb + pt]
    if any(a is None for a in args):
        return None
    known = {k: t for k, (_, t) in FBANK_OPTIONS.items()}
    known.update({"channel": int, "min-duration": float, "output-format": str, "verbose": int})
    rf = _options(args[0], known)
    if rf is None or len(rf[1]) != 2 or rf[1][1] != "ark:-":
        return None
    o = rf[0]
    if o.get("output-format", "kaldi") != "kaldi" or not o.get("round-to-power-of-two", True) or o.get("window-type", "povey") not in WINDOW_TYPES:
        return None
    compute_flags, process_flags = _pitch_flags()
    rc = _options(args[1], {**{k: t for k, (_, t) in compute_flags.items()}, "verbose": int})
    rp = _options(args[2], {**{k: t for k, (_, t) in process_flags.items()}, "verbose": int, "srand": int})
    if rc is None or rp is None or len(rc[1]) != 2 or rc[1][1] != "ark:-" or rp[1] != ["ark:-", "ark:-"]:
        return None
    oc = rc[0]   # what the device extractor refuses (eesen_pitch_create) stays with the reference's tool
    if oc.get("preemphasis-coefficient", 0.0) != 0.0 or oc.get("frames-per-chunk", 0) != 0 or oc.get("simulate-first-pass-online", False) or oc.get("nccf-ballast-online", False):
        return None
    src = _wav_source(rf[1][0])
    if src is None or src != _wav_source(rc[1][0]):
        return None
    pitch = {compute_flags[k][0]: v for k, v in oc.items() if k in compute_flags}
    pitch.update({process_flags[k][0]: v for k, v in rp[0].items() if k in process_flags})
    tol = r[0].get("length-tolerance", 0)
    pipe = FeaturePipeline(source=rf[1][0], fbank={FBANK_OPTIONS[k][0]: v for k, v in o.items() if k in FBANK_OPTIONS}, pitch=pitch, tolerance=tol,
                           channel=o.get("channel", -1), min_duration=o.get("min-duration", 0.0))
    pipe.stages.append((FBANK_PITCH, tol, 0))
    return pipe


def parse_feature_pipeline(rspecifier: str) -> Optional[FeaturePipeline]:
    head, sep, cmd = rspecifier.partition(":")
    if not sep or head.split(",")[0] != "ark" or not cmd.rstrip().endswith("|"):
        return None
    segs = _split_pipe(cmd.rstrip().rstrip("|"))       # quote-aware: an input of paste-feats may be a pipe of its own
    if segs is None:
        return None
    segs = [s.strip() for s in segs]
    if not segs or any(not s for s in segs):
        return None
    pipe = None
    for i, seg in enumerate(segs):
        try:
            argv = shlex.split(seg)
        except ValueError:
            return None
        tool, argv = os.path.basename(argv[0]), argv[1:]
        if i == 0 and tool == "paste-feats":              # featbin/paste-feats.cc over the two extractors: the pipe starts at the audio
            pipe = _parse_paste_head(argv)
            if pipe is None:
                return None
            continue
        if i == 0 and tool == "compute-fbank-feats":      # featbin/compute-fbank-feats.cc: the pipe starts at the audio
            known = {k: t for k, (_, t) in FBANK_OPTIONS.items()}
            known.update({"channel": int, "min-duration": float, "output-format": str})
            r = _options(argv, known)
            if r is None or len(r[1]) != 2 or r[1][1] != "ark:-":
                return None
            o, (src, _) = r
            if o.get("output-format", "kaldi") != "kaldi" or not o.get("round-to-power-of-two", True) or o.get("window-type", "povey") not in WINDOW_TYPES:
                return None
            if src.partition(":")[0].split(",")[0] not in ("ark", "scp") or ":" not in src or src.rstrip().endswith("|"):
                return None
            pipe = FeaturePipeline(source=src, fbank={FBANK_OPTIONS[k][0]: v for k, v in o.items() if k in FBANK_OPTIONS},
                                   channel=o.get("channel", -1), min_duration=o.get("min-duration", 0.0))
            pipe.stages.append((FBANK, 0, 0))
            continue
        if i == 1 and pipe is not None and pipe.fbank is not None and tool == "apply-cmvn":     # reads the head's output: ark:-
            r = _options(argv, {"utt2spk": str, "norm-vars": bool, "norm-means": bool})
            if r is None or len(r[1]) != 3 or r[1][1] != "ark:-" or r[1][2] != "ark:-":
                return None
            o = r[0]
            norm_means, norm_vars = o.get("norm-means", True), o.get("norm-vars", False)
            if norm_vars and not norm_means:
                return None
            if norm_means:
                pipe.cmvn, pipe.utt2spk, pipe.norm_vars = r[1][0], o.get("utt2spk") or None, norm_vars
                pipe.stages.append((CMVN, int(norm_vars), 0))
            continue
        if i == 0:
            if tool == "apply-cmvn":        # featbin/apply-cmvn.cc:36-47
                r = _options(argv, {"utt2spk": str, "norm-vars": bool, "norm-means": bool})
                if r is None or len(r[1]) != 3 or r[1][2] != "ark:-":
                    return None
                o, (stats, src, _) = r
                norm_means, norm_vars = o.get("norm-means", True), o.get("norm-vars", False)
                if norm_vars and not norm_means:
                    return None             # the tool itself refuses this (:55-56): let it say so
                pipe = FeaturePipeline(source=src)
                if norm_means:
                    pipe.cmvn, pipe.utt2spk, pipe.norm_vars = stats, o.get("utt2spk") or None, norm_vars
                    pipe.stages.append((CMVN, int(norm_vars), 0))
            elif tool == "copy-feats":
                r = _options(argv, {})
                if r is None or len(r[1]) != 2 or r[1][1] != "ark:-":
                    return None
                pipe = FeaturePipeline(source=r[1][0])
            else:
                return None
            if pipe.source.partition(":")[0].split(",")[0] not in ("ark", "scp") or pipe.source.rstrip().endswith("|"):
                return None
            continue
        if tool == "splice-feats":          # featbin/splice-feats.cc:36-40: both contexts default to 4
            r = _options(argv, {"left-context": int, "right-context": int})
            if r is None or r[1] != ["ark:-", "ark:-"]:
                return None
            L, R = r[0].get("left-context", 4), r[0].get("right-context", 4)
            if L < 0 or R < 0:
                return None
            pipe.stages.append((SPLICE, L, R))
        elif tool == "subsample-feats":     # featbin/subsample-feats.cc:46-55
            r = _options(argv, {"n": int, "offset": int})
            if r is None or r[1] != ["ark:-", "ark:-"]:
                return None
            n, off = r[0].get("n", 1), r[0].get("offset", 0)
            if n == 0 or off < 0 or (n < 0 and off != 0):
                return None
            pipe.stages.append((SUBSAMPLE, n, off))
        elif tool == "add-deltas":          # featbin/add-deltas.cc:33-38, DeltaFeaturesOptions feature-functions.h: order 2, window 2
            r = _options(argv, {"delta-order": int, "delta-window": int, "truncate": int})
            if r is None or r[1] != ["ark:-", "ark:-"] or r[0].get("truncate", 0) != 0:
                return None
            order, window = r[0].get("delta-order", 2), r[0].get("delta-window", 2)
            if not (0 <= order <= 8 and 0 < window <= 16):
                return None
            pipe.stages.append((DELTAS, order, window))
        else:
            return None
    return pipe


def cmvn_norm(stats: np.ndarray, norm_vars: bool) -> np.ndarray:
    """[2 x dim] float32 (offsets, scales) from a CMVN statistics matrix: eesen_cmvn_norm, i.e. ApplyCmvn's own arithmetic
    (/root/reference/src/feat/cmvn.cc:78-108)."""
    import ctypes as C
    from . import _lib
    stats = np.ascontiguousarray(stats, np.float64)
    if stats.ndim != 2:
        raise _lib.EesenError(-1, "CMVN statistics must be a matrix")
    out = np.empty((2, max(stats.shape[1] - 1, 0)), np.float32)
    _lib.check(_lib.load().eesen_cmvn_norm(stats.ctypes.data_as(C.POINTER(C.c_double)), stats.shape[0], stats.shape[1], int(norm_vars),
                                           out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


class RawUtt:
    """An utterance as the feeder takes it with a pipeline set: the raw matrix, its CMVN vectors, and -- what batch
    assembly and the CTC see -- the shape BEHIND the pipeline."""
    __slots__ = ("raw", "cmvn", "shape")

    def __init__(self, raw: np.ndarray, cmvn: Optional[np.ndarray], shape: Tuple[int, int]):
        self.raw, self.cmvn, self.shape = raw, cmvn, shape


class CmvnTable:
    """RandomAccessDoubleMatrixReaderMapped(cmvn_rspecifier, utt2spk_rspecifier) of apply-cmvn.cc:80-81, or the single
    matrix of its rxfilename form (:115-122); normalisers are computed once per speaker."""

    def __init__(self, spec: str, utt2spk: Optional[str], norm_vars: bool):
        self.norm_vars = norm_vars
        self.global_norm = None
        self.map = None
        self.cache: Dict[str, np.ndarray] = {}
        if spec.partition(":")[0].split(",")[0] in ("ark", "scp") and ":" in spec:
            self.stats = dict(kaldi_io.read_mat64_table(spec))
            if utt2spk:
                self.map = kaldi_io.read_token_map(utt2spk)
        else:
            if utt2spk:
                raise kaldi_io.KaldiIOError("--utt2spk option not compatible with rxfilename as input (did you forget ark:?)")
            self.global_norm = cmvn_norm(kaldi_io.read_mat64_file(spec), norm_vars)

    def lookup(self, utt: str) -> Optional[np.ndarray]:
        if self.global_norm is not None:
            return self.global_norm
        key = utt
        if self.map is not None:
            if utt not in self.map:
                return None
            key = self.map[utt]
        if key not in self.stats:
            return None
        if key not in self.cache:
            self.cache[key] = cmvn_norm(self.stats[key], self.norm_vars)
        return self.cache[key]


def _read_waves(pipe: FeaturePipeline, source: str, warn) -> Iterator[Tuple[str, np.ndarray]]:
    """The wav table as [samples x 1] matrices, with compute-fbank-feats' own checks (compute-fbank-feats.cc:97-139)."""
    want = float(np.float32(pipe.fbank.get("samp_freq", 16000.0)))
    for key, (rate, data) in kaldi_io.read_wav_table(source):
        if data.shape[1] / rate < pipe.min_duration:
            warn(f"File: {key} is too short ({data.shape[1] / rate:g} sec): producing no output.")
            continue
        chan = kaldi_io.select_channel(key, data, pipe.channel, warn)
        if chan is None:
            continue
        if rate != want:
            raise kaldi_io.KaldiIOError(f"Sample frequency mismatch: you specified {want:g} but data has {rate:g} (use --sample-frequency option).  Utterance is {key}")
        yield key, np.ascontiguousarray(chan, np.float32).reshape(-1, 1)


def read_raw(pipe: FeaturePipeline, source: Optional[str] = None, warn=None) -> Iterator[Tuple[str, RawUtt]]:
    """The raw table as (key, RawUtt).  Utterances the reference's filters would not have passed on are dropped the same
    way: no CMVN statistics (apply-cmvn.cc:87-92), no rows (add-deltas.cc:55-58), no frame left by the subsampling
    (subsample-feats.cc:87-92)."""
    warn = warn or (lambda msg: None)
    table = CmvnTable(pipe.cmvn, pipe.utt2spk, pipe.norm_vars) if pipe.cmvn else None
    for key, mat in (_read_waves(pipe, source or pipe.source, warn) if pipe.fbank is not None else kaldi_io.read_mat_table(source or pipe.source)):
        vec = None
        if table is not None:
            vec = table.lookup(key)
            if vec is None:
                warn(f"No normalization statistics available for key {key}, producing no output for this utterance")
                continue
            if vec.shape[1] != pipe.cmvn_dim(mat.shape[1]):
                raise kaldi_io.KaldiIOError(f"Dim mismatch in ApplyCmvn: cmvn 2x{vec.shape[1] + 1}, feats {mat.shape[0]}x{mat.shape[1]}")
        if mat.shape[0] == 0:
            warn(f"Empty feature matrix for key {key}")
            continue
        if pipe.pitch is not None:      # paste-feats' own warning (paste-feats.cc:44-49) where the two extractors' lengths do not meet
            counts = [fbank_num_frames(mat.shape[0], pipe.fbank), pipe.pitch_rows(mat.shape[0])[0]]
            if paste_frames(counts, pipe.tolerance) == 0:
                warn(f"Length mismatch {max(counts)} vs. {min(counts)} for utt {key} exceeds tolerance {pipe.tolerance}")
                continue
        frames = pipe.out_frames(mat.shape[0])
        if frames == 0:
            warn(f"For utterance {key}, output would have no rows, producing no output.")
            continue
        yield key, RawUtt(mat, vec, (frames, pipe.out_dim(mat.shape[1])))
