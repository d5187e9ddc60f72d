"""Inputs and metrics of the per-utterance CTC tests (tests/test_ctc_cases.py on the CPU, tests/test_gpu_ctc_per_utterance.py on the GPU).

A trained CTC network emits spikes: blank at 0.999..., one label near 1 for a frame or two, everything else 1e-10 ... 1e-40, denormal or
exactly 0.  `peaky_case` builds such posteriors: N(0, 1) logits with `heights[s]` added on a monotone alignment of the utterance's labels,
softmax evaluated in float32 so that denormals and exact zeros arise the way a device softmax makes them.

Every comparison is per utterance s over its valid frames (rows t * S + s, t < len_s), against the fp64 oracle on the same float32
probabilities:
  gradient figure   max |diff - diff64| / max |diff64|
  ln p figure       |ln p - ln p64| / max(1, |ln p64|)
  per-frame figure  the worst, over frames whose fp64 row maximum exceeds 1e-6 of the utterance maximum, of (row max error / row max)
`floor` is the same figure of the fp32 oracle.  CASES lists every input the GPU test uses, so that the CPU test can hold the conditions
the GPU bars rely on with the oracle alone.
"""
import numpy as np

FLT_MIN_NORMAL = np.float32(1.17549435e-38)


# ------------------------------------------------------------------------------------------ generators
def softmax32(logits):
    """Row softmax in float32 arithmetic throughout (subtract the maximum, exp, float32 sum, float32 division)."""
    x = np.asarray(logits, np.float32)
    e = np.exp(x - x.max(axis=1, keepdims=True), dtype=np.float32)
    return (e / e.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)


def draw_labels(rng, K, u, label_low=1, repeat=0.2):
    lab = rng.integers(label_low, K, size=u).astype(np.int32)
    for i in range(1, u):
        if rng.random() < repeat:
            lab[i] = lab[i - 1]
    return lab


def num_repeats(lab):
    lab = np.asarray(lab)
    return int(np.sum(lab[1:] == lab[:-1]))


def _spike(rng, logits, S, s, frames_cls, height, wrong, K):
    """Add `height` on the aligned class of every frame of utterance s; a share `wrong` of the frames goes to a random class."""
    cls = np.array(frames_cls, np.int64)
    bad = rng.random(cls.size) < wrong
    bad[-1] = False                                        # (see _alignment)
    cls[bad] = rng.integers(0, K, size=int(bad.sum()))
    logits[np.arange(cls.size) * S + s, cls] += np.float32(height)


def _alignment(rng, length, lab):
    """Monotone alignment: len(lab) distinct frames carry their label (a blank between them where the length allows it), every
    other frame carries blank.  The last frame carries blank: an utterance whose last label first spikes on its last frame puts
    that label's alpha more than 88.7 above the last blank's, where the reference's ln p formula clamps (ExpA) and is simply wrong
    in fp32 -- a reference quirk, not an input of the held regime."""
    u, free = len(lab), length - 1
    if free >= 2 * u:
        at = np.sort(rng.choice(free - u + 1, size=u, replace=False)) + np.arange(u)
    else:
        at = np.sort(rng.choice(free, size=u, replace=False))
    cls = np.zeros(length, np.int64)
    cls[at] = lab
    return cls


def peaky_case(S, T, K, U, heights, seed, label_low=1, wrong=0.05):
    """lens, probs (float32 [T*S x K], row t*S + s), labels.  Lengths sorted in [0.7 T, T], the last is T; the last utterance has exactly
    U labels, the others U//2 .. U; ~20 % adjacent repeats; labels from [label_low, K)."""
    rng = np.random.default_rng(seed)
    lens = np.sort(rng.integers(int(np.ceil(0.7 * T)), T + 1, size=S)).astype(np.int32)
    lens[-1] = T
    logits = rng.standard_normal((T * S, K)).astype(np.float32)
    labels = []
    for s in range(S):
        u = U if s == S - 1 else int(rng.integers(max(1, U // 2), U + 1))
        lab = draw_labels(rng, K, u, label_low)
        assert u + num_repeats(lab) < lens[s]
        labels.append(lab)
        _spike(rng, logits, S, s, _alignment(rng, int(lens[s]), lab), heights[s % len(heights)], wrong, K)
    return lens, softmax32(logits), labels


def dense_case(S, T, K, Umax, seed, min_len_frac=0.6):
    """tests/test_gpu_parity.py: _random_ctc_case (softmax of N(0, 2^2) logits)."""
    from tests.test_gpu_parity import _random_ctc_case
    return _random_ctc_case(S, T, K, Umax, seed, min_len_frac)


def long_case(S, T, K, U, seed):
    """tests/test_gpu_parity.py: _long_label_case."""
    from tests.test_gpu_parity import _long_label_case
    return _long_label_case(S, T, K, U, seed)


def shortest_case(Us, K, height, seed, short_by=0, wrong=0.05):
    """One utterance per entry of Us with len_s = U_s + (adjacent repeats) + 1 - short_by: with short_by = 0 the shortest length at which
    the reference's ln p formula works (one spare frame; almost every lattice position sits on the edge of the reachable region), with
    short_by = 1 the shortest feasible one (the last blank is unreachable).  height None: dense N(0, 2^2) logits; otherwise N(0, 1) with
    `height` along the one label order."""
    rng = np.random.default_rng(seed)
    S = len(Us)
    labels = [draw_labels(rng, K, u) for u in Us]
    lens = np.array([len(l) + num_repeats(l) + 1 - short_by for l in labels], np.int32)
    T = int(lens.max())
    logits = rng.standard_normal((T * S, K)).astype(np.float32) * np.float32(2.0 if height is None else 1.0)
    if height is not None:
        for s, lab in enumerate(labels):
            cls = []
            for i, c in enumerate(lab):
                if i and lab[i - 1] == c:
                    cls.append(0)
                cls.append(int(c))
            cls.append(0)
            _spike(rng, logits, S, s, cls[:int(lens[s])], height, wrong, K)
    return lens, softmax32(logits), labels


def boundary_case(U, seed, K=8):
    """S = 2 for the dispatch by the longest lattice: utterance 1 has exactly U labels on T = 2.2 U + 4 frames, utterance 0 one to
    three labels on about half the frames."""
    rng = np.random.default_rng(seed)
    T = int(2.2 * U) + 4
    lens = np.array([max(8, T // 2 + int(rng.integers(0, 5))), T], np.int32)
    labels = [draw_labels(rng, K, int(rng.integers(1, 4))), draw_labels(rng, K, U)]
    assert U + num_repeats(labels[1]) < T
    logits = rng.standard_normal((T * 2, K)).astype(np.float32)
    for s, h in ((0, 12.0), (1, 4.0)):
        _spike(rng, logits, 2, s, _alignment(rng, int(lens[s]), labels[s]), h, 0.05, K)
    return lens, softmax32(logits), labels


def last_frame_spike_case(height=60.0, seed=0):
    """One utterance whose only label spikes on the LAST frame alone: the last label's alpha ends more than 88.72 above the last blank's, where
    the reference's ln p formula clamps (CTC quirks): the fp32 reference is tens of nats below the true ln p ~ 0."""
    rng = np.random.default_rng(seed)
    T, K = 12, 6
    logits = rng.standard_normal((T, K)).astype(np.float32)
    cls = np.zeros(T, np.int64)
    cls[-1] = 3
    logits[np.arange(T), cls] += np.float32(height)
    return np.array([T], np.int32), softmax32(logits), [np.array([3], np.int32)]


def tie_case(S, T, K, seed):
    """Greedy decoding with exact ties: in a tenth of the frames two classes share the row maximum (the lower index wins in the
    reference); rows whose maximum sits at index 0 and at index K - 1, alone and as one side of a tie."""
    lens, probs, labels = dense_case(S, T, K, 8, seed)
    rng = np.random.default_rng(seed + 1)
    rows = T * S
    probs = probs.copy()
    top = probs.max(axis=1) * np.float32(1.25)
    pick = rng.permutation(rows)
    n = rows // 10
    for r in pick[:n]:                                     # a tie between two random classes
        a, b = rng.choice(K, size=2, replace=False)
        probs[r, a] = probs[r, b] = top[r]
    for r in pick[n:n + n // 4]:                           # 0 against K - 1
        probs[r, 0] = probs[r, K - 1] = top[r]
    for r in pick[n + n // 4:n + n // 2]:                  # K - 1 against a random class
        probs[r, K - 1] = probs[r, rng.integers(1, K - 1)] = top[r]
    for r in pick[n + n // 2:n + 3 * n // 4]:
        probs[r, 0] = top[r]
    for r in pick[n + 3 * n // 4:2 * n]:
        probs[r, K - 1] = top[r]
    return lens, probs, labels


# ------------------------------------------------------------------------------------------ the cases of the GPU test
BOUNDARY_U = (31, 32, 63, 64, 127, 128, 191, 192, 255, 256, 383, 384, 511, 512, 767, 768, 1023, 1024, 1535, 1536)
DENSE_SHAPES = [(3, 12, 7, 4), (8, 60, 46, 6), (4, 50, 31, 25), (5, 150, 46, 60), (3, 300, 46, 120), (2, 600, 20, 250), (33, 40, 100, 10)]
LONG_SHAPES = [(3, 3000, 30, 600), (3, 3000, 30, 1000), (2, 3400, 12, 1600), (2, 2900, 8, 2047)]
SHORTEST_U = (1, 5, 63, 64, 300)

# name -> (builder, args, kwargs, regime); regime: "held" (fp64 bars), "extreme" (heights >= 95), "quirk" (one frame short)
CASES = {
    "peaky_h4_60": (peaky_case, (4, 200, 40, 30, (4, 12, 30, 60), 11), {}, "held"),
    "peaky_denormal": (peaky_case, (4, 200, 40, 30, (40, 60, 80, 86), 12), {}, "held"),
    "peaky_class0": (peaky_case, (3, 300, 40, 40, (4, 12, 30), 13), dict(label_low=0), "held"),
    "peaky_T1500": (peaky_case, (3, 1500, 30, 300, (12, 30, 60), 14), {}, "held"),
    "peaky_long": (peaky_case, (3, 3000, 30, 600, (12, 30, 60), 15), {}, "held"),
    # (heights 95 / 100 / 105 / 120 plus 99: the height at which an utterance has a handful of exact zeros and stays feasible; the seed
    #  is one for which the conditions of tests/test_ctc_cases.py hold -- of seeds 16 .. 59 one made the REFERENCE return non-finite
    #  values, most put more than 5 % of an utterance's frames where the fp32 reference is off by its whole magnitude)
    "extreme": (peaky_case, (5, 200, 40, 30, (95, 99, 100, 105, 120), 24), {}, "extreme"),
    "shortest_dense": (shortest_case, (SHORTEST_U, 20, None, 21), {}, "held"),
    "shortest_h12": (shortest_case, (SHORTEST_U, 20, 12.0, 22), {}, "held"),
    "one_short_dense": (shortest_case, (SHORTEST_U, 20, None, 23), dict(short_by=1), "quirk"),
    "one_short_h12": (shortest_case, (SHORTEST_U, 20, 12.0, 24), dict(short_by=1), "quirk"),
    "frames2": (peaky_case, (40, 1001, 30, 40, (4, 12, 30), 31), {}, "held"),
    "frames8": (peaky_case, (64, 2101, 30, 40, (4, 12, 30), 32), {}, "held"),
}
for _S, _T, _K, _U in DENSE_SHAPES:
    CASES[f"dense_{_S}x{_T}x{_K}"] = (dense_case, (_S, _T, _K, _U, _S * 1000 + _T), {}, "held")
for _S, _T, _K, _U in LONG_SHAPES:
    CASES[f"long_U{_U}"] = (long_case, (_S, _T, _K, _U, _U), {}, "held")
for _U in BOUNDARY_U:
    CASES[f"boundary_U{_U}"] = (boundary_case, (_U, 4000 + _U), {}, "held")

PEAKY_HELD = ("peaky_h4_60", "peaky_denormal", "peaky_class0", "peaky_T1500", "peaky_long")
DENORMAL_CASES = ("peaky_denormal",)
CLASS0_CASES = ("peaky_class0",)
FRAMES_CASES = {"frames2": 2, "frames8": 8}       # name -> frames per wave of the gradient pass (csrc/ctc.hip: ctc_error_diff)


def build(name):
    fn, args, kw, _ = CASES[name]
    lens, probs, labels = fn(*args, **kw)
    S = len(lens)
    return np.asarray(lens, np.int32), np.ascontiguousarray(probs, np.float32), [np.asarray(l, np.int32) for l in labels], probs.shape[0] // S, S


def regime(name):
    return CASES[name][3]


def floor_cap(T):
    """Cap on an utterance's fp32-vs-fp64 gradient floor in the held regime: the exponent of gamma carries ulp(|alpha|) and |alpha|
    grows with T."""
    return 2e-3 if T <= 1500 else 2e-2


def csr(labels):
    ids = np.concatenate(labels).astype(np.int32)
    off = np.concatenate([[0], np.cumsum([len(l) for l in labels])]).astype(np.int32)
    return ids, off


def oracle_pair(lens, probs, labels, T, S):
    """(fp32 oracle, fp64 oracle) on the same float32 probabilities."""
    from oracle import net as onet
    ids, off = csr(labels)
    return tuple(onet.ctc_eval_parallel(probs, T, S, lens, ids, off, p) for p in ("f32", "f64"))


# ------------------------------------------------------------------------------------------ per-utterance metrics
def utt(a, s, S, n):
    """Rows of utterance s (its first n frames) of a [T*S x C] array."""
    return np.asarray(a)[s:n * S:S]


def lattice_classes(lab):
    return np.unique(np.concatenate([[0], np.asarray(lab)]))


def grad_figure(got_s, ref_s):
    """max |got - ref| / max |ref| over one utterance's valid frames (ref: fp64)."""
    ref_s = np.asarray(ref_s, np.float64)
    return float(np.max(np.abs(np.asarray(got_s, np.float64) - ref_s)) / max(float(np.max(np.abs(ref_s))), 1e-300))


def frame_errors(got_s, ref_s):
    """Per frame: (max error of the row, max of the fp64 row)."""
    ref_s = np.asarray(ref_s, np.float64)
    return np.max(np.abs(np.asarray(got_s, np.float64) - ref_s), axis=1), np.max(np.abs(ref_s), axis=1)


def frame_figure(got_s, ref_s, keep=None):
    """The worst relative row error over the frames whose fp64 row maximum exceeds 1e-6 of the utterance maximum (and `keep`)."""
    err, mx = frame_errors(got_s, ref_s)
    sel = mx > 1e-6 * mx.max()
    if keep is not None:
        sel &= keep
    return float(np.max(err[sel] / mx[sel])) if sel.any() else 0.0


def lnp_figure(got, ref):
    return abs(float(got) - float(ref)) / max(1.0, abs(float(ref)))


def broken_frames(d32_s, d64_s):
    """Frames on which the fp32 REFERENCE is off by more than 1e-3 of the utterance maximum (extreme regime: below ~1e-41 the fp32
    reference is not an accurate evaluation)."""
    err, mx = frame_errors(d32_s, d64_s)
    return err > 1e-3 * max(float(mx.max()), 1e-300)
