"""Log-mel filterbank features in float64 numpy, written from the definitions of the reference's compute-fbank-feats
(src/feat/feature-fbank.cc, feature-functions.cc:29-167, mel-computations.cc:32-239), with numpy's rfft for the transform.

Options are a dict keyed like `eesen_fbank_opts_t` (missing keys: the reference's defaults, DEFAULTS below); `window_type` by
name.  Everything after the integer frame geometry is float64: this is the arbiter the device extractor and the reference's own
float32 tool are both measured against.  Dither is not restated (the reference draws it from rand()): dither must be 0 here.
"""
import numpy as np

DEFAULTS = dict(samp_freq=16000.0, frame_shift_ms=10.0, frame_length_ms=25.0, dither=1.0, preemph_coeff=0.97, remove_dc_offset=True,
                window_type="povey", round_to_power_of_two=True, snip_edges=True, num_bins=23, low_freq=20.0, high_freq=0.0,
                vtln_low=100.0, vtln_high=-500.0, htk_mode=False, use_energy=False, energy_floor=0.0, raw_energy=True,
                htk_compat=False, use_log_fbank=True, vtln_warp=1.0, dither_seed=0)
FLT_MIN = float(np.finfo(np.float32).tiny)


def full(opts):
    o = dict(DEFAULTS)
    o.update(opts)
    return o


def geometry(opts):
    """(shift, length, padded length) in samples: WindowShift / WindowSize / PaddedWindowSize, which truncate a double product of
    the float32 options (feature-functions.h:119-128)."""
    o = full(opts)
    sf = float(np.float32(o["samp_freq"]))
    shift = int(sf * 0.001 * float(np.float32(o["frame_shift_ms"])))
    length = int(sf * 0.001 * float(np.float32(o["frame_length_ms"])))
    n = 1
    while n < length:
        n *= 2
    return shift, length, n


def num_frames(nsamp, opts):
    o = full(opts)
    shift, length, _ = geometry(o)
    if o["snip_edges"]:
        return 0 if nsamp < length else 1 + (nsamp - length) // shift
    return int(np.float32(np.float32(np.float32(nsamp) * np.float32(1.0)) / np.float32(shift)) + np.float32(0.5))   # float32, as written


def window_function(opts):
    o = full(opts)
    _, length, _ = geometry(o)
    i = np.arange(length, dtype=np.float64)
    c = np.cos(2.0 * np.pi * i / (length - 1))
    kind = o["window_type"]
    if kind == "hanning":
        return 0.5 - 0.5 * c
    if kind == "hamming":
        return 0.54 - 0.46 * c
    if kind == "povey":
        return (0.5 - 0.5 * c) ** 0.85
    if kind == "rectangular":
        return np.ones(length)
    raise ValueError("Invalid window type " + str(kind))


def mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, np.float64) / 700.0)


def inv_mel(m):
    return 700.0 * (np.exp(np.asarray(m, np.float64) / 1127.0) - 1.0)


def vtln_warp_freq(vtln_low, vtln_high, low, high, warp, f):
    """The three-piece linear warp of MelBanks::VtlnWarpFreq: identity at low and high, f / warp between the inflection points."""
    if f < low or f > high:
        return f
    lo = vtln_low * max(1.0, warp)
    hi = vtln_high * min(1.0, warp)
    scale = 1.0 / warp
    f_lo, f_hi = scale * lo, scale * hi
    if f < lo:
        return low + (f_lo - low) / (lo - low) * (f - low)
    if f < hi:
        return scale * f
    return high + (high - f_hi) / (high - hi) * (f - high)


def mel_filters(opts):
    """Dense [num_bins x N/2] float64 triangular filters over fft bins 0 .. N/2-1 (strict inequalities at the feet)."""
    o = full(opts)
    _, _, n = geometry(o)
    sf = float(np.float32(o["samp_freq"]))
    nyq = 0.5 * sf
    low = float(np.float32(o["low_freq"]))
    hf = float(np.float32(o["high_freq"]))
    high = hf if hf > 0.0 else nyq + hf
    nb = int(o["num_bins"])
    warp = float(np.float32(o["vtln_warp"]))
    vl = float(np.float32(o["vtln_low"]))
    vh = float(np.float32(o["vtln_high"]))
    if vh < 0.0:
        vh += nyq
    m_lo, m_hi = float(mel(low)), float(mel(high))
    delta = (m_hi - m_lo) / (nb + 1)
    m = mel(np.arange(n // 2) * (sf / n))
    filt = np.zeros((nb, n // 2))
    for b in range(nb):
        edges = [m_lo + (b + k) * delta for k in range(3)]
        if warp != 1.0:
            edges = [float(mel(vtln_warp_freq(vl, vh, low, high, warp, float(inv_mel(e))))) for e in edges]
        left, center, right = edges
        inside = (m > left) & (m < right)
        up = (m - left) / (center - left)
        down = (right - m) / (right - center)
        filt[b] = np.where(inside, np.where(m <= center, up, down), 0.0)
    return filt


def extract_windows(wave, opts):
    """[frames x length] float64: the cut (reflected without snip_edges), nothing else."""
    o = full(opts)
    shift, length, _ = geometry(o)
    wave = np.asarray(wave, np.float64)
    n = len(wave)
    t = num_frames(n, o)
    if t == 0:
        return np.zeros((0, length))
    i = np.arange(length)[None, :]
    f = np.arange(t)[:, None]
    if o["snip_edges"]:
        idx = f * shift + i
    else:
        idx = f * shift + shift // 2 - length // 2 + i            # int(shift * (f + 0.5)) - length / 2 + i
        neg = idx < 0
        over = idx >= n
        idx = np.where(neg, (-idx) % n, idx)
        idx = np.where(over, n - 1 - ((idx - n) % n), idx)
    return wave[idx]


def compute(wave, opts):
    """[frames x (num_bins + use_energy)] float64."""
    o = full(opts)
    assert float(o["dither"]) == 0.0, "the restatement has no dither"
    _, length, n = geometry(o)
    nb = int(o["num_bins"])
    x = extract_windows(wave, o)
    if x.shape[0] == 0:
        return np.zeros((0, nb + int(bool(o["use_energy"]))))
    if o["remove_dc_offset"]:
        x = x - x.sum(axis=1, keepdims=True) / length
    raw_energy = (x * x).sum(axis=1)
    c = float(np.float32(o["preemph_coeff"]))
    if c != 0.0:
        prev = np.concatenate([x[:, :1], x[:, :-1]], axis=1)
        x = x - c * prev
    x = x * window_function(o)[None, :]
    energy = raw_energy if o["raw_energy"] else (x * x).sum(axis=1)
    spec = np.fft.rfft(x, n=n, axis=1)[:, : n // 2]
    power = spec.real ** 2 + spec.imag ** 2
    out = power @ mel_filters(o).T
    if o["use_log_fbank"]:
        out = np.log(np.maximum(out, FLT_MIN))
    if o["use_energy"]:
        le = np.log(np.maximum(energy, FLT_MIN))
        floor = float(np.float32(o["energy_floor"]))
        if floor > 0.0:
            le = np.maximum(le, np.log(floor))
        out = np.concatenate([out, le[:, None]], axis=1) if o["htk_compat"] else np.concatenate([le[:, None], out], axis=1)
    return out


def distance(a, ref, opts):
    """max |delta| in the output domain: absolute for log features, relative to the reference matrix's largest value for linear ones
    (the energy column is a log in both)."""
    o = full(opts)
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if a.size == 0:
        return 0.0
    if o["use_log_fbank"]:
        return float(np.max(np.abs(a - ref)))
    nb = int(o["num_bins"])
    c0 = 1 if (o["use_energy"] and not o["htk_compat"]) else 0
    d = float(np.max(np.abs(a[:, c0:c0 + nb] - ref[:, c0:c0 + nb])) / max(float(np.max(np.abs(ref[:, c0:c0 + nb]))), FLT_MIN))
    if o["use_energy"]:
        e = nb if o["htk_compat"] else 0
        d = max(d, float(np.max(np.abs(a[:, e] - ref[:, e]))))
    return d
