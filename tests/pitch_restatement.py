"""numpy restatement of the pitch extractor (eesen_amd/csrc/pitch.hip), written from its description in INTEGRATION.md "Pitch".

Two modes.  `np.float64`: tables, products and sums in double; what the device and the reference's tools are both held against.
`np.float32`: the tables rounded once, every product and sum in float32 and in the kernels' order (taps and window samples are added
one after the other, lowest index first); its distance from the float64 mode is what float32 costs on a case, and three times
that is the bound the device's stages get.  `search` is the Viterbi stage alone and has one arithmetic only: float32, no fused
multiply-add, in the order written in pitch.hip's header, so that fed the device's own NCCF matrix it reproduces the device bit
for bit.
"""
import math

import numpy as np

DEFAULTS = dict(samp_freq=16000.0, frame_shift_ms=10.0, frame_length_ms=25.0, preemph_coeff=0.0, min_f0=50.0, max_f0=400.0,
                soft_min_f0=10.0, penalty_factor=0.1, lowpass_cutoff=1000.0, resample_freq=4000.0, delta_pitch=0.005,
                nccf_ballast=7000.0, lowpass_filter_width=1, upsample_filter_width=5, max_frames_latency=0, frames_per_chunk=0,
                simulate_first_pass_online=False, recompute_frame=500, nccf_ballast_online=False, snip_edges=True)
PROCESS_DEFAULTS = dict(pitch_scale=2.0, pov_scale=2.0, pov_offset=0.0, delta_pitch_scale=10.0, delta_pitch_noise_stddev=0.005,
                        normalization_left_context=75, normalization_right_context=75, delta_window=2, delay=0,
                        add_pov_feature=True, add_normalized_log_pitch=True, add_delta_pitch=True, add_raw_log_pitch=False)
f32 = np.float32


def full(opts):
    o = dict(DEFAULTS)
    o.update({k: v for k, v in opts.items() if k in DEFAULTS})
    return o


def full_process(opts):
    o = dict(PROCESS_DEFAULTS)
    o.update({k: v for k, v in opts.items() if k in PROCESS_DEFAULTS})
    return o


def _sf(v):
    return float(f32(v))     # an option as the float the C struct holds


def geometry(opts):
    """(window, shift, first_lag, last_lag) in down-sampled samples."""
    o = full(opts)
    rf = _sf(o["resample_freq"])
    window = int(rf * 0.001 * _sf(o["frame_length_ms"]))
    shift = int(rf * 0.001 * _sf(o["frame_shift_ms"]))
    half = o["upsample_filter_width"] / (2.0 * rf)
    first = int(math.ceil(rf * (1.0 / _sf(o["max_f0"]) - half)))
    last = int(math.floor(rf * (1.0 / _sf(o["min_f0"]) + half)))
    return window, shift, first, last


def lags(opts):
    """The geometric lag grid in seconds, float32: 1 / max_f0, times (1 + delta_pitch) while it stays at or below 1 / min_f0; each
    value is the float32 rounding of the double product of the one before."""
    o = full(opts)
    lag, top, ratio = f32(1.0 / _sf(o["max_f0"])), f32(1.0 / _sf(o["min_f0"])), 1.0 + _sf(o["delta_pitch"])
    out = []
    while lag <= top:
        out.append(lag)
        lag = f32(float(lag) * ratio)
    return np.array(out, f32)


def _rates(o):
    return int(_sf(o["samp_freq"])), int(_sf(o["resample_freq"]))


def num_output_samples(nsamp, opts, flush):
    """Down-sampled samples of a waveform of nsamp: the output instants k / rate_out inside [0, nsamp / rate_in), less the filter's
    half width (floored to ticks of 1 / lcm of the rates) unless the tail is flushed."""
    o = full(opts)
    rin, rout = _rates(o)
    tick = rin * rout // math.gcd(rin, rout)
    length = nsamp * (tick // rin)
    if not flush:
        width = f32(o["lowpass_filter_width"] / (2.0 * _sf(o["lowpass_cutoff"])))
        length -= int(math.floor(f32(width * f32(tick))))
    if length <= 0:
        return 0
    per_out = tick // rout
    last = length // per_out
    if last * per_out == length:
        last -= 1
    return last + 1


def num_frames(nsamp, opts):
    """(frames of the first pass, frames in all, samples of the first pass, samples in all)."""
    o = full(opts)
    window, shift, _, last = geometry(o)
    n1, n2 = num_output_samples(nsamp, o, False), num_output_samples(nsamp, o, True)
    f1 = 0 if n1 < window + last else (n1 - window - last) // shift + 1
    if n2 < window:
        fa = 0
    elif o["snip_edges"]:
        fa = (n2 - window) // shift + 1
    else:
        fa = int(f32(f32(n2) * f32(1.0) / f32(shift)) + f32(0.5))
    return f1, max(fa, f1), n1, n2


def _filter(t, cutoff, zeros):
    """Hann-windowed sinc at offsets t (seconds, float64)."""
    t = np.asarray(t, np.float64)
    win = np.where(np.abs(t) < zeros / (2.0 * cutoff), 0.5 * (1.0 + np.cos(2.0 * np.pi * cutoff / zeros * t)), 0.0)
    safe = np.where(t != 0.0, t, 1.0)
    return np.where(t != 0.0, np.sin(2.0 * np.pi * cutoff * safe) / (np.pi * safe), 2.0 * cutoff) * win


def downsample_tables(opts):
    """(input samples per unit, output samples per unit, first input index per phase, weight vector per phase [float64])."""
    o = full(opts)
    rin, rout = _rates(o)
    g = math.gcd(rin, rout)
    cutoff, zeros = _sf(o["lowpass_cutoff"]), o["lowpass_filter_width"]
    width = zeros / (2.0 * cutoff)
    first, weights = [], []
    for i in range(rout // g):
        t = i / float(rout)
        lo, hi = int(math.ceil((t - width) * rin)), int(math.floor((t + width) * rin))
        idx = np.arange(lo, hi + 1)
        first.append(lo)
        weights.append(_filter(idx / float(rin) - t, cutoff, zeros) / rin)
    return rin // g, rout // g, first, weights


def downsample(wave, opts, dtype=np.float64):
    """The down-sampled signal with its flushed tail; input samples before the start and past the end count as zero."""
    o = full(opts)
    n_in, n_out, first, weights = downsample_tables(o)
    wave = np.asarray(wave, dtype)
    n2 = num_output_samples(len(wave), o, True)
    out = np.zeros(n2, dtype)
    for ph in range(min(n_out, n2)):
        k = np.arange(ph, n2, n_out)
        base = first[ph] + (k // n_out) * n_in
        acc = np.zeros(len(k), dtype)
        for j, w in enumerate(weights[ph].astype(dtype)):
            idx = base + j
            ok = (idx >= 0) & (idx < len(wave))
            acc = acc + np.where(ok, w * wave[np.clip(idx, 0, max(len(wave) - 1, 0))], dtype(0)) if len(wave) else acc
        out[k] = acc
    return out


def mean_squares(down, n1):
    """(mean square without the flushed tail, with it), float64: sum x^2 / n - (sum x / n)^2."""
    d = np.asarray(down, np.float64)

    def ms(v):
        return float(np.sum(v * v) / len(v) - (np.sum(v) / len(v)) ** 2) if len(v) else 0.0
    return ms(d[:n1]), ms(d)


def upsample_tables(opts):
    """CSR rows of the NCCF up-sampler: (first integer-lag column per output lag, weight vector per output lag [float64])."""
    o = full(opts)
    _, _, first_lag, last_lag = geometry(o)
    rf, zeros = _sf(o["resample_freq"]), o["upsample_filter_width"]
    cutoff = 0.5 * rf
    n_in = last_lag + 1 - first_lag
    pts = (lags(o) + f32(-first_lag / rf)).astype(f32).astype(np.float64)
    width = zeros / (2.0 * cutoff)
    first, weights = [], []
    for t in pts:
        lo = max(int(math.ceil(rf * (t - width))), 0)
        hi = min(int(math.floor(rf * (t + width))), n_in - 1)
        idx = np.arange(lo, hi + 1)
        first.append(lo)
        weights.append(_filter(t - idx / rf, cutoff, zeros) / rf)
    return first, weights


def nccf(down, nsamp, opts, dtype=np.float64):
    """Per frame, on the integer lags: (NCCF with the ballast, NCCF without it, average of e1 * e2, the two mean squares)."""
    o = full(opts)
    window, shift, first_lag, last_lag = geometry(o)
    f1, frames, n1, n2 = num_frames(nsamp, o)
    ms1, ms2 = mean_squares(down, n1)
    nl = last_lag + 1 - first_lag
    flen = window + last_lag
    x = np.zeros((frames, flen), dtype)
    d = np.asarray(down, dtype)
    for f in range(frames):
        seg = d[f * shift:f * shift + flen]
        x[f, :len(seg)] = seg
    if dtype == np.float64:
        mean = x[:, :window].sum(1) / window
    else:
        mean = np.zeros(frames, dtype)
        for k in range(window):
            mean = mean + x[:, k]
        mean = mean / dtype(window)
    x = x - mean[:, None]
    e1 = np.zeros(frames, dtype)
    ip = np.zeros((frames, nl), dtype)
    e2 = np.zeros((frames, nl), dtype)
    lagcol = first_lag + np.arange(nl)
    for k in range(window):
        a = x[:, k]
        b = x[:, lagcol + k]
        e1 = e1 + a * a
        ip = ip + a[:, None] * b
        e2 = e2 + b * b
    norm = e1[:, None] * e2
    ms = np.where(np.arange(frames) < f1, ms1, ms2)
    ballast = ((ms * window) ** 2 * _sf(o["nccf_ballast"])).astype(dtype)
    den = np.sqrt(norm + ballast[:, None])
    with np.errstate(divide="ignore", invalid="ignore"):
        pitch = np.where(den != 0, ip / den, dtype(0)).astype(dtype)
        den0 = np.sqrt(norm)
        pov = np.where(den0 != 0, ip / den0, dtype(0)).astype(dtype)
    if dtype == np.float64:
        avg = norm.sum(1) / nl
    else:
        avg = np.zeros(frames, dtype)
        for k in range(nl):
            avg = avg + norm[:, k]
        avg = avg / dtype(nl)
    return pitch, pov, avg, (ms1, ms2)


def upsample(rows, opts, dtype=np.float64):
    """[frames x integer lags] -> [frames x lag grid] through the CSR table, taps added lowest first."""
    first, weights = upsample_tables(opts)
    rows = np.asarray(rows, dtype)
    out = np.zeros((rows.shape[0], len(first)), dtype)
    for i, (lo, w) in enumerate(zip(first, weights)):
        acc = np.zeros(rows.shape[0], dtype)
        for j, wj in enumerate(w.astype(dtype)):
            acc = acc + wj * rows[:, lo + j]
        out[:, i] = acc
    return out


def reestimate(avg_norm_prod, ms1, ms2, f1, frames, opts):
    """(taken, per-frame scale [float32]) of the energy re-estimate: float32 arithmetic on float32 ballasts, correctly rounded
    division and square root, exactly as the head of the search kernel does it."""
    o = full(opts)
    window = geometry(o)[0]
    scale = np.ones(frames, f32)
    n_re = min(frames, int(o["recompute_frame"])) if f1 < int(o["recompute_frame"]) else 0
    a, b = f32(ms1), f32(ms2)
    if n_re == 0 or f1 == 0:
        return False, scale
    same = a == b or abs(f32(a - b)) <= f32(f32(0.01) * f32(abs(a) + abs(b)))
    if same:
        return False, scale
    nb = _sf(o["nccf_ballast"])
    old = f32((float(a) * window) * (float(a) * window) * nb)
    new = f32((float(b) * window) * (float(b) * window) * nb)
    k = min(f1, n_re)
    anp = np.asarray(avg_norm_prod, f32)[:k]
    scale[:k] = np.sqrt((old + anp) / (new + anp))
    return True, scale


def inter_frame_factor(opts):
    o = full(opts)
    lg = math.log(1.0 + _sf(o["delta_pitch"]))
    return f32(f32(lg * lg) * f32(o["penalty_factor"]))


def search(nccf_pitch, nccf_pov, scale, opts):
    """The Viterbi stage in the kernel's float32 order.  Per frame and state i, with n = nccf * scale[frame] (only where a
    re-estimate was taken):
        local  = (1 - n) + (soft_min_f0 * lag_i) * n
        cand_j = ((j - i) * (j - i)) * factor + prev_j            for j = 0, 1, ...; the first strictly smallest wins
        fwd_i  = cand_best + local;   then fwd -= min(fwd)
    Returns (forward costs after the last frame, back pointers [frames x states] uint16, track [frames], output [frames x 2])."""
    o = full(opts)
    lg = lags(o)
    ns = len(lg)
    n_all = np.asarray(nccf_pitch, f32)
    frames = n_all.shape[0]
    factor = inter_frame_factor(o)
    klag = (f32(o["soft_min_f0"]) * lg).astype(f32)
    idx = np.arange(ns, dtype=f32)
    diff = idx[None, :] - idx[:, None]                      # [i, j] = j - i
    trans = ((diff * diff).astype(f32) * factor).astype(f32)
    prev = np.zeros(ns, f32)
    bp = np.zeros((frames, ns), np.uint16)
    one = f32(1.0)
    for f in range(frames):
        n = n_all[f] if scale is None or scale[f] == one else (n_all[f] * f32(scale[f])).astype(f32)
        local = ((one - n).astype(f32) + (klag * n).astype(f32)).astype(f32)
        cand = (trans + prev[None, :]).astype(f32)
        best = np.argmin(cand, axis=1)                      # the first minimum
        bp[f] = best
        fwd = (cand[np.arange(ns), best] + local).astype(f32)
        prev = (fwd - fwd.min()).astype(f32)
    track = np.zeros(frames, np.int32)
    s = int(np.argmin(prev)) if frames else 0
    for f in range(frames - 1, -1, -1):
        track[f] = s
        s = int(bp[f, s])
    out = np.zeros((frames, 2), f32)
    if frames:
        out[:, 0] = np.asarray(nccf_pov, f32)[np.arange(frames), track]
        out[:, 1] = (1.0 / lg.astype(np.float64)[track]).astype(f32)
    return prev, bp, track, out


def compute(wave, opts, dtype=np.float64):
    """All of (a)-(f) on one waveform: dict of the stage outputs; `out` is the [frames x 2] (NCCF, pitch) matrix or None."""
    o = full(opts)
    f1, frames, n1, n2 = num_frames(len(wave), o)
    down = downsample(wave, o, dtype)
    if frames == 0:
        return dict(frames=0, down=down, out=None, taken=False)
    pitch_i, pov_i, avg, (ms1, ms2) = nccf(down, len(wave), o, dtype)
    pitch_u, pov_u = upsample(pitch_i, o, dtype), upsample(pov_i, o, dtype)
    taken, scale = reestimate(avg, ms1, ms2, f1, frames, o)
    fwd, bp, track, out = search(pitch_u, pov_u, scale if taken else None, o)
    return dict(frames=frames, f1=f1, down=down, nccf_pitch=pitch_u, nccf_pov=pov_u, avg_norm_prod=avg, ms=(ms1, ms2), taken=taken,
                scale=scale, fwd=fwd, bp=bp, track=track, out=out)


def nccf_to_pov(n):
    n = np.minimum(np.abs(np.asarray(n, np.float64)), 1.0)
    r = -5.2 + 5.4 * np.exp(7.5 * (n - 1.0)) + 4.8 * n - 2.0 * np.exp(-10.0 * n) + 4.2 * np.exp(20.0 * (n - 1.0))
    return 1.0 / (1.0 + np.exp(-r))


def process_dim(popts):
    p = full_process(popts)
    return int(bool(p["add_pov_feature"])) + int(bool(p["add_normalized_log_pitch"])) + int(bool(p["add_delta_pitch"])) + int(bool(p["add_raw_log_pitch"]))


def prefix_sums(v):
    """P[t] = sum of v over frames < t, T + 1 entries."""
    return np.concatenate([[0.0], np.cumsum(v)])


def prefix_sums_without_carry(v, chunk=256):
    """A WRONG prefix sum, for the tests' teeth: scanned `chunk` frames at a time as pitch_process_kernel does, but every chunk
    starts again from zero.  Equal to prefix_sums up to `chunk` frames and on no longer input."""
    v = np.asarray(v, np.float64)
    return np.concatenate([[0.0]] + [np.cumsum(v[b:b + chunk]) for b in range(0, len(v), chunk)])


def process(raw, popts, noise=None, prefix=prefix_sums):
    """Post-processing of a [T x 2] (NCCF, pitch) matrix in float64 -> [T + delay x columns].  `noise`: the per-frame standard
    normal draws (None: zero).  `prefix`: how the two pov-weighted prefix sums are formed."""
    p = full_process(popts)
    raw = np.asarray(raw, np.float64)
    T = raw.shape[0]
    nc, lp = raw[:, 0], np.log(raw[:, 1])
    cols = []
    if p["add_pov_feature"]:
        cols.append(p["pov_scale"] * ((1.0001 - np.clip(nc, -1.0, 1.0)) ** 0.15 - 1.0) + p["pov_offset"])
    if p["add_normalized_log_pitch"]:
        pov = nccf_to_pov(nc)
        c1 = prefix(pov)
        c2 = prefix(pov * lp)
        t = np.arange(T)
        b = np.maximum(t - p["normalization_left_context"], 0)
        e = np.minimum(t + p["normalization_right_context"] + 1, T)
        cols.append(p["pitch_scale"] * (lp - (c2[e] - c2[b]) / (c1[e] - c1[b])))
    if p["add_delta_pitch"]:
        w = int(p["delta_window"])
        norm = float(sum(j * j for j in range(-w, w + 1)))
        d = np.zeros(T)
        for j in range(-w, w + 1):
            d += (j / norm) * lp[np.clip(np.arange(T) + j, 0, T - 1)]
        if noise is not None:
            d = d + np.asarray(noise, np.float64) * p["delta_pitch_noise_stddev"]
        cols.append(d * p["delta_pitch_scale"])
    if p["add_raw_log_pitch"]:
        cols.append(lp)
    m = np.stack(cols, 1)
    rows = np.maximum(np.arange(T + int(p["delay"])) - int(p["delay"]), 0)
    return m[rows]
