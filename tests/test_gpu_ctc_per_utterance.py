"""-m gpu: the CTC loss and gradient (csrc/ctc.hip) held PER UTTERANCE against the fp64 oracle, on the posteriors a trained network emits.

tests/test_gpu_parity.py checks the gradient as one max-norm ratio over a whole minibatch of softmax(N(0, 2^2)) rows: an utterance, a frame
range or a class that is wrong by 100 % passes whenever its own magnitude is below 1e-4 of the batch maximum, and no probability is below
1e-5.  Here every comparison is made per utterance s over its valid frames, against the fp64 oracle on the same float32 probabilities
(tests/ctc_cases.py has the inputs and the metrics, tests/test_ctc_cases.py holds the conditions on the inputs without a GPU):

  gradient   max |diff - diff64| / max |diff64|            <  max(1e-4, 3 * floor_s)     (tests/util.diff_bound's rule, per utterance)
  ln p       |ln p - ln p64| / max(1, |ln p64|)            <  max(2e-6, 3 * floor_s(ln p))
  per frame  worst (row max error / row max) over the frames whose fp64 row maximum exceeds 1e-6 of the utterance's
                                                           <= 3 * the same figure of the fp32 oracle
  row sums   |sum_k diff[r, :]| on every valid row         <= max(1e-5, 3 * the fp32 oracle's largest on that utterance)
  padding    rows t >= len_s are exactly 0

floor_s is the fp32 oracle's own distance to fp64 in the same metric.  No bar comes from what the HIP code itself measured; its figures go to
$EESEN_PARITY_OUT/parity_ctc_per_utterance.json (committed from an MI355X run as profiles/parity_ctc_per_utterance.json) for the record only.

Legs: (a) peaky posteriors down to denormal probabilities, class 0 as a label, a lattice above 1024 positions; (b) the dense shapes of
test_ctc_vs_oracle and test_ctc_lattices_above_1024_positions again, per utterance; (c) probabilities of 1e-42 ... 0, where the fp32 reference
is itself off on a few frames: finite, the reference's special cases, and the bars on the other frames; (d) the shortest utterances the
reference's ln p formula works for, and one frame shorter (a reference quirk: finite, ln p = -1e30); (e) both sides of every dispatch step of
the gradient pass and of the row padding; (f) several frames per wave in the gradient pass, ragged lengths, an utterance of no frames;
(g) leading dimensions beyond K; (h) greedy decoding with exact ties.
"""
import ctypes as C
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import ctc_cases as cc
from tests.util import valid_mask

pytestmark = pytest.mark.gpu
TOL, LNP_TOL, ROWSUM_TOL = 1e-4, 2e-6, 1e-5


def _prepare(name):
    lens, probs, labels, T, S = cc.build(name)
    o32, o64 = cc.oracle_pair(lens, probs, labels, T, S)
    o64 = dict(diff=o64["diff"], pzx=o64["pzx"])          # (the fp64 lattices are not compared: hundreds of MB at the long shapes)
    return dict(name=name, lens=lens, probs=probs, labels=labels, T=T, S=S, o32=o32, o64=o64)


@pytest.fixture(scope="module")
def cases():
    """Every case's oracle pair, computed on a few threads while the first tests run (ctypes releases the GIL)."""
    pool = ThreadPoolExecutor(max_workers=8)
    futs = {}

    def get(name):
        if name not in futs:
            futs[name] = pool.submit(_prepare, name)
        return futs[name].result()

    for name in cc.CASES:
        futs[name] = pool.submit(_prepare, name)
    yield get
    pool.shutdown(wait=False, cancel_futures=True)


@pytest.fixture(scope="module")
def report():
    rows = []
    yield rows.append
    out = os.environ.get("EESEN_PARITY_OUT")
    if not out:
        return
    try:
        os.makedirs(out, exist_ok=True)
        json.dump(rows, open(os.path.join(out, "parity_ctc_per_utterance.json"), "w"), indent=1)
    except OSError:
        pass


def _hip(lens, probs, labels, lattice=True):
    from eesen_amd.api import CuMatrix, Ctc
    ctc = Ctc()
    diff = ctc.EvalParallel(lens, CuMatrix.from_numpy(probs), labels).numpy()
    out = dict(diff=diff, pzx=ctc.pzx.copy())
    if lattice:
        ctc._rows = probs.shape[0]
        out["alpha"], out["beta"] = ctc.alpha_beta()
    return out


def _hold_lattice(case, got, tol):
    """alpha and beta against the fp32 oracle, per utterance: the -1e30 sentinel pattern exactly; with `tol` the values element-wise (the same
    operation order up to the hardware exp / log of the log-add: fp32 round-off relative to max(1, |value|))."""
    S, lens = case["S"], case["lens"]
    for which in ("alpha", "beta"):
        g, r = got[which], case["o32"][which]
        assert g.shape == r.shape
        for s in range(S):
            gs, rs = cc.utt(g, s, S, int(lens[s])), cc.utt(r, s, S, int(lens[s]))
            assert np.array_equal(gs == -1e30, rs == -1e30), (which, s)
            if tol is not None:
                m = rs != -1e30
                assert np.max(np.abs(gs[m] - rs[m]) / np.maximum(1.0, np.abs(rs[m]))) < tol, (which, s)
        pad = ~valid_mask(lens, case["T"], S)
        assert np.all(g[pad] == -1e30), which


def _hold(case, got, report, leg, skip=(), extreme=False):
    """The bars of the module docstring on every utterance not in `skip`.  extreme: frames on which the fp32 REFERENCE is off by more than
    1e-3 of the utterance maximum are held to finiteness and the row sums only; an utterance the reference finds infeasible (ln p = -1e30)
    must come out infeasible with the reference's gradient."""
    lens, S, T, o32, o64 = case["lens"], case["S"], case["T"], case["o32"], case["o64"]
    diff, pzx = got["diff"], got["pzx"]
    assert np.all(np.isfinite(diff)) and np.all(np.isfinite(pzx))
    assert np.all(diff[~valid_mask(lens, T, S)] == 0)
    fails = []
    for s in range(S):
        if s in skip:
            continue
        n = int(lens[s])
        g, d32, d64 = cc.utt(diff, s, S, n), cc.utt(o32["diff"], s, S, n), cc.utt(o64["diff"], s, S, n)
        rec = dict(case=case["name"], leg=leg, s=s, frames=n, labels=len(case["labels"][s]), lnp=float(pzx[s]))
        if extreme and o32["pzx"][s] < -1e29:
            rec["infeasible"] = True
            report(rec)
            assert pzx[s] < -1e29, s
            assert np.array_equal(g, d32) and not g.any(), s
            continue
        keep = None
        if extreme:
            broken = cc.broken_frames(d32, d64)
            keep = ~broken
            rec["reference_broken_frames"] = int(broken.sum())
            if broken.any():    # recorded without a bar
                rec["hip_vs_fp32_oracle_on_broken_frames"] = cc.grad_figure(g[broken], d32[broken])
        gk, d32k, d64k = (g, d32, d64) if keep is None else (g[keep], d32[keep], d64[keep])
        floor, fig = cc.grad_figure(d32k, d64k), cc.grad_figure(gk, d64k)
        lfloor, lfig = cc.lnp_figure(o32["pzx"][s], o64["pzx"][s]), cc.lnp_figure(pzx[s], o64["pzx"][s])
        ffloor, ffig = cc.frame_figure(d32, d64, keep), cc.frame_figure(g, d64, keep)
        rs_ref = float(np.max(np.abs(d32.astype(np.float64).sum(axis=1))))
        rs = float(np.max(np.abs(g.astype(np.float64).sum(axis=1))))
        rec.update(floor=floor, hip=fig, lnp_floor=lfloor, lnp_hip=lfig, frame_floor=ffloor, frame_hip=ffig, rowsum_oracle=rs_ref, rowsum_hip=rs)
        report(rec)
        print(f"{case['name']} s={s} n={n}: grad {fig:.3g} (floor {floor:.3g}) lnp {lfig:.3g} (floor {lfloor:.3g}) "
              f"frame {ffig:.3g} (floor {ffloor:.3g}) rowsum {rs:.3g} (oracle {rs_ref:.3g})")
        if not fig < max(TOL, 3 * floor): fails.append((s, "gradient", fig, floor))
        if not lfig < max(LNP_TOL, 3 * lfloor): fails.append((s, "ln p", lfig, lfloor))
        if not ffig <= 3 * ffloor: fails.append((s, "per frame", ffig, ffloor))
        if not rs <= max(ROWSUM_TOL, 3 * rs_ref): fails.append((s, "row sum", rs, rs_ref))
    assert not fails, fails


# ------------------------------------------------------------------------------------------ (a) peaky, held to fp64
@pytest.mark.parametrize("name", cc.PEAKY_HELD)
def test_peaky_posteriors(gpu, cases, report, name):
    case = cases(name)
    got = _hip(case["lens"], case["probs"], case["labels"])
    if name == "peaky_long":
        assert got["alpha"].shape[1] > 1024
    # class 0 as a label: test_ctc_vs_oracle's value check of the lattice; above T = 1500 test_ctc_lattices_above_1024_positions'
    _hold_lattice(case, got, 2e-6 if name in cc.CLASS0_CASES else 5e-6 if case["T"] > 1500 else None)
    _hold(case, got, report, "a")


# ------------------------------------------------------------------------------------------ (b) dense, per utterance
@pytest.mark.parametrize("name", [n for n in cc.CASES if n.startswith(("dense_", "long_"))])
def test_dense_posteriors_per_utterance(gpu, cases, report, name):
    case = cases(name)
    got = _hip(case["lens"], case["probs"], case["labels"])
    _hold_lattice(case, got, 5e-6 if case["T"] > 1500 else 2e-6)
    _hold(case, got, report, "b")


# ------------------------------------------------------------------------------------------ (c) extreme
def test_extreme_posteriors(gpu, cases, report):
    """Spike heights 95 ... 120: lattice-class probabilities of 1e-42 ... 1e-45 and exact zeros.  The contract there is "finite, and the same
    special cases as the reference", plus the bars of (a) on the frames where the fp32 reference itself is an accurate evaluation."""
    case = cases("extreme")
    got = _hip(case["lens"], case["probs"], case["labels"], lattice=False)
    _hold(case, got, report, "c", extreme=True)


# ------------------------------------------------------------------------------------------ (d) shortest utterances
@pytest.mark.parametrize("name", ["shortest_dense", "shortest_h12"])
def test_shortest_utterances(gpu, cases, report, name):
    case = cases(name)
    got = _hip(case["lens"], case["probs"], case["labels"])
    _hold_lattice(case, got, 2e-6)
    _hold(case, got, report, "d")


@pytest.mark.parametrize("name", ["one_short_dense", "one_short_h12"])
def test_one_frame_short_of_the_ln_p_formula(gpu, cases, report, name):
    """len_s = U_s + repeats: a path exists, but the last blank is unreachable, the reference's ln p = -1e30 + log(1 + FLT_MAX) rounds to -1e30
    and its gradient is of the order of FLT_MAX in both precisions (CTC quirks).  Held: finite, and ln p as the fp32 oracle
    has it; the gradient's distance to the fp32 oracle is recorded without a bar."""
    case = cases(name)
    assert np.all(case["o32"]["pzx"] < -1e29)
    got = _hip(case["lens"], case["probs"], case["labels"], lattice=False)
    assert np.all(np.isfinite(got["diff"])) and np.all(np.isfinite(got["pzx"]))
    assert np.all(got["pzx"] < -1e29)
    assert np.all(got["diff"][~valid_mask(case["lens"], case["T"], case["S"])] == 0)
    for s in range(case["S"]):
        n = int(case["lens"][s])
        report(dict(case=name, leg="d", s=s, frames=n, labels=len(case["labels"][s]), lnp=float(got["pzx"][s]),
                    hip_vs_fp32_oracle=cc.grad_figure(cc.utt(got["diff"], s, case["S"], n), cc.utt(case["o32"]["diff"], s, case["S"], n))))


def test_last_label_spiking_on_the_last_frame(gpu):
    """The other face of the same clamp in the reference's ln p formula (tests/ctc_cases.py: last_frame_spike_case): the fp32 reference is tens of
    nats off the true ln p, and the library reproduces the reference, not fp64."""
    lens, probs, labels = cc.last_frame_spike_case()
    o32, o64 = cc.oracle_pair(lens, probs, labels, len(probs), 1)
    got = _hip(lens, probs, labels)
    assert abs(o64["pzx"][0]) < 1e-6 and o32["pzx"][0] < -20
    assert cc.lnp_figure(got["pzx"][0], o32["pzx"][0]) < LNP_TOL
    assert np.all(np.isfinite(got["diff"])) and np.array_equal(got["alpha"] == -1e30, o32["alpha"] == -1e30)


# ------------------------------------------------------------------------------------------ (e) dispatch boundaries
@pytest.mark.parametrize("U", cc.BOUNDARY_U)
def test_dispatch_boundaries(gpu, cases, report, U):
    case = cases(f"boundary_U{U}")
    got = _hip(case["lens"], case["probs"], case["labels"])
    assert got["alpha"].shape[1] == 2 * U + 1
    _hold_lattice(case, got, 5e-6 if case["T"] > 1500 else None)
    _hold(case, got, report, "e")


# ------------------------------------------------------------------------------------------ (f) several frames per wave
@pytest.mark.parametrize("name", list(cc.FRAMES_CASES))
def test_several_frames_per_wave(gpu, cases, report, name):
    """32768 <= rows < 49152 (two frames per wave of the gradient pass) and rows >= 131072 (eight), odd T that is no multiple of the chunk,
    ragged lengths so that chunks straddle len_s.  One utterance of the batch has NO frames: the reference is undefined there (it reads the
    row before the first), so that utterance is held to the library's documented answer -- ln p = -1e30 and all-zero rows -- and every other
    utterance to the oracle, and bit for bit to a run of the same batch in which that utterance has its full length."""
    case = cases(name)
    lens, probs, labels, T, S = case["lens"], case["probs"], case["labels"], case["T"], case["S"]
    assert max(1, min(8, T * S // 16384)) == cc.FRAMES_CASES[name]
    full = _hip(lens, probs, labels, lattice=T > 1500)
    if T > 1500:
        _hold_lattice(case, full, 5e-6)
    _hold(case, full, report, "f")
    e = S // 2
    lens0 = lens.copy(); lens0[e] = 0
    runs = [_hip(lens0, probs, labels, lattice=False) for _ in range(2)]
    assert np.array_equal(runs[0]["diff"], runs[1]["diff"]) and np.array_equal(runs[0]["pzx"], runs[1]["pzx"])      # reproducible run to run
    got = runs[0]
    assert got["pzx"][e] < -1e29 and not got["diff"][e::S].any()
    others = np.arange(S) != e
    assert np.array_equal(got["pzx"][others], full["pzx"][others])
    rows_of_others = np.tile(others, T)
    assert np.array_equal(got["diff"][rows_of_others], full["diff"][rows_of_others])


# ------------------------------------------------------------------------------------------ (g) leading dimensions
def _device_buffer(host):
    from eesen_amd import _lib
    from eesen_amd.api import CuMatrix, _np_ptr
    host = np.ascontiguousarray(host, np.float32).ravel()
    own = CuMatrix(1, host.size, zero=False)
    _lib.check(_lib.load().eesen_dev_copy(0, C.c_void_p(own.ptr), _np_ptr(host), host.nbytes, 1))
    return own


def _download(own, n):
    from eesen_amd import _lib
    from eesen_amd.api import _np_ptr
    buf = np.empty(n, np.float32)
    _lib.check(_lib.load().eesen_dev_copy(0, _np_ptr(buf), C.c_void_p(own.ptr), buf.nbytes, 2))
    return buf


def test_leading_dimensions(gpu, cases):
    """net_out and diff in buffers whose row stride exceeds K (pad4: the next multiple of 4, as CuMatrix allocates; wide: 8 more columns, as in
    tests/test_gpu_ce.py): bit-identical to the tight layout (stride K), and nothing between K and the stride of `diff` is written."""
    from eesen_amd.api import CuMatrix, Ctc
    case = cases("peaky_T1500")
    lens, probs, labels = case["lens"], case["probs"], case["labels"]
    rows, K = probs.shape
    assert K % 4 != 0
    results = {}
    for layout, ld in (("tight", K), ("pad4", (K + 3) & ~3), ("wide", ((K + 3) & ~3) + 8)):
        src = np.full((rows, ld), 0.25, np.float32)        # (a value a kernel that read beyond K would fold into its sums)
        src[:, :K] = probs
        din = _device_buffer(src)
        dout = _device_buffer(np.full(rows * ld + 1, np.nan, np.float32))
        ctc = Ctc()
        ctc.EvalParallel(lens, CuMatrix.view(din.ptr, rows, K, ld, keepalive=din), labels, diff=CuMatrix.view(dout.ptr, rows, K, ld, keepalive=dout))
        raw = _download(dout, rows * ld + 1)
        assert np.isnan(raw[-1]) and np.all(np.isnan(raw[:-1].reshape(rows, ld)[:, K:]))
        results[layout] = (raw[:-1].reshape(rows, ld)[:, :K].copy(), ctc.pzx.copy())
        assert np.all(np.isfinite(results[layout][0]))
    for layout in ("pad4", "wide"):
        assert np.array_equal(results[layout][0], results["tight"][0]) and np.array_equal(results[layout][1], results["tight"][1]), layout
    ref = _hip(lens, probs, labels, lattice=False)          # and the path every other test takes
    assert np.array_equal(ref["diff"], results["tight"][0])


# ------------------------------------------------------------------------------------------ (h) greedy decode
@pytest.mark.parametrize("which", ["peaky", "ties", "ties_wide"])
def test_greedy_decode(gpu, which):
    """ErrorRateMSeq: the row argmax takes the LOWEST index among equal maxima (the reference's FindRowMaxId: strict '<'), at index 0, at index
    K - 1, and across the 64-lane stride of the kernel (K = 150)."""
    from eesen_amd.api import CuMatrix, Ctc
    from oracle import net as onet
    if which == "peaky":
        lens, probs, labels, T, S = cc.build("peaky_h4_60")
    else:
        S, T, K = (4, 120, 12) if which == "ties" else (3, 90, 150)
        lens, probs, labels = cc.tie_case(S, T, K, 3)
    ids, off = cc.csr(labels)
    ctc = Ctc()
    got = ctc.ErrorRateMSeq(lens, CuMatrix.from_numpy(probs), labels)
    assert got == onet.ctc_error_rate_mseq(probs, T, S, lens, ids, off)
    assert got[1] == len(ids) and ctc.stats()["err_tokens"] == got[0]
