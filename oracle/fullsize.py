"""One trainer step of THE REFERENCE ITSELF (oracle/_ref) at a BASELINE configuration's full size, and the compact
fixture of it that travels in tests/golden/ for boxes without the reference library.  TEST INFRASTRUCTURE.

    python -m oracle.fullsize            # (re)generate tests/golden/full_*.npz where /root/reference exists
    python -m oracle.fullsize --backward-leg [NAME ...]   # the reference's backward pass on the fixed top gradient `od`
                                                          # (fixed_top_gradient) -> tests/golden/full_*_bwd*.npz

The step is the one of /root/reference/src/netbin/train-ctc-parallel.cc:195-207 with lr = 1, momentum = 0,
<MaxGrad> 0, which turns the parameter delta into the gradient.  The reference's CTC exists
only as CUDA kernels; oracle/_ref runs their bodies per emulated thread (oracle/ref_build/ref_cuda_emul.cc).
A full step of cfg2 (S=32, T=1000, 4x512 BiLSTM) takes ~12 s on 16 BLAS threads.

The fixture keeps what a size-independent comparison needs: ln p per sequence, per-tensor gradient statistics
(max |g|, sum, sum |g|, sum g^2), a SAMPLE of the gradient (every STRIDE-th element plus every tensor of at most SMALL elements
whole), and every ROW_STRIDE-th row of net_out / diff / in_diff -- each of the samples twice: from the reference step, and from
the reference's backward pass on an fp64 evaluation of ITS OWN CTC (the floor its fp32 CTC round-off imposes), so that every
error metric of tests/util.py::err_metrics can be formed for "HIP vs reference" and for "the reference vs its own fp64 CTC" on
the same elements, with and without the reference library on the box.
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

from eesen_amd import nnet_io, synth

STRIDE = 1009        # gradient sample: every 1009th element of the Net::GetParams-ordered vector (prime: hits every tensor and row phase)
SMALL = 8192         # ... plus every tensor of at most this many elements whole (biases, peepholes: a stride sample would hold 1-4 of them)
ROW_STRIDE = 97      # row sample of the [T*S x .] matrices
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")

# name -> (synth config name, overrides).  full_cfg2 is exactly what bench.py times (seed 777).
CASES = {
    "full_cfg2": ("cfg2", {}),
    "full_cfg4_layer": ("cfg4", dict(layers=1, proj=0)),     # one 1024-cell BiLSTM layer at T=1000: the wide persistent tiles
    # BASELINE.json configs[3]: 5 x 1024 BiLSTM with 512-d <AffineTransform> projections between the layers
    # (asr_egs/wsj/utils/model_topo.py:99-128), K = 51, S = 32, T = 1000 -- exactly what bench.py's cfg4 leg times
    "full_cfg4": ("cfg4", {}),
    # BASELINE.json configs[4] at its 1000-frame length bucket: 6 x 1024 BiLSTM, S = 64 utterances per GPU (two sequence windows
    # of the wide backward tile, the time-multiplexed forward kernel), K = 51
    "full_cfg5_b1000": ("cfg5", dict(T=1000)),
    # BASELINE.json configs[4] at its 3000-FRAME bucket (U = 300 labels: L' = 601, lattice values |alpha| ~ 3e3).  The reference
    # keeps four [(T+2)S x 7H] state buffers per layer (bilstm-layer.h:1131-1136): 6 layers x S = 64 x T = 3000 are 132 GB of
    # them, twice the authoring container's memory, so the bucket is pinned by two cuts that each keep one axis whole:
    #   _l2:  TWO layers at the full S = 64 (the time-multiplexed kernels with two sequence tiles per workgroup, the gate-gradient
    #         buffer beyond 2 GB: T*S*8H*4 B = 6.3 GB, the PL = 10 lattice kernel at S = 64);
    #   _s16: the full SIX-layer stack at S = 16 (how six 1024-cell layers carry the 3000-frame lattice's round-off down).
    "full_cfg5_b3000_l2": ("cfg5", dict(layers=2)),
    "full_cfg5_b3000_s16": ("cfg5", dict(S=16)),
    # round 5: the kernels narrow layers take at --num-sequence 64 (two forward workgroups per CU, two 4-sequence tiles per backward
    # workgroup, no side stream) -- BASELINE configs[1]'s net on 64 utterances ...
    "full_cfg2_s64": ("cfg2", dict(S=64)),
    # ... and the recipes' own width (asr_egs/wsj/utils/model_topo.py: 320 cells per direction on 120-d features) at full length:
    # the 4 x 32 backward tile where K = 4H does not fill the waves' chunk pairs (lstm_bwd_persistent_q4_kernel<6, 4>)
    "full_recipe320": ("cfg2", dict(H=320, D=120)),
}
# cases whose reference step is too long to repeat inside the default GPU suite: the committed fixture (made by this script from
# the reference) is the arbiter unless EESEN_FULLSIZE_LIVE=1
FIXTURE_FIRST = {"full_cfg5_b1000", "full_cfg5_b3000_l2", "full_cfg5_b3000_s16", "full_cfg3", "full_cfg2_s64", "full_recipe320"}
# cases that only fit the host's memory with the layer-by-layer backward of ref_driver.cc (ref_net_backpropagate_lowmem: the
# reference's own per-layer Backpropagate + Update in Net::Backpropagate's order, each layer's state buffers released after use)
LOWMEM = {"full_cfg5_b3000_l2", "full_cfg5_b3000_s16", "full_cfg3"}

# BASELINE.json configs[2]: the GLOBAL minibatch of the 8-GPU run -- 256 utterances, T = 1000, 4 x 512 -- as ONE reference process
# with --num-sequence = 256 ("N ranks x S == reference with --num-sequence = N*S").  The HIP side runs it
# as 8 shards of 32 utterances (parallel.shard_batch: the interleaved deal the ranks use) and sums the gradients.
CFG3 = ("cfg2", dict(S=256))
CFG3_WORLD = 8
# the throughput settings of the recipes (asr_egs/wsj/run_ctc_phn.sh:84-85, utils/model_topo.py:90): what momentum and clipping
# do to the SUMMED gradient over two steps
CFG3_LR, CFG3_MOMENTUM, CFG3_MAX_GRAD, CFG3_STEPS = 4e-5, 0.9, 50.0, 2


def case(name: str):
    cfg_name, over = CFG3 if name == "full_cfg3" else CASES[name]
    cfg = synth.config(cfg_name)
    cfg.update(over)
    return cfg, synth.make_model(**cfg), synth.make_batch(**cfg)


def _ref_net(layers):
    from oracle import refbind
    path = tempfile.mktemp(suffix=".nnet")
    nnet_io.write_nnet(path, layers, binary=True)
    try:
        return refbind.RefNet(path)
    finally:
        os.unlink(path)


def reference_step(layers, batch, blas_threads: int = 0, diff_override=None, lowmem: bool = False) -> dict:
    """Runs the reference. Returns net_out, pzx, diff, in_diff, grads (Net::GetParams order), alpha-free (too large).
    diff_override: backpropagate THIS matrix instead of the reference CTC's own gradient (e.g. an fp64 evaluation of the CTC on the
    reference's probabilities: how far the reference's fp32 CTC round-off moves the reference's own gradients)."""
    from oracle import refbind
    if blas_threads <= 0:
        blas_threads = min(16, os.cpu_count() or 1)
    refbind.set_blas_threads(blas_threads)
    ref = _ref_net(layers)
    before = ref.get_params()
    ref.set_train_options(1.0, 0.0)
    ref.set_seq_lengths(batch.lens)
    net_out = ref.propagate(batch.feats)
    ctc = refbind.cuda_ctc_eval_parallel(net_out, batch.T, batch.S, batch.lens, batch.label_ids, batch.label_off)
    ne, nr = ref.error_rate_mseq(net_out, batch.T, batch.S, batch.lens, batch.label_ids, batch.label_off)
    in_diff = ref.backpropagate(ctc["diff"] if diff_override is None else np.ascontiguousarray(diff_override, np.float32), True,
                                lowmem=lowmem)
    grads = before.astype(np.float64) - ref.get_params().astype(np.float64)    # lr = 1, momentum = 0, no clipping
    return dict(net_out=net_out, pzx=ctc["pzx"], diff=ctc["diff"], in_diff=in_diff, grads=grads.astype(np.float32),
                errors=(ne, nr))


def reference_training_steps(layers, batch, lr: float, momentum: float, steps: int, blas_threads: int = 0, lowmem: bool = False):
    """`steps` trainer steps of the reference on the SAME minibatch with the given options (the layers carry <MaxGrad>):
    the parameter vectors after each step (Net::GetParams order), theta_0 first."""
    from oracle import refbind
    refbind.set_blas_threads(blas_threads if blas_threads > 0 else min(16, os.cpu_count() or 1))
    ref = _ref_net(layers)
    ref.set_train_options(lr, momentum)
    out = [ref.get_params()]
    for _ in range(steps):
        ref.set_seq_lengths(batch.lens)
        net_out = ref.propagate(batch.feats)
        ctc = refbind.cuda_ctc_eval_parallel(net_out, batch.T, batch.S, batch.lens, batch.label_ids, batch.label_off)
        ref.backpropagate(ctc["diff"], False, lowmem=lowmem)
        out.append(ref.get_params())
    return out


def tensor_bounds(layers):
    """[(begin, end)] of every parameter tensor in the Net::GetParams-ordered flat vector."""
    out, i = [], 0
    for L in layers:
        for p in L["params"]:
            out.append((i, i + p.size)); i += p.size
    return out


def tensor_stats(layers, flat) -> np.ndarray:
    """[n_tensors x 4]: max |g|, sum g, sum |g|, sum g^2 per parameter tensor, in Net::GetParams order."""
    out = []
    for a, b in tensor_bounds(layers):
        g = np.asarray(flat[a:b], np.float64)
        out.append([np.max(np.abs(g)), g.sum(), np.abs(g).sum(), np.square(g).sum()])
    assert b == len(flat)
    return np.array(out)


def sample_index(layers) -> np.ndarray:
    """Indices of the gradient sample: every STRIDE-th element, and every tensor of at most SMALL elements whole."""
    bounds = tensor_bounds(layers)
    m = np.zeros(bounds[-1][1], bool)
    m[::STRIDE] = True
    for a, b in bounds:
        if b - a <= SMALL:
            m[a:b] = True
    return np.flatnonzero(m)


def compact(layers, r: dict) -> dict:
    return dict(pzx=r["pzx"], grad_stats=tensor_stats(layers, r["grads"]), grad_sample=r["grads"][sample_index(layers)].copy(),
                net_out_rows=r["net_out"][::ROW_STRIDE].copy(), diff_rows=r["diff"][::ROW_STRIDE].copy(),
                in_diff_rows=r["in_diff"][::ROW_STRIDE].copy(), errors=np.array(r["errors"], np.int64),
                diff_absmax=np.array(np.max(np.abs(r["diff"]))), in_diff_absmax=np.array(np.max(np.abs(r["in_diff"]))))


def reference_floors(layers, batch, r: dict, lowmem: bool = False) -> dict:
    """What the reference's OWN fp32 CTC round-off does to the reference's results, measured by evaluating the CTC in fp64 on the
    reference's probabilities (oracle/eesen_oracle.c, f64 build) and backpropagating THAT through the reference: the distance
    of its fp32 `diff` to the fp64 one, and per gradient tensor (and for in_diff) the shift.  These are the floors below which
    no fp32 implementation with a different summation order can be expected to agree with the reference end to end; the
    fixture carries them -- as max-norm figures and as the SAMPLES of the fp64-CTC run, from which every other metric follows --
    so that the bars of the test are the same with and without the library on the box."""
    from oracle import net as onet
    from tests.util import rel_err, split_params
    arb = onet.ctc_eval_parallel(r["net_out"], batch.T, batch.S, batch.lens, batch.label_ids, batch.label_off, "f64")
    r64 = reference_step(layers, batch, diff_override=arb["diff"], lowmem=lowmem)
    fl = [rel_err(a, b) for (_, _, a), (_, _, b) in zip(split_params(layers, r["grads"]), split_params(layers, r64["grads"]))]
    return dict(floor_diff=np.array(rel_err(r["diff"], arb["diff"])), floor_grads=np.array(fl),
                floor_in_diff=np.array(rel_err(r["in_diff"], r64["in_diff"])), diff64_rows=arb["diff"][::ROW_STRIDE].astype(np.float32),
                in_diff64_rows=r64["in_diff"][::ROW_STRIDE].copy(), grad_sample64=r64["grads"][sample_index(layers)].copy(),
                grad_stats64=tensor_stats(layers, r64["grads"]))


# ------------------------------------------------------------------------------------------ the backward-only leg (no CTC)
# Both sides backpropagate the same FIXED top gradient `od`, regenerated bit for bit from integer hashing on every host, and the
# fixture carries the reference's answer to it.  The reference's own `diff` (13-47 MB per case) does not travel; this does.
# The new keys live in sidecar files beside the step's fixture, each within the 1 MiB committed-file limit, so that the arrays of
# full_<case>.npz stay byte for byte what the reference step wrote:
#   full_<case>_bwd.npz       od_sha256, bwd_grad_stats, bwd_grad_sample (sample_index), bwd_in_diff_seq_absmax [S]
#   full_<case>_bwd_rows.npz  bwd_in_diff_rows [n x D] and bwd_in_diff_row_index [n] (rows t*S+s of in_diff)
BWD_PARTS = ("_bwd", "_bwd_rows")
BWD_ROWS = 32                # in_diff rows per sequence (valid ones; t = 0 and t = len-1 among them) ...
BWD_ROWS_CFG3 = 16           # ... and for cfg3's 256 sequences
_M64 = (1 << 64) - 1


def _splitmix64(x: np.ndarray) -> np.ndarray:
    """splitmix64's output function on a uint64 array (wrapping arithmetic: exact on every host)."""
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _case_key(name: str) -> np.uint64:
    import hashlib
    return np.uint64(int.from_bytes(hashlib.sha256(name.encode()).digest()[:8], "little"))


def od_exponents(S: int) -> np.ndarray:
    """e_s = 8 ((s + s // 8) mod 4): every aligned group of four sequences holds all four powers 1, 2^-8, 2^-16, 2^-24 -- in the
    batch, in each 32-sequence window and in each shard of cfg3's interleaved deal (rank r holds s = r mod 8)."""
    s = np.arange(S)
    return 8 * ((s + s // 8) % 4)


def od_zero_sequences(S: int) -> np.ndarray:
    """Sequences whose top gradient is exactly zero (their in_diff must be exactly zero on both sides)."""
    return np.flatnonzero(np.arange(S) % 11 == 5)


def fixed_top_gradient(name: str, lens, T: int, S: int, K: int) -> np.ndarray:
    """[T*S x K] fp32, row t*S+s, shaped like a CTC gradient: every class n 2^-22 with |n| < 2^18 and one hashed class per row
    -2^-1 on top, the row scaled by 2^-e_s (od_exponents), zero on padding rows and on od_zero_sequences.  Integer hashing
    (splitmix64 over (case, row, class)) and power-of-two scalings only: every value is exact in fp32 and the same on every host."""
    key = _case_key(name)
    rows = np.arange(T * S, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = _splitmix64(key + rows[:, None] * np.uint64(K) + np.arange(K, dtype=np.uint64)[None, :])
        hot = _splitmix64(_splitmix64(key ^ np.uint64(0x5851F42D4C957F2D)) + rows) % np.uint64(K)
    n = (h >> np.uint64(46)).astype(np.int64)                      # 18 bits: 0 .. 2^18 - 1
    n = np.where((h & np.uint64(1)) == 1, -n, n)
    od = n.astype(np.float64) * 2.0 ** -22
    od[np.arange(T * S), hot.astype(np.int64)] -= 0.5
    s = np.arange(T * S) % S
    t = np.arange(T * S) // S
    od *= np.ldexp(1.0, -od_exponents(S))[s][:, None]
    od[(t >= np.asarray(lens)[s]) | np.isin(s, od_zero_sequences(S))] = 0.0
    out = od.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), od)             # exact in fp32
    return out


def od_sha256(od: np.ndarray) -> str:
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(od, "<f4").tobytes()).hexdigest()


def bwd_row_index(name: str, lens, T: int, S: int) -> np.ndarray:
    """Rows t*S+s of in_diff the fixture keeps: per sequence BWD_ROWS valid rows (BWD_ROWS_CFG3 for cfg3) -- t = 0, t = len-1 and
    evenly spaced ones between, their phase staggered across sequences -- plus its first and last padding row, if any."""
    n = BWD_ROWS_CFG3 if name == "full_cfg3" else BWD_ROWS
    out = []
    for s in range(S):
        L = int(lens[s])
        step = (L - 1) / n
        phase = ((s * 0.618034) % 1.0) * step
        ts = {0, L - 1} | {int(phase + k * step) for k in range(n)}
        if L < T:
            ts |= {L, T - 1}
        out += [t * S + s for t in sorted(ts)]
    return np.array(sorted(out), np.int64)


def bwd_compact(name: str, layers, lens, T: int, S: int, in_diff: np.ndarray, grads: np.ndarray) -> dict:
    """The backward leg's keys (both files) from a full in_diff [T*S x D] and gradient vector: what the fixture stores and what the
    test forms on the HIP side."""
    idx = bwd_row_index(name, lens, T, S)
    vm = (np.arange(T)[:, None] < np.asarray(lens)[None, :])
    a = np.abs(np.asarray(in_diff, np.float32)).reshape(T, S, -1).max(axis=2)
    return dict(bwd_grad_stats=tensor_stats(layers, grads), bwd_grad_sample=np.asarray(grads, np.float32)[sample_index(layers)].copy(),
                bwd_in_diff_seq_absmax=np.where(vm, a, 0.0).max(axis=0).astype(np.float32),
                bwd_in_diff_rows=np.asarray(in_diff, np.float32)[idx].copy(), bwd_in_diff_row_index=idx)


def load_fixture(name: str) -> dict:
    """full_<case>.npz with its backward-leg sidecars (where present) merged in: {key: array}."""
    out = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    for part in BWD_PARTS:
        p = os.path.join(GOLDEN, name + part + ".npz")
        if os.path.exists(p):
            out.update(np.load(p))
    return out


def reference_backward(layers, batch, od, blas_threads: int = 0, lowmem: bool = False) -> dict:
    """The reference's forward pass and then its backward pass on `od` (no CTC): in_diff and the gradient (delta, lr = 1)."""
    from oracle import refbind
    refbind.set_blas_threads(blas_threads if blas_threads > 0 else min(16, os.cpu_count() or 1))
    ref = _ref_net(layers)
    before = ref.get_params()
    ref.set_train_options(1.0, 0.0)
    ref.set_seq_lengths(batch.lens)
    ref.propagate(batch.feats)
    in_diff = ref.backpropagate(od, True, lowmem=lowmem)
    grads = before.astype(np.float64) - ref.get_params().astype(np.float64)
    return dict(in_diff=in_diff, grads=grads.astype(np.float32))


def backward_leg_main(names):
    """python -m oracle.fullsize --backward-leg [NAME ...]: the reference's answer to od, written to the sidecars."""
    from oracle import refbind
    assert refbind.build_if_possible(), "oracle/_ref could not be built (needs /root/reference)"
    import time
    for name in (names or list(CASES) + ["full_cfg3"]):
        cfg, layers, batch = case(name)
        od = fixed_top_gradient(name, batch.lens, batch.T, batch.S, cfg["K"])
        t0 = time.time()
        r = reference_backward(layers, batch, od, lowmem=name in LOWMEM)
        sec = time.time() - t0
        c = bwd_compact(name, layers, batch.lens, batch.T, batch.S, r["in_diff"], r["grads"])
        zero = od_zero_sequences(batch.S)
        assert not np.any(r["in_diff"].reshape(batch.T, batch.S, -1)[:, zero]), "zero od, nonzero in_diff"
        rows = {k: c.pop(k) for k in ("bwd_in_diff_rows", "bwd_in_diff_row_index")}
        np.savez_compressed(os.path.join(GOLDEN, name + "_bwd.npz"), od_sha256=np.array(od_sha256(od)), **c)
        np.savez_compressed(os.path.join(GOLDEN, name + "_bwd_rows.npz"), **rows)
        sizes = [os.path.getsize(os.path.join(GOLDEN, name + p + ".npz")) for p in BWD_PARTS]
        print(f"{name}: reference forward + backward on od {sec:.1f} s, {len(rows['bwd_in_diff_row_index'])} in_diff rows, "
              f"sidecars {sizes[0] / 1024:.0f} + {sizes[1] / 1024:.0f} KiB", flush=True)


def cfg3_training_layers(layers):
    """The same weights with the recipes' <MaxGrad> on every trainable layer."""
    out = []
    for L in layers:
        L = dict(L)
        if L["params"]:
            L["max_grad"] = CFG3_MAX_GRAD
        out.append(L)
    return out


def main():
    if "--backward-leg" in sys.argv[1:]:
        return backward_leg_main([a for a in sys.argv[1:] if a != "--backward-leg"])
    from oracle import refbind
    assert refbind.build_if_possible(), "oracle/_ref could not be built (needs /root/reference)"
    import time
    for name in (sys.argv[1:] or list(CASES) + ["full_cfg3"]):
        cfg, layers, batch = case(name)
        low = name in LOWMEM
        t0 = time.time()
        r = reference_step(layers, batch, lowmem=low)
        c = compact(layers, r)
        t1 = time.time()
        c.update(reference_floors(layers, batch, r, lowmem=low))
        t_floor = time.time() - t1
        extra = ""
        if name == "full_cfg3":     # two steps with momentum + <MaxGrad> on the summed gradient of the 256 utterances
            t2 = time.time()
            th = reference_training_steps(cfg3_training_layers(layers), batch, CFG3_LR, CFG3_MOMENTUM, CFG3_STEPS, lowmem=low)
            idx = sample_index(layers)
            for k in range(1, len(th)):
                d = th[k - 1].astype(np.float64) - th[k].astype(np.float64)
                c[f"delta{k}_sample"] = d[idx].astype(np.float32)
                c[f"delta{k}_stats"] = tensor_stats(layers, d)
            c["train_opts"] = np.array([CFG3_LR, CFG3_MOMENTUM, CFG3_MAX_GRAD, CFG3_STEPS])
            extra = f", {CFG3_STEPS} training steps {time.time() - t2:.1f} s"
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), **c)
        print(f"{name}: reference step {t1 - t0:.1f} s (+ {t_floor:.1f} s for the fp64-CTC floors{extra}), sum ln p = "
              f"{r['pzx'].astype(np.float64).sum():.4f}, errors {r['errors']}, floors: diff {float(c['floor_diff']):.2e}, "
              f"gradient tensors up to {float(c['floor_grads'].max()):.2e}", flush=True)


if __name__ == "__main__":
    main()
