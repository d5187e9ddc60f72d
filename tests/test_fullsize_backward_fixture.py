"""CPU: the backward-only leg of the full-size parity tests (tests/test_gpu_reference_fullsize.py).  Both sides backpropagate the
fixed top gradient oracle/fullsize.py::fixed_top_gradient; tests/golden/full_<case>_bwd*.npz hold the reference's answer to it
(`python -m oracle.fullsize --backward-leg`).  Here: the generator reproduces the very od the reference answered, it has the
properties the GPU leg relies on, and the fixtures are complete and consistent -- zero-od sequences and padding exactly zero."""
import numpy as np
import pytest

from eesen_amd import parallel, synth
from oracle import fullsize

NAMES = list(fullsize.CASES) + ["full_cfg3"]


def _shape(name):
    cfg_name, over = fullsize.CFG3 if name == "full_cfg3" else fullsize.CASES[name]
    cfg = synth.config(cfg_name)
    cfg.update(over)
    return cfg, synth.make_batch(**cfg)


def test_fixed_top_gradient_is_shaped_like_a_ctc_gradient():
    T, S, K = 40, 24, 13
    lens = np.sort(np.random.default_rng(3).integers(20, T + 1, S)).astype(np.int32)
    od = fullsize.fixed_top_gradient("probe", lens, T, S, K)
    assert od.dtype == np.float32 and od.shape == (T * S, K)
    assert np.array_equal(od, fullsize.fixed_top_gradient("probe", lens, T, S, K))
    assert not np.array_equal(od, fullsize.fixed_top_gradient("probe2", lens, T, S, K))
    o = od.reshape(T, S, K).astype(np.float64)
    e = fullsize.od_exponents(S)
    zero = fullsize.od_zero_sequences(S)
    assert zero.tolist() == [5, 16]
    for s in range(S):
        v = o[: lens[s], s] * 2.0 ** e[s]               # back to the unscaled values
        if s in zero:
            assert not np.any(o[:, s])
            continue
        assert not np.any(o[lens[s]:, s])               # padding
        hot = v < -0.25                                  # one class per row carries -2^-1
        assert np.all(hot.sum(axis=1) == 1)
        n = np.where(hot, v + 0.5, v) * 2.0 ** 22        # the rest: n 2^-22, |n| < 2^18
        assert np.array_equal(n, np.round(n)) and np.max(np.abs(n)) < 2 ** 18 and np.max(np.abs(n)) > 2 ** 16
    # every aligned group of four sequences holds all four powers: in the batch, in each 32-sequence window, in cfg3's shards
    assert all(sorted(e[g:g + 4]) == [0, 8, 16, 24] for g in range(0, S - 3, 4))
    e256 = fullsize.od_exponents(256)
    for r in range(fullsize.CFG3_WORLD):
        es = e256[parallel.deal_shards(256, fullsize.CFG3_WORLD)[r]]
        assert all(sorted(es[g:g + 4]) == [0, 8, 16, 24] for g in range(0, len(es), 4)), r


@pytest.mark.parametrize("name", NAMES)
def test_backward_leg_fixture_is_complete_and_consistent(name):
    cfg, batch = _shape(name)
    T, S, K, D = batch.T, batch.S, cfg["K"], cfg["D"]
    fx = fullsize.load_fixture(name)
    od = fullsize.fixed_top_gradient(name, batch.lens, T, S, K)
    assert fullsize.od_sha256(od) == str(fx["od_sha256"]), "the generator no longer reproduces the od the reference answered"
    # the gradient: the step fixture's sample positions and tensors, all finite
    assert fx["bwd_grad_stats"].shape == fx["grad_stats"].shape
    assert fx["bwd_grad_sample"].shape == fx["grad_sample"].shape and fx["bwd_grad_sample"].dtype == np.float32
    assert np.all(np.isfinite(fx["bwd_grad_stats"])) and np.all(np.isfinite(fx["bwd_grad_sample"]))
    assert np.all(fx["bwd_grad_stats"][:, 0] > 0)
    # in_diff rows: the documented index, per sequence enough valid rows with t = 0 and t = len - 1, and its padding
    idx, rows, amax = fx["bwd_in_diff_row_index"], fx["bwd_in_diff_rows"], fx["bwd_in_diff_seq_absmax"]
    assert np.array_equal(idx, fullsize.bwd_row_index(name, batch.lens, T, S))
    assert rows.shape == (len(idx), D) and rows.dtype == np.float32 and amax.shape == (S,)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < T * S
    seq, t = idx % S, idx // S
    valid = t < batch.lens[seq]
    n_min = fullsize.BWD_ROWS_CFG3 if name == "full_cfg3" else fullsize.BWD_ROWS
    for s in range(S):
        ts = t[(seq == s) & valid]
        assert len(ts) >= n_min and ts[0] == 0 and ts[-1] == batch.lens[s] - 1, s
        if batch.lens[s] < T:
            assert np.any((seq == s) & ~valid), s
    assert np.all(np.isfinite(rows))
    assert not np.any(rows[~valid]), "padding rows of the reference's in_diff are not zero"
    zero = fullsize.od_zero_sequences(S)
    assert len(zero) and not np.any(rows[np.isin(seq, zero)]) and not np.any(amax[zero])
    for s in sorted(set(range(S)) - set(zero.tolist())):
        r = np.abs(rows[(seq == s) & valid])
        assert 0 < r.max() <= amax[s], s
