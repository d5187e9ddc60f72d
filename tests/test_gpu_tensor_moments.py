"""-m gpu: tensor_moments_kernel (csrc/optim.hip) -- every figure of Net::Info / Net::InfoGradient -- against the fp64 restatement of
MomentStatistics in tests/update_restatement.py, applied to the FILE-order tensors (tests/util.py::split_params).

min and max are exact.  mean, variance, skewness and kurtosis are held within the bound the restatement derives for an fp64 reduction in
another order (n 2^-52 times the sum of the absolute values of the terms, through the normalisers); no fixed relative number anywhere --
the terms of the skewness cancel.  What the cases are for: the (nb, hf, hi) column map and the ld != cols regions that must skip the zero
pads of a padded layer (strictly positive parameters: a pad counted as an entry shows as min = 0); many passes of the 1024-thread loop;
the two-pass form on a large offset; the which = 0 / 1 / 2 buffer selection; tensor order and count per layer kind; a constant tensor.

A constant tensor has variance exactly 0, so skewness and kurtosis are 0 / 0: the kernel returns NaN and the test asserts NaN.  (The
reference's fp32 host evaluation prints round-off garbage there; matching that is not a goal.)"""
import ctypes as C
import re

import numpy as np
import pytest

from tests import update_cases as UC
from tests import update_restatement as R
from tests.util import split_params

pytestmark = pytest.mark.gpu


def hold(net, which, layers, flat, what):
    """TensorMoments(which, every layer) against the restatement of every file-order tensor of `flat`."""
    want = split_params(layers, np.asarray(flat, np.float32))
    k = 0
    for li in range(len(layers)):
        got = net.TensorMoments(which, li)
        assert got.shape == ({"BiLstmParallel": 12, "LstmParallel": 6, "AffineTransform": 2}.get(layers[li]["type"], 0), 6)
        for row in got:
            lj, name, t = want[k]; k += 1
            assert lj == li
            val, bnd = R.moments(t)
            assert row[0] == val[0] and row[1] == val[1], f"{what}: layer {li} {name}: min / max {row[:2]} != {val[:2]}"
            assert np.isfinite(val).all() and np.isfinite(bnd).all()
            for i, fig in ((2, "mean"), (3, "variance"), (4, "skewness"), (5, "kurtosis")):
                assert abs(row[i] - val[i]) <= bnd[i], f"{what}: layer {li} {name}: {fig} {row[i]!r} != {val[i]!r} +- {bnd[i]:.3g}"
    assert k == len(want)


def wide_range(layers, seed):
    n = sum(UC.layer_sizes(layers))
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * np.exp(rng.uniform(-6.0, 6.0, n))).astype(np.float32)


def test_padded_layers_count_the_files_entries_only(gpu):
    from eesen_amd.api import Net
    layers = UC.make_net("padded")
    net = Net.from_layers(layers)
    n = sum(UC.layer_sizes(layers))
    p = np.random.default_rng(1).uniform(0.5, 1.5, n).astype(np.float32)
    net.SetParams(p)
    assert UC.GradInjector(net).pads > 0
    hold(net, 0, layers, p, "padded, positive parameters")
    assert min(net.TensorMoments(0, li)[:, 0].min() for li in range(3)) >= 0.5


@pytest.mark.parametrize("name", ["layers3", "one_wide"])
def test_wide_dynamic_range(gpu, name):
    from eesen_amd.api import Net
    layers = UC.make_net(name)
    net = Net.from_layers(layers)
    p = wide_range(layers, 2)
    net.SetParams(p)
    hold(net, 0, layers, p, name)


def test_large_offset_small_spread(gpu):
    """mean 1000, spread 1e-3 (in fp32: a handful of distinct values): a one-pass sum of squares would lose the variance."""
    from eesen_amd.api import Net
    layers = UC.make_net("layers3")
    net = Net.from_layers(layers)
    n = sum(UC.layer_sizes(layers))
    p = (np.float32(1000.0) + np.float32(1e-3) * np.random.default_rng(3).standard_normal(n).astype(np.float32)).astype(np.float32)
    net.SetParams(p)
    hold(net, 0, layers, p, "offset 1000")
    assert all(1e-8 < v < 1e-5 for li in range(3) for v in net.TensorMoments(0, li)[:, 3])


@pytest.mark.parametrize("name", ["layers3", "padded"])
def test_momentum_buffers_and_accumulators(gpu, name):
    """which = 1 after one SGD step with injected gradients: the statistics of clip(g0) per tensor; which = 2 after SetAccumulators;
    which = 0 meanwhile still the parameters."""
    from eesen_amd.api import Net
    inp = UC.two_step_inputs(name)
    layers = inp["layers"]
    net = Net.from_layers(layers)
    net.SetTrainOptions(UC.HYPER["lr"], 0.0)
    inj = UC.GradInjector(net)
    inj.put(inp["g"][0])
    net.Update()
    hold(net, 1, layers, UC.clip_exact(layers, inp["g"][0]), f"{name} corr")
    a = UC.accumulators(layers, 7)
    a[::7] = 1e-12                                   # (the pads are the only zeros: an accumulator near eps, none AT zero)
    net.SetAccumulators(a)
    hold(net, 2, layers, a, f"{name} accu")
    hold(net, 0, layers, net.GetParams(), f"{name} params")


def test_order_and_count_per_layer_kind(gpu):
    """12 tensors for a BiLstm layer, 6 for an Lstm layer, 2 for an affine one, none for the rest; in the file's order -- each tensor gets
    its own constant, so its row must read that constant."""
    from eesen_amd.api import Net
    rng = np.random.default_rng(4)
    z = lambda *sh: np.zeros(sh, np.float32)
    lstm = dict(type="LstmParallel", input_dim=14, output_dim=6, learn_rate_coef=1.0, max_grad=0.0, params=[z(24, 14), z(24, 6), z(24), z(6), z(6), z(6)])
    bi = UC.make_net("padded")[0]
    bi = dict(bi, input_dim=5, output_dim=14, params=[z(28, 5), z(28, 7), z(28), z(7), z(7), z(7)] * 2)
    layers = [bi, lstm, dict(type="AffineTransform", input_dim=6, output_dim=3, learn_rate_coef=1.0, max_grad=0.0, params=[z(3, 6), z(3)]),
              dict(type="Softmax", input_dim=3, output_dim=3, params=[])]
    k = 0
    for L in layers:
        for i in range(len(L["params"])):
            k += 1
            L["params"][i] = np.full_like(L["params"][i], 0.25 * k)
    net = Net.from_layers(layers)
    counts = [net.TensorMoments(0, li).shape[0] for li in range(4)]
    assert counts == [12, 6, 2, 0]
    k = 0
    for li in range(3):
        for row in net.TensorMoments(0, li):
            k += 1
            assert row[0] == row[1] == row[2] == 0.25 * k and row[3] == 0.0, (li, k, row)


def test_constant_tensors(gpu):
    """The all-zero momentum buffers of a fresh Net, and parameters set to one value (0.25: every partial sum is exact, so the mean is the
    value and every deviation 0): min = max = mean = value, variance = 0, skewness and kurtosis 0 / 0 = NaN."""
    from eesen_amd.api import Net
    layers = UC.make_net("padded")
    net = Net.from_layers(layers)
    n = sum(UC.layer_sizes(layers))
    net.SetParams(np.full(n, 0.25, np.float32))
    for which, value in ((1, 0.0), (0, 0.25)):
        for li in range(3):
            m = net.TensorMoments(which, li)
            want = np.tile(np.array([value, value, value, 0.0, np.nan, np.nan]), (m.shape[0], 1))
            assert np.array_equal(m, want, equal_nan=True), (which, li, m)


def test_error_paths(gpu):
    from eesen_amd import _lib
    from eesen_amd.api import Net, EesenError
    net = Net.from_layers(UC.make_net("layers3"))
    lib = _lib.load()
    buf = np.zeros((12, 6), np.float64)
    n = C.c_int()
    ptr = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.eesen_net_tensor_moments(net.h, 0, 0, ptr, 11, C.byref(n)) != 0 and b"too small" in lib.eesen_last_error()
    assert not buf.any()
    with pytest.raises(EesenError, match="out of range"):
        net.TensorMoments(0, 3)
    with pytest.raises(EesenError, match="out of range"):
        net.TensorMoments(0, -1)
    with pytest.raises(EesenError, match="which"):
        net.TensorMoments(3, 0)
    assert net.TensorMoments(0, 0).shape == (12, 6)          # ... and the handle still works


_FIGS = re.compile(r"\( min (\S+), max (\S+), mean (\S+), variance (\S+), skewness (\S+), kurtosis (\S+) \)")


def test_info_strings_on_a_padded_net(gpu):
    """Net.Info() / Net.InfoGradient(): every printed figure is f"{x:g}" of the restated value; number-of-parameters counts the FILE's."""
    from eesen_amd.api import Net
    inp = UC.two_step_inputs("padded")
    layers = inp["layers"]
    net = Net.from_layers(layers)
    p = wide_range(layers, 6)
    net.SetParams(p)
    net.SetTrainOptions(UC.HYPER["lr"], 0.0)
    inj = UC.GradInjector(net)
    inj.put(inp["g"][0])
    net.Update()
    n = sum(UC.layer_sizes(layers))
    info = net.Info()
    assert info.startswith(f"num-layers 3\ninput-dim 5\noutput-dim 7\nnumber-of-parameters {n / 1e6:g} millions\nlayer 1 : <BiLstmParallel>, input-dim 5, output-dim 12, ")
    grad = net.InfoGradient()
    assert grad.startswith("### Gradient stats :\nLayer 1 : <BiLstmParallel>, ")
    for text, flat, suffix in ((info, net.GetParams(), ""), (grad, UC.clip_exact(layers, inp["g"][0]), "corr_")):
        want = split_params(layers, flat)
        got = _FIGS.findall(text)
        assert len(got) == len(want) == 26
        for figs, (li, name, t) in zip(got, want):
            val, _ = R.moments(t)
            assert list(figs) == [f"{x:g}" for x in val], (li, name, figs, val)
        names = re.findall(r"^  (\w+)", text, flags=re.M)
        lstm = [f"{t}{d}{suffix}" for d in ("_fw_", "_bw_") for t in ("wei_gifo_x", "wei_gifo_m", "bias", "phole_i_c", "phole_f_c", "phole_o_c")]
        assert names == lstm + lstm + (["linearity", "bias"] if not suffix else ["linearity_corr_", "bias_corr_"])
