"""-m gpu: the layers between the recurrences -- AffineTransform (three GEMMs and a column sum per step, under all three GEMM modes, with
the operand bounds Net itself chooses in csrc/net.cpp), <Sigmoid>, <Tanh>, <Softmax> and the row kernels beside them -- held ELEMENT BY
ELEMENT against the fp64 restatement of tests/layer_restatement.py within the rounding bound it derives for each element.  No element
is excluded anywhere, padded rows included.

Everything goes through the public objects: a [Softmax], [Tanh] or [AffineTransform] net hands its kernel the caller's matrix.  Nets and
inputs: tests/layer_cases.py, shared with tests/test_layer_restatement.py, which shows on the CPU that an fp32 evaluation (an emulation
of the plane arithmetic for modes 1 and 2) stays inside these bounds and that every listed mutation -- a per-tensor word where a
per-index vector is due, rows for columns, a stale measurement, a dropped product, a missing bias, a stride that stops at 2^20 -- leaves
them.  The bounds are derived, not measured; the only measured figures are the worst error / bound ratios per (layer, quantity, mode),
written to layers_fp64.json in $EESEN_PARITY_OUT (when set; committed from an MI355X run as profiles/layers_fp64.json) and asserted < 1."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import layer_cases as LC
from tests import layer_restatement as R
from tests.util import split_params

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(12345.0)


@pytest.fixture(scope="module")
def record():
    worst = {}

    def note(layer, quantity, mode, ratio):
        assert ratio < 1.0, f"{layer} {quantity} mode {mode}: worst error / bound {ratio:.3g}"
        q = worst.setdefault(layer, {}).setdefault(quantity, {})
        q[str(mode)] = max(q.get(str(mode), 0.0), float(ratio))

    yield note
    out_dir = os.environ.get("EESEN_PARITY_OUT")
    if not out_dir:
        return
    try:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "layers_fp64.json"), "w") as f:
            json.dump(dict(what="worst |HIP - fp64 restatement| / derived bound, per layer (net), quantity and GEMM mode (-: no GEMM)", worst=worst), f, indent=1)
    except OSError:
        pass


def _filled(rows, cols):
    """A device matrix whose every float, pad columns included, holds the sentinel."""
    from eesen_amd import _lib
    from eesen_amd.api import CuMatrix, _np_ptr
    m = CuMatrix(rows, cols, zero=False)
    buf = np.full(rows * m.stride, SENTINEL, np.float32)
    _lib.check(_lib.load().eesen_dev_copy(0, C.c_void_p(m.ptr), _np_ptr(buf), buf.nbytes, 1))
    return m


def _with_pads(m):
    from eesen_amd import _lib
    from eesen_amd.api import _np_ptr
    buf = np.empty((m.rows, m.stride), np.float32)
    _lib.check(_lib.load().eesen_dev_copy(0, _np_ptr(buf), C.c_void_p(m.ptr), buf.nbytes, 2))
    return buf


def run(layers, lens, x, d):
    """Propagate(x), BackpropagateNoUpdate(d, in_diff) on a fresh Net: (out, in_diff, grads in file order).  in_diff is pre-filled with a
    sentinel: its pad columns must keep it, and nothing unwritten passes for a result."""
    from eesen_amd.api import CuMatrix, Net
    net = Net.from_layers(layers)
    net.SetSeqLengths(lens)
    out = net.Propagate(x).numpy()
    assert out.shape == (x.shape[0], layers[-1]["output_dim"])
    in_diff = _filled(x.shape[0], layers[0]["input_dim"])
    net.BackpropagateNoUpdate(CuMatrix.from_numpy(d), in_diff)
    net.Synchronize()
    full = _with_pads(in_diff)
    cols = layers[0]["input_dim"]
    assert np.all(full[:, cols:].view(np.uint32) == SENTINEL.view(np.uint32)), "in_diff: a pad column was written"
    grads = net.GetGrads() if net.NumParams() else np.zeros(0, np.float32)
    return out, np.ascontiguousarray(full[:, :cols]), grads


def hold(got, want, bound, what):
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.float32, what
    r = LC.worst_ratio(got, want, bound)
    if not r < 1.0:
        i = np.unravel_index(int(np.argmax(np.abs(got.astype(np.float64) - want) - bound)), got.shape)
        raise AssertionError(f"{what}: worst error / bound {r:.3g} at {i}: got {got[i]!r}, want {want[i]!r} +- {bound[i]:.3g}")
    return r


# ------------------------------------------------------------------------------------------------------------ AffineTransform
@pytest.mark.parametrize("mode", LC.MODES)
@pytest.mark.parametrize("name", list(LC.AFFINE))
def test_affine_layer_holds_every_element(gpu, record, name, mode):
    case = LC.affine_case(name)
    layers, front = case["layers"], case["front"]
    try:
        assert gpu.eesen_set_gemm_mode(mode) == 0
        y_front = None
        if front:   # the Affine layer's input, bit for bit: the same kernel on the same matrix gives the same bits
            y_front = run(layers[:1], case["lens"], case["x"], np.zeros_like(case["x"]))[0]
            assert np.array_equal(y_front.view(np.uint32), run(layers[:1], case["lens"], case["x"], np.zeros_like(case["x"]))[0].view(np.uint32))
            assert np.abs(y_front[:, case["tiny"]]).max() <= 2.0 ** -20 and np.abs(y_front).max() <= 1.0
        out, in_diff, grads = run(layers, case["lens"], case["x"], case["d"])
    finally:
        gpu.eesen_set_gemm_mode(-1)
    xa = LC.affine_input(case, y_front)
    want = LC.affine_restated(case, mode, xa)
    if front:       # [activation, Affine]: the net's in_diff is the Affine layer's, times f'(y) in place (activation_diff_kernel)
        fd = R.tanh_diff if front == "Tanh" else R.sigmoid_diff
        g, g_b = want["in_diff"]
        y64 = xa.astype(np.float64)
        slope = (1.0 - y64 * y64) if front == "Tanh" else y64 * (1.0 - y64)
        want["in_diff"] = (fd(g, xa)[0], g_b * np.abs(slope) + fd(np.abs(g) + g_b, xa)[1])
    (_, _, gw), (_, _, gb) = split_params(layers, grads)
    got = dict(out=out, in_diff=in_diff, W_grad=gw.reshape(case["W"].shape), b_grad=gb)
    layer = f"{front + '+' if front else ''}AffineTransform[{name}]"
    for q in ("out", "in_diff", "W_grad", "b_grad"):
        record(layer, q, mode, hold(got[q], *want[q], f"{name} mode {mode} {q}"))
    # exact zeros where an operand row / column is zero
    if not front:
        assert np.all(got["W_grad"][:, case["x"].shape[1] // 2] == 0)
    assert np.all(in_diff[case["x"].shape[0] // 2] == 0)


# ------------------------------------------------------------------------------------------------------------ <Tanh>, <Sigmoid>
@pytest.mark.parametrize("kind", ["Tanh", "Sigmoid"])
@pytest.mark.parametrize("name", list(LC.ACTIVATION))
def test_activation_layer_holds_every_element(gpu, record, name, kind):
    case = LC.activation_case(name)
    x, d = case["x"], case["d"]
    out, in_diff, grads = run([LC.layer_plain(kind, case["width"])], case["lens"], x, d)
    assert grads.size == 0
    f, fd = (R.tanh, R.tanh_diff) if kind == "Tanh" else (R.sigmoid, R.sigmoid_diff)
    record(kind, "out", "-", hold(out, *f(x), f"{kind} {name} out"))
    record(kind, "in_diff", "-", hold(in_diff, *fd(d, out), f"{kind} {name} in_diff"))      # from the y the device returned
    # the saturation branches, exactly
    if kind == "Tanh":
        assert np.all(out[x >= 44.4] == 1) and np.all(out[x <= -44.4] == -1) and (x >= 44.4).sum() > 10
    else:
        assert np.all(out[x <= -88.8] == 0) and np.all(out[x >= 60] == 1) and (x <= -88.8).sum() > 10
        assert np.all(out[x == np.float32(-88.7)] > 0)


# ------------------------------------------------------------------------------------------------------------ <Softmax>
@pytest.mark.parametrize("rows", list(LC.SOFTMAX_ROWS))
@pytest.mark.parametrize("K", LC.SOFTMAX_K)
def test_softmax_layer_holds_every_element(gpu, record, K, rows):
    case = LC.softmax_case(K, rows)
    out, in_diff, grads = run([LC.layer_plain("Softmax", K)], case["lens"], case["x"], case["d"])
    assert grads.size == 0
    record("Softmax", "out", "-", hold(out, *R.softmax(case["x"]), f"softmax K {K} rows {rows}"))
    assert np.array_equal(in_diff.view(np.uint32), case["d"].view(np.uint32))          # backward is the identity (softmax-layer.h:49-57)
    assert np.all(np.abs(out.sum(1, dtype=np.float64) - 1.0) <= K * 2.0 ** -24)
    if K == 1:
        assert np.all(out == 1.0)


# ------------------------------------------------------------------------------------------------------------ log, minus scaled log-priors
@pytest.mark.parametrize("priors", [False, True])
@pytest.mark.parametrize("apply_log", [0, 1])
def test_log_sub_prior_holds_every_element(gpu, record, apply_log, priors):
    """eesen_op_log_sub_prior at 1100 x 1001 (ld 1004): 1,101,100 elements, so log_sub_prior_kernel's grid (4096 x 256 threads) strides
    into its second pass.  Posteriors over 35 decades, some exactly 1; logf within ULP_EXP ulps, the product and the sum one rounding each;
    neither log nor priors: the matrix comes back bit for bit.  Pad columns keep their sentinel."""
    from eesen_amd import _lib
    from eesen_amd.api import _np_ptr
    rows, K = 1100, 1001
    rng = np.random.default_rng(17 + apply_log)
    post = np.exp(rng.uniform(-80.0, 0.0, (rows, K))).astype(np.float32)
    post[rng.random((rows, K)) < 0.01] = 1.0
    m = post if apply_log else np.log(post.astype(np.float64)).astype(np.float32)
    log_pri = np.log(rng.dirichlet(np.full(K, 0.3)) + 1e-30).astype(np.float32) if priors else None
    dev = _filled(rows, K)
    assert dev.stride == 1004
    buf = _with_pads(dev)
    buf[:, :K] = m
    _lib.check(_lib.load().eesen_dev_copy(0, C.c_void_p(dev.ptr), _np_ptr(buf), buf.nbytes, 1))
    _lib.check(gpu.eesen_op_log_sub_prior(0, None, C.c_void_p(dev.ptr), rows, K, dev.stride, apply_log,
                                          log_pri.ctypes.data_as(C.c_void_p) if priors else None, 0.8))
    got = _with_pads(dev)
    assert np.all(got[:, K:].view(np.uint32) == SENTINEL.view(np.uint32))
    want, bound = R.log_sub_prior(m, apply_log, log_pri, 0.8)
    record("log_sub_prior", f"log {apply_log} priors {int(priors)}", "-", hold(np.ascontiguousarray(got[:, :K]), want, bound, "log_sub_prior"))
    if not apply_log and not priors:
        assert np.array_equal(got[:, :K].view(np.uint32), m.view(np.uint32))
