"""CPU: what tests/test_gpu_layers.py holds the Affine, activation and Softmax layers against.
  (a) the fp64 restatement (tests/layer_restatement.py) equals OracleNet(layers, "f64") on every case of tests/layer_cases.py -- output,
      in_diff and gradients -- to 1e-12 (of sum |a||b| for a GEMM result, of max(1, |value|) otherwise);
  (b) a numpy fp32 evaluation -- for the plane modes an emulation of gemm.hip's arithmetic with the scales the design prescribes -- stays
      inside every DERIVED bound; the worst ratio per quantity is printed;
  (c) every listed mutation leaves the bounds on the same inputs; the factor is printed (inf: an fp16 plane overflowed).
The bounds come from counting roundings (module docstring of the restatement); nothing in them was fitted to an observed error."""
import numpy as np
import pytest

from tests import layer_cases as LC
from tests import layer_restatement as R


def _scales(case, xa, mutation=None):
    """The six half_scale vectors of the Affine layer's three GEMMs as net.cpp prescribes them -- or, mutated, as a wrong net.cpp would."""
    W, d = case["W"], case["d"]
    bounded = case["front"] is not None
    hs, am = R.half_scale, R.amax
    xm = xa
    if mutation == "stale_bound":            # Propagate's measurements of ANOTHER input (the previous minibatch)
        xm = np.ascontiguousarray(xa[::-1, ::-1])
    s = dict(fwd_a=hs(1.0) if bounded else hs(am(xm, 1)), fwd_b=hs(am(W, 1)), in_a=hs(am(d, 1)), in_b=hs(am(W, 0)),
             wg_a=hs(am(d, 0)), wg_b=hs(1.0) if bounded else hs(am(xm, 0)))
    if mutation == "per_tensor_word":
        s = dict(fwd_a=s["fwd_a"] if bounded else hs(am(xa, None)), fwd_b=hs(am(W, None)), in_a=hs(am(d, None)), in_b=hs(am(W, None)),
                 wg_a=hs(am(d, None)), wg_b=s["wg_b"] if bounded else hs(am(xa, None)))
    if mutation == "wrong_axis":             # rows where columns are due and the reverse, read at the index the kernel would use
        rows, din, dout = xa.shape[0], xa.shape[1], W.shape[0]
        take = lambda v, n: np.resize(v, n)
        s = dict(fwd_a=s["fwd_a"] if bounded else take(hs(am(xa, 0)), rows), fwd_b=take(hs(am(W, 0)), dout), in_a=take(hs(am(d, 0)), rows),
                 in_b=take(hs(am(W, 1)), din), wg_a=take(hs(am(d, 1)), dout), wg_b=s["wg_b"] if bounded else take(hs(am(xa, 1)), din))
    return s


def affine_fp32(case, mode, xa, mutation=None):
    s = _scales(case, xa, mutation if mutation in ("stale_bound", "per_tensor_word", "wrong_axis") else None)
    W, d, b = case["W"], case["d"], case["b"]
    m = mutation if mutation in ("drop_hi_lo", "drop_lo_planes", "no_bias") else None
    return dict(out=R.gemm_fp32(xa, W, mode, s["fwd_a"], s["fwd_b"], b, m), in_diff=R.gemm_fp32(d, W.T, mode, s["in_a"], s["in_b"], None, m),
                W_grad=R.gemm_fp32(d.T, xa.T, mode, s["wg_a"], s["wg_b"], None, m), b_grad=d.sum(0, dtype=np.float32))


def _close(got, want, scale, what):
    err = np.abs(np.asarray(got, np.float64) - want)
    assert np.all(err <= 1e-12 * scale), (what, float(np.max(err / scale)))


def _oracle(layers, lens, x, d):
    from oracle import net as onet
    ora = onet.OracleNet(layers, "f64")
    ora.set_seq_lengths(lens)
    out = ora.propagate(x)
    in_diff = ora.backpropagate(d, update=False)
    return ora, out, in_diff


# ------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("name", list(LC.AFFINE))
def test_affine_restatement_equals_the_f64_oracle(name):
    case = LC.affine_case(name)
    ora, out, in_diff = _oracle(case["layers"], case["lens"], case["x"], case["d"])
    x64 = case["x"].astype(np.float64)
    if case["front"]:
        xa = ora.acts[1]                     # the oracle's own activation output: the Affine layer restated from the same input
        _close((R.tanh if case["front"] == "Tanh" else R.sigmoid)(x64)[0], xa, 1.0, "front")
    else:
        xa = x64
    W, b, d = (case[k].astype(np.float64) for k in ("W", "b", "d"))
    mag = lambda a, bb: np.abs(a) @ np.abs(bb).T
    _close(R.affine_forward(xa, W, b, 0)[0], out, mag(xa, W) + np.abs(b), "out")
    g = R.affine_in_diff(d, W, 0)[0]
    if case["front"]:
        g = (R.tanh_diff if case["front"] == "Tanh" else R.sigmoid_diff)(g, xa)[0]
    _close(g, in_diff, mag(d, W.T), "in_diff")
    gw, _, gb, _ = R.affine_grads(d, xa, 0)
    fresh = ora.fresh_grads_flat()
    _close(gw.ravel(), fresh[:gw.size], mag(d.T, xa.T).ravel(), "W_grad")
    _close(gb, fresh[gw.size:], np.abs(d).sum(0), "b_grad")


@pytest.mark.parametrize("kind", ["Tanh", "Sigmoid"])
@pytest.mark.parametrize("name", list(LC.ACTIVATION))
def test_activation_restatement_equals_the_f64_oracle(name, kind):
    case = LC.activation_case(name)
    _, out, in_diff = _oracle([LC.layer_plain(kind, case["width"])], case["lens"], case["x"], case["d"])
    f, fd = (R.tanh, R.tanh_diff) if kind == "Tanh" else (R.sigmoid, R.sigmoid_diff)
    _close(f(case["x"])[0], out, 1.0, "out")
    _close(fd(case["d"], out)[0], in_diff, np.maximum(1.0, np.abs(in_diff)), "in_diff")


@pytest.mark.parametrize("K", LC.SOFTMAX_K)
def test_softmax_restatement_equals_the_f64_oracle(K):
    for rows in LC.SOFTMAX_ROWS:
        case = LC.softmax_case(K, rows)
        _, out, in_diff = _oracle([LC.layer_plain("Softmax", K)], case["lens"], case["x"], case["d"])
        _close(R.softmax(case["x"])[0], out, 1.0, "out")
        assert np.array_equal(in_diff, case["d"].astype(np.float64))


# ------------------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("mode", LC.MODES)
@pytest.mark.parametrize("name", list(LC.AFFINE))
def test_an_fp32_evaluation_of_the_affine_layer_stays_inside_the_bounds(name, mode):
    case = LC.affine_case(name)
    xa = LC.affine_input(case)
    want = LC.affine_restated(case, mode, xa)
    got = affine_fp32(case, mode, xa)
    worst = {q: LC.worst_ratio(got[q], *want[q]) for q in want}
    print(f"fp32 numpy / bound, {name} mode {mode}: " + ", ".join(f"{q} {v:.3f}" for q, v in worst.items()))
    assert all(v < 1.0 for v in worst.values()), worst
    if case["front"]:                        # the columns the per-tensor word costs precision by design: tiny, and still held
        assert np.abs(xa[:, case["tiny"]]).max() <= 2.0 ** -20


@pytest.mark.parametrize("name", list(LC.ACTIVATION))
def test_an_fp32_evaluation_of_the_activations_stays_inside_the_bounds(name):
    case = LC.activation_case(name)
    x, d = case["x"], case["d"]
    worst = {}
    for kind, f32, f, fd in (("Tanh", R.tanh_fp32, R.tanh, R.tanh_diff), ("Sigmoid", R.sigmoid_fp32, R.sigmoid, R.sigmoid_diff)):
        y = f32(x)
        worst[kind] = LC.worst_ratio(y, *f(x))
        g = d * (np.float32(1) - y * y) if kind == "Tanh" else d * (y * (np.float32(1) - y))
        worst[kind + "_diff"] = LC.worst_ratio(g, *fd(d, y))
    # the saturation branches, exactly
    assert np.all(R.tanh_fp32(x[x >= 44.4]) == 1) and np.all(R.tanh_fp32(x[x <= -44.4]) == -1)
    assert np.all(R.sigmoid(x[x <= -88.8])[0] == 0) and np.all(R.sigmoid(x[x <= -88.8])[1] == 0) and np.all(R.sigmoid_fp32(x[x <= -88.8]) == 0)
    assert np.all(R.sigmoid(x[x == np.float32(-88.7)])[0] > 0) and np.all(R.sigmoid_fp32(x[x == np.float32(-88.7)]) > 0)
    assert R.tanh(np.float32(1e-8))[1] < 2.0 ** -22          # absolute, about 2^-23 where (e - 1) / (e + 1) cancels
    print(f"fp32 numpy / bound, activations {name}: " + ", ".join(f"{q} {v:.3f}" for q, v in worst.items()))
    assert all(v < 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("K", LC.SOFTMAX_K)
def test_an_fp32_evaluation_of_softmax_stays_inside_the_bounds(K):
    for rows in LC.SOFTMAX_ROWS:
        case = LC.softmax_case(K, rows)
        want, bound = R.softmax(case["x"])
        got = R.softmax_fp32(case["x"])
        r = LC.worst_ratio(got, want, bound)
        print(f"fp32 numpy / bound, softmax K {K} rows {rows}: {r:.3f}")
        assert r < 1.0
        assert np.all(np.abs(got.sum(1, dtype=np.float64) - 1.0) <= K * 2.0 ** -24)
        if K == 1:
            assert np.all(got == 1.0) and np.all(want == 1.0)
        if K >= 63:                          # the spread rows reach the denormals and exact zeros, the -3e38 classes exact zeros
            assert (want[3] < 2.0 ** -126).any() and (got[3] == 0).any() and (got[5] == 0).any()


# ------------------------------------------------------------------------------------------------------------ (c)
def _factor(got, want_bound):
    r = LC.worst_ratio(got, *want_bound)
    return np.inf if np.isnan(r) else r


@pytest.mark.parametrize("mutation", R.GEMM_MUTATIONS)
def test_every_gemm_mutation_leaves_the_bounds(mutation):
    """Per net: the worst error / bound of the mutated evaluation over the quantities the mutation can reach.  The scale mutations exist
    in mode 2 only, and not on the operand that carries the word 1.0; the bias is the forward GEMM's.  Every net must catch the mutation
    on some quantity, and every quantity must catch it on some net (a weight gradient over K = 2100 rows carries a summation term of
    K 2^-24 that hides a lost plane: `tall` is there for split-K, the short-K nets are the ones with teeth for W_grad)."""
    seen = {}
    for name in ("ragged", "tile", "tall", "tanh_affine"):
        case = LC.affine_case(name)
        xa = LC.affine_input(case)
        want = LC.affine_restated(case, 2, xa)
        with np.errstate(over="ignore", invalid="ignore"):
            got = affine_fp32(case, 2, xa, mutation)
        reach = ("out",) if mutation == "no_bias" else ("out", "W_grad") if mutation == "stale_bound" else ("out", "in_diff", "W_grad")
        if mutation == "stale_bound" and case["front"]:
            continue                         # (nothing is measured behind an activation layer: nothing to go stale)
        fac = {q: _factor(got[q], want[q]) for q in reach}
        print(f"{mutation} {name}: error / bound " + ", ".join(f"{q} {v:.3g}" for q, v in fac.items()))
        assert max(fac.values()) > 10.0, (mutation, name, fac)                 # not a near miss
        for q, v in fac.items():
            seen[q] = max(seen.get(q, 0.0), v)
    assert all(v > 10.0 for v in seen.values()), (mutation, seen)


def test_every_row_kernel_mutation_leaves_the_bounds():
    fac = {}
    for K in (65, 130, 4097):
        case = LC.softmax_case(K, 21)
        want = R.softmax(case["x"])
        with np.errstate(over="ignore", invalid="ignore"):
            fac[f"softmax_no_max K {K}"] = _factor(R.softmax_fp32(case["x"], "no_max"), want)
            fac[f"softmax_first_64 K {K}"] = _factor(R.softmax_fp32(case["x"], "first_64"), want)
    case = LC.activation_case("wide")
    x, d = case["x"], case["d"]
    y = R.sigmoid_fp32(x)
    fac["sigmoid_derivative_as_1-y^2"] = _factor(d * (np.float32(1) - y * y), R.sigmoid_diff(d, y))
    for kind, f32, f in (("tanh", R.tanh_fp32, R.tanh), ("sigmoid", R.sigmoid_fp32, R.sigmoid)):
        y = f32(x).reshape(-1).copy()
        y[2 ** 20:] = 0.0                    # the strided pass stops at 2^20 elements: the rest keeps the buffer's zeros
        fac[f"{kind}_stride_stops_at_2^20"] = _factor(y.reshape(x.shape), f(x))
    for k, v in fac.items():
        print(f"{k}: error / bound {v:.3g}")
    assert all(v > 10.0 for v in fac.values()), fac
