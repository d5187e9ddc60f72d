"""The nets and inputs of the layer tests, in ONE place: tests/test_layer_restatement.py (CPU: the restatement against the oracle, an
fp32 evaluation inside the bounds, every mutation outside them) and tests/test_gpu_layers.py (the kernels, through Net) draw the very
same arrays.  Rows are T * S (row t * S + s), lens ragged; these layers compute the padded rows too, as the reference does.

Every net has ONE trainable layer, so nothing compounds.  Affine operands are scaled per row AND per column by independent powers of
two (x rows 2^[-15, 15], x columns 2^[-12, 12], W rows 2^[-10, 10], W columns 2^[-8, 8], out_diff rows 2^[-15, 15], columns 2^[-10, 10]):
a GEMM that scales its fp16 planes by the wrong vector, or by one word per tensor, then misses the per-element bound by orders of
magnitude where a max-norm comparison sees nothing."""
import functools

import numpy as np

from tests import layer_restatement as R
from tests.update_cases import worst_ratio          # noqa: F401  (shared with the update-rule tests)

#            name          din   dout   S    T   layer in front
AFFINE = {"ragged":       (13,   11,    3,   7,  None),        # guarded tiles; pad columns (ld 16 / 12); col_sums with fewer rows than row blocks
          "tile":         (64,   256,   8,   32, None),        # interior 128 x 128 tiles, unguarded
          "big":          (64,   1024,  16,  64, None),        # forward on the 256 x 256 flavour (16 tiles); weight gradient K = 1024, no split
          "tall":         (40,   46,    7,   300, None),       # weight gradient K = 2100 >= 2048, one tile: split-K, ragged last chunk
          "tanh_affine":  (40,   46,    5,   30, "Tanh"),      # x_is_bounded: the word 1.0 forward and in the weight gradient
          "sigm_affine":  (13,   11,    3,   7,  "Sigmoid")}
MODES = (0, 1, 2)
EDGES = np.array([s * v for v in (0.0, 1e-8, 1e-4, 1.0, 44.3, 44.4, 60.0, 88.7, 104.0) for s in (1.0, -1.0)], np.float32)
ACTIVATION = {"edges": (13, 3, 7), "wide": (1030, 4, 275)}      # width, S, T;  wide: 1,133,000 elements, 84,424 of them past 2^20
SOFTMAX_K = (1, 2, 63, 64, 65, 130, 4097)
SOFTMAX_ROWS = {21: (3, 7), 24: (4, 6)}                         # rows: (S, T);  21: the last workgroup (4 rows) partly idle


def lens_of(S, T, seed):
    lens = np.random.default_rng(seed).integers(1, T + 1, S).astype(np.int32)
    lens[0] = T
    return lens


def _pow2(rng, n, lo, hi):
    return np.ldexp(1.0, rng.integers(lo, hi + 1, n))


def _scaled(rng, r, c, rexp, cexp):
    base = rng.standard_normal((r, c))
    base = np.where(np.abs(base) < 1e-3, 1e-3, base)                  # (no accidental zeros: the zero row / column are placed on purpose)
    return (base * _pow2(rng, r, -rexp, rexp)[:, None] * _pow2(rng, c, -cexp, cexp)[None, :]).astype(np.float32)


def _ro(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def layer_affine(din, dout, W, b):
    return dict(type="AffineTransform", input_dim=din, output_dim=dout, learn_rate_coef=1.0, max_grad=0.0, params=[W, b])


def layer_plain(kind, dim):
    return dict(type=kind, input_dim=dim, output_dim=dim, params=[])


def tiny_columns(din):
    return [2, din - 1] if din < 20 else [3, 17, din - 1]


@functools.lru_cache(maxsize=None)
def affine_case(name):
    """dict(layers, front, S, T, lens, x, d, W, b, tiny): x is the NET's input [rows x din] -- the Affine layer's own input where
    front is None, the activation layer's otherwise; d the out_diff [rows x dout]."""
    din, dout, S, T, front = AFFINE[name]
    rng = np.random.default_rng(sorted(AFFINE).index(name) + 100)
    rows = S * T
    W = _scaled(rng, dout, din, 10, 8)
    W[dout // 3] = 0.0                                                # one all-zero row of W
    b = (rng.standard_normal(dout) * _pow2(rng, dout, -6, 6)).astype(np.float32)
    d = _scaled(rng, rows, dout, 15, 10)
    d[rows // 2] = 0.0                                                # one all-zero row of out_diff
    tiny = []
    if front is None:
        x = _scaled(rng, rows, din, 15, 12)
        x[:, din // 2] = 0.0                                          # one all-zero column of x
        layers = [layer_affine(din, dout, W, b)]
    else:
        x = (rng.standard_normal((rows, din)) * 2.0).astype(np.float32)
        tiny = tiny_columns(din)
        for c in tiny:   # activation outputs of at most 2^-20 in every row: tanh(v) ~ v, sigmoid(v) ~ e^v
            x[:, c] = (np.clip(rng.standard_normal(rows), -2, 2) * 2.0 ** -22 if front == "Tanh" else rng.uniform(-30.0, -14.5, rows)).astype(np.float32)
        layers = [layer_plain(front, din), layer_affine(din, dout, W, b)]
    return _ro(dict(name=name, layers=layers, front=front, S=S, T=T, lens=lens_of(S, T, rows), x=x, d=d, W=W, b=b, tiny=tiny))


def affine_input(case, y_front=None):
    """The Affine layer's own input: the net's input, or -- behind an activation layer -- that layer's output: y_front as the device
    returned it (GPU test, bit for bit), else the fp32 numpy evaluation (CPU test)."""
    if case["front"] is None:
        return case["x"]
    if y_front is not None:
        return y_front
    return (R.tanh_fp32 if case["front"] == "Tanh" else R.sigmoid_fp32)(case["x"])


def affine_restated(case, mode, xa):
    """Everything the Affine layer of `case` computes from its input xa, restated: dict quantity -> (value, bound)."""
    bounded = case["front"] is not None
    gw, gw_b, gb, gb_b = R.affine_grads(case["d"], xa, mode, bounded)
    out = dict(out=R.affine_forward(xa, case["W"], case["b"], mode, bounded), in_diff=R.affine_in_diff(case["d"], case["W"], mode),
               W_grad=(gw, gw_b), b_grad=(gb, gb_b))
    for q, (v, bnd) in out.items():     # results stay inside the normal fp32 range (the bounds carry no underflow term)
        mag = np.abs(v) + bnd
        assert np.isfinite(v).all() and mag.max() < 2.0 ** 100 and (mag[mag > 0].min() > 2.0 ** -100), (case["name"], q)
    return out


@functools.lru_cache(maxsize=None)
def activation_case(name):
    """dict(width, S, T, lens, x, d): the edge values (EDGES) on every row of `edges`, sprinkled over `wide`."""
    width, S, T = ACTIVATION[name]
    rng = np.random.default_rng(7 + width)
    rows = S * T
    x = (rng.standard_normal((rows, width)) * 3.0).astype(np.float32)
    flat = x.reshape(-1)
    if name == "edges":
        flat[:] = np.resize(EDGES, flat.size)
        flat[EDGES.size * 12:] = (rng.standard_normal(flat.size - EDGES.size * 12) * 3.0).astype(np.float32)
    else:
        idx = rng.choice(flat.size, 40 * EDGES.size, replace=False)
        flat[idx] = np.resize(EDGES, idx.size)
        flat[2 ** 20 - 9: 2 ** 20 + 9] = EDGES                           # ... and across the boundary of the strided pass
    assert np.all(np.abs(np.abs(flat.astype(np.float64)) - R.LN_FLT_MAX) > 1e-3) and np.all(np.abs(np.abs(flat.astype(np.float64)) - R.LN_FLT_MAX / 2) > 1e-3)
    d = (rng.standard_normal((rows, width)) * _pow2(rng, rows, -8, 8)[:, None]).astype(np.float32)
    return _ro(dict(name=name, width=width, S=S, T=T, lens=lens_of(S, T, width), x=x, d=d))


SOFTMAX_KINDS = ("normal4", "one_plus_60", "all_equal", "spread_120", "offset_1e4", "some_minus_3e38")


@functools.lru_cache(maxsize=None)
def softmax_case(K, rows):
    """dict(K, S, T, lens, x, d): row r is of kind SOFTMAX_KINDS[r % 6].  No infinities, no NaN."""
    S, T = SOFTMAX_ROWS[rows]
    rng = np.random.default_rng(1000 * K + rows)
    x = np.empty((rows, K), np.float64)
    for r in range(rows):
        kind = SOFTMAX_KINDS[r % len(SOFTMAX_KINDS)]
        v = rng.standard_normal(K) * 4.0
        if kind == "one_plus_60":
            v = rng.standard_normal(K)
            v[rng.integers(K)] += 60.0
        elif kind == "all_equal":
            v[:] = rng.standard_normal() * 4.0
        elif kind == "spread_120":                                    # beyond 104: classes underflow to exactly 0, others to denormals
            v = rng.permutation(np.linspace(0.0, -120.0, K)) + 3.0
        elif kind == "offset_1e4":
            v += 1e4
        elif kind == "some_minus_3e38" and K > 1:
            gone = rng.random(K) < 0.25
            gone[rng.integers(K)] = False
            v[gone] = -3e38
        x[r] = v
    x = x.astype(np.float32)
    assert np.isfinite(x).all()
    d = rng.standard_normal((rows, K)).astype(np.float32)
    return _ro(dict(K=K, S=S, T=T, lens=lens_of(S, T, K + rows), x=x, d=d))
