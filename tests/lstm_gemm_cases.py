"""The nets and inputs of the LSTM-layer GEMM tests, in ONE place: tests/test_lstm_gemm_restatement.py (CPU: an fp32 evaluation inside the
bounds, every mutation outside them) and tests/test_gpu_lstm_gemms.py (the kernels, through Net) draw the very same arrays.  Rows are
T * S (row t * S + s), lens ragged.  ONE trainable layer is under test per case (`hold`); a layer below it only produces its input.

Operands of a layer that reads the NET's input: x is scaled per row (frame) by 2^[-15, 15] and per column by 2^[-12, 12]; W_x carries the
INVERSE column scales (so they cancel in every product) and row scales of its own, 2^[-15, 15]: the pre-activations span some 60
binades, a share of them lies in [-4, 4] where the gates are neither linear nor saturated, and a GEMM that scales its fp16 planes by
the wrong vector, the wrong half of a vector, a stale measurement or one word per tensor misses the per-element bound by orders of
magnitude where a max-norm comparison sees nothing.  One all-zero row of W_x, one all-zero column of x.  The gradient of the layer's
output is scaled per SEQUENCE by 2^[-15, 15] and per column by 2^[-10, 10], one sequence all zero.  One cell per direction is TINY
(tiny_cells): its column of that gradient is 2^-30 of the others' and its column of W_m zero, so that nothing flows into it through the
recurrence and its four gate-gradient columns stay 2^-30 of the tensor's largest -- the columns a per-tensor word loses altogether,
however long the sum over the frames is.  The held layer of `upper`, which reads an LSTM layer's output (|x| < 1), gets W_x rows
2^[-10, 10] and columns 2^[-8, 8]; those of the forward cases: _upper_wx."""
import functools

import numpy as np

from tests import lstm_gemm_restatement as LR
from tests.layer_cases import _pow2, _ro, _scaled, lens_of
from tests.update_cases import worst_ratio          # noqa: F401

MODES = (0, 1, 2)
BI, UNI = "BiLstmParallel", "LstmParallel"
#             name      kind  D    H    S   T
BACKWARD = {"ragged":  (BI,  13,  32,  3,  7),      # guarded tiles everywhere; fewer rows than the reductions have row blocks
            "tile":    (BI,  128, 32,  8,  32),     # interior tiles: in_diff 256 x 128, W_x gradient 256 x 128
            "tall":    (BI,  40,  32,  16, 130),    # weight gradients over K = 2080 >= 2048 rows: split-K, ragged last chunk
            "uni":     (UNI, 24,  32,  5,  9),      # one direction: no second half of any bound vector
            "wide":    (BI,  16,  128, 8,  16)}     # W_m gradient 512 x 128: interior tiles
UPPER = {"upper":      (BI,  13,  32,  8,  20)}     # two layers, the UPPER one held: x = the lower layer's m, the word 1.0 in its W_x gradient
#             name        H    S   T   environment of the Net                              the plan's input_gemm
FORWARD = {"whole":      (64,  4,  33, dict(EESEN_GATE_FWD="0"),                      "whole, recurrence"),
           "quadrants":  (64,  32, 33, dict(EESEN_GATE_FWD="0", EESEN_FWD_QUAD="1"),  "needed quadrants"),
           "ends":       (64,  32, 33, dict(EESEN_GATE_FWD="0", EESEN_FWD_QUAD="0"),  "both ends"),
           "gated":      (64,  32, 8,  dict(EESEN_GATE_FWD="1"),                      "gated"),
           "gated_rest": (64,  20, 9,  dict(EESEN_GATE_FWD="1"),                      "gated"),      # rows 128..179: the plain remainder GEMM
           "dropout":    (64,  8,  12, dict(EESEN_GATE_FWD="0"),                      "whole, recurrence")}
SINGLE = {"single":      (BI,  40,  32,  5,  11)}   # a single layer, forward: x row bounds MEASURED
DROP_P = 0.75


def lstm_layer(kind, D, H, params):
    nd = 2 if kind == BI else 1
    return dict(type=kind, input_dim=D, output_dim=nd * H, learn_rate_coef=1.0, max_grad=0.0, params=params)


def _plain_params(rng, nd, D, H, scale):
    u = lambda *sh: rng.uniform(-scale, scale, sh).astype(np.float32)
    return [p for _ in range(nd) for p in (u(4 * H, D), u(4 * H, H), u(4 * H), u(H), u(H), u(H))]


def _recurrent_params(rng, H):
    """W_m, bias, peepholes of one direction: ordinary sizes."""
    return (rng.uniform(-0.3, 0.3, (4 * H, H)).astype(np.float32), rng.standard_normal(4 * H).astype(np.float32),
            [rng.uniform(-0.5, 0.5, H).astype(np.float32) for _ in range(3)])


def tiny_cells(H):
    """The tiny cell of each direction (module docstring)."""
    return [H // 5, H - 3]


def _held_layer(rng, kind, D, H, Wx, neutral):
    nd = 2 if kind == BI else 1
    params = []
    for dirn in range(nd):
        Wm, b, peep = _recurrent_params(rng, H)
        Wm[:, tiny_cells(H)[dirn]] = 0.0
        if neutral:
            Wm, peep = np.zeros_like(Wm), [np.zeros_like(p) for p in peep]
        params += [np.ascontiguousarray(Wx[dirn * 4 * H:(dirn + 1) * 4 * H]), Wm, b] + peep
    return lstm_layer(kind, D, H, params)


def _net_input_operands(rng, rows, D, G4):
    """x [rows x D] and W_x [G4 x D] of a layer that reads the net's input (module docstring)."""
    colx = rng.integers(-12, 13, D)
    bx = rng.standard_normal((rows, D)); bx = np.where(np.abs(bx) < 1e-3, 1e-3, bx)
    bw = rng.standard_normal((G4, D)); bw = np.where(np.abs(bw) < 1e-3, 1e-3, bw)
    x = (bx * _pow2(rng, rows, -15, 15)[:, None] * np.ldexp(1.0, colx)[None, :]).astype(np.float32)
    Wx = (bw * _pow2(rng, G4, -15, 15)[:, None] * np.ldexp(1.0, -colx)[None, :]).astype(np.float32)
    x[:, D // 2] = 0.0                                                # one all-zero column of x
    Wx[G4 // 3] = 0.0                                                 # one all-zero row of W_x
    return x, Wx


def _upper_wx(rng, G4, K):
    """W_x of a HELD layer that reads an LSTM layer's output, for the forward cases: rows 0.05 x 2^[0, 30], columns 2^[-4, 4].  A gate
    shows its pre-activation only while that is of order 1 -- below, the activation's own rounding hides it, above, it saturates -- so
    the rows a wrong scale must hurt are the SMALLEST ones, with pre-activations of order 1, and the others lie up to 2^30 above them."""
    base = rng.standard_normal((G4, K)); base = np.where(np.abs(base) < 1e-3, 1e-3, base)
    Wx = (0.05 * base * _pow2(rng, G4, 0, 30)[:, None] * _pow2(rng, K, -4, 4)[None, :]).astype(np.float32)
    Wx[G4 // 3] = 0.0                                                 # one all-zero row of W_x
    return Wx


def _top_gradient(rng, S, T, nd, H):
    seq = _pow2(rng, S, -15, 15)
    seq[S // 2] = 0.0                                                 # one all-zero sequence
    base = rng.standard_normal((T * S, nd * H)); base = np.where(np.abs(base) < 1e-3, 1e-3, base)
    col = _pow2(rng, nd * H, -10, 10)
    for dirn in range(nd):
        col[dirn * H + tiny_cells(H)[dirn]] *= 2.0 ** -30
    return (base * np.tile(seq, T)[:, None] * col[None, :]).astype(np.float32)


def _seed(name):
    return 4000 + sorted(list(BACKWARD) + list(UPPER) + list(FORWARD) + list(SINGLE)).index(name)


@functools.lru_cache(maxsize=None)
def backward_case(name):
    """dict(layers, hold, S, T, lens, x [the NET's input], d [the gradient of the net's output], zero_col, zero_seq)."""
    two = name in UPPER
    kind, D, H, S, T = (UPPER if two else BACKWARD)[name]
    rng = np.random.default_rng(_seed(name))
    nd, rows = (2 if kind == BI else 1), S * T
    if two:
        x = rng.standard_normal((rows, D)).astype(np.float32)
        lower = lstm_layer(BI, D, H, _plain_params(rng, 2, D, H, 0.5))
        layers = [lower, _held_layer(rng, kind, 2 * H, H, _scaled(rng, nd * 4 * H, 2 * H, 10, 8), False)]
        layers[1]["params"][0][(4 * H) // 3] = 0.0
    else:
        x, Wx = _net_input_operands(rng, rows, D, nd * 4 * H)
        layers = [_held_layer(rng, kind, D, H, Wx, False)]
    for L in layers:
        _ro(dict(enumerate(L["params"])))
    return _ro(dict(name=name, layers=layers, hold=len(layers) - 1, S=S, T=T, lens=lens_of(S, T, _seed(name)), x=x,
                    d=_top_gradient(rng, S, T, nd, H), zero_col=None if two else D // 2, zero_seq=S // 2))


@functools.lru_cache(maxsize=None)
def forward_case(name):
    """dict(layers, hold, S, T, lens, x, env, plan, dropout): the held layer has W_m = 0 and zero peepholes."""
    rng = np.random.default_rng(_seed(name))
    if name in SINGLE:
        kind, D, H, S, T = SINGLE[name]
        x, Wx = _net_input_operands(rng, S * T, D, 8 * H)
        layers, env, plan = [_held_layer(rng, kind, D, H, Wx, True)], dict(EESEN_GATE_FWD="0"), None
    else:
        H, S, T, env, plan = FORWARD[name]
        D = 13
        drop = name == "dropout"
        x = rng.standard_normal((S * T, D)).astype(np.float32)
        lower = lstm_layer(BI, D, H, _plain_params(rng, 2, D, H, 0.5))
        if drop:     # half of the lower layer's cells wide open (every gate's bias + 20): c grows by 1 a frame, |m| -> 1 -- times 4 in the mask
            lower["dropout"] = dict(forward=DROP_P, fw_step=True)
            for dirn in range(2):
                for q in range(4):
                    lower["params"][6 * dirn + 2][q * H:q * H + H // 2] += 20.0
        layers = [lower, _held_layer(rng, BI, 2 * H, H, _upper_wx(rng, 8 * H, 2 * H), True)]
    for L in layers:
        _ro(dict(enumerate(L["params"])))
    return _ro(dict(name=name, layers=layers, hold=len(layers) - 1, S=S, T=T, lens=lens_of(S, T, _seed(name)), x=x, env=env, plan=plan,
                    dropout=name == "dropout"))


def cpu_mask(case):
    """A forward-dropout mask for the CPU tests (the device draws its own): 0 or 1 / (1 - p), per frame and cell."""
    rows, w = case["S"] * case["T"], case["layers"][0]["output_dim"]
    keep = np.random.default_rng(99).random((rows, w)) >= DROP_P
    return (keep / (1.0 - DROP_P)).astype(np.float32)


def held_input(case, m_lower=None, mask=None):
    """The held layer's own input: the net's input, or the lower layer's m (as the device returned it, or from the plain recurrence on
    the CPU) -- times the forward-dropout mask where the case has one."""
    if case["hold"] == 0:
        return case["x"]
    if m_lower is None:
        m_lower = LR.recurrence(case["layers"][0], case["x"], case["lens"], case["S"], case["T"])["m"]
    if case.get("dropout"):
        m_lower = (m_lower * (cpu_mask(case) if mask is None else mask)).astype(np.float32)
    return m_lower


def x_bounded(case):
    """Net::x_is_bounded for the held layer: behind an LSTM layer without forward dropout."""
    return case["hold"] > 0 and not case.get("dropout")
