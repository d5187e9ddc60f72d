"""The nets and inputs of the "bf16 forward" tests (eesen_net_set_forward_precision(1 | 2)), in ONE place:
tests/test_bf16_forward_restatement.py (CPU: an fp32 evaluation inside the bounds, every mutation outside them) and
tests/test_gpu_bf16_forward_fp64.py (the kernels, through Net) draw the very same arrays.  Rows are T * S (row t * S + s), lens ragged.
The generators are those of tests/lstm_gemm_cases.py: rows, columns and sequences span tens of binades, with one all-zero row of W_x
and one all-zero column of x.

GEMM cases (the one-product body of gemm_split_body, gemm.hip), observed through a held BiLSTM layer with zero W_m and zero peepholes,
as the FORWARD cases of lstm_gemm_cases are:
    ragged    D = 13, H = 32, S = 3, T = 7: guarded tiles, K no multiple of 16
    interior  a lower BiLSTM layer (H = 32) feeds the held one with K = 64, H = 64 at S = 16, T = 8: 128 rows x 512 columns, every
              tile whole -- the unguarded instantiation
    ends      two BiLSTM layers, H = 256, S = 32, T = 40: the smallest shape at which fwd_early (net.cpp) plans the early middle
              (T >= 32, r0 = 512 < r1 = 768) -- WHERE the lower recurrence leaves room on its CUs (RecPlan::leaves_room: a tile of at
              most 8 units).  Under precision 2 it does (the fp32-class narrow tile): the middle rows run on the side stream with the
              token of extra LDS.  Under precision 1 the lower layer runs the 16-unit bf16 tile, which does not: "whole, recurrence".
              Created with EESEN_FWD_QUAD=0, as the `ends` case of lstm_gemm_cases is, because of the next case.
    quadrants the same net and input WITHOUT that switch, under precision 2 only: fwd_quad_rule (net.cpp) excludes the "needed
              quadrants" schedule where the held layer's own recurrence has no row guard -- the bf16 kernel <.,4,1,2,false> of
              precision 1 -- but under precision 2 that recurrence is the fp32-class narrow tile, which has one: the two ends run
              as four quadrant launches of the one-product body, two of them on the side stream under capped LDS.
    affine    the AffineTransform cases of tests/layer_cases.py, as the net's last layer on the net's own input (AFFINE_LAST), and
              behind an LstmParallel layer of din cells, on the m the device returned (AFFINE_BEHIND: the four cases without an
              activation in front).  Net::forward_pass launches an Affine layer's GEMM by ONE call, on the main stream and without
              extra LDS, whatever follows it; nothing else reads its output but the next layer, so it is observed as the last one.

Recurrence cases (lstm_fwd_persistent_bf_kernel<H / 256,4,1,2,false>), one layer each: RECURRENCE.  The four tiles bf_plan_shape
(rec_plan.cpp) admits, BOTH directions with weights of ordinary size (W_x +-0.3, W_m +-2 / sqrt(H), bias N(0, 1), peepholes +-0.5),
so that each direction's recurrent product m_prev W_m^T is of the size of the pre-activation it enters; one LstmParallel layer, whose
tile is the same <1,4,1,2,false> (the plan shape does not depend on the direction count).  Inputs N(0, 1) times a per-SEQUENCE scale
2^[-15, 15].  The input and output gates' rows of W_x are times 2^-15 everywhere, so that i and o do not saturate where a loud
sequence's g and f do -- there their pre-activations are of order 1, where a gate shows them best: c = g i + c_prev f is an exact zero
wherever i is one and the state is (half of a sequence's first frame), m = tanh(c) o wherever o is, and more than half of a loud
sequence's c and m would be held by nothing (tests/test_bf16_forward_restatement.py asserts that share per quantity).  Variations:
  * bi256_small_fw, bi256_small_bw: ONE direction's W_m and W_x times 2^-20, zero bias -- the forward direction in the one, the
    backward direction in the other -- so that its pre-activations lie 20 binades under the other direction's in the same tensor.
    The device's tanh is 1 - 2 rcp(1 + e), absolute error 2^-24 and up: a g of 2^-20 times a QUIET sequence's scale would lie under
    its own bound, and c and m with it, so these two cases take their sequence scales from 2^[4, 15];
  * bi512_tiny, the "tiny state" case: the inputs times 2^-20 (no sequence scale), no bias on g, and the g rows of W_x times 2^8 --
    g is 2^-12 and c and m smaller still in every frame, yet some 2^9 above tanh's absolute error (at inputs times 2^-20 alone
    they lie under it).  The recurrent product's roundings are far under that error here: the case holds the cell at tiny state,
    not the product."""
import functools

import numpy as np

from tests import lstm_gemm_cases as LC
from tests import lstm_gemm_restatement as LR
from tests.layer_cases import AFFINE, _pow2, _ro, affine_case, lens_of      # noqa: F401
from tests.update_cases import worst_ratio          # noqa: F401

BI, UNI = LC.BI, LC.UNI
PRECISIONS = (1, 2)
#          name        D    H(lower) H    S    T
GEMM = {"ragged":     (13,  None,    32,  3,   7),
        "interior":   (13,  32,      64,  16,  8),
        "ends":       (13,  256,     256, 32,  40),
        "quadrants":  (13,  256,     256, 32,  40)}       # the arrays of `ends`
# the switches a case's Net is created under (tuning.h), and the held layer's "input_gemm" of Plan() per forward precision
GEMM_ENV = {"ends": {"EESEN_FWD_QUAD": "0"}}
WHOLE, BOTH_ENDS = "whole, recurrence", "middle under the recurrence below, both ends, recurrence"
QUADRANTS = "middle under the recurrence below, needed quadrants, recurrence, late quadrants beside it"
GEMM_PLAN = {"interior": {1: WHOLE, 2: WHOLE}, "ends": {1: WHOLE, 2: BOTH_ENDS}, "quadrants": {2: QUADRANTS}}
GEMM_RUNS = [(n, p) for n in GEMM for p in PRECISIONS if p in GEMM_PLAN.get(n, PRECISIONS)]
AFFINE_LAST = tuple(AFFINE)
AFFINE_BEHIND = tuple(n for n, c in AFFINE.items() if c[4] is None)
#                name              kind H     S   T  tiny   the 2^-20 direction
RECURRENCE = {"bi256_s20":        (BI,  256,  20, 8, False, None),   # ragged second sequence tile
              "bi512_tiny":       (BI,  512,  16, 6, True,  None),
              "bi768_s16":        (BI,  768,  16, 6, False, None),
              "bi1024_s32":       (BI,  1024, 32, 6, False, None),   # 256 workgroups, co-resident
              "uni256_s32":       (UNI, 256,  32, 8, False, None),   # one direction: 32 workgroups, the same tile as bi256
              "bi256_small_fw":   (BI,  256,  16, 6, False, 0),
              "bi256_small_bw":   (BI,  256,  16, 6, False, 1)}
REC_D = 40


def kernel_row(H):
    """The row of kRecKernels, as Plan() prints it (tests/recurrence_cases.py: fwd_bf)."""
    return "lstm_fwd_persistent_bf_kernel<%d,4,1,2,false>" % (H // 256)


def bf16_layers(layers):
    """LSTM layers of a net that bf_plan_shape puts on the bf16 recurrence kernel under precision 1."""
    return sum(L["type"] in (BI, UNI) and (L["output_dim"] // (2 if L["type"] == BI else 1)) % 256 == 0 and
               L["output_dim"] // (2 if L["type"] == BI else 1) <= 1024 for L in layers)


def _seed(name):
    return 7000 + sorted(list(GEMM) + list(RECURRENCE)).index(name)


@functools.lru_cache(maxsize=None)
def gemm_case(name):
    """dict(layers, hold, S, T, lens, x): the held layer has W_m = 0 and zero peepholes."""
    D, Hl, H, S, T = GEMM[name]
    name = "ends" if name == "quadrants" else name
    rng = np.random.default_rng(_seed(name))
    if Hl is None:
        x, Wx = LC._net_input_operands(rng, S * T, D, 8 * H)
        layers = [LC._held_layer(rng, BI, D, H, Wx, True)]
    else:
        x = rng.standard_normal((S * T, D)).astype(np.float32)
        lower = LC.lstm_layer(BI, D, Hl, LC._plain_params(rng, 2, D, Hl, 0.5 if Hl < 128 else 0.1))
        layers = [lower, LC._held_layer(rng, BI, 2 * Hl, H, LC._upper_wx(rng, 8 * H, 2 * Hl), True)]
    for L in layers:
        _ro(dict(enumerate(L["params"])))
    return _ro(dict(name=name, layers=layers, hold=len(layers) - 1, S=S, T=T, lens=lens_of(S, T, _seed(name)), x=x))


@functools.lru_cache(maxsize=None)
def affine_behind_case(name):
    """dict(layers, S, T, lens, x, W, b): [LstmParallel of din cells, the AffineTransform of affine_case(name)]."""
    case = affine_case(name)
    din = case["W"].shape[1]
    rng = np.random.default_rng(7100 + sorted(AFFINE).index(name))
    x = rng.standard_normal((case["S"] * case["T"], 13)).astype(np.float32)
    lower = LC.lstm_layer(UNI, 13, din, LC._plain_params(rng, 1, 13, din, 0.5))
    _ro(dict(enumerate(lower["params"])))
    return _ro(dict(name=name, layers=[lower, case["layers"][-1]], S=case["S"], T=case["T"], lens=case["lens"], x=x, W=case["W"], b=case["b"]))


@functools.lru_cache(maxsize=None)
def recurrence_case(name):
    """dict(layers [one], kind, H, S, T, lens, x, tiny, small, row)."""
    kind, H, S, T, tiny, small = RECURRENCE[name]
    rng = np.random.default_rng(_seed(name))
    nd = 2 if kind == BI else 1
    x = rng.standard_normal((S * T, REC_D))
    x = x * (2.0 ** -20 if tiny else np.tile(_pow2(rng, S, -15 if small is None else 4, 15), T)[:, None])
    params = []
    for dirn in range(nd):
        Wx = rng.uniform(-0.3, 0.3, (4 * H, REC_D))
        Wx[H:2 * H] *= 2.0 ** -15
        Wx[3 * H:] *= 2.0 ** -15
        Wm = rng.uniform(-2.0, 2.0, (4 * H, H)) / np.sqrt(H)
        b = rng.standard_normal(4 * H)
        if tiny:
            b[:H] = 0.0
            Wx[:H] *= 2.0 ** 8
        if dirn == small:
            Wx, Wm, b = Wx * 2.0 ** -20, Wm * 2.0 ** -20, np.zeros(4 * H)
        params += [Wx.astype(np.float32), Wm.astype(np.float32), b.astype(np.float32)] + [rng.uniform(-0.5, 0.5, H).astype(np.float32) for _ in range(3)]
    layer = LC.lstm_layer(kind, REC_D, H, params)
    _ro(dict(enumerate(layer["params"])))
    return _ro(dict(name=name, layers=[layer], kind=kind, H=H, S=S, T=T, lens=lens_of(S, T, _seed(name)), x=x.astype(np.float32), tiny=tiny,
                    small=small, row=kernel_row(H)))


def rounded_operands(layers, hold, x):
    """(layers with round_bf16 applied to the held layer's W_x -- an Affine layer's W --, round_bf16(x)): what the variant must not be
    able to tell from the originals."""
    from oracle.bf16_forward import round_bf16
    out = [dict(L) for L in layers]
    p = list(out[hold]["params"])
    for k in ((0,) if out[hold]["type"] == "AffineTransform" else range(0, len(p), 6)):
        p[k] = round_bf16(p[k])
    out[hold]["params"] = p
    return out, round_bf16(x)


def held_input(case, m_lower=None):
    """The held layer's own input: the net's input, or the lower layer's m (as the device returned it, or from a plain recurrence on the CPU)."""
    if len(case["layers"]) == 1:
        return case["x"]
    if m_lower is None:
        m_lower = LR.recurrence(case["layers"][0], case["x"], case["lens"], case["S"], case["T"])["m"]
    return m_lower
