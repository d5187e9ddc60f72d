"""Plain numpy fp64 restatements of the layers between the recurrences -- AffineTransform, <Sigmoid>, <Tanh>, <Softmax> -- forward and
backward, each value with an ABSOLUTE rounding bound per element.  What tests/test_gpu_layers.py holds Net::forward_pass /
Net::backpropagate_impl (csrc/net.cpp) and their kernels (csrc/gemm.hip, optim.hip, ctc.hip, lstm.hip::col_sums) against.

The operations, as the reference states them:
    AffineTransform  affine-trans-layer.h:161-219   y = x W^T + b;  in_diff = d W;  W_grad = d^T x;  b_grad = column sums of d
    Sigmoid          sigmoid-layer.h:44-51          y = 1 / (1 + exp(-x));          in_diff = d y (1 - y)
    Tanh             tanh-layer.h:44-51             y = (e - 1) / (e + 1), e = exp(2x), 1 where e overflows;   in_diff = d (1 - y^2)
    Softmax          softmax-layer.h:44-57          y_k = exp(x_k - m) / sum_j exp(x_j - m), m = max x;        in_diff = d (a copy)
(the device formulas are quoted at activation_kernel / activation_diff_kernel of optim.hip and softmax_rows_kernel of ctc.hip).

Every bound is DERIVED by counting roundings, with 2^-24 per fp32 operation; nothing is measured.  The one constant not read off the code is
ULP_EXP, the error of the device's expf / logf in ulps: no copy of the HIP math-function accuracy table was at hand, so ULP_EXP = 2 is an
ASSUMPTION (the published table lists both functions below that).

GEMM results C = A B^T (+ bias), A [M x K], B [N x K]:
    bound = sum_k (eps_a |b| + eps_b |a|) + c_mode sum_k |a||b| + (K + 3) 2^-24 (sum_k |a||b| + |bias|)
  * the last term: a K-term sum in ANY order (split-K and its reduce pass included) is within (K - 1) 2^-24 of sum |terms|; + the bias
    add, + the alpha / beta epilogue, + margin for the second-order terms;
  * mode 0 (fp32 MFMA chain): eps = 0, c = 0;
  * mode 1 (three bf16 planes by TRUNCATION, six products; gemm.hip split_stage_a/b/c, PL = 3): the split itself is exact; the three
    dropped products mid lo', lo mid', lo lo'.  With |mid| < 2^-7 |a| and |lo| < 2^-15 |a| (a truncation to 8 significant bits leaves
    less than 2^-7 of the leading bit) they sum to less than (2 2^-22 + 2^-30) |a b|: C1.  (The comment in gemm.hip says 2^-23: that is
    the typical size, not the worst case, and it is not what this bound uses.);
  * mode 2 (two fp16 planes of the operand times a power of two; PL = 2): hi = fp16(a s), lo = fp16(a s - hi), both to nearest:
    |a - (hi + lo) / s| <= max(2^-22 |a|, 2^-25 / s) (where lo is an fp16 denormal its quantum is 2^-24: half of it) and 0 for a = 0:
    eps;  the dropped lo lo' <= 2^-22 |a b|: c.  s = half_scale(bound) (gemm.hip:377-383): the power of two that brings `bound` into
    [2^14, 2^15), 2^126 for a zero bound.  The bound the design prescribes per operand and index (net.cpp forward_pass /
    backpropagate_impl): forward -- per row of x, per row of W; input gradient -- per row of d, per column of W; weight gradient -- per
    column of d, per column of x; and the single word 1.0 in place of the x vector behind an activation or softmax layer
    (Net::x_is_bounded).
Bias gradient (col_sums): (rows + 3) 2^-24 sum_r |d_rc|.

Sigmoid, Tanh: held against the TRUE functions in fp64.  With e^ = e (1 + d1), |d1| <= ULP_EXP 2^-23:
  * tanh: (e^ - 1) / (e^ + 1) moves by (1 - y^2) / 2 d1 (the derivative of the quotient), then three roundings (e - 1, e + 1, the
    division) of |y|: (1 - y^2) / 2 ULP_EXP 2^-23 + 3 2^-24 |y| -- absolute, about 2^-23 at 0 where the quotient cancels;
  * sigmoid: 1 / (1 + e^), e = exp(-x): y (1 - y) ULP_EXP 2^-23 + 2 2^-24 y + one denormal quantum (2^-149) where y underflows;
  * saturation is exact: exp(2x) = inf -> 1;  exp(2x) = 0 -> -1 (both inside the tanh bound: the true value rounds to +-1);
    exp(-x) = inf -> 1 / (1 + inf) = 0 EXACTLY, although the true value (below 2^-128) is a representable denormal: where -x is above
    ln(FLT_MAX) the restated value is 0 with bound 0;
  * derivatives from the y the DEVICE returned: d (1 - y y): the square and the difference round (2^-24 (y^2 + |1 - y^2|) |d|; one
    rounding and 2^-24 |1 - y^2| alone where the compiler contracts to an fma), the product rounds: 2^-24 |d (1 - y^2)|.  d y (1 - y):
    three roundings of the result.  Plus a denormal quantum.
Softmax, relative bound of y_k: 2^-24 |x_k - m| (the subtraction's rounding, through exp) + ULP_EXP 2^-23 (expf) for the numerator; the
same, weighted by y_j, for the denominator; + (ceil(K / 64) + 8) 2^-24 for the lane's chain, the six butterfly steps of the wave sum
and the division.  Plus one denormal quantum where y_k underflows."""
import numpy as np

from oracle.bf16_forward import round_bf16

U = 2.0 ** -24
ULP_EXP = 2.0                   # ASSUMED (see above): ulps of the device expf / logf
C1 = 2.0 ** -21 + 2.0 ** -30    # mode 1: the three dropped products
C2 = 2.0 ** -22                 # mode 2: the dropped lo lo'
TINY = 2.0 ** -149              # one fp32 denormal quantum
LN_FLT_MAX = 88.72283905206835  # exp() of anything above overflows fp32

f64 = lambda a: np.asarray(a, np.float64)


def half_scale(amax):
    """gemm.hip:377-383, vectorised: 2^(14 - floor(log2 amax)), clamped as the biased exponent is (zero / denormal bound -> 2^126)."""
    amax = np.asarray(amax, np.float32)
    e = ((amax.view(np.uint32) >> 23) & 0xFF).astype(np.int64)
    s = np.clip(127 + 14 + 127 - e, 1, 253)
    return np.ldexp(1.0, (s - 127).astype(np.int64))


def amax(a, axis):
    return np.abs(np.asarray(a, np.float32)).max(axis=axis) if np.asarray(a).size else np.zeros(0, np.float32)


def plane_eps(a, scale):
    """mode 2: per element of a [R x K], the distance of (hi + lo) / s from a; scale [R] or a scalar."""
    a = np.abs(f64(a))
    s = np.broadcast_to(f64(scale), (a.shape[0],))[:, None]
    return np.where(a == 0, 0.0, np.maximum(2.0 ** -22 * a, 2.0 ** -25 / s))


def gemm(a, b, mode, scale_a=None, scale_b=None, bias=None, bf16_operands=False):
    """C = a b^T + bias in fp64 and its bound; a [M x K], b [N x K]; scale_*: half_scale of the prescribed bounds (mode 2).
    bf16_operands: the "bf16 forward" variant (eesen_net_set_forward_precision; gemm.hip: the nprod == 1 body) -- BOTH operands
    rounded to nearest-even bf16, which IS the statement (include/eesen_hip.h), so the value is round(a) round(b)^T + bias; a product
    of two 8-bit significands is exact in fp32, so there is no plane term and only mode 0's accumulation term remains, on the rounded
    operands.  The variant does not look at the GEMM mode: `mode` is ignored."""
    if bf16_operands:
        a, b, mode = round_bf16(a), round_bf16(b), 0
    a, b = f64(a), f64(b)
    K = a.shape[1]
    val = a @ b.T
    aa, ab = np.abs(a), np.abs(b)
    mag = aa @ ab.T
    bound = np.zeros_like(val)
    if mode == 2:
        bound += plane_eps(a, scale_a) @ ab.T + aa @ plane_eps(b, scale_b).T + C2 * mag
    elif mode == 1:
        bound += C1 * mag
    else:
        assert mode == 0
    if bias is not None:
        val = val + f64(bias)[None, :]
        mag = mag + np.abs(f64(bias))[None, :]
    return val, bound + (K + 3) * U * mag


def affine_forward(x, W, b, mode, x_bounded=False, bf16_operands=False):
    """affine-trans-layer.h:161-166.  x [rows x din], W [dout x din], b [dout]."""
    sx = half_scale(1.0) if x_bounded else half_scale(amax(x, 1))
    return gemm(x, W, mode, sx, half_scale(amax(W, 1)), b, bf16_operands)


def affine_in_diff(d, W, mode):
    """affine-trans-layer.h:168-172: d W.  d [rows x dout]."""
    return gemm(d, f64(W).T, mode, half_scale(amax(d, 1)), half_scale(amax(W, 0)))


def affine_grads(d, x, mode, x_bounded=False):
    """affine-trans-layer.h:174-219 (the gradients of Update): d^T x [dout x din] and the column sums of d, each with its bound."""
    sx = half_scale(1.0) if x_bounded else half_scale(amax(x, 0))
    gw, gw_b = gemm(f64(d).T, f64(x).T, mode, half_scale(amax(d, 0)), sx)
    d = f64(d)
    return gw, gw_b, d.sum(0), (d.shape[0] + 3) * U * np.abs(d).sum(0)


def sigmoid(x):
    x = f64(x)
    with np.errstate(over="ignore"):
        y = 1.0 / (1.0 + np.exp(-x))
    bound = y * (1.0 - y) * ULP_EXP * 2 * U + 2 * U * y + TINY
    sat = -x > LN_FLT_MAX          # (the cases keep every input 1e-3 away from the threshold: no expf error moves it across)
    return np.where(sat, 0.0, y), np.where(sat, 0.0, bound)


def tanh(x):
    y = np.tanh(f64(x))
    return y, (1.0 - y * y) / 2 * ULP_EXP * 2 * U + 3 * U * np.abs(y)


def sigmoid_diff(d, y):
    """in_diff from the layer's OUTPUT y (sigmoid-layer.h:48-51)."""
    d, y = f64(d), f64(y)
    v = d * (y * (1.0 - y))
    return v, 3 * U * np.abs(v) + TINY


def tanh_diff(d, y):
    d, y = f64(d), f64(y)
    f = 1.0 - y * y
    v = d * f
    return v, U * np.abs(d) * (y * y + np.abs(f)) + U * np.abs(v) + TINY


def tanh_diff_fma_bound(d, y):
    """What tanh_diff's bound shrinks to where 1 - y y is ONE fma (one rounding fewer): for the record, never asserted."""
    d, y = f64(d), f64(y)
    f = 1.0 - y * y
    return U * np.abs(d) * np.abs(f) + U * np.abs(d * f) + TINY


def softmax(x):
    """Rows of x [rows x K]."""
    x = f64(x)
    K = x.shape[1]
    m = x.max(1, keepdims=True)
    z = x - m
    e = np.exp(z)
    y = e / e.sum(1, keepdims=True)
    term = U * np.abs(z) + ULP_EXP * 2 * U
    with np.errstate(invalid="ignore", over="ignore"):
        den = np.where(y > 0, y * term, 0.0).sum(1, keepdims=True)       # (0 x a huge |z|: a class that has left the sum)
    rel = term + den + (-(-K // 64) + 8) * U
    return y, y * rel + TINY


def log_sub_prior(m, apply_log, log_prior, prior_scale):
    """net-output-extract.cc:103-112: (apply_log ? log m : m) - prior_scale log_prior[col]; logf within ULP_EXP ulps, the product and
    the sum one rounding each.  Without priors and without the log the matrix is untouched: bound 0."""
    m = f64(m)
    v = np.log(m) if apply_log else m.copy()
    bound = ULP_EXP * 2 * U * np.abs(v) if apply_log else np.zeros_like(v)
    if log_prior is not None:
        t = -float(np.float32(prior_scale)) * f64(log_prior)[None, :]
        v = v + t
        bound = bound + U * np.abs(t) + U * np.abs(v)
    return v, bound


# ------------------------------------------------------------------------------------------------------------ fp32 evaluations
# What the CPU test holds against the bounds: the same operations in numpy fp32 -- for the plane modes an emulation of gemm.hip's
# arithmetic (planes through numpy.float16 / bf16 truncation, the three or six products accumulated in fp32) -- and, with mutation=,
# evaluated WRONG on purpose.
GEMM_MUTATIONS = ("per_tensor_word", "wrong_axis", "stale_bound", "drop_hi_lo", "drop_lo_planes", "no_bias")


def _f16_planes(a, scale):
    s = np.asarray(scale, np.float64).astype(np.float32)
    a = np.asarray(a, np.float32) * (s[:, None] if s.ndim else s)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = a.astype(np.float16)
        lo = (a - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float32), lo.astype(np.float32)


def _bf16_trunc(a):
    return (np.asarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def gemm_fp32(a, b, mode, scale_a=None, scale_b=None, bias=None, mutation=None):
    """a b^T + bias as the device forms it, in numpy fp32.  scale_*: the scales to USE (the caller passes wrong ones to mutate them)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        if mode == 0:
            c = a @ b.T
        elif mode == 1:
            ah = _bf16_trunc(a); am = _bf16_trunc(a - ah); al = a - ah - am
            bh = _bf16_trunc(b); bm = _bf16_trunc(b - bh); bl = b - bh - bm
            c = ah @ bh.T + (ah @ bm.T + am @ bh.T) + (ah @ bl.T + al @ bh.T + am @ bm.T)
        else:
            ah, al = _f16_planes(a, scale_a)
            bh, bl = _f16_planes(b, scale_b)
            c = ah @ bh.T
            if mutation not in ("drop_hi_lo", "drop_lo_planes"):
                c = c + ah @ bl.T + al @ bh.T
            elif mutation == "drop_hi_lo":
                c = c + al @ bh.T                                    # one of the two cross products gone
            ia = (1.0 / np.asarray(scale_a, np.float64)).astype(np.float32)
            ib = (1.0 / np.asarray(scale_b, np.float64)).astype(np.float32)
            c = c * (ia[:, None] if ia.ndim else ia) * (ib[None, :] if ib.ndim else ib)
        if bias is not None and mutation != "no_bias":
            c = c + np.asarray(bias, np.float32)[None, :]
    return c.astype(np.float32)


def sigmoid_fp32(x):
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        return (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float32)


def tanh_fp32(x):
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(np.float32(2) * x)
        return np.where(np.isinf(e), np.float32(1), (e - np.float32(1)) / (e + np.float32(1))).astype(np.float32)


def softmax_fp32(x, mutation=None):
    """mutation: "no_max" (exp of the raw logits), "first_64" (the sum stops after one stride of the wave)."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        z = x if mutation == "no_max" else x - x.max(1, keepdims=True)
        e = np.exp(z)
        s = (e[:, :64] if mutation == "first_64" else e).sum(1, keepdims=True, dtype=np.float32)
        return (e / s).astype(np.float32)
