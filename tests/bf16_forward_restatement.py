"""Plain numpy fp64 restatement of ONE STEP of the "bf16 forward" recurrence (eesen_net_set_forward_precision(1):
lstm_fwd_persistent_bf_kernel<CPW,4,1,2,false>, eesen_amd/csrc/lstm_persistent.hip and lstm_fwd_bf_step.inc), every element of the gate
activations, the cell state c and the output m with an ABSOLUTE rounding bound, in the manner of tests/layer_restatement.py and
tests/lstm_gemm_restatement.py (whose gemm -- in its bf16_operands form --, shifted, gate_activation and ULP_HW are reused; the roundings
themselves are oracle.bf16_forward's round_bf16 / bf16_planes).  What tests/test_gpu_bf16_forward_fp64.py holds the kernel against; the
GEMM of the variant (gemm.hip: the nprod == 1 body) is layer_restatement.gemm(bf16_operands=True).

ONE STEP DEEP in m AND c: step t of sequence s is restated from the m and the c the DEVICE stored for the previous step (t - 1 forward,
t + 1 backward; zeros at the boundary and on padded frames, which is also what the kernel carries: lstm_fwd_bf_step.inc zeroes c and m
of a frame t >= len and keeps that c), so neither a rounding flip of m nor a drift of c travels down the chain.

    pre   = gx + round_bf16(m_prev) (hi + lo)^T        gx = round(x) round(W_x)^T + b (the variant's input GEMM, with ITS bound);
                                                       hi = round_bf16(W_m), lo = round_bf16(W_m - hi)  (bf16_planes(W_m, 2) = hi + lo)
    g     = tanh(pre_g)     i = sigmoid(pre_i + p_i c_prev)     f = sigmoid(pre_f + p_f c_prev)
    c     = g i + c_prev f  h = tanh(c)                         o = sigmoid(pre_o + p_o c)            m = h o
(bilstm-parallel-layer.h:116-148, in the kernel's order).  rec_round=False leaves m_prev and W_m unrounded: the fp32-class recurrence
that eesen_net_set_forward_precision(2) keeps.

Bounds, counted from the kernel's code; nothing is measured (ULP_HW is lstm_gemm_restatement's ASSUMED constant):
  * pre: gx's own bound, plus the recurrent sum's accumulation term (H + 3) 2^-24 (sum_k |m_r| (|hi| + |lo|) + |gx|).  The products
    are exact (8-bit significands).  A term passes through at most 64 CPW + 8 = H / 4 + 8 additions -- its wave's 2 CPW MFMAs of 32
    products each (lo plane first), then the eight additions of the waves' partial sums onto gx -- which (H + 3) covers at every
    admitted H >= 256; gx is one of the addends, hence its place in the magnitude (as the bias has in layer_restatement.gemm).  Plus
    2^-126 per product and addition for underflow;
  * a peephole argument pre + p c: the bound of pre, |p| times the bound of c, and TWO roundings (the product, the sum) -- where the
    compiler contracts to an fma there is one, inside this;
  * the gates: lstm_gemm_restatement.gate_activation of the argument known to within that bound;
  * c = g i + c_prev f: the gates' bounds through the products, and three roundings -- g i, c_prev f, the sum (with an fma one of the
    products does not round: inside this) -- of the magnitudes at their bounds; their second-order term; 2^-126 each for underflow;
  * h = tanh(c): gate_activation again, c known to within its bound;   m = h o: the two bounds through the product, one rounding.
Padded frames: 0 +- 0."""
import numpy as np

from oracle.bf16_forward import bf16_planes, round_bf16
from tests import layer_restatement as R
from tests import lstm_gemm_restatement as LR

U, FLUSH, f64 = R.U, LR.FLUSH, R.f64
QUANTITIES = ("gates", "c", "m")


def wm_planes(Wm):
    """(hi, lo) of W_m as the kernel holds it."""
    Wm = np.asarray(Wm, np.float32)
    hi = round_bf16(Wm)
    lo = round_bf16(Wm - hi)
    assert np.array_equal(hi + lo, bf16_planes(Wm, 2))
    return hi, lo


def _peephole(pre, pre_b, p, c, c_b):
    t = p * c
    t_b = np.abs(p) * c_b
    arg = pre + t
    return arg, pre_b + t_b + U * (np.abs(t) + t_b) + U * (np.abs(arg) + pre_b + t_b)


def step_restated(layer, x, lens, S, T, m_dev, c_dev, rec_round=True):
    """dict quantity -> (value, bound): gates [R x nd 4H], c, m [R x nd H], from the layer's input x [R x D] and the buffers m_dev, c_dev
    the device handed out (Net.DebugLayerBuffer 2 and 1)."""
    P = LR.unpack(layer)
    nd, H, rows = P["nd"], P["H"], S * T
    assert m_dev.shape == c_dev.shape == (rows, nd * H)
    gx, gx_b = LR.gemm(x, P["Wx"], 0, bias=P["b"], bf16_operands=True)
    live = LR.live_rows(lens, S, T)[:, None]
    out = {q: (np.zeros((rows, nd * (4 if q == "gates" else 1) * H)), np.zeros((rows, nd * (4 if q == "gates" else 1) * H))) for q in QUANTITIES}
    for dirn in range(nd):
        m_prev, c_prev = LR.shifted(m_dev, S, dirn, H), f64(LR.shifted(c_dev, S, dirn, H))
        if rec_round:
            hi, lo = wm_planes(P["Wm"][dirn])
            W, Wmag, m_r = f64(hi) + f64(lo), np.abs(f64(hi)) + np.abs(f64(lo)), f64(round_bf16(m_prev))
        else:
            W, m_r = f64(P["Wm"][dirn]), f64(m_prev)
            Wmag = np.abs(W)
        cols = slice(dirn * 4 * H, (dirn + 1) * 4 * H)
        g_x, g_xb = gx[:, cols], gx_b[:, cols]
        pre = g_x + m_r @ W.T
        pre_b = g_xb + (H + 3) * U * (np.abs(m_r) @ Wmag.T + np.abs(g_x) + g_xb) + FLUSH * 2 * (H + 3)
        blk = lambda a, k: a[:, k * H:(k + 1) * H]
        p_i, p_f, p_o = (f64(v)[None, :] for v in P["peep"][dirn])
        g, g_b = LR.gate_activation(blk(pre, 0), blk(pre_b, 0), True)
        i, i_b = LR.gate_activation(*_peephole(blk(pre, 1), blk(pre_b, 1), p_i, c_prev, 0.0), False)
        f, f_b = LR.gate_activation(*_peephole(blk(pre, 2), blk(pre_b, 2), p_f, c_prev, 0.0), False)
        GI, CF = (np.abs(g) + g_b) * (np.abs(i) + i_b), np.abs(c_prev) * (np.abs(f) + f_b)
        c = g * i + c_prev * f
        prop = GI - np.abs(g * i) + np.abs(c_prev) * f_b
        c_b = prop + U * (GI + CF) + U * (np.abs(c) + prop + U * (GI + CF)) + 3 * FLUSH
        h, h_b = LR.gate_activation(c, c_b, True)
        o, o_b = LR.gate_activation(*_peephole(blk(pre, 3), blk(pre_b, 3), p_o, c, c_b), False)
        HO = (np.abs(h) + h_b) * (np.abs(o) + o_b)
        m = h * o
        m_b = HO - np.abs(m) + U * HO + FLUSH
        for q, v, b, w in (("gates", np.hstack([g, i, f, o]), np.hstack([g_b, i_b, f_b, o_b]), 4 * H), ("c", c, c_b, H), ("m", m, m_b, H)):
            out[q][0][:, dirn * w:(dirn + 1) * w] = np.where(live, v, 0.0)
            out[q][1][:, dirn * w:(dirn + 1) * w] = np.where(live, b, 0.0)
    for q, (v, b) in out.items():
        assert np.isfinite(v).all() and np.isfinite(b).all(), q
    return out


def vacuous_share(pairs, lens, S, T):
    """Per sequence: the share of its live elements, over all the (value, bound) pairs given, whose bound exceeds |value| (where the
    comparison would pass a zero)."""
    live = LR.live_rows(lens, S, T)
    share = np.zeros(S)
    for s in range(S):
        r = live & (np.arange(S * T) % S == s)
        hits = [(b[r] > np.abs(v[r])) for v, b in pairs]
        share[s] = sum(h.sum() for h in hits) / sum(h.size for h in hits)
    return share


# ------------------------------------------------------------------------------------------------------------ fp32 evaluations
# What the CPU test holds against the bounds: the variant's arithmetic in numpy fp32 -- operands rounded to nearest even, fp32
# accumulation in k order, in 16-wide blocks as the MFMA takes them -- and, with mutation=, evaluated WRONG on purpose.
GEMM_MUTATIONS = ("truncated", "only_a_rounded", "only_b_rounded", "unrounded", "bf16_accumulator", "k_tail_dropped")
REC_MUTATIONS = ("wm_one_plane", "wm_unrounded", "m_unrounded", "m_truncated", "c_two_steps_back", "shifts_swapped",
                 # confined to ONE direction (the other is evaluated right): each direction's recurrent product must be within reach
                 "wm_one_plane_forward", "wm_one_plane_backward", "stale_m_backward", "no_product_backward")


def _acc16(a, b, acc=None, acc_round=None):
    """acc + a b^T in fp32, the k blocks of 16 in turn."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    acc = np.zeros((a.shape[0], b.shape[0]), np.float32) if acc is None else acc
    for k0 in range(0, a.shape[1], 16):
        acc = acc + a[:, k0:k0 + 16] @ b[:, k0:k0 + 16].T
        if acc_round is not None:
            acc = acc_round(acc)
    return acc


def gemm_fp32(a, b, bias=None, mutation=None):
    """round(a) round(b)^T + bias as gemm.hip's one-product body forms it, in numpy fp32."""
    assert mutation is None or mutation in GEMM_MUTATIONS
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    rnd = R._bf16_trunc if mutation == "truncated" else round_bf16
    ar = a if mutation in ("only_b_rounded", "unrounded") else rnd(a)
    br = b if mutation in ("only_a_rounded", "unrounded") else rnd(b)
    if mutation == "k_tail_dropped":
        K16 = a.shape[1] // 16 * 16
        ar, br = ar[:, :K16], br[:, :K16]
    with np.errstate(over="ignore", invalid="ignore"):
        c = _acc16(ar, br, acc_round=round_bf16 if mutation == "bf16_accumulator" else None)
        if bias is not None:
            c = c + np.asarray(bias, np.float32)[None, :]
    return c.astype(np.float32)


def layer_fp32(layer, x, lens, S, T, mutation=None):
    """The layer FREE-RUNNING in numpy fp32 with the variant's roundings: dict(gates, c, m) -- the CPU tests' stand-in for the buffers
    the device hands out."""
    assert mutation is None or mutation in REC_MUTATIONS
    P = LR.unpack(layer)
    nd, H, rows = P["nd"], P["H"], S * T
    gx = gemm_fp32(x, P["Wx"], P["b"])
    gates, c_all, m_all = np.zeros((rows, nd * 4 * H), np.float32), np.zeros((rows, nd * H), np.float32), np.zeros((rows, nd * H), np.float32)
    lens = np.asarray(lens)
    f1 = np.float32
    for dirn in range(nd):
        Wm = np.asarray(P["Wm"][dirn], np.float32)
        hi, lo = wm_planes(Wm)
        if mutation == "wm_one_plane" or mutation == ("wm_one_plane_forward", "wm_one_plane_backward")[dirn]:
            lo = np.zeros_like(lo)
        if mutation == "no_product_backward" and dirn == 1:
            hi, lo = np.zeros_like(hi), np.zeros_like(lo)
        p_i, p_f, p_o = (np.asarray(v, np.float32)[None, :] for v in P["peep"][dirn])
        cp, cpp, mp, mpp = (np.zeros((S, H), np.float32) for _ in range(4))
        fwd_order = (dirn == 0) != (mutation == "shifts_swapped")
        for t in (range(T) if fwd_order else range(T - 1, -1, -1)):
            r = slice(t * S, (t + 1) * S)
            m_kept = mp
            if mutation == "stale_m_backward" and dirn == 1:      # the first 32 cells' m from two steps back: one wave's block not yet replaced
                mp = np.hstack([mpp[:, :32], mp[:, 32:]])
            m_r = mp if mutation == "m_unrounded" else R._bf16_trunc(mp) if mutation == "m_truncated" else round_bf16(mp)
            rec = _acc16(m_r, Wm) if mutation == "wm_unrounded" else _acc16(m_r, hi, _acc16(m_r, lo))
            pre = gx[r, dirn * 4 * H:(dirn + 1) * 4 * H] + rec
            c_in = cpp if mutation == "c_two_steps_back" else cp
            g = LR.tanh_dev_fp32(pre[:, :H])
            i = LR.sigmoid_dev_fp32(pre[:, H:2 * H] + p_i * c_in)
            f = LR.sigmoid_dev_fp32(pre[:, 2 * H:3 * H] + p_f * c_in)
            c = (g * i + c_in * f).astype(f1)
            h = LR.tanh_dev_fp32(c)
            o = LR.sigmoid_dev_fp32(pre[:, 3 * H:] + p_o * c)
            m = (h * o).astype(f1)
            live = (t < lens)[:, None]
            g, i, f, o, c, m = (np.where(live, v, f1(0)) for v in (g, i, f, o, c, m))
            gates[r, dirn * 4 * H:(dirn + 1) * 4 * H] = np.hstack([g, i, f, o])
            c_all[r, dirn * H:(dirn + 1) * H], m_all[r, dirn * H:(dirn + 1) * H] = c, m
            cpp, cp, mpp, mp = cp, c, m_kept, m
    return dict(gates=gates, c=c_all, m=m_all)
