"""Plain numpy fp64 restatements of the dense GEMMs and reductions AROUND an LSTM layer -- the input->gates GEMM, the input gradient, the
W_x and W_m gradients, the bias and peephole reductions -- each value with an ABSOLUTE rounding bound per element, in the manner of
tests/layer_restatement.py (whose gemm, half_scale, plane_eps and gemm_fp32 are reused).  What tests/test_gpu_lstm_gemms.py holds
Net::forward_pass / Net::backpropagate_impl (csrc/net.cpp), gemm.hip and lstm.hip::lstm_bias_peep_pass1/2 against, under all three
GEMM modes, with the operand bounds Net itself chooses.  The recurrences are NOT restated here (tests/test_gpu_recurrence_*.py hold
them): the backward quantities are restated from the buffers the device handed out through eesen_net_debug_layer_buffer -- the gate
gradients DG, the output m, the cell state c, bit for bit -- and from the case's x and parameters.

Column order everywhere: the model file's.  Gate matrices [rows x ndir 4H]: per direction the blocks g, i, f, o of H columns (the order
of the W_x rows); state matrices [rows x ndir H].  Row t S + s.

The operations (bilstm-parallel-layer.h; net.cpp backpropagate_impl), and the bounds Net prescribes for mode 2 (two fp16 planes):
    G        = x W_x^T + b            one GEMM over both directions       (rows of x | the word 1.0 behind an LSTM layer without forward
                                                                           dropout,  rows of W_x -- the backward direction's 4H further on)
    in_diff  = DG W_x                 K = ndir 4H                          (rows of DG,  columns of W_x)
    W_x grad = DG^T x                 K = rows (split-K from 2048)         (columns of DG,  columns of x | the word 1.0)
    W_m grad = DG_dir^T m_shifted     per direction; m one frame toward    (the direction's own 4H of the DG column bounds,  the word 1.0)
                                      the recurrence's source, 0 at the boundary
    b grad   = column sums of DG;   peephole grads = column sums of d_i c', d_f c', d_o c   (c' = c one frame toward the source)
The GEMM bound is layer_restatement.gemm's (its K term covers any summation order, split-K included) PLUS an underflow term, which the
Affine cases avoid by construction and these cannot: a gate that is all but closed (sigmoid(-80) ~ 2^-115) leaves gate gradients down
to the denormals.  An fp32 operation whose result falls below 2^-126 loses at most 2^-126 (FLUSH; less where denormals are kept): an
operand element (or, in mode 1, one of its three planes) read as 0 costs 2^-126 |the other factor|, each of the K products and each
accumulation 2^-126, and the mode-2 epilogue, which multiplies the accumulator by the row's inverse power BEFORE the column's
(gemm_epilogue: acc * inv[row] * inv[col]), 2^-126 times the column's inverse power:
    n 2^-126 (sum_k |a| + sum_k |b| + 2 K) + 2^-126 (3 + 1 / s_b[column] in mode 2),   n = 3 in mode 1, else 1.
It is some 2^-95 at the largest operands of these cases: nothing a value of interest notices.

Bias / peephole reductions (lstm_bias_peep_pass1/2): per row block of ceil(R / 64) rows four strided chains of ceil(ceil(R / 64) / 4)
additions, the LDS fold of the four (3), the 64 blocks (64), and the product d c (1): every term passes through at most that many
roundings, so the sum is within  (ceil(ceil(R / 64) / 4) + 3 + 64 + 1 + 1) 2^-24 sum |d c|  (+ 1: the second-order terms), plus
2^-126 per term and addition for underflow (as above).

The forward GEMM is observed THROUGH the gates: with W_m = 0 and zero peepholes every step's pre-activation is exactly G (the recurrent
product adds exact zeros), and the gate activations that overwrite G are g = tanh(G), i, f, o = sigmoid(G) -- 0 on padded frames.
Device formulas (lstm.hip / lstm_persistent.hip: sigmoidf_, tanhf_), e = __expf(z) = v_exp_f32(z log2 e):
    sigmoid(x) = rcp(1 + e),  z = -x;        tanh(x) = 1 - 2 rcp(1 + e),  z = 2x.
ULP_HW = 1 ulp each for v_exp_f32 and v_rcp_f32 is an ASSUMPTION: it is the figure of the project's own comment in lstm.hip, not one
read off an ISA accuracy table.  Counting: e^ = e (1 + de), |de| <= ULP_HW 2^-23 + 2 2^-24 |z| (the instruction; the product z log2 e
and the rounded constant, each moving the exponent by 2^-24 |z log2 e| ln 2);  s = fl(1 + e): 2^-24;  rcp: ULP_HW 2^-23.  With
r = 1 / (1 + e) and e / (1 + e) = 1 - r:  r^ = r (1 + eta), |eta| <= (1 - r) de + 2^-24 + ULP_HW 2^-23.  Hence
    sigmoid: y = r:        y (1 - y) de + y (1 + 2 ULP_HW) 2^-24  + 2^-126 (a denormal quotient may be flushed)
    tanh:    y = 1 - 2 r:  (1 - y^2) / 2 de + (1 - y) (1 + 2 ULP_HW) 2^-24 + 2^-24 |y|   (2 r is exact; the difference, or the fma, rounds once)
Both saturate exactly where e is inf or 0, inside these bounds.  The gate's bound for a pre-activation known to within b:
|f^(G^) - f(G)| <= sup |f'| b + the activation term at G^: f' is even and falls with |x|, so the supremum over [G - b, G + b] is f' at
the point nearest 0; the activation term is taken with every factor at its worst point of that interval."""
import numpy as np

from tests import layer_restatement as R

U = R.U
ULP_HW = 1.0                    # ASSUMED (see above): ulps of v_exp_f32 and of v_rcp_f32
FLUSH = 2.0 ** -126             # the smallest normal fp32: what a flushed denormal loses at most
RED_RB = 64                     # row blocks of lstm_bias_peep_pass1
f64 = R.f64
hs, am = R.half_scale, R.amax

MUTATIONS = R.GEMM_MUTATIONS + ("fw_rows_for_bw", "dir0_cols_for_dir1", "word_for_measured", "unshifted_m", "peephole_shift_swapped")


# ------------------------------------------------------------------------------------------------------------ the layer's tensors
def unpack(layer):
    """dict(nd, H, D, Wx [nd 4H x D], Wm [nd][4H x H], b [nd 4H], peep [nd][3][H]) of a (Bi)LstmParallel layer dict."""
    nd = 2 if layer["type"].startswith("BiLstm") else 1
    p = layer["params"]
    assert len(p) == 6 * nd
    H, D = p[3].size, layer["input_dim"]
    return dict(nd=nd, H=H, D=D, Wx=np.vstack([p[6 * d].reshape(4 * H, D) for d in range(nd)]), Wm=[p[6 * d + 1].reshape(4 * H, H) for d in range(nd)],
                b=np.concatenate([p[6 * d + 2].ravel() for d in range(nd)]), peep=[[p[6 * d + 3 + k].ravel() for k in range(3)] for d in range(nd)])


def shifted(a, S, dirn, H, like_dir=None):
    """Columns of direction dirn of a state matrix [T S x nd H], one frame toward the recurrence's source (t - 1 forward, t + 1 backward),
    zeros at the boundary.  like_dir: shift as THAT direction would (the mutations)."""
    blk = np.asarray(a)[:, dirn * H:(dirn + 1) * H]
    out = np.zeros_like(blk)
    if (dirn if like_dir is None else like_dir) == 0:
        out[S:] = blk[:-S]
    else:
        out[:-S] = blk[S:]
    return out


def live_rows(lens, S, T):
    return (np.arange(T)[:, None] < np.asarray(lens)[None, :]).reshape(T * S)


# ------------------------------------------------------------------------------------------------------------ a plain recurrence
def _sig(a):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-a))


def recurrence(layer, x, lens, S, T, d=None, dtype=np.float32):
    """The layer in plain fp64 numpy (bilstm-parallel-layer.h:109-204, 461-600; padded frames give zeros): dict(gates, c, m[, DG]) as
    `dtype`.  The CPU tests' stand-in for the buffers the device hands out; d: the gradient of m."""
    P = unpack(layer)
    nd, H = P["nd"], P["H"]
    rows = S * T
    pre = f64(x) @ f64(P["Wx"]).T + f64(P["b"])[None, :]
    gates, c, m = np.zeros((rows, nd * 4 * H)), np.zeros((rows, nd * H)), np.zeros((rows, nd * H))
    lens = np.asarray(lens)
    for dirn in range(nd):
        Wm, (pi, pf, po) = f64(P["Wm"][dirn]), (f64(v) for v in P["peep"][dirn])
        cp, mp = np.zeros((S, H)), np.zeros((S, H))
        for t in (range(T) if dirn == 0 else range(T - 1, -1, -1)):
            r = slice(t * S, (t + 1) * S)
            a = pre[r, dirn * 4 * H:(dirn + 1) * 4 * H] + mp @ Wm.T
            g, i, f = np.tanh(a[:, :H]), _sig(a[:, H:2 * H] + pi * cp), _sig(a[:, 2 * H:3 * H] + pf * cp)
            cc = g * i + cp * f
            o = _sig(a[:, 3 * H:] + po * cc)
            live = (t < lens)[:, None]
            g, i, f, o, cc = (np.where(live, v, 0.0) for v in (g, i, f, o, cc))
            mm = o * np.tanh(cc)
            gates[r, dirn * 4 * H:(dirn + 1) * 4 * H] = np.hstack([g, i, f, o])
            c[r, dirn * H:(dirn + 1) * H], m[r, dirn * H:(dirn + 1) * H] = cc, mm
            cp, mp = cc, mm
    out = dict(gates=gates.astype(dtype), c=c.astype(dtype), m=m.astype(dtype))
    if d is None:
        return out
    DG = np.zeros((rows, nd * 4 * H))
    d = f64(d)
    for dirn in range(nd):
        Wm, (pi, pf, po) = f64(P["Wm"][dirn]), (f64(v) for v in P["peep"][dirn])
        cs = shifted(c, S, dirn, H)
        dgn, carry = np.zeros((S, 4 * H)), np.zeros((S, H))
        for t in (range(T - 1, -1, -1) if dirn == 0 else range(T)):
            r = slice(t * S, (t + 1) * S)
            G = gates[r, dirn * 4 * H:(dirn + 1) * 4 * H]
            g, i, f, o = (G[:, k * H:(k + 1) * H] for k in range(4))
            ct, cprev = c[r, dirn * H:(dirn + 1) * H], cs[r]
            dm = d[r, dirn * H:(dirn + 1) * H] + dgn @ Wm
            h = np.tanh(ct)
            do = o * (1 - o) * (dm * h)
            dc = (1 - h * h) * (dm * o) + carry + dgn[:, H:2 * H] * pi + dgn[:, 2 * H:3 * H] * pf + do * po
            live = (t < lens)[:, None]
            dgn = np.where(live, np.hstack([(1 - g * g) * (dc * i), i * (1 - i) * (dc * g), f * (1 - f) * (dc * cprev), do]), 0.0)
            carry = np.where(live, dc * f, 0.0)
            DG[r, dirn * 4 * H:(dirn + 1) * 4 * H] = dgn
    out["DG"] = DG.astype(dtype)
    return out


def gemm(a, b, mode, scale_a=None, scale_b=None, bias=None, bf16_operands=False):
    """layer_restatement.gemm plus the underflow term of the module docstring (bf16_operands: of the ROUNDED operands, one plane)."""
    val, bound = R.gemm(a, b, mode, scale_a, scale_b, bias, bf16_operands)
    if bf16_operands:
        a, b, mode = R.round_bf16(a), R.round_bf16(b), 0
    n = 3 if mode == 1 else 1
    uf = n * (np.abs(f64(a)).sum(1)[:, None] + np.abs(f64(b)).sum(1)[None, :] + 2 * f64(a).shape[1]) + 3
    if mode == 2:
        uf = uf + (1.0 / np.broadcast_to(f64(scale_b), (f64(b).shape[0],)))[None, :]
    return val, bound + FLUSH * uf


# ------------------------------------------------------------------------------------------------------------ the scales of mode 2
def prescribed_scales(P, x, DG, x_bounded):
    """half_scale of the bounds net.cpp prescribes for the layer's GEMMs.  x_bounded: the layer reads an LSTM layer's output without
    forward dropout (the word 1.0 in place of the x vectors)."""
    s = dict(fwd_a=hs(1.0) if x_bounded else hs(am(x, 1)), fwd_b=hs(am(P["Wx"], 1)))
    if DG is not None:
        s.update(in_a=hs(am(DG, 1)), in_b=hs(am(P["Wx"], 0)), wx_a=hs(am(DG, 0)), wx_b=hs(1.0) if x_bounded else hs(am(x, 0)),
                 wm_a=hs(am(DG, 0)), wm_b=hs(1.0))
    return s


# ------------------------------------------------------------------------------------------------------------ backward quantities
def reduction_depth(R_rows):
    rows_per = -(-R_rows // RED_RB)
    return -(-rows_per // 4) + 3 + RED_RB + 1


def col_reduction(terms):
    """Column sums of terms [R x n] as lstm_bias_peep_pass1/2 form them: (value, bound)."""
    t = f64(terms)
    return t.sum(0), (reduction_depth(t.shape[0]) + 1) * U * np.abs(t).sum(0) + FLUSH * (t.shape[0] + reduction_depth(t.shape[0]))


def peephole_terms(P, DG, c, S, dirn, swapped=False):
    """[d_i c', d_f c', d_o c] of one direction, each [R x H]; swapped: c' shifted the way the OTHER direction's is (the mutation)."""
    H = P["H"]
    d = f64(DG)[:, dirn * 4 * H:(dirn + 1) * 4 * H]
    cs = f64(shifted(c, S, dirn, H, 1 - dirn if swapped else dirn))
    ct = f64(c)[:, dirn * H:(dirn + 1) * H]
    return [d[:, H:2 * H] * cs, d[:, 2 * H:3 * H] * cs, d[:, 3 * H:] * ct]


def backward_restated(layer, x, DG, m, c, S, mode, x_bounded):
    """dict quantity -> (value, bound): in_diff [R x D]; Wx_grad [nd 4H x D]; Wm_grad<dir> [4H x H]; b_grad [nd 4H]; peep_grad<dir> [3 x H]."""
    P = unpack(layer)
    nd, H = P["nd"], P["H"]
    s = prescribed_scales(P, x, DG, x_bounded)
    out = dict(in_diff=gemm(DG, f64(P["Wx"]).T, mode, s["in_a"], s["in_b"]),
               Wx_grad=gemm(f64(DG).T, f64(x).T, mode, s["wx_a"], s["wx_b"]),
               b_grad=col_reduction(DG))
    for dirn in range(nd):
        cols = slice(dirn * 4 * H, (dirn + 1) * 4 * H)
        out[f"Wm_grad{dirn}"] = gemm(f64(DG)[:, cols].T, f64(shifted(m, S, dirn, H)).T, mode, s["wm_a"][cols], s["wm_b"])
        v, b = zip(*(col_reduction(t) for t in peephole_terms(P, DG, c, S, dirn)))
        out[f"peep_grad{dirn}"] = (np.stack(v), np.stack(b))
    for q, (v, bnd) in out.items():     # nothing comes near the top of the fp32 range
        assert np.isfinite(v).all() and (np.abs(v) + bnd).max() < 2.0 ** 100, q
    return out


def grads_by_quantity(layer, flat):
    """The layer's gradients in Net::GetGrads order (per direction W_x, W_m, bias, p_i, p_f, p_o) -> the quantities above."""
    P = unpack(layer)
    nd, H, D = P["nd"], P["H"], P["D"]
    flat = np.asarray(flat)
    assert flat.size == nd * (4 * H * D + 4 * H * H + 7 * H)
    out, i, wx, b = {}, 0, [], []
    for dirn in range(nd):
        wx.append(flat[i:i + 4 * H * D].reshape(4 * H, D)); i += 4 * H * D
        out[f"Wm_grad{dirn}"] = flat[i:i + 4 * H * H].reshape(4 * H, H); i += 4 * H * H
        b.append(flat[i:i + 4 * H]); i += 4 * H
        out[f"peep_grad{dirn}"] = flat[i:i + 3 * H].reshape(3, H); i += 3 * H
    out["Wx_grad"], out["b_grad"] = np.vstack(wx), np.concatenate(b)
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------------------ the gates
def _exp_err(zmax):
    return ULP_HW * 2 * U + 2 * U * zmax


def gate_activation(G, b, tanh):
    """f(G) and its bound for a pre-activation the device knows to within b (see the module docstring)."""
    G, b = f64(G), f64(b)
    near = np.sign(G) * np.maximum(np.abs(G) - b, 0.0)           # the point of [G - b, G + b] nearest 0
    zmax = (np.abs(G) + b) * (2.0 if tanh else 1.0)
    k = (1 + 2 * ULP_HW) * U
    if tanh:
        y, yn, ylo = np.tanh(G), np.tanh(near), np.tanh(G - b)
        return y, (1 - yn * yn) * b + (1 - yn * yn) / 2 * _exp_err(zmax) + (1 - ylo) * k + U
    y, yn, yhi = _sig(G), _sig(near), _sig(G + b)
    return y, yn * (1 - yn) * b + yn * (1 - yn) * _exp_err(zmax) + yhi * k + FLUSH


def gates_restated(layer, x, lens, S, T, mode, x_bounded, bf16_operands=False):
    """The gate activations of a layer whose W_m and peepholes are zero: (value, bound, G, bound of G), each [R x nd 4H]; padded frames
    0 +- 0.  bf16_operands: the GEMM of the bf16 forward variant (layer_restatement.gemm)."""
    P = unpack(layer)
    assert all(not np.any(w) for w in P["Wm"]) and all(not np.any(v) for d in P["peep"] for v in d), "the layer is not neutralised"
    s = prescribed_scales(P, x, None, x_bounded)
    G, Gb = gemm(x, P["Wx"], mode, s["fwd_a"], s["fwd_b"], P["b"], bf16_operands)
    assert np.isfinite(G).all() and (np.abs(G) + Gb).max() < 2.0 ** 100
    H, nd = P["H"], P["nd"]
    val, bound = np.zeros_like(G), np.zeros_like(G)
    for dirn in range(nd):
        for q in range(4):
            cols = slice(dirn * 4 * H + q * H, dirn * 4 * H + (q + 1) * H)
            val[:, cols], bound[:, cols] = gate_activation(G[:, cols], Gb[:, cols], q == 0)
    live = live_rows(lens, S, T)[:, None]
    return np.where(live, val, 0.0), np.where(live, bound, 0.0), G, Gb


# ------------------------------------------------------------------------------------------------------------ fp32 evaluations
def sigmoid_dev_fp32(x):
    """sigmoidf_ in numpy fp32 (exp and the quotient correctly rounded: inside the device's ULP_HW)."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        return (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float32)


def tanh_dev_fp32(x):
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        return (np.float32(1) - np.float32(2) * (np.float32(1) / (np.float32(1) + np.exp(np.float32(2) * x)))).astype(np.float32)


def gates_fp32(P, G32, lens, S, T):
    H, nd = P["H"], P["nd"]
    out = np.zeros_like(G32)
    for dirn in range(nd):
        for q in range(4):
            cols = slice(dirn * 4 * H + q * H, dirn * 4 * H + (q + 1) * H)
            out[:, cols] = (tanh_dev_fp32 if q == 0 else sigmoid_dev_fp32)(G32[:, cols])
    return np.where(live_rows(lens, S, T)[:, None], out, np.float32(0))


def col_reduction_fp32(terms32):
    """lstm_bias_peep_pass1/2's shape in numpy fp32: 64 row blocks, four strided partial sums each, the fold, the blocks."""
    t = np.asarray(terms32, np.float32)
    Rr = t.shape[0]
    rows_per = -(-Rr // RED_RB)
    tot = np.zeros(t.shape[1], np.float32)
    for rb in range(RED_RB):
        blk = t[rb * rows_per:min(Rr, (rb + 1) * rows_per)]
        ch = [blk[k::4].sum(0, dtype=np.float32) if blk[k::4].size else np.zeros(t.shape[1], np.float32) for k in range(4)]
        tot = tot + (((ch[0] + ch[1]) + ch[2]) + ch[3])
    return tot
