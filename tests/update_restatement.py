"""Plain numpy restatements of the three update rules of csrc/optim.hip (sgd_update_kernel, adaptive_update_kernel) and of MomentStatistics
(tensor_moments_kernel), each value with an ABSOLUTE rounding bound per element.

The rules, operation for operation as optim.hip and the reference state them (bilstm-layer.h:846-955, trainable-layer.h:65-114):
    c  = mmt * c_prev + g                      the momentum fold
    c  = clip(c, +-max_grad)  if max_grad > 0
    SGD:      p -= (lr * coef) * c
    Adagrad:  a += c^2                          RMSProp:  a = rho * a + (1 - rho) * c^2
    both:     p -= lr * c / sqrt(a + eps)       (learn_rate_coef is NOT applied)
Every constant is first rounded to fp32, as the C-ABI carries it; lr * coef and 1 - rho are formed in fp32 (Net::update, capi.cpp).

The bounds are DERIVED, first order, with u = 2^-24 per fp32 operation -- nothing in them is measured:
  * a * b + c evaluated fused (one rounding, u |a b + c|) or unfused (u |a b| + u |a b + c|): both inside 2 u max(|a b|, |a b + c|);
  * the clip is exact, and 1-Lipschitz: it never widens a bound, and where |c| passes max_grad by more than its bound the result is
    +-max_grad bit for bit (bound 0);
  * corr: 2 u max(|mmt c_prev|, |c|);
  * accu: 8 u |a'| (c^2, the two products, the sum: at most 4 roundings of positive terms; the rest is margin);
  * SGD parameter: 2 u max(|lr coef c|, |p'|);
  * adaptive parameter, step = lr c / sqrt(a' + eps): 32 u |step| + 2 u |p'|.  First-order count of the step: a' (4 u -> 2 u through the
    root), + eps (u / 2), sqrtf and the reciprocal (2 ulp each allowed on the device), the two products (2 u): about 8 u; with the error
    of a' taken at its full 8 u bound, 16 u.  The factor is doubled to 32 as the margin for the non-IEEE device sqrt and reciprocal;
  * plus, for every quantity, the bounds of its inputs propagated to first order: mmt dc_prev into corr; (lr coef) dc + dp into the SGD
    parameter; 2 k |c| dc + k_a da into accu (k, k_a the rule's weights); |d step / dc| dc + |step| da / (2 (a' + eps)) + dp into the
    adaptive parameter, where dc here is the bound of c just derived (the fold's own rounding reaches a' and the step too).

mutation=: the restatement evaluated WRONG on purpose, to show that the bounds reject it (tests/test_update_restatement.py part c)."""
import numpy as np

U = 2.0 ** -24
MUTATIONS = ("clip_before_momentum", "accu_from_unclipped", "rho_swapped", "eps_outside_sqrt", "coef_in_adaptive", "momentum_0.8", "no_clip")


def constants(lr, mmt, eps=1e-6, rho=0.9):
    """The scalars as the library holds them: fp32 each, 1 - rho formed in fp32 (eesen_net_set_adaptive_options)."""
    rho32 = np.float32(rho)
    return dict(lr=np.float32(lr), mmt=np.float32(mmt), eps=np.float32(eps), rho=rho32, one_minus_rho=np.float32(1.0) - rho32)


def _clip(c, mg):
    return np.where(mg > 0, np.minimum(np.maximum(c, -mg), mg), c)


def update(rule, p, c_prev, g, a, coef, max_grad, k, dtype=np.float64, mutation=None, dp=0.0, dc_prev=0.0, da=0.0):
    """One step of `rule` on flat arrays; coef and max_grad per element (fp32 values), k = constants(...).
    Returns dict(p, corr, accu, p_bound, corr_bound, accu_bound, step, surely_clipped); accu / accu_bound are None under SGD.
    dtype=np.float32 evaluates every operation in fp32, unfused, in the kernel's order (what part b holds against the bounds)."""
    assert rule in ("SGD", "Adagrad", "RMSProp") and (mutation is None or mutation in MUTATIONS)
    t = dtype
    p, c_prev, g = (np.asarray(x, np.float32).astype(t) for x in (p, c_prev, g))
    mg = np.asarray(max_grad, np.float32).astype(t)
    lr, mmt, eps, rho, omr = (t(k[n]) for n in ("lr", "mmt", "eps", "rho", "one_minus_rho"))
    lr_coef = (np.float32(k["lr"]) * np.asarray(coef, np.float32)).astype(t)      # fp32 product (Net::update: lr * L.coef)
    if mutation == "momentum_0.8":
        mmt = t(np.float32(0.8))
    if mutation == "clip_before_momentum":
        raw = mmt * c_prev + _clip(g, mg)
        c = raw
    else:
        raw = mmt * c_prev + g
        c = raw if mutation == "no_clip" else _clip(raw, mg)
    # ---- bounds (always in fp64, from the values just computed)
    f = lambda x: np.asarray(x, np.float64)
    raw_b = 2 * U * np.maximum(np.abs(f(mmt) * f(c_prev)), np.abs(f(raw))) + abs(float(mmt)) * f(dc_prev)
    surely = (f(mg) > 0) & (np.abs(f(raw)) - f(mg) > raw_b)
    c_b = np.where(surely, 0.0, raw_b)
    out = dict(corr=c, corr_bound=c_b, surely_clipped=surely, accu=None, accu_bound=None)
    if rule == "SGD":
        stepv = lr_coef * c
        pn = p - stepv
        out.update(p=pn, step=stepv, p_bound=2 * U * np.maximum(np.abs(f(stepv)), np.abs(f(pn))) + np.abs(f(lr_coef)) * c_b + f(dp))
        return out
    a = np.asarray(a, np.float32).astype(t)
    g2 = (raw * raw) if mutation == "accu_from_unclipped" else (c * c)
    if rule == "RMSProp":
        ka, kc = (omr, rho) if mutation == "rho_swapped" else (rho, omr)
        an = ka * a + kc * g2
    else:
        ka, kc = t(1), t(1)
        an = a + g2
    root = (np.sqrt(an) + eps) if mutation == "eps_outside_sqrt" else np.sqrt(an + eps)
    scale = t(1) / root
    lr_e = lr_coef if mutation == "coef_in_adaptive" else lr
    stepv = lr_e * scale * c
    pn = p - stepv
    s2 = f(an) + float(eps)
    a_b = 8 * U * np.abs(f(an)) + 2 * float(kc) * np.abs(f(c)) * c_b + float(ka) * f(da)
    dstep_dc = float(lr) / np.sqrt(s2) * (1.0 + float(kc) * f(c) ** 2 / s2)
    p_b = (32 * U * np.abs(f(stepv)) + 2 * U * np.abs(f(pn)) + dstep_dc * c_b + np.abs(f(stepv)) * float(ka) * f(da) / (2 * s2) + f(dp))
    out.update(p=pn, step=stepv, accu=an, p_bound=p_b, accu_bound=a_b)
    return out


# ------------------------------------------------------------------------------------------------------------ MomentStatistics
EPS64 = 2.0 ** -52


def moments(x):
    """MomentStatistics (utils-functions.h:50-82) of the fp32 entries `x`, in fp64, in the reference's two-pass form: mean; then the
    central power sums about THAT mean; variance = S2 / n, skewness = S3 / variance^1.5 / n, kurtosis = S4 / variance^2 / n - 3.
    Returns (values[6], bounds[6]) in the order min, max, mean, variance, skewness, kurtosis.  min and max are exact (bound 0).  The
    others carry the bound of an fp64 reduction in ANOTHER order -- n 2^-52 times the sum of the absolute values of the terms -- taken
    through the normalisers to first order, with the error of the mean propagated into every central sum (d/dmean of sum e^k is
    k sum e^(k-1)) and that of the variance into the two ratios.  A constant tensor has variance 0: skewness and kurtosis are 0 / 0 = NaN,
    and so are their bounds."""
    v = np.asarray(x, np.float32).astype(np.float64).ravel()
    n = v.size
    ne = n * EPS64
    mean = v.sum() / n
    d_mean = ne * np.abs(v).sum() / n + EPS64 * abs(mean)
    e = v - mean
    ae = np.abs(e)
    d_e = d_mean + EPS64 * ae                       # per element: the mean's error and the subtraction's rounding
    s2, s3, s4 = (e ** 2).sum(), (e ** 3).sum(), (e ** 4).sum()
    d_s2 = (ne + 4 * EPS64) * s2 + 2 * (ae * d_e).sum()
    d_s3 = (ne + 6 * EPS64) * (ae ** 3).sum() + 3 * (ae ** 2 * d_e).sum()
    d_s4 = (ne + 8 * EPS64) * s4 + 4 * (ae ** 3 * d_e).sum()
    var = s2 / n
    d_var = d_s2 / n + EPS64 * var
    with np.errstate(divide="ignore", invalid="ignore"):
        skew = np.float64(s3) / np.float64(var) ** 1.5 / n
        k3 = np.float64(s4) / (np.float64(var) * var) / n
        kurt = k3 - 3.0
        d_skew = d_s3 / np.float64(var) ** 1.5 / n + abs(skew) * (1.5 * d_var / var + 8 * EPS64)       # (pow: a few ulp on any libm)
        d_kurt = d_s4 / (np.float64(var) * var) / n + abs(k3) * (2 * d_var / var + 4 * EPS64) + EPS64 * abs(kurt)
    return (np.array([v.min(), v.max(), mean, var, skew, kurt]), np.array([0.0, 0.0, d_mean, d_var, d_skew, d_kurt]))
