"""CPU: what tests/test_gpu_update_rules.py and tests/test_gpu_tensor_moments.py hold the kernels of csrc/optim.hip against.
  (a) the fp64 restatement (tests/update_restatement.py) equals orc_sgd_update / orc_adaptive_update of the oracle's f64 build;
  (b) a numpy fp32 evaluation of the unmutated rules stays inside the restatement's DERIVED bounds, on the very inputs of the GPU tests
      (tests/update_cases.py);
  (c) every mutation of the rules leaves those bounds on at least 1 % of the elements of the same inputs -- the GPU test has teeth.
The bounds come from counting roundings (module docstring of the restatement); nothing in them was fitted to an observed error."""
import ctypes as C

import numpy as np
import pytest

from tests import update_cases as UC
from tests import update_restatement as R

# which rules a mutation is visible under
APPLIES = {"clip_before_momentum": UC.RULES, "momentum_0.8": UC.RULES, "no_clip": UC.RULES, "accu_from_unclipped": ("Adagrad", "RMSProp"),
           "eps_outside_sqrt": ("Adagrad", "RMSProp"), "coef_in_adaptive": ("Adagrad", "RMSProp"), "rho_swapped": ("RMSProp",)}


def two_steps(name, rule):
    """The inputs of both steps of the GPU two-step test with the fp64 restatement of each: step 2 starts from what the device would
    hold after step 1 -- c1 = clip(g0) exactly, p and accu rounded to fp32."""
    inp = UC.two_step_inputs(name)
    L = inp["layers"]
    zero = np.zeros_like(inp["p0"])
    s1 = dict(p=inp["p0"], c_prev=zero, g=inp["g"][0], a=inp["a0"])
    r1 = UC.restate(L, rule, **s1)
    assert np.array_equal(r1["corr"].astype(np.float32), UC.clip_exact(L, inp["g"][0]))
    s2 = dict(p=r1["p"].astype(np.float32), c_prev=r1["corr"].astype(np.float32), g=inp["g"][1],
              a=inp["a0"] if rule == "SGD" else r1["accu"].astype(np.float32))
    return L, [(s1, r1), (s2, UC.restate(L, rule, **s2))]


def _quantities(rule):
    return ("p", "corr") if rule == "SGD" else ("p", "corr", "accu")


@pytest.mark.parametrize("rule", UC.RULES)
def test_restatement_equals_the_f64_oracle(rule):
    from oracle import cbind
    lib = cbind.load("f64")
    k = R.constants(**UC.HYPER)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    d = C.c_double
    for name in ("layers3", "padded"):
        layers, steps = two_steps(name, rule)
        for s, r in steps:
            p, a = s["p"].astype(np.float64), s["a"].astype(np.float64)
            c = float(k["mmt"]) * s["c_prev"].astype(np.float64) + s["g"].astype(np.float64)     # the fold lives in the oracle's gradient GEMMs
            i = 0
            for Lyr, n in zip(layers, UC.layer_sizes(layers)):
                pp, cc, aa = (np.ascontiguousarray(x[i:i + n]) for x in (p, c, a))
                mg = d(float(np.float32(Lyr["max_grad"])))
                if rule == "SGD":
                    lib.orc_sgd_update(C.c_long(n), ptr(pp), ptr(cc), d(float(k["lr"] * np.float32(Lyr["learn_rate_coef"]))), mg)
                else:
                    lib.orc_adaptive_update(C.c_long(n), ptr(pp), ptr(cc), ptr(aa), d(float(k["lr"])), mg, d(float(k["eps"])), d(float(k["rho"])),
                                            d(float(k["one_minus_rho"])), int(rule == "RMSProp"))
                sl = slice(i, i + n)
                assert np.array_equal(cc, r["corr"][sl])                                         # the clip is exact
                assert np.allclose(pp, r["p"][sl], rtol=4 * 2.0 ** -52, atol=0)
                if rule != "SGD":
                    assert np.allclose(aa, r["accu"][sl], rtol=4 * 2.0 ** -52, atol=0)
                i += n


@pytest.mark.parametrize("name", UC.NETS)
@pytest.mark.parametrize("rule", UC.RULES)
def test_an_fp32_evaluation_stays_inside_the_bounds(name, rule):
    layers, steps = two_steps(name, rule)
    worst = {}
    for s, r in steps:
        f = UC.restate(layers, rule, dtype=np.float32, **s)
        for q in _quantities(rule):
            assert f[q].dtype == np.float32
            worst[q] = max(worst.get(q, 0.0), UC.worst_ratio(f[q], r[q], r[q + "_bound"]))
        assert np.array_equal(f["corr"][r["surely_clipped"]], r["corr"][r["surely_clipped"]].astype(np.float32))
    print(f"fp32 numpy / bound, {name} {rule}: " + ", ".join(f"{q} {v:.3f}" for q, v in worst.items()))
    assert all(v < 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_leaves_the_bounds(mutation):
    """Per applicable rule and net: the share of elements on which the mutated restatement is outside the bound of at least one
    quantity, at the step where it can show (step 2: c_prev != 0).  At least 1 % each; the printed figures go into the summary."""
    for rule in APPLIES[mutation]:
        for name in ("layers3", "padded"):
            layers, steps = two_steps(name, rule)
            s, r = steps[1]
            with np.errstate(over="ignore", invalid="ignore"):
                m = UC.restate(layers, rule, mutation=mutation, **s)
            out = np.zeros(r["p"].size, bool)
            ratios = []
            for q in _quantities(rule):
                err = np.abs(m[q] - r[q])
                bad = ~(err <= r[q + "_bound"])
                out |= bad
                sel = bad & (r[q + "_bound"] > 0) & np.isfinite(err)
                if sel.any():
                    ratios.append(np.max(err[sel] / r[q + "_bound"][sel]))
            share = out.mean()
            print(f"{mutation} {rule} {name}: outside the bounds on {100 * share:.1f} % of the elements, largest error / bound {max(ratios):.3g}")
            assert share >= 0.01, (mutation, rule, name, share)
            assert max(ratios) >= 1e3        # not a near miss: the exact factors in the bounds carry no weight


def test_moments_restatement_is_the_reference_two_pass_form():
    """Against a direct transcription of utils-functions.h:50-82 in extended precision, and its own bounds against a reversed-order
    fp64 evaluation (another reduction order is exactly what the bounds are for)."""
    rng = np.random.default_rng(3)
    for x in (rng.standard_normal(1000) * np.exp(rng.uniform(-6, 6, 1000)), 1000.0 + 1e-3 * rng.standard_normal(128), rng.uniform(0.5, 1.5, 37)):
        x = x.astype(np.float32)
        val, bnd = R.moments(x)
        v = x.astype(np.longdouble)
        mean = v.sum() / v.size
        e = v - mean
        var = (e * e).sum() / v.size
        want = [v.min(), v.max(), mean, var, (e ** 3).sum() / var ** np.longdouble(1.5) / v.size, (e ** 4).sum() / (var * var) / v.size - 3]
        rv = x[::-1].astype(np.float64)
        rmean = np.add.reduce(rv) / rv.size          # (pairwise, another order)
        re_ = rv - rmean
        rvar = np.add.reduce(re_ * re_) / rv.size
        other = [rv.min(), rv.max(), rmean, rvar, np.add.reduce(re_ ** 3) / rvar ** 1.5 / rv.size, np.add.reduce(re_ ** 4) / (rvar * rvar) / rv.size - 3]
        for i in range(6):
            assert abs(float(want[i]) - val[i]) <= bnd[i] + 2.0 ** -52 * abs(val[i]), (i, want[i], val[i], bnd[i])
            assert abs(other[i] - val[i]) <= bnd[i], (i, other[i], val[i], bnd[i])
        assert np.all(bnd[2:] < 1e-5 * np.abs(val[2:]))      # ... and the bounds still pin every printed digit (%g shows six)
    val, bnd = R.moments(np.full(50, 0.25, np.float32))
    assert val[0] == val[1] == val[2] == 0.25 and val[3] == 0 and np.isnan(val[4]) and np.isnan(val[5])


def test_info_figures_print_as_the_stream_operator_does():
    """_g of eesen_amd/api.py against printf's %g, which is what operator<< of a default stream prints (include/eesen_hip_info.h): both
    formatters arrange the same doubles, so a NaN with the sign bit set must read -nan on both sides."""
    from eesen_amd.api import _g
    libc = C.CDLL(None)
    libc.snprintf.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_double]
    buf = C.create_string_buffer(64)
    nan = float("nan")
    for v in (0.0, -0.0, 1.0, -1.5, 1e-5, 123456.0, 1234567.0, 0.000123456789, 1e300, -1e-300, float("inf"), -float("inf"), nan,
              np.copysign(nan, -1.0), 2.5e-7, 99999.95, 0.1 + 0.2):
        libc.snprintf(buf, 64, b"%g", C.c_double(v))
        assert _g(float(v)) == buf.value.decode(), (v, _g(float(v)), buf.value)
