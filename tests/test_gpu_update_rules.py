"""-m gpu: sgd_update_kernel and adaptive_update_kernel (csrc/optim.hip), as Net::update launches them per layer block, held ELEMENT BY
ELEMENT against the fp64 restatement of tests/update_restatement.py within the rounding bound it derives for each element.

The test feeds gradients of its own choosing (tests/update_cases.py::GradInjector: the file-order -> internal map is read off the library,
pads get 0); Update() needs no Propagate.  State goes in and out through SetParams / GetParams / SetAccumulators / GetAccumulators.  The
momentum buffer has no getter: after the first step of a fresh Net it must equal clip(g0) bit for bit, which shows in the min / max of
TensorMoments(1, layer) and, under SGD, in the parameters (lr * coef is a power of two: p1 = fl(p0 - lr coef c1), one rounding whether
fused or not); test_sgd_momentum_buffer_over_five_steps reads it back exactly through zeroed parameters.

Inputs, nets and hyper-parameters: tests/update_cases.py, shared with tests/test_update_restatement.py, which shows on the CPU that an fp32
evaluation stays inside these bounds and that every listed mutation of the rules leaves them by >= 4e5 x.  The bounds are derived, not
measured; the only measured figures are the worst error / bound ratios per rule and quantity, written to update_rules.json in
$EESEN_PARITY_OUT (when set; committed from an MI355X run as profiles/update_rules.json) for the record and asserted < 1."""
import json
import os

import numpy as np
import pytest

from tests import update_cases as UC
from tests.util import split_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def record():
    worst = {}

    def note(rule, quantity, ratio):
        worst.setdefault(rule, {})
        worst[rule][quantity] = max(worst[rule].get(quantity, 0.0), float(ratio))

    yield note
    out_dir = os.environ.get("EESEN_PARITY_OUT")
    if not out_dir:
        return
    try:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "update_rules.json"), "w") as f:
            json.dump(dict(what="worst |HIP - fp64 restatement| / derived bound, per rule and quantity", worst=worst), f, indent=1)
    except OSError:
        pass


def make(layers, rule, p=None, a=None):
    from eesen_amd.api import Net
    net = Net.from_layers(layers)
    net.SetTrainOptions(UC.HYPER["lr"], UC.HYPER["mmt"])
    net.SetUpdateAlgorithm(rule, UC.HYPER["eps"], UC.HYPER["rho"])
    inj = UC.GradInjector(net)
    if p is not None:
        net.SetParams(p)
    if a is not None and rule != "SGD":
        net.SetAccumulators(a)
    return net, inj


def hold(layers, got, want, bound, what):
    """Every element of every tensor within its bound; returns the worst ratio."""
    worst = 0.0
    for (li, name, g), (_, _, w), (_, _, b) in zip(split_params(layers, got), split_params(layers, want), split_params(layers, bound)):
        r = UC.worst_ratio(g, w, b)
        assert r < 1.0, f"{what}: layer {li} {name}: worst error / bound {r:.3g} at element {int(np.argmax(np.abs(g.astype(np.float64) - w) - b))}"
        worst = max(worst, r)
    return worst


def step_and_hold(net, inj, layers, rule, c_prev, g, what, record):
    """One Update() from the state the device holds, every element of p (and accu) against the restatement of exactly that step."""
    p_in = net.GetParams()
    a_in = net.GetAccumulators() if rule != "SGD" else np.zeros_like(p_in)
    inj.put(g)
    net.Update()
    r = UC.restate(layers, rule, p_in, c_prev, g, a_in)
    p_out = net.GetParams()
    assert np.isfinite(p_out).all()
    record(rule, "p", hold(layers, p_out, r["p"], r["p_bound"], f"{what} p"))
    if rule != "SGD":
        record(rule, "accu", hold(layers, net.GetAccumulators(), r["accu"], r["accu_bound"], f"{what} accu"))
    # where mmt c + g passes max_grad by more than its bound the applied step is that of +-max_grad exactly
    s = r["surely_clipped"]
    mg = UC.per_element(layers, "max_grad")
    assert s.sum() >= 10 and np.all(np.abs(r["corr"][s]) == mg[s])
    delta = p_in.astype(np.float64) - p_out.astype(np.float64)
    assert np.all(np.abs(delta[s] - r["step"][s]) <= r["p_bound"][s]), what
    return p_in, p_out, r


def moments_minmax(net, layers):
    out = []
    for li in range(len(layers)):
        out += [tuple(row[:2]) for row in net.TensorMoments(1, li)]
    return out


@pytest.mark.parametrize("name", UC.NETS)
@pytest.mark.parametrize("rule", UC.RULES)
def test_two_steps_from_a_fresh_net(gpu, name, rule, record):
    inp = UC.two_step_inputs(name)
    layers = inp["layers"]
    net, inj = make(layers, rule, inp["p0"], inp["a0"])
    assert (inj.pads > 0) == (name == "padded")
    # step 1: c_prev = 0, so the momentum buffer becomes clip(g0) bit for bit
    c1 = UC.clip_exact(layers, inp["g"][0])
    p0, p1, r1 = step_and_hold(net, inj, layers, rule, np.zeros_like(c1), inp["g"][0], f"{name} {rule} step 1", record)
    assert np.array_equal(r1["corr"].astype(np.float32), c1)
    want = [(float(t.min()), float(t.max())) for _, _, t in split_params(layers, c1)]
    assert moments_minmax(net, layers) == want
    if rule == "SGD":
        lrc = (np.float32(UC.HYPER["lr"]) * UC.per_element(layers, "learn_rate_coef")).astype(np.float32)
        assert np.array_equal(p1, p0 - lrc * c1)          # (lrc * c1 is exact: one fp32 rounding either way)
    # step 2: every input known exactly -- c1, and p / accu as read back -- so nothing compounds
    step_and_hold(net, inj, layers, rule, c1, inp["g"][1], f"{name} {rule} step 2", record)


def test_sgd_momentum_buffer_over_five_steps(gpu, record):
    """SetParams(0) before each Update: GetParams() == -lr coef corr exactly (powers of two), so corr is read back bit for bit each step and
    the next step restated from it.  SetParams must leave corr alone, or step 2 would already miss."""
    layers = UC.make_net("layers3")
    net, inj = make(layers, "SGD")
    lrc = (np.float32(UC.HYPER["lr"]) * UC.per_element(layers, "learn_rate_coef")).astype(np.float64)
    assert np.all(np.log2(lrc) == np.round(np.log2(lrc)))
    zero = np.zeros(lrc.size, np.float32)
    c_prev = zero
    for k in range(5):
        g = UC.gradients(layers, 100 + k)
        net.SetParams(zero)
        inj.put(g)
        net.Update()
        corr = (-net.GetParams().astype(np.float64) / lrc).astype(np.float32)
        assert np.array_equal(-(corr.astype(np.float64) * lrc), net.GetParams().astype(np.float64))
        r = UC.restate(layers, "SGD", zero, c_prev, g, zero)
        if k == 0:
            assert np.array_equal(corr, UC.clip_exact(layers, g))
        record("SGD", "corr", hold(layers, corr, r["corr"], r["corr_bound"], f"step {k + 1} corr"))
        mg = UC.per_element(layers, "max_grad")
        assert np.all(np.abs(corr[mg > 0]) <= mg[mg > 0]) and np.abs(corr[mg == 0]).max() > 1.0      # clipped where asked, and only there
        c_prev = corr


@pytest.mark.parametrize("rule", ["Adagrad", "RMSProp"])
def test_adaptive_rules_ignore_learn_rate_coef(gpu, rule):
    """layers3's coefficients 0.5 and 2 must not appear: the same bits as with a coefficient of 1 everywhere."""
    inp = UC.two_step_inputs("layers3")
    res = []
    for layers in (inp["layers"], [dict(L, learn_rate_coef=1.0) for L in inp["layers"]]):
        net, inj = make(layers, rule, inp["p0"], inp["a0"])
        for g in inp["g"]:
            inj.put(g)
            net.Update()
        res.append((net.GetParams(), net.GetAccumulators()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert not np.array_equal(res[0][0], inp["p0"])


@pytest.mark.parametrize("rule", UC.RULES)
def test_pads_stay_zero_on_a_padded_net(gpu, rule):
    """Three steps on `padded` (6 cells per direction, 5 / 12 input columns): 1 / sqrt(0 + eps) * 0 in the pad cells must stay 0.  One
    Propagate afterwards must give the bits of a second Net built from GetParams() of the first -- its pads are zero by construction."""
    from eesen_amd.api import Net
    inp = UC.two_step_inputs("padded")
    layers = inp["layers"]
    net, inj = make(layers, rule, inp["p0"], inp["a0"])
    for k in range(3):
        inj.put(UC.gradients(layers, 200 + k))
        net.Update()
    p = net.GetParams()
    assert np.isfinite(p).all() and not np.array_equal(p, inp["p0"])
    feats = np.random.default_rng(9).standard_normal((12, 5)).astype(np.float32)
    outs = []
    for n in (net, Net.from_layers(UC.with_params(layers, p))):
        n.SetSeqLengths([6, 5])
        outs.append(n.Propagate(feats).numpy())
    assert outs[0].shape == (12, 7) and np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("rule", UC.RULES)
def test_a_raised_error_word_leaves_everything_untouched(gpu, rule, capfd, record):
    """The flag word of the recurrence kernels (Net._raise_error_word, the hook of the recovery tests) raised before Update(): parameters,
    accumulators and the momentum buffers of every layer stay bit-identical; the host then reports and recovers as the recovery tests
    expect, and the next Update() is an ordinary step."""
    inp = UC.two_step_inputs("layers3")
    layers = inp["layers"]
    net, inj = make(layers, rule, inp["p0"], inp["a0"])
    inj.put(inp["g"][0])
    net.Update()
    before = (net.GetParams(), net.GetAccumulators() if rule != "SGD" else None, [net.TensorMoments(1, li) for li in range(len(layers))])
    capfd.readouterr()
    inj.put(inp["g"][1])
    net._raise_error_word(1)
    net.Update()
    after = (net.GetParams(), net.GetAccumulators() if rule != "SGD" else None, [net.TensorMoments(1, li) for li in range(len(layers))])
    err = capfd.readouterr().err
    assert "gave up waiting for a peer workgroup" in err and "were NOT applied" in err and "one-launch-per-step kernels" in err
    net.RecurrenceInfo()
    assert net.recoveries == 1
    assert np.array_equal(before[0], after[0])
    if rule != "SGD":
        assert np.array_equal(before[1], after[1])
    for b, a in zip(before[2], after[2]):
        assert np.array_equal(b.view(np.uint64), a.view(np.uint64))
    # recovered: the same gradients now make the step of the restatement
    step_and_hold(net, inj, layers, rule, UC.clip_exact(layers, inp["g"][0]), inp["g"][1], f"{rule} after the recovery", record)
    assert net.RecurrenceInfo() is not None and net.recoveries == 1
