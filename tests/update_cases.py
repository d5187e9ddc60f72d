"""The nets, hyper-parameters and inputs of the update-rule and tensor-statistics tests, in ONE place: tests/test_update_restatement.py
(CPU: the restatement against the oracle, an fp32 evaluation inside the bounds, every mutation outside them) and
tests/test_gpu_update_rules.py / tests/test_gpu_tensor_moments.py (the kernels of csrc/optim.hip) draw the very same arrays.

Everything here is in FILE order (Net::GetParams order, tests/util.py::split_params); the device's internal order -- gate-interleaved rows,
padded cells and input columns -- is read off the library by GradInjector below and never assumed."""
import ctypes as C

import numpy as np

RULES = ("SGD", "Adagrad", "RMSProp")
# lr and every learn_rate_coef are powers of two: lr * coef and lr * coef * c are then exact products, which is what lets
# test_sgd_momentum_buffer_over_five_steps read the momentum buffer back bit for bit.
HYPER = dict(lr=2.0 ** -9, mmt=0.9, eps=1e-6, rho=0.9)


def _bilstm(din, H, coef, max_grad, rng):
    ps = []
    for _ in range(2):
        ps += [rng.uniform(-0.1, 0.1, (4 * H, din)), rng.uniform(-0.1, 0.1, (4 * H, H)), rng.uniform(-0.1, 0.1, 4 * H),
               rng.uniform(-0.1, 0.1, H), rng.uniform(-0.1, 0.1, H), rng.uniform(-0.1, 0.1, H)]
    return dict(type="BiLstmParallel", input_dim=din, output_dim=2 * H, learn_rate_coef=coef, max_grad=max_grad,
                params=[p.astype(np.float32) for p in ps])


def _affine(din, dout, coef, max_grad, rng):
    return dict(type="AffineTransform", input_dim=din, output_dim=dout, learn_rate_coef=coef, max_grad=max_grad,
                params=[rng.uniform(-0.1, 0.1, (dout, din)).astype(np.float32), rng.uniform(-0.1, 0.1, dout).astype(np.float32)])


def make_net(name, seed=11):
    """layers3: every block its own (learn_rate_coef, max_grad), one of them without a clip.  one_wide: a 3.15 M-float block, longer than
    one pass of either update grid (2048 * 256 * 4 and 4096 * 256 elements).  padded: 6 cells per direction and 5 / 12 input columns, all
    padded to multiples of 4 inside the library."""
    rng = np.random.default_rng(seed)
    if name == "layers3":
        return [_bilstm(8, 4, 1.0, 0.05, rng), _bilstm(8, 4, 0.5, 0.0, rng), _affine(8, 12, 2.0, 1e-3, rng)]
    if name == "one_wide":
        return [_bilstm(256, 512, 1.0, 0.05, rng), _affine(1024, 4, 0.5, 0.0, rng)]
    if name == "padded":
        return [_bilstm(5, 6, 1.0, 0.05, rng), _bilstm(12, 6, 0.5, 0.0, rng), _affine(12, 7, 2.0, 1e-3, rng)]
    raise KeyError(name)


NETS = ("layers3", "one_wide", "padded")


def layer_sizes(layers):
    return [int(sum(p.size for p in L["params"])) for L in layers]


def with_params(layers, flat):
    """The same topology carrying `flat` (file order)."""
    out, i = [], 0
    for L in layers:
        ps = []
        for p in L["params"]:
            ps.append(np.asarray(flat[i:i + p.size], np.float32).reshape(p.shape).copy()); i += p.size
        out.append(dict(L, params=ps))
    assert i == flat.size
    return out


def per_element(layers, key):
    """learn_rate_coef / max_grad of every file-order element (fp32, as the C-ABI carries them)."""
    return np.concatenate([np.full(n, np.float32(L[key]), np.float32) for L, n in zip(layers, layer_sizes(layers))])


def fp32_neighbours(x):
    x = np.float32(x)
    return np.nextafter(x, np.float32(0)), np.nextafter(x, np.float32(np.inf))


def gradients(layers, seed):
    """g = normal * exp(U(-12, 3)); about 1 % of the entries replaced, in rotation, by +-max_grad, the fp32 neighbours of max_grad on both
    sides (either sign), +-0 and -- on layers with a clip only -- +-1e30.  No denormals."""
    rng = np.random.default_rng(seed)
    out = []
    for L, n in zip(layers, layer_sizes(layers)):
        g = (rng.standard_normal(n) * np.exp(rng.uniform(-12.0, 3.0, n))).astype(np.float32)
        g[np.abs(g) < 1e-30] = 0.0
        mg = np.float32(L["max_grad"])
        below, above = fp32_neighbours(mg if mg > 0 else np.float32(1.0))
        base = mg if mg > 0 else np.float32(1.0)      # (a layer without a clip: the same rotation around 1, where nothing must happen)
        specials = [base, -base, below, above, -below, -above, np.float32(0.0), np.float32(-0.0)]
        if mg > 0:
            specials += [np.float32(1e30), np.float32(-1e30)]
        idx = rng.choice(n, size=max(len(specials), n // 100), replace=False)
        for k, i in enumerate(idx):
            g[i] = specials[k % len(specials)]
        out.append(g)
    return np.concatenate(out)


def parameters(layers, seed):
    """uniform in +-0.1"""
    n = sum(layer_sizes(layers))
    return np.random.default_rng(seed).uniform(-0.1, 0.1, n).astype(np.float32)


def accumulators(layers, seed):
    """log-uniform in [1e-12, 1e4], every 7th exactly 0"""
    n = sum(layer_sizes(layers))
    a = np.exp(np.random.default_rng(seed).uniform(np.log(1e-12), np.log(1e4), n)).astype(np.float32)
    a[::7] = 0.0
    return a


def two_step_inputs(name, seed=5):
    """What the two-step tests feed: the net, its start state and the gradients of both steps."""
    layers = make_net(name)
    return dict(layers=layers, p0=parameters(layers, seed), a0=accumulators(layers, seed + 1),
                g=[gradients(layers, seed + 2), gradients(layers, seed + 3)])


def restate(layers, rule, p, c_prev, g, a, **kw):
    """tests/update_restatement.py::update with this module's hyper-parameters and the layers' own constants per element."""
    from tests import update_restatement as R
    return R.update(rule, p, c_prev, g, a, per_element(layers, "learn_rate_coef"), per_element(layers, "max_grad"), R.constants(**HYPER), **kw)


def clip_exact(layers, g):
    """clip(g) in fp32: what the momentum buffer must hold, bit for bit, after the first step of a fresh Net (c_prev = 0)."""
    mg = per_element(layers, "max_grad")
    g = np.asarray(g, np.float32)
    return np.where(mg > 0, np.minimum(np.maximum(g, -mg), mg), g).astype(np.float32)


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the elements (0 / 0 counts as 0, anything non-zero over a zero bound as inf)."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / np.asarray(bound, np.float64))
    return float(np.max(r)) if r.size else 0.0


# ------------------------------------------------------------------------------------------------------------ the device side
def dev_write(ptr, host):
    from eesen_amd import _lib
    host = np.ascontiguousarray(host, np.float32)
    _lib.check(_lib.load().eesen_dev_copy(0, C.c_void_p(ptr), host.ctypes.data_as(C.c_void_p), C.c_long(host.nbytes), 1))


class GradInjector:
    """Feeds a Net gradients of the test's choosing, in file order, without a setter: arange(n) written into the fresh-gradient buffer
    comes back through GetGrads() as the internal index of every file-order entry.  The internal slots the map does not reach are the
    pads (padded cells / input columns, row padding); they get 0."""

    def __init__(self, net):
        self.net = net
        self.ptr, self.n = net.grad_buffer()
        assert 0 < self.n <= 2 ** 24, "indices must be exact in fp32"
        net.Synchronize()
        dev_write(self.ptr, np.arange(self.n, dtype=np.float32))
        got = net.GetGrads()
        self.map = got.astype(np.int64)
        assert np.array_equal(self.map.astype(np.float32), got)
        assert self.map.size == net.NumParams() and self.map.min() >= 0 and self.map.max() < self.n
        assert np.unique(self.map).size == self.map.size, "two file entries share an internal slot"
        self.pads = self.n - self.map.size
        self.put(np.zeros(self.map.size, np.float32))

    def put(self, g_file):
        g_file = np.asarray(g_file, np.float32)
        assert g_file.size == self.map.size
        internal = np.zeros(self.n, np.float32)
        internal[self.map] = g_file
        self.net.Synchronize()
        dev_write(self.ptr, internal)
        assert np.array_equal(self.net.GetGrads().view(np.uint32), g_file.view(np.uint32))     # every file entry reached, sign of zero included
