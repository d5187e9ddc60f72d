"""-m gpu: the host resources between the kernels -- pinned staging slots, their events, the guard hooks of the loss objects.

Two statements about behaviour, not about any one implementation of those resources:

* what a minibatch computes does not depend on what the long-lived handles staged before (tests/test_gpu_parity.py holds that for
  the device buffers of the Net and the synchronous CTC path; this is the same idea on the deferred and pinned paths: the feeder's
  four pinned slots, the Net's host-input and length staging, the label / target staging and the deferred result slots of Ctc and CE);
* a loss object hooked onto a Net's error word survives either destruction order."""
import ctypes as C
import re

import numpy as np
import pytest

from eesen_amd import frontend as fe, synth
from tests.util import valid_mask

pytestmark = pytest.mark.gpu

D0 = 5                                                      # raw feature columns
PIPELINE = [(fe.CMVN, 1, 0), (fe.SPLICE, 1, 1), (fe.DELTAS, 2, 2)]   # 5 -> 5 -> 15 -> 45 columns: rows padded to 48 floats
CFG = {**synth.config("small_bi"), "D": 45}
# (S, T): each of the two alternating slots of every object grows at least twice and is then reused for something smaller; S rises
# and falls (the metadata slots)
SHAPES = [(2, 5), (3, 9), (8, 17), (5, 40), (2, 5), (8, 17), (3, 9)]


class _Minibatch:
    def __init__(self, S, T, seed):
        rng = np.random.default_rng(seed)
        K = CFG["K"]
        self.S, self.T = S, T
        self.lens = np.sort(rng.integers(max(1, int(np.ceil(0.8 * T))), T + 1, size=S)).astype(np.int32)
        self.lens[-1] = T
        self.utts = [fe.RawUtt(rng.standard_normal((int(n), D0)).astype(np.float32),
                               np.stack([0.1 * rng.standard_normal(D0), 1.0 + 0.1 * rng.random(D0)]).astype(np.float32), (int(n), CFG["D"]))
                     for n in self.lens]
        self.labels = [rng.integers(1, K, size=max(1, int(n) // 10)).astype(np.int32) for n in self.lens]
        self.targets = np.where(valid_mask(self.lens, T, S), rng.integers(0, K, size=T * S), 0).astype(np.int32)


class _Handles:
    """One Net, Ctc, CE and Feeder (CMVN + splice + deltas); both loss objects guard on the Net."""

    def __init__(self, layers):
        from eesen_amd.api import Net, Ctc, CE, Feeder
        self.net = Net.from_layers(layers)
        self.ctc, self.ce, self.feeder = Ctc(), CE(), Feeder()
        self.feeder.set_pipeline(PIPELINE)
        self.ctc.SetGuard(self.net)
        self.ce.SetGuard(self.net)

    def propagate_host(self, a, ld):
        """Net::Propagate from a HOST matrix whose rows are ld floats apart (the Python wrapper always hands over dense rows)."""
        from eesen_amd.api import CuMatrix, check, _np_ptr
        p, co, ldo = C.c_void_p(), C.c_int(), C.c_int()
        check(self.net.lib.eesen_net_propagate(self.net.h, _np_ptr(a), a.shape[0], ld, 0, C.byref(p), C.byref(co), C.byref(ldo)))
        return CuMatrix.view(p.value, a.shape[0], co.value, ldo.value, keepalive=self.net)

    def step(self, mb):
        """-> (assembled feeder matrix, net_out from the device matrix, net_out from the host matrix, CTC diff, CE diff)"""
        slot = self.feeder.submit(mb.utts)
        feats = self.feeder.acquire(slot)
        self.net.SetSeqLengths(mb.lens)
        out_dev = self.net.Propagate(feats).numpy()
        assembled = feats.numpy()
        self.feeder.release(slot)
        assert assembled.shape == (mb.T * mb.S, CFG["D"])
        wide = np.full((assembled.shape[0], CFG["D"] + 3), np.nan, np.float32)   # what lies between the rows is never read
        wide[:, :CFG["D"]] = assembled
        out = self.propagate_host(wide, wide.shape[1])
        d_ctc = self.ctc.EvalParallel(mb.lens, out, mb.labels, want_pzx=False)
        self.ctc.ErrorRateMSeq(mb.lens, out, mb.labels, deferred=True)
        d_ce = self.ce.EvalParallel(out, mb.targets, None, mb.lens, want_obj=False)
        return assembled, out_dev, out.numpy(), d_ctc.numpy(), d_ce.numpy()


def test_staging_slots_regrow_without_changing_a_result(gpu):
    layers = synth.make_model(**CFG)
    batches = [_Minibatch(S, T, 300 + i) for i, (S, T) in enumerate(SHAPES)]
    fresh, ctc_sum, ce_sum = [], {}, {}
    for mb in batches:                              # handles that have only ever seen this one minibatch
        h = _Handles(layers)
        fresh.append(h.step(mb))
        for tot, st in ((ctc_sum, h.ctc.stats()), (ce_sum, h.ce.stats())):
            for k, v in st.items():
                tot[k] = tot.get(k, 0) + v          # in call order: the very additions the long-lived objects make
        assert h.ctc.Dropped() == 0 and h.ce.Dropped() == 0
    h = _Handles(layers)
    for i, mb in enumerate(batches):
        got = h.step(mb)
        for name, g, f in zip(("feeder matrix", "net_out (device input)", "net_out (host input)", "CTC diff", "CE diff"), got, fresh[i]):
            assert np.array_equal(g, f), (name, i, SHAPES[i])
    assert h.ctc.stats() == ctc_sum and ctc_sum["sequences"] == sum(S for S, _ in SHAPES) and ctc_sum["ref_tokens"] > 0
    assert h.ce.stats() == ce_sum and ce_sum["frames"] == sum(S * T for S, T in SHAPES)
    assert h.ctc.Dropped() == 0 and h.ce.Dropped() == 0


def _loaded_hip_runtime():
    """The HIP runtime libeesen_hip.so brought into this process (to create a second stream), or None."""
    with open("/proc/self/maps") as f:
        for line in f:
            m = re.search(r"(/\S*libamdhip64\.so\S*)", line)
            if m:
                return C.CDLL(m.group(1))
    return None


def test_guard_hooks_survive_either_destruction_order(gpu):
    from eesen_amd.api import Net, Ctc, CE, CuMatrix, EesenError
    cfg = synth.config("small_bi")
    layers = synth.make_model(**cfg)
    batch = synth.make_batch(**cfg)
    S, T, K = cfg["S"], cfg["T"], cfg["K"]
    tg = np.where(valid_mask(batch.lens, T, S), np.arange(T * S) % K, 0).astype(np.int32)
    a = Net.from_layers(layers)
    a.SetTrainOptions(0.0, 0.0)
    ctc, ce = Ctc(), CE()
    ctc.SetGuard(a)
    ce.SetGuard(a)

    def evaluate(ctc, ce, out):
        ctc.EvalParallel(batch.lens, out, batch.labels, want_pzx=False)
        ctc.ErrorRateMSeq(batch.lens, out, batch.labels, deferred=True)
        ce.EvalParallel(out, tg, None, batch.lens, want_obj=False)

    def step(net, ctc, ce):
        net.SetSeqLengths(batch.lens)
        evaluate(ctc, ce, net.Propagate(batch.feats))

    # (a) a minibatch computed under a raised error word is in no total, of either object
    step(a, ctc, ce)
    one = (ctc.stats(), ce.stats())
    assert one[0]["sequences"] == S and one[0]["ref_tokens"] > 0 and one[1]["sequences"] == S
    a._raise_error_word(2)        # what the forward milestone waiter stores when it gives up (lstm_persistent.hip)
    step(a, ctc, ce)
    a.Synchronize()
    assert ctc.Dropped() == 1 and ce.Dropped() == 1
    assert (ctc.stats(), ce.stats()) == one

    # (b) the Net goes first: the loss objects go on counting and never read its freed word
    rng = np.random.default_rng(4)
    x = rng.standard_normal((T * S, K))
    p = np.exp(x - x.max(1, keepdims=True))
    probs = CuMatrix.from_numpy((p / p.sum(1, keepdims=True)).astype(np.float32))
    a.lib.eesen_net_destroy(a.h)
    a.h = None
    evaluate(ctc, ce, probs)
    two = (ctc.stats(), ce.stats())
    assert ctc.Dropped() == 1 and ce.Dropped() == 1
    assert two[0]["sequences"] == 2 * S and two[0]["frames"] == 2 * int(batch.lens.sum()) and two[0]["ref_tokens"] == 2 * one[0]["ref_tokens"]
    assert two[1]["sequences"] == 2 * S and two[1]["frames"] == 2 * T * S

    # (c) the loss objects go first: unhooked by hand, and while still hooked
    b = Net.from_layers(layers)
    b.SetTrainOptions(0.0, 0.0)
    for obj in (ctc, ce):
        obj.SetGuard(b)
        obj.SetGuard(None)
    ctc2, ce2 = Ctc(), CE()
    ctc2.SetGuard(b)
    ce2.SetGuard(b)
    step(b, ctc2, ce2)
    for obj, destroy in ((ctc, b.lib.eesen_ctc_destroy), (ce, b.lib.eesen_ce_destroy), (ctc2, b.lib.eesen_ctc_destroy), (ce2, b.lib.eesen_ce_destroy)):
        assert destroy(obj.h) == 0
        obj.h = None
    ctc3, ce3 = Ctc(), CE()
    step(b, ctc3, ce3)
    b.Synchronize()
    assert ctc3.stats()["sequences"] == S and ce3.stats()["sequences"] == S and ctc3.Dropped() == 0 and ce3.Dropped() == 0

    # (d) a Net on another stream is refused, by each entry point under its own name
    hip = _loaded_hip_runtime()
    st = C.c_void_p()
    if hip is not None and hip.hipStreamCreateWithFlags(C.byref(st), 1) == 0 and st.value:
        other = Net.from_layers(layers, stream=st.value)
        with pytest.raises(EesenError, match="eesen_ctc_set_guard"):
            ctc3.SetGuard(other)
        with pytest.raises(EesenError, match="eesen_ce_set_guard"):
            ce3.SetGuard(other)
        step(b, ctc3, ce3)                          # refused means unchanged: both still evaluate, hooked to nothing
        assert ctc3.stats()["sequences"] == 2 * S and ce3.stats()["sequences"] == 2 * S
        other.lib.eesen_net_destroy(other.h)
        other.h = None
        assert hip.hipStreamDestroy(st) == 0
