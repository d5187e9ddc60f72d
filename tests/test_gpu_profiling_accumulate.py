"""-m gpu: profiling mode 2 (eesen_ctc_set_profiling / eesen_ce_set_profiling) on every phase clock of the loss objects -- the loss, the
alignment, the decoder, the time stamps and CE.  In mode 2 the phase times are summed over the calls since the last read and
cleared by that read; back in mode 0 a read gives the last call's.  (tests/test_gpu_ctc_mbr.py holds the same for the MBR sums.)

Every phase is >= 0 and < 1 s, the bound of the other time tests, and the phase that always launches a kernel is > 0.  Nothing fixes
a ratio between one call and two, so none is asserted.
"""
import numpy as np
import pytest

from tests import ctc_cases as cc

pytestmark = pytest.mark.gpu

# clock: (the phases in order, the phase that always launches a kernel)
CLOCKS = {
    "loss": (("log", "alpha_beta", "error_diff"), "alpha_beta"),
    "align": (("log", "sweep", "traceback"), "sweep"),
    "decode": (("topc", "beam", "hyp"), "beam"),
    "stamps": (("lattices", "sweep", "stamps"), "sweep"),
    "ce": (("ce",), "ce"),
}


def _clock(name):
    """(obj, call, read) of one clock at dense_3x12x7."""
    from eesen_amd.api import CE, Ctc, CuMatrix
    lens, probs, labels, T, S = cc.build("dense_3x12x7")
    dev = CuMatrix.from_numpy(probs)
    if name == "ce":
        ce = CE()
        targets = np.random.default_rng(5).integers(0, probs.shape[1], size=T * S).astype(np.int32)
        return ce, lambda: ce.EvalParallel(dev, targets, frame_num_utt=lens), ce.PhaseTimes
    ctc = Ctc()
    if name == "loss":
        return ctc, lambda: ctc.EvalParallel(lens, dev, labels), ctc.PhaseTimes
    if name == "align":
        return ctc, lambda: ctc.AlignParallel(lens, dev, labels), ctc.AlignTimes
    if name == "decode":
        return ctc, lambda: ctc.DecodeParallel(lens, dev, beam=4, max_classes=3, nbest=2), ctc.DecodeTimes
    ctc.DecodeParallel(lens, dev, beam=4, max_classes=3, nbest=2)
    return ctc, lambda: ctc.DecodeStamps(lens, dev), ctc.StampTimes


@pytest.mark.parametrize("name", list(CLOCKS))
def test_mode_2_sums_and_clears_and_mode_0_reads_the_last_call(gpu, name):
    phases, main = CLOCKS[name]
    obj, call, read = _clock(name)
    obj.SetProfiling(True)
    call()
    call()
    two = read()
    print(name, "two calls, mode 2:", two)
    assert tuple(two) == phases and all(0 <= v < 1 for v in two.values()) and two[main] > 0
    assert read() == dict.fromkeys(phases, 0.0)          # read and cleared
    obj.SetProfiling(False)
    call()
    one = read()
    print(name, "one call, mode 0:", one)
    assert all(0 <= v < 1 for v in one.values()) and one[main] > 0
