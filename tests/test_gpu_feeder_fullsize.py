"""-m gpu: the three kernels of csrc/feeder.hip (interleave_kernel, feat_stage_kernel, feat_paste_kernel) past one pass of their capped
grids and at the limits eesen_feeder_set_pipeline accepts, on the cases of tests/feeder_cases.py (whose conditions
tests/test_feeder_cases.py holds on the CPU).

Everything is bit for bit against restatements the project already has: eesen_amd.batching.interleave, oracle/frontend.py and
numpy.hstack.  Every check of a feeder slot reads the slot's whole stride (tests/feeder_slot.py): pad columns and the rows past an
utterance's end are +0 as bits.

* the assemblies of 2.1 M float4 items (D = 40) and 2.16 M float items (D = 13, one matrix a row-strided view, one utterance empty);
* a 4400-frame utterance among short and empty ones through splice, CMVN, deltas and subsampling (the deltas take four passes), and a
  1400-frame one through the repeat branch of subsample-feats;
* utterances the pipeline empties in the middle of a batch, nothing filtered out beforehand, the one that enters empty with None for
  its CMVN vectors;
* add-deltas at order 8 and window 16, splice-feats at 64 frames of context, and the refusals just beyond;
* paste-feats joining 6100 rows of four tables;
* one slot through batches of changing width, length and pipeline, and the same list on two slots;
* one slot whose next batch is submitted while the net still reads the previous one.
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from eesen_amd import frontend as fe, synth
from eesen_amd.batching import interleave
from oracle import frontend as ofe
from tests import feeder_cases as fc
from tests.feeder_slot import same_bits, slot_matrix

pytestmark = pytest.mark.gpu
KIND = {"cmvn": fe.CMVN, "splice": fe.SPLICE, "subsample": fe.SUBSAMPLE, "deltas": fe.DELTAS}


def _stages(named):
    return [(KIND[s[0]], int(s[1]), int(s[2]) if len(s) > 2 else 0) for s in named]


def _ld(D):
    return (D + 3) // 4 * 4


def _out_dim(named, D):
    for s in named:
        D *= (1 + s[1] + s[2]) if s[0] == "splice" else (1 + s[1]) if s[0] == "deltas" else 1
    return D


@functools.lru_cache(maxsize=None)
def _oracle(case):
    """The case's utterances behind its pipeline, per utterance ([0 x D] where the tools write nothing): computed once."""
    c = getattr(fc, case)()
    D = _out_dim(c["stages"], c["mats"][0].shape[1])
    outs = [ofe.run_pipeline(c["stages"], m, c["stats"]) for m in c["mats"]]
    return tuple(np.zeros((0, D), np.float32) if o is None else o for o in outs)


def _norms(c):
    """Per utterance the [2 x Dc] offsets and scales of the case's CMVN stage, None for an utterance without frames; None without such
    a stage."""
    nv = dict((s[0], s[1]) for s in c["stages"]).get("cmvn")
    if nv is None:
        return None
    norm = fe.cmvn_norm(c["stats"], bool(nv))
    return [norm if m.shape[0] else None for m in c["mats"]]


def _run_case(case, slots=2):
    """The case as ONE batch through a fresh feeder: (the feeder, the slot's whole matrix, its columns)."""
    from eesen_amd.api import Feeder
    c = getattr(fc, case)()
    f = Feeder(slots=slots)
    f.set_pipeline(_stages(c["stages"]))
    slot = f.submit_raw(c["mats"], _norms(c))
    cols = f.acquire(slot).cols
    return f, slot_matrix(f, slot), cols


def _submit_plain(mats):
    from eesen_amd.api import Feeder
    f = Feeder()
    slot = f.submit(mats)
    got = f.acquire(slot)
    return (got.rows, got.cols, got.stride), slot_matrix(f, slot)


@functools.lru_cache(maxsize=None)
def _first_run(case):
    """The first device result of a case that is run twice (run to run): ((rows, cols, stride), matrix) of the assembly, (matrix,
    cols) of the stages."""
    if case == "assembly_scalar":
        return _submit_plain(fc.assembly_scalar())
    _, host, cols = _run_case(case)
    return host, cols


# ------------------------------------------------------------------------------------------------ assembly past one pass
@pytest.mark.parametrize("case,D", [("assembly_vec", 40), ("assembly_scalar", 13)])
def test_assembly_past_one_pass(gpu, case, D):
    mats = getattr(fc, case)()
    want, lens, T = interleave([np.ascontiguousarray(m) for m in mats], D)
    dims, host = _first_run(case) if case == "assembly_scalar" else _submit_plain(mats)
    assert dims == (T * len(mats), D, _ld(D)) and host.shape == (T * len(mats), _ld(D))
    bits = host.view(np.uint32)
    assert np.array_equal(bits[:, :D], want.view(np.uint32)), "frames and the zero rows past an utterance's end, bit for bit"
    assert not bits[:, D:].any(), "pad columns are +0"
    t = np.arange(T)[:, None] >= lens[None, :]
    assert not bits.reshape(T, len(mats), -1)[t].any(), "padded rows are +0"


# ------------------------------------------------------------------------------------------------ stages past one pass
@pytest.mark.parametrize("case", ["stages_long", "repeat_long"])
def test_stages_past_one_pass(gpu, case):
    c = getattr(fc, case)()
    want = _oracle(case)
    host, cols = _first_run(case) if case == "stages_long" else _run_case(case)[1:]
    T, S = want[c["long"]].shape[0], len(want)
    assert T == max(w.shape[0] for w in want) and cols == want[c["long"]].shape[1]
    assert host.shape == (T * S, _ld(cols)), "the assembled T is the long utterance's"
    assert same_bits(host, want), "per utterance the oracle; zero past an utterance's end and in an empty utterance's column"
    for s, w in enumerate(want):
        assert not host.reshape(T, S, -1)[w.shape[0]:, s].view(np.uint32).any(), s
    assert any(w.shape[0] == 0 for w in want) or case == "repeat_long"


# ------------------------------------------------------------------------------------------------ emptied utterances inside a batch
def test_emptied_utterances_inside_a_batch(gpu):
    from eesen_amd.api import EesenError
    c = fc.emptied()
    want = _oracle("emptied")
    norms = _norms(c)
    assert [n is None for n in norms] == [False, False, True, False, False], "None only for the utterance that enters without frames"
    f, host, cols = _run_case("emptied")
    assert cols == 72 and host.shape == (6 * 5, 72)
    for m, w in zip(c["mats"], want):
        assert f.pipeline_shape(m.shape[1], m.shape[0]) == w.shape
    assert [w.shape[0] for w in want] == [6, 0, 0, 3, 0]
    assert same_bits(host, want), "survivors equal the oracle, the emptied utterances' columns are zero"
    cube = host.reshape(6, 5, -1).view(np.uint32)
    for s in c["gone"]:
        assert not cube[:, s].any(), s
    # None for an utterance that has frames is still refused, and takes no slot
    norm = next(n for n in norms if n is not None)
    with pytest.raises(EesenError, match="null CMVN vectors") as e:
        f.submit_raw(c["mats"], [norm, None, None, norm, norm])
    assert e.value.code == -1
    with pytest.raises(EesenError, match="null CMVN vectors"):
        f.submit_raw(c["mats"], [None] * 5)
    assert same_bits(slot_matrix(f, f.submit_raw(c["mats"], norms)), want), "and the feeder works on"


# ------------------------------------------------------------------------------------------------ the limits of set_pipeline
@pytest.mark.parametrize("name", sorted(fc.LIMIT_PIPELINES))
def test_stage_limits(gpu, name):
    from eesen_amd.api import Feeder
    stages = fc.LIMIT_PIPELINES[name]
    mats = [m for _, m in fc.limit_utts()]
    want = [ofe.run_pipeline(stages, m) for m in mats]
    f = Feeder()
    f.set_pipeline(_stages(stages))
    for m, w in zip(mats, want):
        assert f.pipeline_shape(m.shape[1], m.shape[0]) == w.shape
    host = slot_matrix(f, f.submit_raw(mats))
    assert host.shape == (max(fc.LIMIT_LENS) * len(mats), _ld(want[0].shape[1]))
    assert same_bits(host, want), name


def test_stage_limit_refusals(gpu):
    from eesen_amd.api import Feeder, EesenError
    f = Feeder()
    for stages, message in fc.LIMIT_REFUSALS:
        with pytest.raises(EesenError, match=re.escape(message)) as e:
            f.set_pipeline(_stages(stages))
        assert e.value.code == -1, stages                      # EESEN_ERR_INVALID
    m = np.ones((4, 3), np.float32)                             # a refused pipeline replaces nothing: still the plain assembly
    assert np.array_equal(slot_matrix(f, f.submit_raw([m]))[:, :3], m)


# ------------------------------------------------------------------------------------------------ paste past one pass
def test_paste_past_one_pass(gpu):
    from eesen_amd import _lib
    from eesen_amd.api import paste_feats
    tabs, frames = fc.paste_long()
    got = paste_feats(tabs, fc.PASTE_TOLERANCE)
    S = frames.shape[1]
    assert len(got) == S and got[2] is None and got[3] is None
    lib = _lib.load()
    for s in range(S):
        fr = np.ascontiguousarray(frames[:, s], np.int32)
        rows = C.c_int(-1)
        assert lib.eesen_feat_paste_frames(fr.ctypes.data_as(C.POINTER(C.c_int)), len(tabs), fc.PASTE_TOLERANCE, C.byref(rows)) == 0
        assert (0 if got[s] is None else got[s].shape[0]) == rows.value, s
        if got[s] is None:
            continue
        assert rows.value == fc.PASTE_SHORTEST[s]
        want = np.hstack([t[s][:rows.value] for t in tabs])
        assert got[s].shape == want.shape and np.array_equal(got[s].view(np.uint32), want.view(np.uint32)), s
    assert got[1].size > fc.STAGE_PASS


# ------------------------------------------------------------------------------------------------ slot reuse
def _run_reuse(slots):
    """The `reuse` list through one feeder, in order: the slot's whole matrix after every batch."""
    from eesen_amd.api import Feeder
    f = Feeder(slots=slots)
    out = []
    for stages, mats in fc.reuse():
        if stages:
            f.set_pipeline(_stages(stages))
            slot = f.submit_raw(mats)
        else:
            slot = f.submit(mats)
        out.append((slot, slot_matrix(f, slot)))
    return out


def test_slot_reuse(gpu):
    one = _run_reuse(1)
    lds = []
    for (slot, host), (stages, mats) in zip(one, fc.reuse()):
        D = _out_dim(stages, mats[0].shape[1])
        want = [ofe.run_pipeline(stages, m) for m in mats]
        want = [np.zeros((0, D), np.float32) if w is None else w for w in want]
        assert slot == 0 and host.shape[1] == _ld(D)
        assert same_bits(host, want), (stages, [m.shape for m in mats])
        lds.append((D, host.shape[1]))
    assert lds == [(40, 40), (13, 16), (39, 40), (117, 120), (40, 40)]
    two = _run_reuse(2)
    assert [slot for slot, _ in two] == [0, 1, 0, 1, 0]
    for (_, a), (_, b) in zip(one, two):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------ one slot under a consumer
def test_one_slot_under_a_consumer(gpu):
    """slots = 1: a submit must wait until the consumer of the slot's previous batch has read it.  Three batches; for each: submit,
    acquire, Propagate on the view, release -- and the next submit at once, nothing read back or synchronised in between.  A net's
    output is valid until its next Propagate, so each batch goes to a net of its own made from the same layers (one compute stream:
    the three forward passes still run one after the other, each reading the slot the next submit is waiting to overwrite); the three
    outputs are read at the end and equal the outputs of the same net fed the host-interleaved matrices, bit for bit."""
    from eesen_amd.api import Net, Feeder
    cfg = synth.config("tiny_bi"); cfg.update(D=13)
    layers = synth.make_model(**cfg)
    rng = np.random.default_rng(11)
    batches = [[rng.standard_normal((t, 13)).astype(np.float32) for t in lens] for lens in ([300, 120, 7], [40, 300, 299, 1], [150, 2, 300])]
    f = Feeder(slots=1)
    nets, outs = [Net.from_layers(layers) for _ in batches], []
    for net, mats in zip(nets, batches):
        net.SetSeqLengths([m.shape[0] for m in mats])
        slot = f.submit(mats)
        outs.append(net.Propagate(f.acquire(slot)))
        f.release(slot)
    got = [o.numpy() for o in outs]
    ref = Net.from_layers(layers)
    for mats, g in zip(batches, got):
        ref.SetSeqLengths([m.shape[0] for m in mats])
        want = ref.Propagate(interleave(mats, 13)[0]).numpy()
        assert g.shape == want.shape and np.array_equal(g.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------ run to run
@pytest.mark.parametrize("case", ["assembly_scalar", "stages_long"])
def test_run_to_run(gpu, case):
    first = _first_run(case)[0 if case == "stages_long" else 1]
    second = _submit_plain(fc.assembly_scalar())[1] if case == "assembly_scalar" else _run_case(case)[1]
    assert first.shape == second.shape and np.array_equal(first.view(np.uint32), second.view(np.uint32))
