"""GPU: CMVN statistics on the device (eesen_cmvn_stats_parallel, the feeder's statistics tap) against tests/golden/cmvn_stats.npz, i.e.
what the reference's compute-cmvn-stats wrote.  On the exact cases (tests/cmvn_stats_cases.py) the device is held to the fixture bit
for bit; on the wide case to the first-order bound of any fp64 summation order, n * 2^-53 * sum |t_i|.  The tap is held bit for bit to
the stand-alone call on the same boundary's features."""
import functools

import numpy as np
import pytest

from tests import cmvn_stats_cases as cc
from tests import paste_cases as pc

pytestmark = pytest.mark.gpu
CMVN, SPLICE, SUBSAMPLE, DELTAS, FBANK, FBANK_PITCH = 1, 2, 3, 4, 5, 6


@functools.lru_cache(maxsize=None)
def gold():
    return cc.load()


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def report(name, got, want):
    d = np.abs(got - want)
    print(f"{name}: max |device - fixture| = {d.max():.3e} at {np.unravel_index(np.argmax(d), d.shape)}")


@pytest.mark.parametrize("tag", ["u", "w"])
def test_every_shape_alone(gpu, tag):
    """S = 1: every exact utterance in a call of its own, and the empty one."""
    from eesen_amd import api
    g = gold()
    items = [(cc.name_of(T, D),) + cc.utt(T, D) for T, D in cc.SHAPES] + ([("inf7x3",) + cc.inf_utt()] if tag == "w" else [])
    for n, x, w in items:
        got = api.cmvn_stats([x], [w] if tag == "w" else None)[0]
        report(f"{n}/{tag}", got, g[f"shapes/{tag}/{n}"])
        assert same_bits(got, g[f"shapes/{tag}/{n}"]), n
    T, D = cc.EMPTY
    got = api.cmvn_stats([np.zeros((T, D), np.float32)], [np.zeros(0, np.float32)] if tag == "w" else None)[0]
    assert got.shape == (2, D + 1) and not got.any()


def test_three_ragged_with_an_empty_one_and_wide_strides(gpu):
    """S = 3 at D = 40, an utterance without a frame between them; the matrices are column slices of wider ones (row stride 56); and
    weights for one utterance only (None: all ones)."""
    from eesen_amd import api
    g = gold()
    mats, ws = [], []
    for T, D in [cc.D40[0], cc.EMPTY, cc.D40[1]]:
        x, w = cc.utt(T, D)
        wide = np.full((T, 56), np.nan, np.float32)
        wide[:, 8:48] = x
        mats.append(wide[:, 8:48])
        ws.append(w)
    assert mats[0].strides[0] == 56 * 4
    got = api.cmvn_stats(mats)
    assert same_bits(got[0], g["shapes/u/u257x40"]) and not got[1].any() and same_bits(got[2], g["shapes/u/u3000x40"])
    got = api.cmvn_stats(mats, [None, None, ws[2]])
    assert same_bits(got[0], g["shapes/u/u257x40"]) and not got[1].any() and same_bits(got[2], g["shapes/w/u3000x40"])
    # per speaker and global: sums of the utterances' matrices on the host (what the tool does)
    d40 = api.cmvn_stats([cc.utt(T, D)[0] for T, D in cc.D40])
    assert same_bits(d40[0] + d40[1], g["d40/u/spkA"]) and same_bits(d40[2], g["d40/u/spkB"])
    assert np.array_equal((d40[0] + d40[1] + d40[2]).astype(np.float32), g["d40/u/global"])


@pytest.mark.parametrize("T,D", cc.LONG)
def test_batch_of_33_and_alone_give_the_same_bits(gpu, T, D):
    from eesen_amd import api
    g = gold()
    items = cc.b33(T, D)
    for tag in ("u", "w"):
        ws = [w for _, _, w in items] if tag == "w" else None
        got = api.cmvn_stats([x for _, x, _ in items], ws)
        again = api.cmvn_stats([x for _, x, _ in items], ws)
        assert all(same_bits(a, b) for a, b in zip(got, again)), "two runs differ"
        long = got[cc.B33_AT]
        report(f"b33 {cc.name_of(T, D)}/{tag}", long, g[f"shapes/{tag}/{cc.name_of(T, D)}"])
        assert same_bits(long, g[f"shapes/{tag}/{cc.name_of(T, D)}"]), "the long utterance differs inside the batch"
        for i in (0, 16, 18, 32):      # its neighbours and the ends against the restatement: says which one where the hash would not
            n, x, w = items[i]
            assert same_bits(got[i], cc.restate(x, w if tag == "w" else None)), n
        assert cc.matrices_hash(got) == str(g[f"b33_{T}x{D}/{tag}/hash"])


@pytest.mark.parametrize("tag", ["u", "w"])
def test_wide_case_within_the_order_bound_and_reproducible(gpu, tag):
    from eesen_amd import api
    x, w = cc.wide_utt()
    wv = w if tag == "w" else None
    exact, bound = cc.restate(x, wv), cc.order_bound(x, wv)
    alone = api.cmvn_stats([x], [wv] if wv is not None else None)[0]
    err = np.abs(alone - exact)
    print(f"wide/{tag}: max |device - fsum| / bound = {np.max(err[bound > 0] / bound[bound > 0]):.3e}; reference: "
          f"{np.max(np.abs(gold()[f'wide/{tag}'] - exact)[bound > 0] / bound[bound > 0]):.3e}")
    assert np.all(err <= bound)
    # alone, twice, and between other utterances of its width at another position: equal bits
    others = [cc.exact_utt(f"w{i}", 1 + 97 * i, 7) for i in range(4)]
    mats = [o[0] for o in others[:3]] + [x] + [others[3][0]]
    ws = [o[1] for o in others[:3]] + [w] + [others[3][1]] if wv is not None else None
    batch = api.cmvn_stats(mats, ws)
    assert same_bits(batch[3], alone) and same_bits(api.cmvn_stats([x], [wv] if wv is not None else None)[0], alone)


def test_stand_alone_refusals(gpu):
    from eesen_amd import api
    from eesen_amd._lib import EesenError
    x = np.zeros((4, 3), np.float32)
    with pytest.raises(EesenError, match="does not match"):
        api.cmvn_stats([x, np.zeros((4, 5), np.float32)])
    with pytest.raises(EesenError, match="wrong dimension"):
        api.cmvn_stats([x], [np.ones(3, np.float32)])
    with pytest.raises(EesenError, match="empty minibatch"):
        api.cmvn_stats([])


# ---------------------------------------------------------------------------------------------- the feeder's tap
def unpack(host, frames, S, D):
    """The per-utterance matrices of an assembled [T*S x ld] slot."""
    T = host.shape[0] // S
    cube = host.reshape(T, S, host.shape[1])
    return [np.ascontiguousarray(cube[:f, s, :D]) for s, f in enumerate(frames)]


def read_slot(f, slot):
    from eesen_amd.api import CuMatrix
    got = f.acquire(slot)
    host = CuMatrix.view(got.ptr, got.rows, got.stride, got.stride, got.device, keepalive=f).numpy()
    f.release(slot)
    return host, got.cols


def raw_mats():
    """Ragged D = 23 matrices (rows not 16-byte aligned), longer than one chunk of the kernel and shorter."""
    return [cc.exact_utt(f"tap{i}", T, 23)[0] for i, T in enumerate([300, 7, 161, 1, 1000])]


def test_tap_at_every_boundary_of_a_splice_deltas_pipeline(gpu):
    from eesen_amd import api
    stages = [(SPLICE, 1, 1), (DELTAS, 2, 2)]
    mats = raw_mats()
    for b in range(len(stages) + 1):
        # the boundary's own features: a feeder whose pipeline ends there, tap off
        ref = api.Feeder()
        ref.set_pipeline(stages[:b])
        host, D = read_slot(ref, ref.submit_raw(mats))
        feats = unpack(host, [m.shape[0] for m in mats], len(mats), D)
        want = api.cmvn_stats(feats)
        f = api.Feeder()
        f.set_pipeline(stages)
        f.set_stats_tap(b)
        slot = f.submit_raw(mats)
        got = f.stats(slot)
        assert len(got) == len(mats) and got[0].shape == (2, D + 1) and D == 23 * [1, 3, 9][b]
        for s, (a, w) in enumerate(zip(got, want)):
            assert same_bits(a, w), (b, s)
            if b == 0:
                assert same_bits(a, cc.restate(mats[s]))
        # with the tap on, acquire returns what it returns with the tap off
        on, _ = read_slot(f, slot)
        f.set_stats_tap(-1)
        off, _ = read_slot(f, f.submit_raw(mats))
        assert np.array_equal(on.view(np.uint32), off.view(np.uint32))


def test_tap_on_a_plain_submit_and_slot_reuse(gpu):
    from eesen_amd import api
    f = api.Feeder(slots=2)
    f.set_stats_tap(0)
    mats = raw_mats()
    slots = [f.submit(mats[:3]), f.submit(mats[3:]), f.submit(mats[1:4])]
    assert slots[2] == slots[0]
    want = api.cmvn_stats(mats)
    for a, w in zip(f.stats(slots[1]), want[3:]):
        assert same_bits(a, w)
    for a, w in zip(f.stats(slots[2]), want[1:4]):
        assert same_bits(a, w)


@pytest.mark.parametrize("head", ["fbank", "fbank_pitch"])
def test_tap_on_the_head_stages(gpu, head):
    """The statistics of what the filterbank (+ pitch) head writes, at dither 0, against the stand-alone extractors' output."""
    from eesen_amd import api
    c = pc.load_golden()["tol2_16k"]
    waves = [np.asarray(w, np.float32) for w in c["waves"]]
    fb = api.Fbank(**c["fbank"]).compute(waves)
    f = api.Feeder()
    f.set_fbank(**c["fbank"])
    if head == "fbank":
        feats = fb
        f.set_pipeline([(FBANK, 0, 0), (DELTAS, 2, 2)])
    else:
        pt = api.Pitch(**c["pitch"]).compute(waves, process=True)
        feats = api.paste_feats([fb, pt], c["tolerance"])
        f.set_pitch(**c["pitch"])
        f.set_pipeline([(FBANK_PITCH, c["tolerance"], 0), (DELTAS, 2, 2)])
    f.set_stats_tap(1)
    D = next(m.shape[1] for m in feats if m is not None)
    kept = [m if m is not None else np.zeros((0, D), np.float32) for m in feats]
    assert sum(m.shape[0] > 0 for m in kept) >= 2
    got = f.stats(f.submit_raw([w.reshape(-1, 1) for w in waves]))
    for s, (a, w) in enumerate(zip(got, api.cmvn_stats(kept))):
        assert same_bits(a, w), s


def test_tap_refusals(gpu):
    from eesen_amd import api
    from eesen_amd._lib import EesenError
    f = api.Feeder()
    mats = raw_mats()[:2]
    with pytest.raises(EesenError) as e:
        f.stats(0)
    assert e.value.code == -3                      # nothing submitted (and the tap is off)
    slot = f.submit_raw(mats)
    with pytest.raises(EesenError, match="tap is off") as e:
        f.stats(slot)
    assert e.value.code == -3
    with pytest.raises(EesenError) as e:
        f.set_stats_tap(1)                         # no pipeline: boundary 0 only
    assert e.value.code == -1
    with pytest.raises(EesenError) as e:
        f.set_stats_tap(-2)
    assert e.value.code == -1
    f.set_stats_tap(0)
    with pytest.raises(EesenError, match="without the statistics tap") as e:
        f.stats(slot)                              # submitted before the tap was set
    assert e.value.code == -3
    f.set_pipeline([(SPLICE, 1, 1), (DELTAS, 2, 2)])
    f.set_stats_tap(2)
    with pytest.raises(EesenError, match="beyond this pipeline") as e:
        f.set_pipeline([(SPLICE, 1, 1)])           # would leave the tap beyond the last boundary
    assert e.value.code == -1
    # the refused pipeline left no trace, and a refused batch leaves none either: the next batch takes the next slot
    a = f.submit_raw(mats)
    with pytest.raises(EesenError):
        f.submit_raw([np.zeros((0, 23), np.float32)])
    b = f.submit_raw(mats)
    assert b == (a + 1) % 2
    assert f.stats(a)[0].shape == (2, 23 * 9 + 1)
    for x, y in zip(f.stats(a), f.stats(b)):
        assert same_bits(x, y)


def test_bench_entry_answers(gpu):
    from eesen_amd import api
    ms = api.cmvn_stats_bench([cc.utt(257, 40)[0]] * 4, iters=3)
    assert 0.0 < ms < 100.0
