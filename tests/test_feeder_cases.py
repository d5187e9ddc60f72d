"""CPU: the conditions the feeder's full-size GPU tests rely on (tests/feeder_cases.py), held with the restatements alone, so that a
later edit of a case cannot silently take it back under a cap; and oracle/frontend.py at the limits set_pipeline accepts against the
reference's own add-deltas and splice-feats (tests/golden/frontend_edges.npz, oracle/make_golden_frontend_edges.py)."""
import json

import numpy as np
import pytest

from eesen_amd.batching import interleave
from oracle import frontend as ofe
from tests import feeder_cases as fc


@pytest.mark.parametrize("case,D,two_longest", [(fc.assembly_vec, 40, 3300), (fc.assembly_scalar, 13, 2600)])
def test_assemblies_lie_past_one_pass(case, D, two_longest):
    mats = case()
    lens = [m.shape[0] for m in mats]
    assert len(mats) == 64 and all(m.shape[1] == D and m.dtype == np.float32 for m in mats)
    assert sorted(lens)[-2:] == [two_longest, two_longest] and sorted(lens)[-3] < two_longest
    out, _, T = interleave(mats, D)
    items = out.size // 4 if D % 4 == 0 else out.size         # from the restatement's matrix, not from constants typed twice
    assert items > fc.INTERLEAVE_PASS, (items, fc.INTERLEAVE_PASS)
    valid, padding = fc.second_pass_rows(lens, D)
    print(f"{case.__name__}: T {T}, {items} items, rows wholly in the second pass: {valid} of frames, {padding} of padding")
    assert valid >= 3 and padding >= 3
    if case is fc.assembly_scalar:
        assert min(lens) == 0
        assert sum(not m.flags.c_contiguous for m in mats) == 1, "one matrix is a row-strided view"
    else:
        assert min(lens) >= 1


@pytest.mark.parametrize("case", [fc.stages_long, fc.repeat_long])
def test_long_stage_cases_lie_past_one_pass(case):
    c = case()
    long = c["mats"][c["long"]]
    assert all(m.shape[0] < long.shape[0] for i, m in enumerate(c["mats"]) if i != c["long"])
    sizes = [x.size for x in fc.boundaries(c["stages"], long, c["stats"])]
    print(f"{case.__name__}: the long utterance's outputs hold {sizes} elements, one pass covers {fc.STAGE_PASS}")
    for k in c["past"]:
        assert sizes[k] > fc.STAGE_PASS, (c["stages"][k], sizes[k])
    assert len(c["stages"]) - 1 in c["past"], "the last stage at least"
    if case is fc.stages_long:
        assert c["past"] == tuple(range(len(c["stages"]))) and sizes[2] > 3 * fc.STAGE_PASS, "every stage; the deltas need four passes"
        assert sorted(m.shape[0] for m in c["mats"]) == [0, 1, 2, 7, 300, 4400] and 0 < c["long"] < len(c["mats"]) - 1
        assert c["stats"].shape == (2, 121), "statistics of the 120-column boundary"


def test_paste_long_lies_past_one_pass():
    from eesen_amd.frontend import paste_frames
    tabs, frames = fc.paste_long()
    assert [int(f) for f in frames.min(axis=0)] == fc.PASTE_SHORTEST and tuple(t[0].shape[1] for t in tabs) == fc.PASTE_WIDTHS
    rows = [paste_frames(frames[:, s], fc.PASTE_TOLERANCE) for s in range(frames.shape[1])]
    assert rows == [3, 6100, 0, 0, 250]
    assert frames[:, 2].max() > 0 and frames[:, 3].min() > 0, "one dropped by an empty input, one by the tolerance rule"
    assert frames[:, [0, 1, 4]].max(axis=0).tolist() != frames[:, [0, 1, 4]].min(axis=0).tolist(), "inputs longer than the join"
    joined = np.hstack([t[1][:rows[1]] for t in tabs])
    assert joined.size > fc.STAGE_PASS, joined.size


def test_emptied_utterances():
    c = fc.emptied()
    got = [ofe.run_pipeline(c["stages"], m, c["stats"]) for m in c["mats"]]
    assert tuple(i for i, g in enumerate(got) if g is None) == c["gone"] == (1, 2, 4)
    assert [m.shape[0] for m in c["mats"]] == [20, 2, 0, 9, 1]
    assert [g.shape for g in got if g is not None] == [(6, 72), (3, 72)]


def test_reuse_list():
    batches = fc.reuse()
    dims, floats, rows = [], [], []
    for stages, mats in batches:
        outs = [ofe.run_pipeline(stages, m) for m in mats]
        D = next(o.shape[1] for o in outs if o is not None)
        T = max(o.shape[0] for o in outs if o is not None)
        dims.append(D)
        rows.append(T * len(mats))
        floats.append(T * len(mats) * ((D + 3) // 4 * 4))
    assert dims == [40, 13, 39, 117, 40], "float4, scalar, scalar, scalar, float4"
    assert [len(st) for st, _ in batches] == [0, 0, 1, 2, 0]
    assert rows[1] < rows[0] and floats[1] < floats[0], "larger then smaller"
    assert rows[-1] > max(rows[:-1]) and floats[-1] > max(floats[:-1]), "the last batch makes the slot's matrix grow"
    assert any(m.shape[0] == 0 for m in batches[1][1])


def test_limits_fit_the_scale_table():
    sc = ofe.delta_scales(8, 16)
    assert sum(len(s) for s in sc) == 1161 <= fc.DELTA_LDS
    assert [len(s) for s in sc] == [1 + 32 * o for o in range(9)]
    assert sum(len(s) for s in sc) > 4 * 256, "the LDS fill loop of a 256-thread workgroup goes round more than once"
    for stages in fc.LIMIT_PIPELINES.values():
        for s in stages:
            assert (s[0] == "deltas" and s[1] <= 8 and 1 <= s[2] <= 16) or (s[0] == "splice" and s[1] + s[2] <= 64)
    for stages, _ in fc.LIMIT_REFUSALS:
        (s,) = stages
        assert (s[0] == "deltas" and (s[1] == 9 or s[2] == 17)) or (s[0] == "splice" and s[1] + s[2] == 65)


def test_oracle_at_the_limits_against_the_reference_tools():
    """Splices: the fixture exactly.  Deltas: |oracle - fixture| <= n_taps * 2^-24 * sum_j |w_j * x_j| per element (the reference's
    AddVec is a BLAS saxpy: only the order of rounding differs)."""
    gold = np.load(fc.GOLDEN)
    utts = fc.limit_utts()
    assert str(gold["hash"]) == fc.input_hash([m for _, m in utts]), "the generator of the inputs has drifted from the fixture"
    assert json.loads(str(gold["names"])) == sorted(fc.LIMIT_PIPELINES)
    assert [m.shape for _, m in utts] == [(t, fc.LIMIT_D) for t in fc.LIMIT_LENS]
    worst = 0.0
    for name, stages in sorted(fc.LIMIT_PIPELINES.items()):
        for k, raw in utts:
            ref = gold[f"out/{name}/{k}"]
            mine = ofe.run_pipeline(stages, raw)
            assert mine.shape == ref.shape and ref.dtype == np.float32, (name, k)
            bound = fc.limit_bound(stages, raw)
            if bound is None:
                assert np.array_equal(mine.view(np.uint32), ref.view(np.uint32)), (name, k)
                continue
            diff = np.abs(mine.astype(np.float64) - ref.astype(np.float64))
            ratio = float(np.max(diff[bound > 0] / bound[bound > 0], initial=0.0))
            worst = max(worst, ratio)
            assert np.all(diff <= bound), (name, k, ratio)
    print(f"oracle/frontend.py against the reference's add-deltas at the limits: worst |difference| / bound {worst:.4f}")
    assert sum(st[-1][0] == "deltas" for st in fc.LIMIT_PIPELINES.values()) == 4 and len(fc.LIMIT_PIPELINES) == 7
