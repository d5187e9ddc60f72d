"""-m gpu: Plan() of one recurrent layer, every field, against what the commit before the planner was moved out of the kernel file
answered for the same shape and switches (tests/golden/plans.json).

The plan names the instantiation that runs a layer's recurrence, its tile, grid, windows and launches, and the registers and LDS the
device reports for the very host stub the launcher uses ("vgprs", "lds_bytes", "free_vgprs_per_simd_lane"): a table row whose name
and address disagree, a clamp that drifted, or a switch that no longer reaches the selection shows here as a changed field.

Cases: one recurrent layer of the given width, an affine layer to 46 outputs and a softmax; 40 inputs, 8 frames, one Propagate
before Plan() (the forward plan depends on the layer's exchange buffer being reserved).  8 frames are enough: a plan depends on T
only through T < 2, the 2 GB offset limits and the backward chunk, which the full-size tests cover.  The switches are read when a
Net is created, so each case sets its own before it creates one.

`python -m tests.test_gpu_plans --record FILE` writes the answers of the library that is built in the tree.  The committed file was
recorded twice on the earlier commit; the two recordings agree on every case -- also on the ones whose forward tile depends on what the
residency census of the narrow tile saw on the idle device (512 cells at 64 sequences: two workgroups per CU).
"""
import json
import os

import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plans.json")
D, T, K = 40, 8, 46
SWITCHES = ("EESEN_PERSISTENT", "EESEN_FWD_SPLIT", "EESEN_FWD_F16", "EESEN_FWD_MUX", "EESEN_FWD_NARROW2", "EESEN_FWD_T16_SMALL",
            "EESEN_BWD_Q4", "EESEN_BWD_Q4_ST8", "EESEN_BWD_KSPLIT", "EESEN_BWD_MUX", "EESEN_BWD_F16")
# (layer kind, cells, sequences, switches, recurrent dropout, SetForwardPrecision)
_BI, _UNI = "BiLstmParallel", "LstmParallel"
CASES = [(_BI, H, S, {}, False, 0) for H, S in ((512, 16), (512, 32), (512, 64), (320, 10), (320, 32), (256, 32), (768, 32),
                                                (1024, 16), (1024, 32), (1024, 64), (20, 17))]
CASES += [(_BI, 512, 32, {}, True, 0), (_BI, 1024, 32, {}, False, 1), (_UNI, 1024, 32, {}, False, 0)]
CASES += [(_BI, 1024, 64, e, False, 0) for e in ({"EESEN_FWD_SPLIT": "0"},
                                                 {"EESEN_FWD_SPLIT": "0", "EESEN_FWD_MUX": "0", "EESEN_BWD_MUX": "0"},
                                                 {"EESEN_BWD_F16": "0"}, {"EESEN_BWD_KSPLIT": "0"})]
CASES += [(_BI, 512, 32, e, False, 0) for e in ({"EESEN_FWD_SPLIT": "0"}, {"EESEN_FWD_F16": "0"}, {"EESEN_BWD_Q4": "0"})]
CASES += [(_BI, 512, 64, e, False, 0) for e in ({"EESEN_BWD_Q4_ST8": "0"}, {"EESEN_BWD_Q4_ST8": "2"}, {"EESEN_FWD_NARROW2": "0"})]
CASES += [(_BI, 512, 16, {"EESEN_FWD_T16_SMALL": "0"}, False, 0), (_BI, 512, 32, {"EESEN_PERSISTENT": "0"}, False, 0)]


def case_id(case):
    kind, H, S, env, drop, prec = case
    name = f"{'bi' if kind == _BI else 'uni'}{H}_s{S}"
    name += "".join(f"-{k[len('EESEN_'):]}={v}" for k, v in sorted(env.items()))
    return name + ("-dropout" if drop else "") + ("-bf16" if prec else "")


IDS = [case_id(c) for c in CASES]


def plan_of(case, setenv, delenv):
    from eesen_amd import synth
    from eesen_amd.api import Net
    kind, H, S, env, drop, prec = case
    for k in SWITCHES:
        delenv(k)
    for k, v in env.items():
        setenv(k, v)
    cfg = dict(kind=kind, layers=1, H=H, D=D, K=K, S=S, T=T)
    layers = synth.make_model(**cfg); batch = synth.make_batch(**cfg)
    if drop:
        layers[0]["dropout"] = dict(recurrent=0.25, rec_step=True, nml=True)
    net = Net.from_layers(layers); net.SetDropoutSeed(5); net.SetForwardPrecision(prec)
    net.SetSeqLengths(batch.lens)
    net.Propagate(batch.feats)
    plan = net.Plan()
    for k in env:
        delenv(k)
    return plan


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_plan_is_what_it_was(gpu, golden, monkeypatch, case):
    name = case_id(case)
    plan = plan_of(case, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    print(name, json.dumps(plan))
    assert plan == golden[name]


if __name__ == "__main__":
    import sys
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", "usage: python -m tests.test_gpu_plans --record FILE"
    rec = {case_id(c): plan_of(c, os.environ.__setitem__, lambda k: os.environ.pop(k, None)) for c in CASES}
    json.dump(rec, open(sys.argv[2], "w"), indent=1, sort_keys=True)
    print(f"{len(rec)} plans -> {sys.argv[2]}")
