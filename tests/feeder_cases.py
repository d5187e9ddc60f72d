"""Case list of the feeder's full-size tests (tests/test_feeder_cases.py on the CPU, tests/test_gpu_feeder_fullsize.py on the GPU):
the shapes at which the three kernels of eesen_amd/csrc/feeder.hip go round their grid-stride loops more than once, the limits
`set_pipeline` accepts, utterances a pipeline empties in the middle of a batch, and a list of batches for one slot.  Every input is a
function of its case's name alone; nothing is stored but tests/golden/frontend_edges.npz (the reference's own add-deltas and
splice-feats at the `limits` options, made by oracle/make_golden_frontend_edges.py).

A stage is named as oracle/frontend.py takes it: ("cmvn", norm_vars), ("splice", L, R), ("subsample", n, offset), ("deltas", order,
window).  tests/test_feeder_cases.py holds, with the restatements alone, the conditions the GPU checks rely on -- above all that each
`*_long` case and each assembly really lies past one pass of its kernel's grid.
"""
import hashlib
import os

import numpy as np

from oracle import frontend as ofe

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend_edges.npz")

# The two caps, restated.  Each kernel is a grid-stride loop over work items, 256 threads to a workgroup:
#   interleave_kernel   Feeder::assemble launches min(cdiv(n, 256), 256 * 32) workgroups (`const int blocks = ...`); an item is a
#                       float4 of the output when D % 4 == 0, otherwise a float
#   feat_stage_kernel, feat_paste_kernel   stage_grid(biggest, S): at most 2048 workgroups along x, utterance = blockIdx.y; an item
#                       is one output element of that utterance
INTERLEAVE_PASS = 8192 * 256
STAGE_PASS = 2048 * 256
DELTA_LDS = 1200            # floats of `s_sc`, the delta windows' LDS array in feat_stage_kernel


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def _mats(name, lens, D):
    """Utterance matrices [t x D] float32 with per-column scales and offsets, a function of `name` alone."""
    rng = np.random.default_rng(_seed(name))
    scale, shift = rng.uniform(0.5, 3.0, D), rng.uniform(-2.0, 2.0, D)
    return [(rng.standard_normal((int(t), D)) * scale + shift).astype(np.float32) for t in lens]


def stats_for(name, D):
    """A [2 x (D+1)] CMVN statistics matrix of dimension D, as `stats_for` of tests/test_gpu_frontend.py makes them."""
    rng = np.random.default_rng(_seed(name + "/stats"))
    st = np.zeros((2, D + 1))
    st[0, :D] = rng.standard_normal(D) * 50
    st[1, :D] = 100 + rng.random(D) * 400
    st[0, D] = 57
    return st


def input_hash(mats):
    return hashlib.sha256(b"".join(np.ascontiguousarray(m, "<f4").tobytes() for m in mats)).hexdigest()[:16]


# ---------------------------------------------------------------------------------------------- assemblies past one pass
def assembly_vec():
    """D = 40 (float4 items), S = 64: the utterances at 9 and 63 have 3300 frames, the other 62 have 1 .. 3270."""
    rng = np.random.default_rng(_seed("assembly_vec/lens"))
    lens = rng.integers(1, 3271, 64)
    lens[9] = lens[63] = 3300
    return _mats("assembly_vec", lens, 40)


def assembly_scalar():
    """D = 13 (ld 16, float items), S = 64: the utterances at 0 and 40 have 2600 frames, the rest 0 .. 2500, the one at 17 none; the
    matrix at 3 is a row-strided view (every other column block of a wider array)."""
    rng = np.random.default_rng(_seed("assembly_scalar/lens"))
    lens = rng.integers(0, 2501, 64)
    lens[0] = lens[40] = 2600
    lens[17] = 0
    mats = _mats("assembly_scalar", lens, 13)
    wide = np.zeros((mats[3].shape[0], 32), np.float32)
    wide[:, 5:18] = mats[3]
    mats[3] = wide[:, 5:18]
    assert mats[3].strides[0] == 128 and not mats[3].flags.c_contiguous
    return mats


def second_pass_rows(lens, D):
    """(valid, padding): how many output rows t*S + s of the assembly lie wholly in the interleave's second pass (every item index of
    the row >= INTERLEAVE_PASS) and hold a frame of their utterance / zero padding."""
    lens = np.asarray(lens)
    S, T = len(lens), int(lens.max())
    dv = D // 4 if D % 4 == 0 else D
    first = -(-INTERLEAVE_PASS // dv)
    r = np.arange(first, T * S)
    valid = (r // S) < lens[r % S]
    return int(valid.sum()), int((~valid).sum())


# ---------------------------------------------------------------------------------------------- stages past one pass
def stages_long():
    """dict(stages, mats, stats, long, past): 4400 x 40 in the middle of utterances of 7, 1, 0, 300 and 2 frames through
    splice(1,1) -> cmvn(norm_vars) -> deltas(2,2) -> subsample(3,0); every stage's output of the long utterance lies past STAGE_PASS."""
    stages = [("splice", 1, 1), ("cmvn", True), ("deltas", 2, 2), ("subsample", 3, 0)]
    return dict(stages=stages, mats=_mats("stages_long", [7, 1, 4400, 0, 300, 2], 40), stats=stats_for("stages_long", 120), long=2, past=(0, 1, 2, 3))


def repeat_long():
    """1400 x 40 beside short utterances through splice(2,2) -> subsample(-2,0): the repeat branch t / (-n) writes 560,000 elements.  The
    splice in front of it writes 280,000: only the last stage is held past STAGE_PASS."""
    stages = [("splice", 2, 2), ("subsample", -2, 0)]
    return dict(stages=stages, mats=_mats("repeat_long", [3, 1400, 1, 64], 40), stats=None, long=1, past=(1,))


def emptied():
    """D = 8, lengths 20, 2, 0, 9, 1 through cmvn(False) -> splice(1,1) -> subsample(3,2) -> deltas(2,2): the utterances of 2 and 1 frames
    are emptied by the subsampling and the one of 0 frames enters empty, each between utterances that survive."""
    stages = [("cmvn", False), ("splice", 1, 1), ("subsample", 3, 2), ("deltas", 2, 2)]
    return dict(stages=stages, mats=_mats("emptied", [20, 2, 0, 9, 1], 8), stats=stats_for("emptied", 8), gone=(1, 2, 4))


def boundaries(stages, feats, stats=None):
    """The matrix behind every stage, one stage of oracle/frontend.run_pipeline at a time: [x_1, .., x_n], None from the stage on that
    leaves no frame (and for an utterance that enters without one: the reference's tools cannot hold such a matrix)."""
    out, x = [], np.asarray(feats, np.float32)
    for st in stages:
        x = ofe.run_pipeline([st], x, stats) if x is not None else None
        out.append(x)
    return out


# ---------------------------------------------------------------------------------------------- the limits of set_pipeline
LIMIT_LENS = [1, 2, 7, 40]
LIMIT_D = 3
LIMIT_PIPELINES = {
    "deltas_8_16": [("deltas", 8, 16)],
    "deltas_8_1": [("deltas", 8, 1)],
    "deltas_1_16": [("deltas", 1, 16)],
    "splice_40_24": [("splice", 40, 24)],
    "splice_64_0": [("splice", 64, 0)],
    "splice_0_64": [("splice", 0, 64)],
    "splice_2_2_deltas_8_16": [("splice", 2, 2), ("deltas", 8, 16)],
}
# just beyond: order 9, window 17, context 65 -- (stages, what the refusal's message names)
LIMIT_REFUSALS = [([("deltas", 9, 16)], "add-deltas: order 0..8, window 1..16"), ([("deltas", 8, 17)], "add-deltas: order 0..8, window 1..16"),
                  ([("splice", 65, 0)], "splice-feats: context must be 0..64 frames"), ([("splice", 0, 65)], "splice-feats: context must be 0..64 frames"),
                  ([("splice", 40, 25)], "splice-feats: context must be 0..64 frames")]


def limit_utts():
    return [(f"lim_u{i}", m) for i, m in enumerate(_mats("limits", LIMIT_LENS, LIMIT_D))]


def reference_tail(stages):
    """The stages as the reference's tools behind a pipe: `splice-feats ... ark:- ark:- | add-deltas ... ark:- ark:- |`."""
    cmd = {"splice": "splice-feats --left-context={} --right-context={} ark:- ark:- |", "deltas": "add-deltas --delta-order={} --delta-window={} ark:- ark:- |"}
    return " ".join(cmd[s[0]].format(s[1], s[2]) for s in stages)


def deltas_bound(feats, order, window):
    """Per element of add-deltas' output, n_taps * 2^-24 * sum_j |w_j * x_j|: the first-order bound of any fp32 evaluation order of the
    tap sum (products and additions rounded, fused or not), n_taps = 1 + 2 * o * window the window length of the element's order o."""
    x = np.asarray(feats, np.float64)
    T, D = x.shape
    out = np.zeros((T, D * (order + 1)))
    for o, sc in enumerate(ofe.delta_scales(order, window)):
        half = (sc.size - 1) // 2
        acc = np.zeros((T, D))
        for j in range(-half, half + 1):
            acc += abs(float(sc[j + half])) * np.abs(x[np.clip(np.arange(T) + j, 0, T - 1)])
        out[:, o * D:(o + 1) * D] = sc.size * 2.0 ** -24 * acc
    return out * (1 + 2.0 ** -40)     # (the bound's own sum rounds)


def limit_bound(stages, raw):
    """The bound on |oracle - reference| for a `limits` pipeline on `raw`: None where it must be exact (splices only: copies), else the
    deltas' bound on what the stages in front of them (copies) hand them."""
    if stages[-1][0] != "deltas":
        return None
    assert all(s[0] == "splice" for s in stages[:-1])
    return deltas_bound(ofe.run_pipeline(stages[:-1], raw), stages[-1][1], stages[-1][2])


# ---------------------------------------------------------------------------------------------- paste past one pass
PASTE_WIDTHS = (43, 1, 40, 3)
PASTE_TOLERANCE = 2
PASTE_SHORTEST = [3, 6100, 0, 1, 250]


def paste_long():
    """(tables, frames [4 x 5]): S = 5, the shortest input's rows PASTE_SHORTEST and the others up to 2 rows longer -- but for utterance 3,
    whose third input is 3 rows longer (dropped by the tolerance rule); utterance 2 has an empty input (dropped).  Utterance 1 joins to
    6100 x 87 = 530,700 elements."""
    rng = np.random.default_rng(_seed("paste_long"))
    S, n = len(PASTE_SHORTEST), len(PASTE_WIDTHS)
    frames = np.array(PASTE_SHORTEST)[None, :] + rng.integers(0, PASTE_TOLERANCE + 1, (n, S))
    frames[np.arange(S) % n, np.arange(S)] = PASTE_SHORTEST       # the shortest input differs from utterance to utterance
    frames[2, 3] = PASTE_SHORTEST[3] + PASTE_TOLERANCE + 1
    tabs = [[rng.normal(0.0, 1.0, (int(frames[j, s]), w)).astype(np.float32) for s in range(S)] for j, w in enumerate(PASTE_WIDTHS)]
    return tabs, frames


# ---------------------------------------------------------------------------------------------- one slot, batch after batch
def reuse():
    """[(stages, mats)] for one slot, in order: larger then smaller; float4, scalar, float4 interleave; no pipeline, one stage (the
    result ends in the slot's second packed buffer), two stages (it ends in the first); and a last batch whose assembled matrix holds
    more rows (and floats) than any before it, so that the slot's matrix grows after it was reused."""
    spec = [([], [500, 300], 40), ([], [7, 3, 0, 5], 13), ([("splice", 1, 1)], [40, 12], 13), ([("splice", 1, 1), ("deltas", 2, 2)], [9], 13),
            ([], [640, 640, 1], 40)]
    return [(st, _mats(f"reuse/{i}", lens, D)) for i, (st, lens, D) in enumerate(spec)]
