"""The cases of tests/test_gpu_recurrence_dropout.py (and what tests/test_dropout_cases.py holds of them without a GPU): one
BiLstmParallel layer with recurrent dropout per case, at every tile the DROP = true recurrence kernels of
eesen_amd/csrc/lstm_persistent.hip ship in.

  CASES      shape -> cells, sequences, frames and the rows of the kernel table that rec_plan.cpp takes there on a whole 256-CU device
             (read from lstm_fwd_plan / lstm_bwd_plan; the GPU test asserts them through Plan())
  VARIANTS   which dropout recipes run at which shape
  UNREACHED  DROP = true rows no case names, with the reason
  lengths / features / top gradients / masks: deterministic generators (a function of the shape, and of the recipe for the masks);
             the shape_* functions take (H, S, T, ndir) instead of a key of CASES (tests/recurrence_cases.py draws from them)
  seq_worst  the per-sequence metrics: the worst rel_err (max-norm) and the worst p999 of err_metrics over a case's sequences, each
             over that sequence's valid rows
"""
import copy

import numpy as np

from eesen_amd import synth
from tests.util import err_metrics, rel_err

D = 40           # input width of every case
P_REC = 0.25     # recurrent dropout probability
P_FWD = 0.2      # forward dropout probability of the one case that adds it

# shape -> H, S, T, forward row <CPW,MT,NT,true,false>, backward row <CPW,ST,true>, launches per pass (sequence windows).
# T: the smallest that still has a frame before and after the planted all-dropped frame of a length-T sequence and a shorter
# random length next to the lengths 1 and 2; 6 where the batch is large.
CASES = {
    "bi64_s8":    dict(H=64,   S=8,  T=8,  fwd=(1, 2, 1), bwd=(1, 16),  launches=1),
    "bi64_s12":   dict(H=64,   S=12, T=8,  fwd=(1, 2, 1), bwd=(1, 8),   launches=1),
    "bi128_s8":   dict(H=128,  S=8,  T=8,  fwd=(1, 2, 1), bwd=(2, 16),  launches=1),
    "bi128_s32":  dict(H=128,  S=32, T=8,  fwd=(1, 1, 2), bwd=(2, 8),   launches=1),
    "bi256_s24":  dict(H=256,  S=24, T=8,  fwd=(1, 1, 2), bwd=(4, 8),   launches=1),
    "bi256_s80":  dict(H=256,  S=80, T=6,  fwd=(1, 1, 4), bwd=(4, 16),  launches=1),
    "bi320_s10":  dict(H=320,  S=10, T=12, fwd=(2, 2, 1), bwd=(8, 8),   launches=1),
    "bi512_s32":  dict(H=512,  S=32, T=8,  fwd=(2, 1, 2), bwd=(8, 8),   launches=1),
    "bi512_s64":  dict(H=512,  S=64, T=6,  fwd=(2, 1, 4), bwd=(8, 16),  launches=1),
    "bi768_s16":  dict(H=768,  S=16, T=8,  fwd=(4, 1, 4), bwd=(16, 8),  launches=1),
    "bi1024_s32": dict(H=1024, S=32, T=8,  fwd=(4, 1, 4), bwd=(16, 16), launches=1),
    "bi1024_s64": dict(H=1024, S=64, T=6,  fwd=(4, 1, 4), bwd=(16, 16), launches=2),
}
# DROP = true rows of the table that no case reaches: row -> reason
UNREACHED = {
    "lstm_fwd_persistent_kernel<4,2,1,true,false>":
        "CPW = 4 on the 32 x 4 tile needs a BiLSTM of more than 512 cells that is no multiple of 16 (else the 16 x 16 tile is taken): at "
        "least 2 x 516 / 4 = 258 workgroups, and at 131 registers one workgroup fits a CU.  Asked on an MI355X (256 CUs) at H = 520, "
        "S = 8 with recurrent dropout, Plan() answers 'per-step kernels (lstm.hip)' for the forward pass (260 workgroups are not "
        "co-resident; the backward pass takes lstm_bwd_persistent_kernel<16,16,true> on 66): a 256-CU device never runs the row (dropout exists for the bidirectional layer only).",
}

# recipe -> the layer's dropout options.  "generated": the masks are drawn on the device and read back (the production path).
RECIPES = {
    "rnndrop":     dict(recurrent=P_REC, rec_step=True, rnndrop=True),
    "nml":         dict(recurrent=P_REC, rec_step=True, nml=True),
    "rnndrop_seq": dict(recurrent=P_REC, rec_seq=True, rnndrop=True),          # an [S x 2H] mask repeated over time
    "nml_fwd":     dict(forward=P_FWD, fw_step=True, recurrent=P_REC, rec_step=True, nml=True),
    "generated":   dict(recurrent=P_REC, rec_step=True, rnndrop=True),
}
_BOTH = ("bi64_s12", "bi320_s10", "bi512_s32", "bi1024_s64")     # both modes; the two modes alternate over the other shapes
VARIANTS = []
_alt = 0
for _name in CASES:
    if _name in _BOTH:
        VARIANTS += [(_name, "rnndrop"), (_name, "nml")]
    else:
        VARIANTS.append((_name, ("rnndrop", "nml")[_alt % 2])); _alt += 1
    if _name == "bi320_s10":
        VARIANTS.append((_name, "rnndrop_seq"))
    if _name == "bi512_s64":
        VARIANTS += [(_name, "nml_fwd"), (_name, "generated")]
IDS = [f"{c}-{r}" for c, r in VARIANTS]


def fwd_row(case):
    return "lstm_fwd_persistent_kernel<%d,%d,%d,true,false>" % CASES[case]["fwd"]


def bwd_row(case):
    return "lstm_bwd_persistent_kernel<%d,%d,true>" % CASES[case]["bwd"]


def _shape(case):
    c = CASES[case]
    return c["H"], c["S"], c["T"], 2


# ---- the generators, as functions of a shape (H cells per direction, S sequences, T frames, ndir directions): what the case-keyed
# functions below and tests/recurrence_cases.py both draw from.  The seed holds H, S and T only, so that this module's inputs are what
# they were before the generators took a shape.
def shape_rng(H, S, T, salt):
    return np.random.default_rng([H, S, T, salt])


def shape_layout(H, S, T, ndir=2):
    rng = shape_rng(H, S, T, 1)
    lens = rng.integers(3, T + 1, size=S).astype(np.int32)
    special, keep = set(), None
    for z in range(0, S, 16):
        at = z + rng.permutation(min(16, S - z))[:3]
        for a, n in zip(at, (T, 1, 2)):       # (a ragged last tile of fewer than three sequences: as many of them as it has)
            lens[a] = n
        special.update(int(a) for a in at)
        if z == 0:
            keep = int(at[0])
    drop = next((s for s in range(16 * ((S - 1) // 16), S) if s not in special), None)
    if drop is not None:
        lens[drop] = T
    return lens, keep, drop


def shape_lengths(H, S, T, ndir=2):
    """[S] int32.  Every 16-sequence tile holds a sequence of length T, one of length 1 and one of length 2, at places that differ
    from tile to tile; the rest are random in [3, T] (and the last tile holds a second sequence of length T: planted())."""
    return shape_layout(H, S, T, ndir)[0]


def shape_layer(kind, H):
    """[the one recurrent layer] of `kind` (BiLstmParallel / LstmParallel) with synth.make_model's weights."""
    return copy.deepcopy(synth.make_model(kind=kind, layers=1, H=H, D=D, K=4)[:1])


def shape_features(H, S, T, ndir, lens):
    """[T*S x D] fp32: N(0, 1) on valid rows, zero on padding."""
    x = shape_rng(H, S, T, 2).standard_normal((T, S, D)).astype(np.float32)
    x[np.arange(T)[:, None] >= lens[None, :]] = 0.0
    return x.reshape(T * S, D)


def shape_top_gradients(H, S, T, ndir, lens):
    """([(profile, od [T*S x ndir*H])], zero): profile "a" N(0, 1) on valid rows; "b" the same scaled, in every aligned group of four
    sequences, by 1, 2^-8, 2^-16, 2^-24, and every other group holds one sequence (`zero`) whose od is zero."""
    base = shape_rng(H, S, T, 3).standard_normal((T, S, ndir * H)).astype(np.float32)
    base[np.arange(T)[:, None] >= lens[None, :]] = 0.0
    b = base * (2.0 ** (-8.0 * (np.arange(S) % 4))).astype(np.float32)[None, :, None]
    zero = [4 * g + 1 for g in range(S // 4) if g % 2 == 1]
    b[:, zero, :] = 0.0
    return [("a", base.reshape(T * S, ndir * H)), ("b", b.reshape(T * S, ndir * H))], zero


# ---- the same, by a key of CASES
def _rng(case, salt):
    return shape_rng(*_shape(case)[:3], salt)


def lengths(case):
    """[S] int32.  Every 16-sequence tile holds a sequence of length T, one of length 1 and one of length 2, at places that differ
    from tile to tile (so the two sequence windows of bi1024_s64 get different patterns); the rest are random in [3, T]."""
    return shape_layout(*_shape(case))[0]


def planted(case):
    """(keep, drop): the sequence whose masks keep every cell (the length-T one of the first tile) and the sequence that has every
    cell dropped at frame T // 2, which under RNNDrop restarts the cell there: of length T, in the LAST tile (the second window of
    bi1024_s64), the first of its sequences that is none of the tile's T / 1 / 2 ones."""
    return shape_layout(*_shape(case))[1:]


def layer(case, recipe=None):
    """[the one BiLstmParallel layer] with synth.make_model's weights; recipe None: no dropout (the twin)."""
    L = shape_layer("BiLstmParallel", CASES[case]["H"])
    if recipe:
        L[0]["dropout"] = dict(RECIPES[recipe])
    return L


def features(case, lens):
    """[T*S x D] fp32: N(0, 1) on valid rows, zero on padding."""
    return shape_features(*_shape(case), lens)


def top_gradients(case, lens):
    """([(profile, od [T*S x 2H])], zero): profile "a" N(0, 1) on valid rows; "b" the same scaled, in every aligned group of four
    sequences, by 1, 2^-8, 2^-16, 2^-24, and every other group holds one sequence (`zero`) whose od is zero."""
    return shape_top_gradients(*_shape(case), lens)


def _draw(rng, rows, cols, p):
    return np.where(rng.random((rows, cols)) - p > 0, 1.0 / (1.0 - p), 0.0).astype(np.float32)


def masks(case, recipe):
    """dict(fwd [T*S x 2H] | None, rec [(T+2)*S x 2H], or [S x 2H] for a sequence mask): values in {0, 1 / (1 - p)}, random per (row,
    direction, unit), with the two planted sequences of planted().  Row (t + 1) * S + s of a time-step mask applies to frame t.
    A sequence mask has one row per sequence, so only the all-kept sequence can be planted in it."""
    c = CASES[case]; S, T, H = c["S"], c["T"], c["H"]
    o = RECIPES[recipe]
    rng = _rng(case, 4 + sorted(RECIPES).index(recipe))
    keep, drop = planted(case)
    kept = np.float32(1.0 / (1.0 - P_REC))
    if o.get("rec_seq"):
        rec = _draw(rng, S, 2 * H, P_REC)
        rec[keep] = kept
    else:
        rec = _draw(rng, (T + 2) * S, 2 * H, P_REC).reshape(T + 2, S, 2 * H)
        rec[:, keep] = kept
        rec[T // 2 + 1, drop] = 0.0
        rec = rec.reshape((T + 2) * S, 2 * H)
    fwd = _draw(rng, T * S, 2 * H, P_FWD) if o.get("forward", 0) > 0 else None
    return dict(fwd=fwd, rec=rec)


def step_mask(case, rec):
    """[T x S x 2H]: the recurrent mask value that applies to frame t of sequence s, from either mask shape."""
    c = CASES[case]; S, T, H = c["S"], c["T"], c["H"]
    if rec.shape[0] == S:
        return np.broadcast_to(rec[None], (T, S, 2 * H))
    return rec.reshape(T + 2, S, 2 * H)[1:T + 1]


def oracle_run(layers, feats, lens, ods, prec, mk=None):
    """The layer on oracle.net.OracleNet in `prec` with the masks `mk` (masks()): (out, [(in_diff, fresh gradients) per od])."""
    from oracle import net as onet
    H = layers[0]["output_dim"] // 2
    ora = onet.OracleNet(layers, prec); ora.set_train_options(1.0, 0.0); ora.set_seq_lengths(lens)
    if mk is not None:
        ora.set_dropout_masks(0, fwd=mk["fwd"], rec_fw=mk["rec"][:, :H], rec_bw=mk["rec"][:, H:])
    out = ora.propagate(feats)
    back = []
    for _, od in ods:
        in_diff = ora.backpropagate(od, update=False)
        back.append((in_diff, ora.fresh_grads_flat()))
    return out, back


def seq_worst(got, ref, lens, blocks=1):
    """got, ref: [T x S x C].  Per sequence (and per block of C / blocks columns: the directions of a layer output), over the
    sequence's valid rows: rel_err (max-norm) and the p999 of err_metrics.  Returns the worst of each over the sequences."""
    T, S, C = ref.shape
    w = C // blocks
    worst = dict(maxnorm=0.0, p999=0.0)
    for s in range(S):
        n = int(lens[s])
        for b in range(blocks):
            g, r = got[:n, s, b * w:(b + 1) * w], ref[:n, s, b * w:(b + 1) * w]
            worst["maxnorm"] = max(worst["maxnorm"], rel_err(g, r))
            worst["p999"] = max(worst["p999"], err_metrics(g, r)["p999"])
    return worst
