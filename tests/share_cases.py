"""The cases of tests/test_gpu_recurrence_share.py (and what tests/test_share_cases.py holds of them without a GPU): one recurrent
layer per case, as in tests/recurrence_cases.py, on a device this process SHARES (EESEN_GPU_SHARE=n: rec_plan.cpp sizes every grid
against 1/n of the CUs).  There the planner answers sequence windows -- the same kernel launched 2, 4 or 8 times with
LstmLayerDev::s_begin / s_count set -- where it answers one launch on a whole device; takes the time-multiplexed kernels at exactly
two windows only; has no residency census; leaves the narrow forward tile and the 8-sequence backward tile at smaller shapes; and
sends shapes that are persistent on a whole device to the per-step kernels.

  CASES     name -> layer kind, cells, sequences, frames, switches (the A/B switches of tuning.h only), recurrent-dropout recipe
            (tests/dropout_cases.py RECIPES) or None, the SHARE, the forward row, the backward row, launches per pass.  Rows and
            launches were read from Plan() under the share on an MI355X (256 CUs) and the GPU test asserts them
  PER_STEP  the same for shapes of which a pass has no persistent tile under the share (rc.PER_STEP_KERNELS, 0 launches)
  SHARE1    "<base>@share1" -> the same shape, switches and recipe on a whole device: run for the comparison of a sequence's bits with
            and without windows; their plans belong to tests/test_gpu_plans.py and the rows module and are not asserted here
  lengths / features / top_gradients / layer / masks: the generators of tests/dropout_cases.py, by a name of ALL

A case is named <rc name>[-recipe]@share<n>, <rc name> as tests/recurrence_cases.py names the shape and its switches.

The shapes are the smallest at which each path is reached; their plans were first derived by hand from rec_plan.cpp and the register
and LDS figures of tests/golden/plans.json, then read from the device.  The device answered as derived but for:
  bi512_s32@share2   the forward pass takes the WIDE plane tile <2,4,2,2,true>, not the narrow one: 2 x 64 x 2 = 256 narrow
                     workgroups exceed 128 CUs, and two per CU are only taken where a census has seen them (none under a share).
                     Kept: the case is there for its backward pass, the two-tile 4 x 32 row taken by the planner itself
  bi1024_s64-BWD_F16=0-BWD_MUX=0-FWD_MUX=0-FWD_SPLIT=0@share2 was added so that the plain fp32 rows at 1024 cells have a share-1 twin on
                     the same rows (without it the twin runs the multiplexed kernels and no bits are compared)
  bi512_s128-FWD_SPLIT=0@share4 was added for the coverage tests/test_share_cases.py asks for: an fp32 forward row in 8 launches (the
                     wide fp32 tile is one workgroup per CU: 64 workgroups per 16 sequences on 64 CUs), with the exchange-layout fetch
"""
from tests import dropout_cases as dc
from tests import recurrence_cases as rc
from tests.dropout_cases import D, oracle_run, seq_worst  # noqa: F401
from tests.recurrence_cases import (PER_STEP_KERNELS, _BI, _UNI, _F32, _F32_WIDE, bwd_gen, bwd_ksplit, bwd_ksplit_h, bwd_q4,  # noqa: F401
                                    fwd_bf, fwd_f32)

SHARES = (2, 4, 8)


def _case(kind, H, S, share, fwd, bwd, launches, env=None, recipe=None):
    return dict(kind=kind, H=H, S=S, T=6 if S >= 64 else 8, env=dict(env or {}), recipe=recipe, share=share, fwd=fwd, bwd=bwd,
                launches=launches)


def base_name(c):
    """<rc name>[-recipe]: the shape, its switches and its dropout recipe -- what a case shares with its share-1 twin."""
    return rc.case_name(c["kind"], c["H"], c["S"], c["env"]) + (f"-{c['recipe']}" if c["recipe"] else "")


def case_name(c):
    return f"{base_name(c)}@share{c['share']}"


_PS = PER_STEP_KERNELS
_TABLE = [
    # ---- half a device
    # four windows of both plane tiles; PX is cleared per window, DGH / EX are indexed behind s_begin
    _case(_BI, 1024, 64, 2, fwd_bf(4, 4, 2, 2, True), bwd_ksplit_h(4), (4, 4)),
    # four windows: the multiplexed rows must NOT be taken; the exchange-layout fetch behind a window offset
    _case(_BI, 1024, 64, 2, fwd_f32(4, 1, 4, False, True), bwd_ksplit(4), (4, 4), _F32_WIDE),
    # ... and the same with the multiplexed rows switched off, which changes nothing under the share and leaves the share-1 twin the
    # plain rows in two launches: the wide fp32 tile and the fp32 K-split tile compared bit for bit between 4 windows and 2
    _case(_BI, 1024, 64, 2, fwd_f32(4, 1, 4, False, True), bwd_ksplit(4), (4, 4), {**_F32_WIDE, "EESEN_FWD_MUX": "0", "EESEN_BWD_MUX": "0"}),
    # on a whole device the backward pass is the multiplexed row; here the plain one, in windows
    _case(_BI, 768, 64, 2, fwd_bf(3, 4, 2, 2, True), bwd_ksplit(3), (4, 4)),
    # windows with one direction
    _case(_UNI, 1024, 64, 2, fwd_bf(4, 4, 2, 2, True), bwd_ksplit_h(4), (2, 2)),
    # the narrow tile gives way without a census; the 4 x 32 tile fits in neither form: windows of the generic backward tile
    _case(_BI, 512, 64, 2, fwd_bf(2, 4, 2, 2, True), bwd_gen(8, 16), (2, 2)),
    # rmask behind a window offset (masks planted as in tests/test_gpu_recurrence_dropout.py)
    _case(_BI, 512, 64, 2, fwd_f32(2, 1, 4, True, False), bwd_gen(8, 16, True), (2, 2), recipe="nml"),
    _case(_BI, 512, 64, 2, fwd_f32(2, 1, 4, True, False), bwd_gen(8, 16, True), (2, 2), recipe="rnndrop"),
    # the one-tile 4 x 32 row no longer fits: the two-tile form, chosen by the planner and not by EESEN_BWD_Q4_ST8=2
    _case(_BI, 512, 32, 2, fwd_bf(2, 4, 2, 2, True), bwd_q4(8, 8), (1, 1)),
    # ---- a quarter
    _case(_BI, 512, 64, 4, fwd_bf(2, 4, 2, 2, True), bwd_gen(8, 16), (4, 4)),
    _case(_BI, 512, 128, 4, fwd_bf(2, 4, 2, 2, True), bwd_gen(8, 16), (8, 8)),      # eight windows: the loop bound of pick_windows
    # eight windows of the wide fp32 tile, its exchange-layout fetch behind seven different window offsets
    _case(_BI, 512, 128, 4, fwd_f32(2, 1, 4, False, True), bwd_gen(8, 16), (8, 8), _F32),
    _case(_BI, 256, 64, 4, fwd_bf(1, 4, 2, 2, True), bwd_gen(4, 16), (2, 2)),       # the backward sequence tile flips from 8 to 16
    _case(_BI, 200, 64, 4, fwd_f32(1, 1, 2, False, False), bwd_gen(4, 16), (2, 2)),  # no multiple of 32: plain fetch, generic tile
    # ---- an eighth
    _case(_BI, 256, 128, 8, fwd_bf(1, 4, 2, 2, True), bwd_gen(4, 16), (8, 8)),
    # ---- persistent on a whole device, per step under the share
    _case(_BI, 1024, 32, 4, _PS, _PS, (0, 0)),       # 128 workgroups per 16 sequences exceed 64 CUs
    _case(_BI, 512, 128, 8, _PS, _PS, (0, 0)),
]
TABLE = {case_name(c): c for c in _TABLE}
assert len(TABLE) == len(_TABLE)
CASES = {n: c for n, c in TABLE.items() if _PS not in (c["fwd"], c["bwd"])}
PER_STEP = {n: c for n, c in TABLE.items() if _PS in (c["fwd"], c["bwd"])}
# every case's shape, switches and recipe on a whole device, once per base
SHARE1 = {}
for _c0 in _TABLE:
    SHARE1.setdefault(base_name(_c0) + "@share1", dict(_c0, share=1, fwd=None, bwd=None, launches=None))
ALL = {**TABLE, **SHARE1}


def twin(name):
    """The share-1 case of the same shape, switches and recipe."""
    return base_name(ALL[name]) + "@share1"


def at_share(share):
    """The names of ALL that run under `share`, in table order."""
    return [n for n, c in ALL.items() if c["share"] == share]


def _c(name):
    c = ALL[name]
    return c["H"], c["S"], c["T"], 2 if c["kind"] == _BI else 1


def ndir(name):
    return _c(name)[3]


def lengths(name):
    return dc.shape_lengths(*_c(name))


def features(name, lens):
    return dc.shape_features(*_c(name), lens)


def top_gradients(name, lens):
    return dc.shape_top_gradients(*_c(name), lens)


def layer(name):
    L = dc.shape_layer(ALL[name]["kind"], ALL[name]["H"])
    if ALL[name]["recipe"]:
        L[0]["dropout"] = dict(dc.RECIPES[ALL[name]["recipe"]])
    return L


def masks(name):
    """The planted masks of the case's recipe (tests/dropout_cases.py masks(): that module's, at the same shape), or None."""
    c = ALL[name]
    if not c["recipe"]:
        return None
    shape = f"bi{c['H']}_s{c['S']}"
    assert c["kind"] == _BI and (dc.CASES[shape]["H"], dc.CASES[shape]["S"], dc.CASES[shape]["T"]) == (c["H"], c["S"], c["T"])
    return dc.masks(shape, c["recipe"])


def seq_tile(row):
    """Sequences per tile of a row, as pick_windows is given it (rec_plan.cpp): 16 x MT forward on the fp32 tiles, 16 on the plane
    tiles and the K-split ones, ST on the generic backward tile.  (The 4 x 32 tile walks the whole batch in one launch.)"""
    kernel, args = row[:-1].split("<")
    a = args.split(",")
    if kernel == "lstm_fwd_persistent_kernel":
        return 16 * int(a[1])
    if kernel == "lstm_bwd_persistent_kernel":
        return int(a[1])
    if kernel == "lstm_bwd_persistent_q4_kernel":
        return int(a[1])
    assert kernel in ("lstm_fwd_persistent_bf_kernel", "lstm_bwd_persistent_ksplit_kernel", "lstm_bwd_persistent_ksplit_h_kernel"), row
    return 16


def family(row):
    """plane (forward on fp16 / bf16 planes), f32 (forward), generic (backward), ksplit (backward, both forms), q4, or None (per step)."""
    if row == _PS:
        return None
    kernel = row.split("<")[0]
    return {"lstm_fwd_persistent_bf_kernel": "plane", "lstm_fwd_persistent_kernel": "f32", "lstm_bwd_persistent_kernel": "generic",
            "lstm_bwd_persistent_ksplit_kernel": "ksplit", "lstm_bwd_persistent_ksplit_h_kernel": "ksplit",
            "lstm_bwd_persistent_q4_kernel": "q4"}[kernel]


# The whole training step under a share (part of the same module): 2 x BiLSTM(512) + affine + softmax + CTC
STEP = dict(cfg=dict(kind=_BI, layers=2, H=512, D=40, K=46, S=64, T=12), shares=(2, 4))
