"""The cases of tests/test_gpu_recurrence_rows.py (and what tests/test_recurrence_cases.py holds of them without a GPU): one recurrent
layer per case, at a shape and with the switches at which rec_plan.cpp takes a given row of the recurrence kernel table
(kRecKernels, eesen_amd/csrc/lstm_persistent.hip) for the forward pass and another for the backward pass.

  CASES           name -> layer kind, cells, sequences, frames, switches (the A/B switches of tuning.h only), the forward row, the
                  backward row, launches per pass.  Rows are named as Plan() prints them; the shapes are read from fwd_tile,
                  bf_plan_shape, lstm_fwd_plan and lstm_bwd_plan for a whole 256-CU device, and the GPU test asserts through Plan()
                  that the device takes exactly these rows
  HELD_ELSEWHERE  row -> the module and case that already hold it per sequence or step by step (their tables are imported)
  UNREACHED       row -> why no shape runs it
  PER_STEP        name -> a shape at which Plan() must answer "per-step kernels (lstm.hip)" for the named passes
  lengths / features / top_gradients / layer: the generators of tests/dropout_cases.py, by a name of CASES or PER_STEP

Every row of the table is in exactly one of HELD_ELSEWHERE, UNREACHED and the rows only CASES names (tests/test_recurrence_cases.py);
a case whose other pass runs a row that another module holds (the narrow plane tile at 320 cells) leaves that row with its module.

Every case here runs on a whole device.  What the planner answers on a SHARED one (EESEN_GPU_SHARE > 1: sequence windows of 2, 4 and
8 launches, other tiles, per-step kernels at shapes that are persistent here) is tests/share_cases.py's table, run by
tests/test_gpu_recurrence_share.py.
"""
from tests import dropout_cases as dc
from tests.dropout_cases import D, oracle_run, seq_worst  # noqa: F401  (the metrics and the oracle are that module's)

PER_STEP_KERNELS = "per-step kernels (lstm.hip)"
_BI, _UNI = "BiLstmParallel", "LstmParallel"
_b = lambda v: "true" if v else "false"


def fwd_f32(cpw, mt, nt, drop, xchg):
    return "lstm_fwd_persistent_kernel<%d,%d,%d,%s,%s>" % (cpw, mt, nt, _b(drop), _b(xchg))


def fwd_bf(cpw, nt, ap, wp, f16):
    return "lstm_fwd_persistent_bf_kernel<%d,%d,%d,%d,%s>" % (cpw, nt, ap, wp, _b(f16))


def fwd_mux(xchg):
    return "lstm_fwd_persistent_mux_kernel<4,4,%s>" % _b(xchg)


def bwd_gen(cpw, st, drop=False):
    return "lstm_bwd_persistent_kernel<%d,%d,%s>" % (cpw, st, _b(drop))


def bwd_q4(cpw, st):
    return "lstm_bwd_persistent_q4_kernel<%d,%d>" % (cpw, st)


def bwd_ksplit(cpw):
    return "lstm_bwd_persistent_ksplit_kernel<%d>" % cpw


def bwd_ksplit_h(cpw):
    return "lstm_bwd_persistent_ksplit_h_kernel<%d>" % cpw


def bwd_ksplit_mux(cpw):
    return "lstm_bwd_persistent_ksplit_mux_kernel<%d>" % cpw


def _case(kind, H, S, fwd, bwd, env=None, launches=(1, 1)):
    # T: 8, or 6 where the batch is large (as in tests/dropout_cases.py)
    return dict(kind=kind, H=H, S=S, T=6 if S >= 64 else 8, env=dict(env or {}), fwd=fwd, bwd=bwd, launches=launches)


def case_name(kind, H, S, env):
    """bi128_s32-FWD_SPLIT=0: the naming of tests/test_gpu_plans.py."""
    return f"{'bi' if kind == _BI else 'uni'}{H}_s{S}" + "".join(f"-{k[len('EESEN_'):]}={v}" for k, v in sorted(env.items()))


_F32 = {"EESEN_FWD_SPLIT": "0"}                          # every recurrence on the fp32-input MFMA
_F32_WIDE = {"EESEN_FWD_SPLIT": "0", "EESEN_BWD_F16": "0"}
_ST8 = {"EESEN_BWD_Q4_ST8": "2"}                         # two 4-sequence tiles per workgroup wherever that applies
_BF3 = {"EESEN_FWD_F16": "0"}                            # the narrow forward tile on three bf16 planes
_WIDE = {"EESEN_FWD_NARROW2": "0"}                       # the wide forward tile where the narrow one would run two per CU

_TABLE = [
    # the fp32 tiles at widths that are no multiple of 32 (no exchange-layout fetch, no plane kernel, no 4 x 32 backward tile)
    _case(_BI, 36, 8, fwd_f32(1, 2, 1, False, False), bwd_gen(1, 16)),
    _case(_BI, 40, 32, fwd_f32(1, 1, 2, False, False), bwd_gen(1, 8)),
    _case(_BI, 72, 32, fwd_f32(1, 1, 2, False, False), bwd_gen(2, 8)),
    _case(_BI, 100, 8, fwd_f32(1, 2, 1, False, False), bwd_gen(2, 16)),
    _case(_BI, 200, 32, fwd_f32(1, 1, 2, False, False), bwd_gen(4, 8)),
    _case(_BI, 240, 80, fwd_f32(1, 1, 4, False, False), bwd_gen(4, 16)),
    _case(_BI, 264, 32, fwd_f32(2, 1, 2, False, False), bwd_gen(8, 8)),
    _case(_BI, 300, 8, fwd_f32(2, 2, 1, False, False), bwd_gen(8, 16)),
    _case(_BI, 400, 48, fwd_f32(2, 1, 4, False, False), bwd_gen(8, 16)),
    # between 512 and 1024 cells: a ragged last 32-cell chunk (528 = 16.5 chunks), and whole chunks that are no multiple of 256
    _case(_BI, 528, 16, fwd_f32(4, 1, 4, False, False), bwd_gen(16, 8)),
    _case(_BI, 640, 16, fwd_f32(4, 1, 4, False, True), bwd_gen(16, 8)),
    _case(_UNI, 516, 8, fwd_f32(4, 2, 1, False, False), bwd_gen(16, 16)),
    # the fp32 tiles with the exchange-layout fetch, the 4 x 32 backward tile below them
    _case(_BI, 64, 8, fwd_f32(1, 2, 1, False, False), bwd_gen(1, 16), _F32),     # (S <= 8: the 4 x 32 tile is not taken)
    _case(_BI, 128, 32, fwd_f32(1, 1, 2, False, True), bwd_q4(2, 4), _F32),
    _case(_BI, 320, 32, fwd_f32(2, 1, 2, False, True), bwd_q4(6, 4), _F32),
    _case(_BI, 256, 80, fwd_f32(1, 1, 4, False, True), bwd_q4(4, 8), _F32),
    _case(_BI, 512, 48, fwd_f32(2, 1, 4, False, True), bwd_q4(8, 8), _F32),
    _case(_BI, 1024, 64, fwd_mux(True), bwd_ksplit_mux(4), _F32_WIDE),
    _case(_BI, 1024, 32, fwd_f32(4, 1, 4, False, True), bwd_ksplit(4), _F32_WIDE),
    # the product path: two fp16 planes forward, the 4 x 32 tile backward in its one- and two-tile forms
    _case(_BI, 128, 32, fwd_bf(1, 2, 2, 2, True), bwd_q4(2, 4)),
    _case(_BI, 256, 32, fwd_bf(1, 2, 2, 2, True), bwd_q4(4, 4)),
    _case(_BI, 128, 32, fwd_bf(1, 2, 2, 2, True), bwd_q4(2, 8), _ST8),
    _case(_BI, 256, 32, fwd_bf(1, 2, 2, 2, True), bwd_q4(4, 8), _ST8),
    _case(_BI, 320, 32, fwd_bf(2, 2, 2, 2, True), bwd_q4(6, 8), _ST8),
    # three bf16 planes
    _case(_BI, 128, 32, fwd_bf(1, 2, 3, 3, False), bwd_q4(2, 4), _BF3),
    _case(_BI, 512, 32, fwd_bf(2, 2, 3, 3, False), bwd_q4(8, 4), _BF3),
    # the wide plane tile below 1024 cells
    _case(_BI, 256, 80, fwd_bf(1, 4, 2, 2, True), bwd_q4(4, 8), _WIDE),
    _case(_BI, 512, 64, fwd_bf(2, 4, 2, 2, True), bwd_q4(8, 8), _WIDE),
    # 768 cells: three chunks per wave, forward and behind the K split
    _case(_BI, 768, 32, fwd_bf(3, 4, 2, 2, True), bwd_ksplit(3)),
    _case(_BI, 768, 64, fwd_bf(3, 4, 2, 2, True), bwd_ksplit_mux(3), launches=(2, 1)),
]
CASES = {case_name(c["kind"], c["H"], c["S"], c["env"]): c for c in _TABLE}
assert len(CASES) == len(_TABLE)

# Shapes whose named passes have no persistent tile.  fwd / bwd: the row Plan() must name, PER_STEP_KERNELS for a pass on lstm.hip.
PER_STEP = {
    # more than 1024 cells: more than 4 (forward) and 16 (backward) 32-cell chunks per wave
    "bi1280_s8": dict(kind=_BI, H=1280, S=8, T=8, env={}, fwd=PER_STEP_KERNELS, bwd=PER_STEP_KERNELS, launches=(0, 0)),
    "uni2048_s8": dict(kind=_UNI, H=2048, S=8, T=8, env={}, fwd=PER_STEP_KERNELS, bwd=PER_STEP_KERNELS, launches=(0, 0)),
    # 2 x 520 / 4 = 260 workgroups of the 32 x 4 forward tile are not co-resident on 256 CUs
    "bi520_s8": dict(kind=_BI, H=520, S=8, T=8, env={}, fwd=PER_STEP_KERNELS, bwd=bwd_gen(16, 16), launches=(0, 1)),
    # a frame's rows of Y (17 x 40 floats) do not start on a 128-byte line (rec_plan.cpp: line_aligned); those of DG (17 x 160) do
    "bi20_s17": dict(kind=_BI, H=20, S=17, T=8, env={}, fwd=PER_STEP_KERNELS, bwd=bwd_gen(1, 8), launches=(0, 1)),
}
ALL = {**CASES, **PER_STEP}
assert len(ALL) == len(CASES) + len(PER_STEP)


def _held_elsewhere():
    from tests import bf16_forward_cases as bf16
    from tests import test_gpu_recurrence_planes as planes
    held = {}
    for case in dc.CASES:                         # the DROP = true rows
        held.setdefault(dc.fwd_row(case), f"tests/test_gpu_recurrence_dropout.py {case} (tests/dropout_cases.py CASES)")
        held.setdefault(dc.bwd_row(case), f"tests/test_gpu_recurrence_dropout.py {case} (tests/dropout_cases.py CASES)")
    for row in dc.UNREACHED:
        held[row] = "tests/dropout_cases.py UNREACHED"
    for name, (kind, H, S, T, bwd) in planes.SHAPES.items():   # the fp16-plane rows at the shipped widths
        ft = fwd_bf(H // 256, 4, 2, 2, True) if H % 256 == 0 and H >= 768 else fwd_bf((H // 32 + 7) // 8, 2, 2, 2, True)
        held.setdefault(ft, f"tests/test_gpu_recurrence_planes.py {name}")
        if bwd == "ksplit_h":
            held.setdefault(bwd_ksplit_h(H // 256), f"tests/test_gpu_recurrence_planes.py {name}")
    for name, (_, H, *_) in bf16.RECURRENCE.items():   # config 4's bf16 forward: per element, one step deep in m and c, both directions
        held.setdefault(fwd_bf(H // 256, 4, 1, 2, False), f"tests/test_gpu_bf16_forward_fp64.py {name} (tests/bf16_forward_cases.py RECURRENCE)")
    return held


HELD_ELSEWHERE = _held_elsewhere()

UNREACHED = {
    bwd_ksplit(2): "CPW = H / 256 = 2 is 512 cells, and bwd_ksplit_shape (rec_plan.cpp) takes the K-split tiles from 768 cells on: below that "
                   "the 4 x 32 tile runs (or, with EESEN_BWD_Q4=0, the generic one).  The planner's own bounds exclude the row.",
    bwd_ksplit_h(2): "as lstm_bwd_persistent_ksplit_kernel<2>: bwd_planes_shape admits CPW = 2 but requires bwd_ksplit_shape, which demands "
                     "H >= 768.",
    bwd_ksplit_mux(2): "as lstm_bwd_persistent_ksplit_kernel<2>: the multiplexed form is only looked at inside bwd_ksplit_shape (H >= 768).",
    fwd_mux(False): "XCHG = false is taken without an exchange buffer or when the buffer's block offsets pass 32 bits (small_xchg).  The "
                    "multiplexed kernel needs whole 32-cell chunks and a persistent Net, and for those net.cpp always reserves the buffer; and "
                    "small_xchg fails only from T x S x ndir x H x 4 >= 2^31 bytes on (4096 frames at 1024 cells and 64 sequences), where "
                    "lstm_fwd_plan has already returned no plan, because (T + 2) x S x ndir x H x 4 bytes of Y pass the same 2^31.",
}


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
    return dc.shape_layer(ALL[name]["kind"], ALL[name]["H"])


def masks(name):
    """No case of this table has dropout (tests/dropout_cases.py holds those rows; tests/share_cases.py runs two under a share)."""
    return None


def line_aligned(name):
    """rec_plan.cpp's condition on the forward pass: a frame's rows of Y, [S x ndir * H] floats, are whole 128-byte lines."""
    H, S, _, nd = _c(name)
    return (S * nd * H * 4) % 128 == 0
