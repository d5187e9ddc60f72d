"""A numpy transcription of the reference's frame-level cross-entropy, src/net/ce-loss.cc, quirks included
(the arbiter of eesen_ce_* and of train-ce-parallel's report lines; pinned to the reference by
tests/test_ce_restatement_vs_reference.py).

    ce = CERestatement(report_step)
    diff, line = ce.eval_parallel(y, targets, mask, S)     # line: the progress text of this call, or None
    ce.report()                                            # FRAME_ACCURACY line, with the true ratio (deliberate deviation)
"""
from __future__ import annotations

import numpy as np


def _g(v) -> str:
    """operator<< of a double with the default stream precision (6 significant digits, %g)."""
    return f"{float(v):g}"


def ce_call(y: np.ndarray, targets, mask) -> tuple:
    """One EvalParallel's arithmetic (ce-loss.cc:104-142): diff = (y - onehot) * mask in float32 (AddMat, MulRowsVec);
    correct = rows with mask == 1 whose FindRowMaxId (first maximum) is the target (:128-135); obj = -sum of
    log(y) * onehot * mask with the log in float32 (ApplyLog) and the sum in float64."""
    y = np.asarray(y, np.float32)
    tg = np.asarray(targets, np.int64)
    mask = np.asarray(mask, np.float32)
    rows, K = y.shape
    onehot = np.zeros_like(y)
    onehot[np.arange(rows), tg] = 1.0                      # :106-115
    diff = (y + np.float32(-1.0) * onehot) * mask[:, None]  # :119-125
    diff = np.where(mask[:, None] == 0, np.float32(0), diff).astype(np.float32)   # padded rows: 0 (the sign of 0 * y dropped)
    arg = np.argmax(y, axis=1)                              # :128-135
    correct = int(np.sum((mask == 1) & (arg == tg)))
    logy = np.log(y[np.arange(rows), tg]).astype(np.float32)   # :137-142, only the target column survives MulElements
    obj = -float(np.sum(logy.astype(np.float64) * mask.astype(np.float64)))
    return diff, obj, correct


class CERestatement:
    def __init__(self, report_step: int = 100):
        self.report_step = report_step                     # ce-loss.h:47
        self.frames = self.sequences = self.correct = 0    # :35-36
        self.obj = 0.0
        self.frames_progress = self.sequences_progress = self.correct_progress = 0
        self.obj_progress = 0.0

    def eval_parallel(self, y, targets, mask, S: int):
        """ce-loss.cc:94-169.  Returns (diff, progress line or None)."""
        diff, obj, correct = ce_call(y, targets, mask)
        rows = np.asarray(y).shape[0]
        self.correct += correct; self.correct_progress += correct
        self.obj += obj; self.obj_progress += obj            # :144-145
        self.sequences_progress += S; self.sequences += S    # :146-147
        self.frames_progress += rows; self.frames += rows    # :148-149: num_frames = NumRows(), padded rows included
        self.last_obj, self.last_correct = obj, correct
        line = None
        if self.sequences_progress > self.report_step:       # :153, strictly greater
            line = (f"After {self.sequences} sequences ({_g(self.frames / (100.0 * 3600))}Hr): "
                    f"CE-Obj = {_g(self.obj_progress / self.sequences_progress)}"
                    f"Frame-level CE-Obj = {_g(self.obj_progress / self.frames_progress)}"     # (no space: the reference's text)
                    f"   FrameAcc = {_g(100.0 * (self.correct_progress / self.frames_progress))}%"
                    f" obj_progress_=  {_g(self.obj_progress)}"
                    f" sequences_progress_=  {self.sequences_progress}"
                    f" frames_progress_=  {self.frames_progress}")
            self.sequences_progress = self.frames_progress = self.correct_progress = 0   # :162-165
            self.obj_progress = 0.0
        return diff, line

    def eval(self, y, targets):
        """ce-loss.cc:30-92: every row counts, sequences += 1."""
        return self.eval_parallel(y, targets, np.ones(np.asarray(y).shape[0], np.float32), 1)

    def report(self) -> str:
        """ce-loss.cc:171-175 with the true ratio: the reference's 100.0*(correct_/frames_) divides two int32."""
        return f"\nFRAME_ACCURACY >> {_g(100.0 * (self.correct / self.frames))}% <<"

    def report_reference(self) -> str:
        """The reference's own text: integer division, 0 or 100."""
        return f"\nFRAME_ACCURACY >> {_g(100.0 * (self.correct // self.frames))}% <<"
