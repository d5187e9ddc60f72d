"""CPU: tests/ce_restatement.py against the reference's own CE (src/net/ce-loss.cc, compiled where it lies in CPU mode with the
flags of oracle/ref_build/Makefile and linked against the objects it built under oracle/_ref/obj) on random minibatches: diff,
objective, correct counts, the progress lines byte for byte and the Report text (integer division there).  Skips where the
reference or its objects are absent."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from tests.ce_restatement import CERestatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from oracle.refbind import REFERENCE_ROOT as REF   # where the reference lies (compiled in place by oracle/ref_build)
OBJ = os.path.join(ROOT, "oracle", "_ref", "obj")
FLAGS = ["-std=c++11", "-O2", "-w", "-fPIC", "-msse", "-msse2", f"-I{REF}/src", f"-I{REF}/tools/CLAPACK", "-DHAVE_CLAPACK",
         "-DKALDI_DOUBLEPRECISION=0", "-DHAVE_POSIX_MEMALIGN", "-DHAVE_EXECINFO_H=1", "-DHAVE_CXXABI_H",
         "-include", os.path.join(ROOT, "oracle", "ref_build", "blas_rename.h")]


def _openblas():
    import scipy
    libs = glob.glob(os.path.join(os.path.dirname(scipy.__file__), "..", "scipy.libs", "libscipy_openblas*.so"))
    return os.path.abspath(libs[0]) if libs else None


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not (os.path.isdir(REF) and os.path.isdir(OBJ)):
        pytest.skip("needs the reference sources and oracle/_ref/obj (built by __graft_entry__.build() where the reference exists)")
    blas = _openblas()
    if blas is None:
        pytest.skip("no OpenBLAS to link the reference against")
    d = tmp_path_factory.mktemp("ce_ref")
    objs = sorted(glob.glob(os.path.join(OBJ, d_, "*.o")) for d_ in ("base", "cpucompute", "gpucompute", "util"))
    objs = [o for group in objs for o in group]
    exe = str(d / "ce_ref_driver")
    cmd = ["g++"] + FLAGS + [os.path.join(REF, "src", "net", "ce-loss.cc"), os.path.join(ROOT, "tests", "native", "ce_ref_driver.cc")] + objs + \
          ["-o", exe, blas, "-Wl,-rpath," + os.path.dirname(blas), "-lpthread", "-ldl", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _softmax(rng, rows, K):
    x = rng.standard_normal((rows, K)).astype(np.float32) * 3
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def _calls(seed):
    rng = np.random.default_rng(seed)
    calls = []
    for K, S in ((7, 3), (51, 4), (130, 5), (3, 0), (33, 2)):   # S = 0: CE::Eval
        s = max(S, 1)
        T = int(rng.integers(4, 12))
        rows = T * s
        lens = rng.integers(1, T + 1, size=s) if S else np.array([T])
        lens[0] = T
        y = _softmax(rng, rows, K)
        mask = np.zeros(rows, np.float32)
        tg = np.zeros(rows, np.int32)               # the trainer's target_host: 0 on padded rows (train-ce-parallel.cc:143-151)
        for q in range(s):
            mask[q:lens[q] * s:s] = 1
            tg[q:lens[q] * s:s] = rng.integers(0, K, size=lens[q])
        # some rows the net gets right, so the counts are not all zero
        right = (mask == 1) & (rng.random(rows) < 0.4)
        tg[right] = np.argmax(y[right], axis=1)
        calls.append((y, tg, mask, S))
    return calls


@pytest.mark.parametrize("report_step", [0, 4, 100])
def test_restatement_equals_reference_ce(driver, tmp_path, report_step):
    calls = _calls(11 + report_step)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        np.array([len(calls), report_step], np.int32).tofile(f)
        for y, tg, mask, S in calls:
            np.array([y.shape[0], y.shape[1], S], np.int32).tofile(f)
            y.tofile(f); tg.astype(np.int32).tofile(f); mask.tofile(f)
    r = subprocess.run([driver, str(inp), str(outp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    res = CERestatement(report_step)
    raw = open(outp, "rb").read()
    off, lines = 0, []
    for y, tg, mask, S in calls:
        rows, K = y.shape
        ref_diff = np.frombuffer(raw, np.float32, rows * K, off).reshape(rows, K); off += rows * K * 4
        ref_obj = np.frombuffer(raw, np.float64, 1, off)[0]; off += 8
        ref_correct, ref_frames = np.frombuffer(raw, np.int32, 2, off); off += 8
        diff, line = res.eval(y, tg) if S == 0 else res.eval_parallel(y, tg, mask, S)
        np.testing.assert_array_equal(diff, ref_diff + np.float32(0))   # (+0: the reference's padded rows may hold -0)
        assert abs(res.obj - ref_obj) <= 1e-6 * abs(ref_obj)
        assert res.correct == ref_correct and res.frames == ref_frames
        if line is not None:
            lines.append(line)
    ref_lines = re.findall(r"(After \d+ sequences .*)$", r.stderr, flags=re.M)
    assert len(ref_lines) == len(lines)
    for a, b in zip(lines, ref_lines):   # the text, byte for byte, but for the last digit of the printed objectives
        na, nb = re.split(r"[-+0-9.e]+", a), re.split(r"[-+0-9.e]+", b)
        assert na == nb, (a, b)
        for x, z in zip(re.findall(r"[-+]?[0-9.]+(?:e[-+]?\d+)?", a), re.findall(r"[-+]?[0-9.]+(?:e[-+]?\d+)?", b)):
            assert abs(float(x) - float(z)) <= 1e-5 * max(abs(float(z)), 1e-30), (a, b)
    assert report_step != 0 or len(lines) == len(calls)
    assert r.stdout == res.report_reference()
