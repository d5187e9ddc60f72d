"""CPU: the reference's own, unmodified src/netbin/train-ce-parallel.cc compiles against the C++ seam (include/eesen_seam
shadows net/ce-loss.h and net/net.h; eesen::CE / eesen::Net of include/eesen_hip_net.h) with the flags of the `seam` target
of oracle/ref_build/Makefile.  Syntax only: the binary would need the reference's objects and a GPU.  Skips without the reference."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from oracle.refbind import REFERENCE_ROOT as REF   # where the reference lies (compiled in place by oracle/ref_build)


def test_reference_ce_trainer_compiles_against_the_seam():
    src = os.path.join(REF, "src", "netbin", "train-ce-parallel.cc")
    if not os.path.exists(src):
        pytest.skip("needs the reference sources")
    cmd = ["g++", "-I" + os.path.join(ROOT, "include", "eesen_seam"), "-I" + os.path.join(ROOT, "include"), "-std=c++11", "-O2", "-w",
           "-fPIC", "-msse", "-msse2", f"-I{REF}/src", f"-I{REF}/tools/CLAPACK", "-DHAVE_CLAPACK", "-DKALDI_DOUBLEPRECISION=0",
           "-DHAVE_POSIX_MEMALIGN", "-DHAVE_EXECINFO_H=1", "-DHAVE_CXXABI_H", "-include", os.path.join(ROOT, "oracle", "ref_build", "blas_rename.h"),
           "-fsyntax-only", src]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    # the shadow header is what made eesen::CE the seam's: without it the reference's own CE (a CuMatrix of its own) is pulled in
    assert os.path.exists(os.path.join(ROOT, "include", "eesen_seam", "net", "ce-loss.h"))
