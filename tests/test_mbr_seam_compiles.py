"""CPU: eesen::Ctc::EditDistanceParallel, eesen::Ctc::MbrNbest and its Mbr result of the C++ seam (include/eesen_hip_net.h) compile in a
host written against it (tests/native/seam_mbr_use.cc), with the flags of the `seam` target of oracle/ref_build/Makefile.  Syntax only.
The seam builds on the reference's base / cpucompute headers: skips without the reference sources."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from oracle.refbind import REFERENCE_ROOT as REF   # where the reference lies (compiled in place by oracle/ref_build)


def test_mbr_compiles_against_the_seam():
    if not os.path.exists(os.path.join(REF, "src", "base", "kaldi-common.h")):
        pytest.skip("needs the reference sources")
    cmd = ["g++", "-I" + os.path.join(ROOT, "include", "eesen_seam"), "-I" + os.path.join(ROOT, "include"), "-std=c++11", "-O2", "-w",
           "-fPIC", "-msse", "-msse2", f"-I{REF}/src", f"-I{REF}/tools/CLAPACK", "-DHAVE_CLAPACK", "-DKALDI_DOUBLEPRECISION=0",
           "-DHAVE_POSIX_MEMALIGN", "-DHAVE_EXECINFO_H=1", "-DHAVE_CXXABI_H", "-include", os.path.join(ROOT, "oracle", "ref_build", "blas_rename.h"),
           "-fsyntax-only", os.path.join(ROOT, "tests", "native", "seam_mbr_use.cc")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
