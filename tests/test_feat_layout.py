"""csrc/feat_layout.h without a GPU: tests/native/feat_layout_check.cc, a program of its own built with the address and
undefined-behaviour sanitizers (the runtimes linked statically: the program needs nothing from its environment).  It holds the
filterbank's and the pitch tracker's batch tables and their frame bounds, the front end's stage boundaries, paste-feats' row rule and
the carving of the block that carries a batch's tables, against expectations written out by hand."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "feat_layout_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "native", "feat_layout_check.cc"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("0 failures") and "runtime error" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
