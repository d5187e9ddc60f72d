"""CPU: the --mbr options of both ctc-decode tools (eesen_amd/bin/ctc-decode, python -m eesen_amd.ctc_decode) are documented by --help
in the same words, and their misuse is refused with the same words before a model is read or a device is touched: --mbr-scale or
--mbr-units without --mbr=true, and a scale that is no number."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "eesen_amd", "bin", "ctc-decode")
HOSTS = [("python", [sys.executable, "-m", "eesen_amd.ctc_decode"]), ("native", [NATIVE])]
TAIL = ["no-such-model.nnet", "ark:no-such-feats.ark", "ark:/dev/null"]
OPTIONS = ("--mbr", "--mbr-scale", "--mbr-units")
NEEDS = "ERROR (ctc-decode:main()) --mbr-scale and --mbr-units need --mbr=true"


def _run(cmd, *args):
    if cmd[0] == NATIVE and not os.path.exists(NATIVE):
        from eesen_amd import build
        build.build()
    r = subprocess.run(list(cmd) + list(args), capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    return r.returncode, r.stderr


def _errors(err):
    return [l for l in err.splitlines() if l.startswith("ERROR")]


@pytest.mark.parametrize("name,cmd", HOSTS)
def test_help_documents_the_options(name, cmd):
    rc, err = _run(cmd, "--help")
    assert rc == 0
    lines = {l.split(":")[0].strip(): l for l in err.splitlines() if l.startswith("  --")}
    for o in OPTIONS:
        assert o in lines, (o, sorted(lines))
    assert "(bool, default = false)" in lines["--mbr"] and "(bool, default = false)" in lines["--mbr-units"]
    assert '(string, default = "")' in lines["--mbr-scale"] and "(default: 1.0)" in lines["--mbr-scale"]


def test_both_tools_document_them_alike():
    texts = [_run(cmd, "--help")[1] for _, cmd in HOSTS]
    pick = lambda t: [l for l in t.splitlines() if l.startswith("  --mbr")]
    assert pick(texts[0]) == pick(texts[1]) and len(pick(texts[0])) == 3


@pytest.mark.parametrize("option", ["--mbr-scale=0.5", "--mbr-units=true", "--mbr-units"])
def test_an_mbr_option_needs_mbr(option):
    for name, cmd in HOSTS:
        for more in ([], ["--mbr=false"]):
            rc, err = _run(cmd, option, *more, *TAIL)
            assert rc == 255 and _errors(err) == [NEEDS], (name, err[-500:])


def test_a_scale_that_does_not_parse():
    for name, cmd in HOSTS:
        rc, err = _run(cmd, "--mbr=true", "--mbr-scale=flat", *TAIL)
        assert rc == 255 and _errors(err) == ['ERROR (ctc-decode:main()) Invalid floating-point option "flat" of --mbr-scale'], (name, err[-500:])


def test_well_formed_options_pass_the_checks():
    """... and fail later, on the model that does not exist (or on the missing device); together with --rescore too."""
    for name, cmd in HOSTS:
        for more in ([], ["--rescore=true", "--rescore-bonus=0.5"], ["--mbr-units=false"]):
            rc, err = _run(cmd, "--mbr", "--mbr-scale=0.25", "--mbr_units=T", *more, *TAIL)
            assert rc == 255 and len(_errors(err)) == 1 and "mbr" not in _errors(err)[0], (name, err[-500:])
        rc, err = _run(cmd, "--mbr-units=false", *TAIL)          # not asking for it is no misuse
        assert rc == 255 and len(_errors(err)) == 1 and "mbr" not in _errors(err)[0], (name, err[-500:])
        rc, err = _run(cmd, "--mbr=perhaps", *TAIL)
        assert rc == 255 and "Invalid format for boolean argument" in err, (name, err[-500:])
