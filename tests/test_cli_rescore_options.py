"""CPU: the --rescore options of both ctc-decode tools (eesen_amd/bin/ctc-decode, python -m eesen_amd.ctc_decode) are documented by
--help and their misuse is refused with the same words before a model is read or a device is touched: a --rescore-* option without
--rescore=true, and values of the three options whose default is the first pass's that are no number or no boolean."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "eesen_amd", "bin", "ctc-decode")
HOSTS = [("python", [sys.executable, "-m", "eesen_amd.ctc_decode"]), ("native", [NATIVE])]
TAIL = ["no-such-model.nnet", "ark:no-such-feats.ark", "ark:/dev/null"]
OPTIONS = ("--rescore", "--rescore-lm", "--rescore-lm-weight", "--rescore-bonus", "--rescore-lm-eos")


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
    assert "(bool, default = false)" in lines["--rescore"]
    for o in OPTIONS[1:]:
        assert '(string, default = "")' in lines[o], lines[o]


def test_both_tools_document_them_alike():
    texts = [_run(cmd, "--help")[1] for _, cmd in HOSTS]
    pick = lambda t: [l for l in t.splitlines() if l.startswith("  --rescore")]
    assert pick(texts[0]) == pick(texts[1]) and len(pick(texts[0])) == 5


@pytest.mark.parametrize("option", ["--rescore-lm=second.arpa", "--rescore-lm-weight=0.5", "--rescore-bonus=1", "--rescore-lm-eos=true"])
def test_a_rescore_option_needs_rescore(option):
    seen = []
    for name, cmd in HOSTS:
        for more in ([], ["--rescore=false"]):
            rc, err = _run(cmd, option, *more, *TAIL)
            assert rc == 255, (name, err[-500:])
            assert _errors(err) == ["ERROR (ctc-decode:main()) --rescore-lm, --rescore-lm-weight, --rescore-bonus and --rescore-lm-eos need --rescore=true"], (name, err[-500:])
            seen.append(_errors(err))
    assert all(e == seen[0] for e in seen)


@pytest.mark.parametrize("args,words", [(["--rescore-lm-weight=heavy"], 'Invalid floating-point option "heavy" of --rescore-lm-weight'),
                                        (["--rescore-bonus=x1"], 'Invalid floating-point option "x1" of --rescore-bonus'),
                                        (["--rescore-lm-eos=Maybe"], "Invalid format for boolean argument [expected true or false] of --rescore-lm-eos: maybe")])
def test_values_that_do_not_parse(args, words):
    for name, cmd in HOSTS:
        rc, err = _run(cmd, "--rescore=true", *args, *TAIL)
        assert rc == 255 and _errors(err) == ["ERROR (ctc-decode:main()) " + words], (name, err[-500:])


def test_well_formed_options_pass_the_checks():
    """... and fail later, on the model that does not exist (or on the missing device)."""
    for name, cmd in HOSTS:
        rc, err = _run(cmd, "--rescore", "--rescore-lm-weight=0.5", "--rescore_bonus=-1e-1", "--rescore-lm-eos=F", *TAIL)
        assert rc == 255 and len(_errors(err)) == 1 and "rescore" not in _errors(err)[0], (name, err[-500:])
        rc, err = _run(cmd, "--rescore=maybe", *TAIL)
        assert rc == 255 and "Invalid format for boolean argument" in err, (name, err[-500:])
