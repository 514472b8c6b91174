"""CPU: the headless driver's command line, byte for byte against tests/golden/headless_cli.json -- the exit status, stdout and
stderr that the driver gave for every line of tests/headless_cli_cases.py before its main() was split into a parser and named
parts.  Every case ends before any GPU call (an argument error, a plan_slabs error, or -help), so a machine without a GPU
gives the same bytes as one with eight."""
import json
import os
import subprocess

import pytest

from headless_cli_cases import CASES, EXE, GOLDEN, run_case

with open(GOLDEN) as _f:
    RECORDED = json.load(_f)


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        from gpufluidsimulator_amd import build
        build.build()
    return EXE


def test_the_golden_file_holds_the_cases_and_none_reached_a_device():
    assert [c["args"] for c in RECORDED] == CASES
    for c in RECORDED:
        assert "gfx950" not in c["stderr"], c["args"]                 # (the message of a run that went looking for a device)
        assert "z-slabs" not in c["stdout"], c["args"]                # (the slab run's first line: in front of fork and threads)
        assert c["status"] in (0, 1), c["args"]
        assert not any("tmp" in a for a in c["args"]), c["args"]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_command_line_answers_as_recorded(exe, i):
    got = run_case(exe, CASES[i])
    assert got == RECORDED[i], " ".join(CASES[i])


@pytest.mark.parametrize("lead", [[], ["-benchmark"]], ids=["plain", "benchmark"])
def test_a_bad_logstyle_is_refused_without_a_device(exe, lead):
    out = subprocess.run([exe] + lead + ["-n=4096", "-log=benchmark.txt", "-logstyle=bad"], capture_output=True, text=True,
                         stdin=subprocess.DEVNULL, timeout=60)
    assert out.returncode != 0
    lines = [ln for ln in out.stderr.splitlines() if not ln.startswith("note: no OpenGL")]
    assert len(lines) == 1 and "-logstyle" in lines[0], out.stderr
    assert "gfx950" not in out.stderr
    assert len(out.stderr.splitlines()) - len(lines) == (0 if lead else 1)
