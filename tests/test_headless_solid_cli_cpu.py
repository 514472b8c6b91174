"""CPU: the forms of the headless driver's -solid=<k>:..., -solidcell, -solidband, -solidvel and -solidspin options (the
obstacle slots of sph_obstacle_select), in the manner of tests/test_headless_cli_cpu.py with a case list of its own: every case
of tests/headless_solid_cli_cases.py ends before any GPU call with the status and the line written down there."""
import os
import subprocess

import pytest

from headless_cli_cases import EXE
from headless_solid_cli_cases import CASES


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        from gpufluidsimulator_amd import build
        build.build()
    return EXE


@pytest.mark.parametrize("i", range(len(CASES)))
def test_a_solid_option_answers_as_written_down(exe, i):
    args, status, piece = CASES[i]
    out = subprocess.run([exe] + args, capture_output=True, text=True, stdin=subprocess.DEVNULL, timeout=60)
    assert out.returncode == status, (args, out.stderr)
    assert "gfx950" not in out.stderr, args                             # (the message of a run that went looking for a device)
    if status:
        assert out.stdout == "" and len(out.stderr.splitlines()) == 1 and piece in out.stderr, (args, out.stderr)
    else:
        assert out.stderr == "" and piece in out.stdout, (args, out.stdout)


def test_the_help_of_the_releases_before_the_slots_is_unchanged(exe):
    """-help keeps its recorded text (tests/golden/headless_cli.json); the slots have a help of their own"""
    out = subprocess.run([exe, "-benchmark", "-help"], capture_output=True, text=True, stdin=subprocess.DEVNULL, timeout=60)
    assert out.returncode == 0 and "-solid" not in out.stdout and "-obstaclemesh" in out.stdout
