"""GPU: a body through the host class and the headless driver (ParticleSystem::setObstacleBody / getObstacleState under
sph_headless -solidbody=<k>:...): a paddle on a hinge, and one that floats, in the 4096-particle dam -- the state the driver
writes and the lines it prints per slot equal the C-ABI path bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from gpufluidsimulator_amd import capi, ic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLESS = os.path.join(ROOT, "gpufluidsimulator_amd", "sph_headless")
DT = float(ic.DEFAULT_DT)
BOX, GRID = (4.0, 4.0, 4.0), (64, 64, 64)
PADDLE, PIVOT, OMEGA = ((-1.75, -1.75, -1.75), (0.25, 0.05, 0.12)), (-1.7, -1.8, -1.75), (300.0, -200.0, 4000.0)
F = np.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _run(tmp_path, body_option, body):
    f = tmp_path / "state.bin"
    out = subprocess.run([HEADLESS, "-benchmark", "-n=4096", "-box=4", "-nowarmup", "-i=5",
                          "-solid=3:box:" + ",".join(str(v) for v in PADDLE[0] + PADDLE[1]), "-solidcell=3:0.0625",
                          "-solidspin=3:" + ",".join(str(v) for v in PIVOT + OMEGA), body_option, f"-out={f}"],
                         capture_output=True, text=True, timeout=300)                # a fresh child process
    assert out.returncode == 0, out.stderr
    raw = np.fromfile(f, dtype=np.float32).reshape(2, 4096, 4)
    words = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("solid 3")]
    assert len(words) == 2 and words[0][1] == "3:" and words[1][1:3] == ["3", "body:"], out.stdout
    w, b = words
    assert [w[2], w[6], w[11], w[15]] == ["offset", "quaternion", "J", "L"] and [b[3], b[7], b[11]] == ["offset", "velocity", "omega"]
    pos, vel = ic.dam_break_lattice((16, 16, 16), BOX, jitter=True)
    with capi.Context(4096, box=BOX, grid=GRID) as c:
        c.build_obstacle([capi.Shape.box(*PADDLE)], 0.0625, slot=3)
        c.set_obstacle_pose(PIVOT, (1.0, 0.0, 0.0, 0.0), OMEGA, slot=3)
        c.set_obstacle_body(slot=3, **body)
        c.upload(pos, vel)
        c.step(DT, 5)
        st = c.download()
        ob, ps, load = c.obstacle(slot=3), c.obstacle_pose(slot=3), c.obstacle_load(slot=3)
    assert np.array_equal(_bits(raw[0, :, :3]), _bits(st["pos"])) and np.array_equal(_bits(raw[1, :, :3]), _bits(st["vel"]))
    assert np.array_equal(_bits(np.array(w[3:6], F)), _bits(ob["offset"]))
    assert np.array_equal(_bits(np.array(w[7:11], np.float64)), _bits(ps["quat"]))
    assert np.array_equal(_bits(np.array(w[12:15], np.float64)), _bits(load["J"]))
    assert np.array_equal(_bits(np.array(w[16:19], np.float64)), _bits(load["L"]))
    assert np.array_equal(_bits(np.array(b[4:7], F)), _bits(ob["offset"]))
    assert np.array_equal(_bits(np.array(b[8:11], F)), _bits(ob["velocity"]))
    assert np.array_equal(_bits(np.array(b[12:15], F)), _bits(ps["omega"]))
    assert load["steps"] == 5
    return ob, ps


def test_a_headless_wheel_on_a_hinge_turns_about_its_axis_only(tmp_path):
    body = dict(dof=capi.BODY_HINGE, inertia=(40.0, 0.0, 0.0), axis=(0.0, 0.0, 2.0), torque=(0.0, 0.0, -2.0e9))
    ob, ps = _run(tmp_path, "-solidbody=3:hinge,0,0,2,40,-2e9", body)
    om = ps["omega"]
    assert om[0] == 0 and om[1] == 0 and om[2] != 0 and om[2] != F(4000.0)       # about z, and the fluid and the torque changed it
    assert not ob["offset"].any() and not ob["velocity"].any()                   # a hinge does not translate


def test_a_headless_float_moves_and_tumbles(tmp_path):
    body = dict(dof=capi.BODY_FREE_XYZ | capi.BODY_SPIN, mass=3000.0, inertia=(30.0, 90.0, 60.0), accel=(0.0, -107910.0, 0.0),
                lo=(-1e30,) * 3, hi=(1e30,) * 3)
    ob, ps = _run(tmp_path, "-solidbody=3:float,3000,30,90,60,-107910", body)
    assert ob["velocity"].all() and ob["offset"].all() and not np.array_equal(ps["omega"], np.array(OMEGA, F))
