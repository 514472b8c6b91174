"""GPU: obstacles through the host class and the headless driver (sph_headless -obstacle=...: ParticleSystem::setObstacles /
setObstacleMotion on top of sph_obstacle_build) -- the state the driver writes equals the C-ABI path bit for bit, the options'
forms, and the refusal next to -gpus=N."""
import os
import subprocess

import numpy as np
import pytest

from gpufluidsimulator_amd import capi, ic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gpufluidsimulator_amd", "sph_headless")
DT = float(ic.DEFAULT_DT)
BOX, GRID = (4.0, 4.0, 4.0), (64, 64, 64)


def _run(args):
    return subprocess.run([EXE, "-benchmark", "-n=4096", "-box=4", "-nowarmup"] + args, capture_output=True, text=True, timeout=300)


def test_headless_obstacles_equal_the_c_abi_path(tmp_path):
    f = tmp_path / "state.bin"
    out = _run(["-i=5", "-obstacle=box:-1.5,-1.7,-1.75,0.1875,0.375,0.1875,0.03", "-obstacle=plane:-1.75,-1.85,0,-0.5,1,0",
                "-obstacle=!sphere:-1,-1,-1,1.6", "-obstacle=capsule:-1.9,-1.6,-1.9,-1.6,-1.6,-1.6,0.05", "-obstaclecell=0.0625",
                "-obstaclevel=200,0,-50", f"-out={f}"])
    assert out.returncode == 0, out.stderr
    assert "Throughput = " in out.stdout
    raw = np.fromfile(f, dtype=np.float32).reshape(2, 4096, 4)
    shapes = [capi.Shape.box((-1.5, -1.7, -1.75), (0.1875, 0.375, 0.1875), 0.03), capi.Shape.halfspace((-1.75, -1.85, 0), (-0.5, 1, 0)),
              capi.Shape.sphere((-1, -1, -1), 1.6, invert=True), capi.Shape.capsule((-1.9, -1.6, -1.9), (-1.6, -1.6, -1.6), 0.05)]
    pos, vel = ic.dam_break_lattice((16, 16, 16), BOX, jitter=True)
    with capi.Context(4096, box=BOX, grid=GRID) as c, capi.Context(4096, box=BOX, grid=GRID) as b:
        c.build_obstacle(shapes, 0.0625)
        c.set_obstacle_motion(velocity=(200.0, 0.0, -50.0))
        c.upload(pos, vel); b.upload(pos, vel)
        c.step(DT, 5); b.step(DT, 5)
        st = c.download()
        assert (st["pos"] != b.download()["pos"]).any(axis=1).sum() > 300          # (the solids did move particles)
    assert np.array_equal(raw[0, :, :3].view(np.uint32), st["pos"].view(np.uint32))
    assert np.array_equal(raw[1, :, :3].view(np.uint32), st["vel"].view(np.uint32))


def test_headless_refuses_obstacles_on_several_gpus_and_bad_forms():
    out = _run(["-i=1", "-gpus=2", "-onegpu", "-obstacle=sphere:0,0,0,0.1"])
    assert out.returncode != 0 and "-obstacle" in out.stderr
    for bad in ("-obstacle=sphere:0,0,0", "-obstacle=cube:0,0,0,1", "-obstacle=box:0,0,0,1,1", "-obstacle=plane:0,0,0,1,0,0,5,6",
                "-obstacle=0,0,0,1"):
        out = _run(["-i=1", bad])
        assert out.returncode != 0 and "-obstacle" in out.stderr, bad
    out = _run(["-i=1", "-obstaclevel=1,0,0"])
    assert out.returncode != 0 and "-obstacle" in out.stderr
    out = _run(["-i=1", "-obstacle=sphere:0,0,0,-1"])               # the form is fine; the library refuses the value, and the class aborts
    assert out.returncode != 0 and "radius" in out.stderr
