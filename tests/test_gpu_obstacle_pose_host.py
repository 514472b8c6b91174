"""GPU: the posed obstacle and the load sensor through the host class (ParticleSystem::setObstaclePose / clearObstaclePose /
senseObstacleLoad / getObstacleLoad on top of sph_obstacle_set_pose and sph_obstacle_set_sensor) -- the state and the load the
class gives equal the C-ABI path bit for bit.  The class is driven by the test program sph_pose_probe (csrc/sph_pose_probe.cpp):
the headless driver has no option for the pose yet."""
import os
import subprocess

import numpy as np
import pytest

from gpufluidsimulator_amd import capi, ic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gpufluidsimulator_amd", "sph_pose_probe")
DT = float(ic.DEFAULT_DT)
BOX, GRID = (4.0, 4.0, 4.0), (64, 64, 64)
CENTRE, HALF, ROUND, SPACING = (-1.75, -1.75, -1.75), (0.25, 0.05, 0.12), 0.01, 0.0625
OFF, VEL = (0.03, -0.02, 0.04), (50.0, 0.0, -20.0)
PIVOT, QUAT, OMEGA = (-1.7, -1.8, -1.75), (0.9, 0.2, -0.3, 0.25), (300.0, -200.0, 4000.0)
UPDATES = 5


@pytest.mark.parametrize("drop", [False, True], ids=["posed", "pose dropped"])
def test_the_host_class_equals_the_c_abi_path(tmp_path, drop):
    f = tmp_path / "state.bin"
    numbers = [*CENTRE, *HALF, ROUND, SPACING, *OFF, *VEL, *PIVOT, *QUAT, *OMEGA]
    out = subprocess.run([EXE, str(f), str(UPDATES), str(int(drop))] + [repr(float(v)) for v in numbers], capture_output=True,
                         text=True, timeout=300)                                     # a fresh child process
    assert out.returncode == 0, out.stderr
    raw = np.fromfile(f, dtype=np.uint8)
    state = raw[:2 * 4096 * 16].view(np.float32).reshape(2, 4096, 4)
    load = raw[2 * 4096 * 16:].view(np.float64)
    assert load.shape == (6,)
    pos, vel = ic.dam_break_lattice((16, 16, 16), BOX, jitter=True)
    with capi.Context(4096, box=BOX, grid=GRID) as c, capi.Context(4096, box=BOX, grid=GRID) as b:
        c.build_obstacle([capi.Shape.box(CENTRE, HALF, ROUND)], SPACING)
        c.set_obstacle_motion(offset=OFF, velocity=VEL)
        c.set_obstacle_pose(PIVOT, QUAT, OMEGA)
        if drop:
            c.set_obstacle_pose(None)
        c.set_obstacle_sensor(True)
        c.upload(pos, vel); b.upload(pos, vel)
        c.step(DT, UPDATES); b.step(DT, UPDATES)
        st, want = c.download(), c.obstacle_load()
        assert (st["pos"] != b.download()["pos"]).any(axis=1).sum() > 100             # (the solid did move particles)
        assert (c.obstacle_pose() is None) == drop
    assert np.array_equal(state[0, :, :3].view(np.uint32), st["pos"].view(np.uint32))
    assert np.array_equal(state[1, :, :3].view(np.uint32), st["vel"].view(np.uint32))
    assert want["steps"] == UPDATES and np.abs(want["J"]).max() > 0
    assert np.array_equal(load[:3].view(np.uint64), want["J"].view(np.uint64))
    assert np.array_equal(load[3:].view(np.uint64), want["L"].view(np.uint64))
