"""GPU: the obstacle slots through the host class (ParticleSystem::selectObstacle / selectedObstacle / clearAllObstacles, and
clearObstacles() on the selected slot, on top of sph_obstacle_select) -- the particles and the load the class gives equal the
C-ABI path bit for bit.  The class is driven by the test program sph_set_probe (csrc/sph_set_probe.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from gpufluidsimulator_amd import capi, ic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gpufluidsimulator_amd", "sph_set_probe")
DT = float(ic.DEFAULT_DT)
BOX, GRID = (4.0, 4.0, 4.0), (64, 64, 64)
CENTRE, HALF, ROUND, SPACING = (-1.75, -1.75, -1.75), (0.25, 0.05, 0.12), 0.01, 0.0625
OFF, VEL = (0.03, -0.02, 0.04), (50.0, 0.0, -20.0)
PIVOT, QUAT, OMEGA = (-1.7, -1.8, -1.75), (0.9, 0.2, -0.3, 0.25), (300.0, -200.0, 4000.0)
RAMP = capi.Shape.halfspace((-1.75, -1.85, 0.0), (-0.5, 1.0, 0.0))
UPDATES = 5


@pytest.mark.parametrize("slot", [1, 3])
def test_the_host_class_equals_the_c_abi_path(tmp_path, slot):
    f = tmp_path / "state.bin"
    numbers = [*CENTRE, *HALF, ROUND, SPACING, *OFF, *VEL, *PIVOT, *QUAT, *OMEGA]
    out = subprocess.run([EXE, str(f), str(UPDATES), str(slot)] + [repr(float(v)) for v in numbers], capture_output=True,
                         text=True, timeout=300)                                     # a fresh child process
    assert out.returncode == 0, out.stderr
    # the selection and the installed mask: fresh, both installed (slot 0 selected last), the box cleared, all cleared
    assert out.stdout.split("\n")[:4] == ["sel 0 mask 0", "sel 0 mask %d" % (1 | 1 << slot), "sel %d mask 1" % slot, "sel 0 mask 0"]
    raw = np.fromfile(f, dtype=np.uint8)
    state = raw[:2 * 4096 * 16].view(np.float32).reshape(2, 4096, 4)
    load = raw[2 * 4096 * 16:].view(np.float64)
    assert load.shape == (6,)
    pos, vel = ic.dam_break_lattice((16, 16, 16), BOX, jitter=True)
    with capi.Context(4096, box=BOX, grid=GRID) as c, capi.Context(4096, box=BOX, grid=GRID) as b:
        c.build_obstacle([RAMP], SPACING, slot=0)
        c.build_obstacle([capi.Shape.box(CENTRE, HALF, ROUND)], SPACING, slot=slot)
        c.set_obstacle_motion(offset=OFF, velocity=VEL, slot=slot)
        c.set_obstacle_pose(PIVOT, QUAT, OMEGA, slot=slot)
        c.set_obstacle_sensor(True, slot=slot)
        b.build_obstacle([RAMP], SPACING)                                             # the ramp alone: what the box adds is seen
        c.upload(pos, vel); b.upload(pos, vel)
        c.step(DT, UPDATES); b.step(DT, UPDATES)
        st, want = c.download(), c.obstacle_load(slot=slot)
        assert (st["pos"] != b.download()["pos"]).any(axis=1).sum() > 100
        assert c.obstacle_load(slot=0)["steps"] == 0
    assert np.array_equal(state[0, :, :3].view(np.uint32), st["pos"].view(np.uint32))
    assert np.array_equal(state[1, :, :3].view(np.uint32), st["vel"].view(np.uint32))
    assert want["steps"] == UPDATES and np.abs(want["J"]).max() > 0
    assert np.array_equal(load[:3].view(np.uint64), want["J"].view(np.uint64))
    assert np.array_equal(load[3:].view(np.uint64), want["L"].view(np.uint64))


# ---- the headless driver: -solid=<k>:... on top of the class -----------------------------------------------------------------------
HEADLESS = os.path.join(ROOT, "gpufluidsimulator_amd", "sph_headless")


def test_headless_solids_equal_the_c_abi_path(tmp_path):
    """slot 0 through the -obstacle family (the ramp), slot 1 a union of two shapes that translates, slot 3 a box that spins
    (-solidspin: the identity quaternion, the sensor on); the state the driver writes and the lines it prints per slot at the
    end -- offset, quaternion, J and L with 9 / 17 digits, so they read back exactly -- equal the C-ABI path"""
    f = tmp_path / "state.bin"
    out = subprocess.run([HEADLESS, "-benchmark", "-n=4096", "-box=4", "-nowarmup", "-i=5", "-obstacle=plane:-1.75,-1.85,0,-0.5,1,0",
                          "-obstaclecell=0.0625", "-solid=1:box:-1.5,-1.7,-1.75,0.1875,0.375,0.1875,0.03",
                          "-solid=1:capsule:-1.9,-1.6,-1.9,-1.6,-1.6,-1.6,0.05", "-solidcell=1:0.0625", "-solidvel=1:200,0,-50",
                          "-solid=3:box:-1.75,-1.75,-1.75,0.25,0.05,0.12", "-solidcell=3:0.0625", "-solidspin=3:-1.7,-1.8,-1.75,300,-200,4000",
                          f"-out={f}"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    raw = np.fromfile(f, dtype=np.float32).reshape(2, 4096, 4)
    lines = {int(ln.split()[1].rstrip(":")): ln.split() for ln in out.stdout.splitlines() if ln.startswith("solid ")}
    assert sorted(lines) == [0, 1, 3]
    pos, vel = ic.dam_break_lattice((16, 16, 16), BOX, jitter=True)
    with capi.Context(4096, box=BOX, grid=GRID) as c:
        c.build_obstacle([RAMP], 0.0625)
        c.build_obstacle([capi.Shape.box((-1.5, -1.7, -1.75), (0.1875, 0.375, 0.1875), 0.03),
                          capi.Shape.capsule((-1.9, -1.6, -1.9), (-1.6, -1.6, -1.6), 0.05)], 0.0625, slot=1)
        c.set_obstacle_motion(velocity=(200.0, 0.0, -50.0), slot=1)
        c.build_obstacle([capi.Shape.box((-1.75, -1.75, -1.75), (0.25, 0.05, 0.12))], 0.0625, slot=3)
        c.set_obstacle_pose((-1.7, -1.8, -1.75), (1.0, 0.0, 0.0, 0.0), (300.0, -200.0, 4000.0), slot=3)
        c.set_obstacle_sensor(True, slot=3)
        c.upload(pos, vel)
        c.step(DT, 5)
        st = c.download()
        for k, w in lines.items():      # solid k: offset x y z quaternion w x y z J x y z L x y z
            assert [w[2], w[6], w[11], w[15]] == ["offset", "quaternion", "J", "L"], w
            ps, load = c.obstacle_pose(slot=k), c.obstacle_load(slot=k)
            assert np.array_equal(np.array(w[3:6], np.float32).view(np.uint32), c.obstacle(slot=k)["offset"].view(np.uint32)), k
            quat = ps["quat"] if ps is not None else np.array([1.0, 0.0, 0.0, 0.0])
            assert np.array_equal(np.array(w[7:11], np.float64).view(np.uint64), quat.view(np.uint64)), k
            assert np.array_equal(np.array(w[12:15], np.float64).view(np.uint64), load["J"].view(np.uint64)), k
            assert np.array_equal(np.array(w[16:19], np.float64).view(np.uint64), load["L"].view(np.uint64)), k
        assert np.abs(c.obstacle_load(slot=3)["J"]).max() > 0 and c.obstacle_pose(slot=3)["quat"][0] < 1.0
    assert np.array_equal(raw[0, :, :3].view(np.uint32), st["pos"].view(np.uint32))
    assert np.array_equal(raw[1, :, :3].view(np.uint32), st["vel"].view(np.uint32))
