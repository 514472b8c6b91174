"""The scenes of tests/test_gpu_obstacle_set.py as plain numpy -- TEST INFRASTRUCTURE in the style of obstacle_cases.py: the
solids of every slot, and the model's slots built from them with obstacle_model.rasterise (the device's raster bit for bit).
tests/test_obstacle_set_model_cpu.py holds every scene to its conditions on the dam as uploaded; the GPU tests assert them again on
the output of the obstacle-free twin."""
import functools

import numpy as np

import obstacle_model as om
import obstacle_pose_model as pm
import obstacle_set_model as sm
from gpufluidsimulator_amd import ic

F = np.float32
BOX, GRID = (4.0, 4.0, 4.0), (64, 64, 64)
BMIN, BMAX = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)
S = 1.0 / 16.0
EPS, DAMP, MASS = F(1e-5), F(-0.75), F(65.0)
ZERO = (0.0, 0.0, 0.0)
N = 15 * 15 * 15                                   # 3375: the last wave and the last mover tile are partial
VEL_SEED = 41
SKEW = (0.9, 0.2, -0.3, 0.25)                      # (w, x, y, z), not normalised: a skew axis
LOCAL = ((-1.95, -2.1, -1.95), (-1.55, -1.4, -1.55))

# A solid: shapes, spacing, bounds (None: the box), off, u, and the pose's pivot, quat, omega (pivot None: unposed), sensor.
RAMP = dict(shapes=[om.halfspace((-1.75, -1.85, 0.0), (-0.5, 1.0, 0.0))], spacing=S, bounds=None, off=ZERO, u=ZERO, pivot=None,
            sensor=False)
# the spinning paddle of tests/test_gpu_obstacle_pose.py: a local lattice, so the ramp lifts particles INTO it from outside
PADDLE = dict(shapes=[om.box((-1.75, -1.75, -1.75), (0.25, 0.05, 0.12))], spacing=S, bounds=LOCAL, off=(0.03, -0.02, 0.04),
              u=(50.0, 0.0, -20.0), pivot=(-1.7, -1.8, -1.75), quat=SKEW, omega=(300.0, -200.0, 4000.0), sensor=True)
# a translating bar across the paddle on a fine local lattice: bricks of 1/8, so most of the dam is outside its guard
BAR = dict(shapes=[om.box((-1.8, -1.68, -1.7), (0.06, 0.2, 0.1))], spacing=S / 2, bounds=((-1.9, -1.9, -1.82), (-1.7, -1.46, -1.58)),
           off=(-0.01, 0.015, 0.0), u=(-30.0, 60.0, 10.0), pivot=None, sensor=True)
# the paddle with the identity pose about a far pivot: the posed arithmetic with no rotation to show for it
IDENTITY_POSED = dict(PADDLE, quat=(1.0, 0.0, 0.0, 0.0), omega=ZERO, pivot=(1.1, 1.3, 0.77))
SCENE = {0: RAMP, 1: PADDLE, 3: BAR}               # the scene of "one step equals the model": slot 2 stays empty
# two overlapping solids whose order can be seen
OVERLAP_A = dict(shapes=[om.sphere((-1.8, -1.75, -1.75), 0.16)], spacing=S, bounds=None, off=ZERO, u=ZERO, pivot=None, sensor=False)
OVERLAP_B = dict(shapes=[om.box((-1.68, -1.75, -1.75), (0.1, 0.2, 0.2))], spacing=S, bounds=LOCAL, off=ZERO, u=(40.0, 0.0, 0.0), pivot=None,
                 sensor=True)


@functools.lru_cache(maxsize=None)
def _dam_arrays():
    pos, _ = ic.dam_break_lattice((15, 15, 15), BOX, jitter=True)      # fills [-2, -1.53]^3
    vel = np.random.default_rng(VEL_SEED).normal(0, 100, pos.shape).astype(F)
    return pos, vel


def dam():
    pos, vel = _dam_arrays()
    return pos.copy(), vel.copy()


def pose_of(solid):
    return None if solid["pivot"] is None else pm.pose(solid["pivot"], solid["quat"], solid["omega"])


def grid_of(solid):
    lo, hi = solid["bounds"] if solid["bounds"] is not None else (BMIN, BMAX)
    return om.lattice(solid["spacing"], lo, hi)


def model_slot(solid, grid=None, phi=None):
    """The model's slot of a solid; grid and phi as the device reports them, or (CPU) rasterised here."""
    if grid is None:
        grid = grid_of(solid)
        phi = om.rasterise(solid["shapes"], grid)
    return sm.slot(grid, phi, solid["off"], solid["u"], pose_of(solid))


def model_slots(scene):
    return {k: model_slot(s) for k, s in scene.items()}


def push(pos, vel, slots):
    return sm.push(pos, vel, slots, BMIN, BMAX, EPS, DAMP, MASS)
